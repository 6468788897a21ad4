// mover_sweep_noise_host_check.cpp -- stand-alone driver of the host code of the seeded sensor noise under movers in sweeps
// (csrc/lrc_movers.hip: lrc_scan_noisy_mover_sweeps_dev, lrc_scan_noisy_mover_sweeps_compact) for a sanitizer build: every refusal
// the two calls make, with and without a set and in empty calls too, on handles that live on the host (a context, scenes, mover
// sets and tables that no device ever saw), with the model's own checks from the real csrc/lrc_noise.hip.  Every refusal must come
// with the call's name and the offender in the message and before the unit that launches is entered (the stubs below count their
// calls).  Uses no GPU: no call that would reach a device function is made.  Build and run from csrc/:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I. -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined ../../tools/mover_sweep_noise_host_check.cpp lrc_movers.hip lrc_noise.hip \
//         -o mover_sweep_noise_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "lrc_internal.h"

// ---- what lrc_movers.hip and lrc_noise.hip expect of the other units ----
static std::string g_err;
static int g_entered = 0;      // calls that reached a unit that launches
int fail(int code, const std::string& msg) { g_err = msg; return code; }
int movers_scan_dev(lrc_scene*, lrc_movers*, const MoverScan&, const lrc_hits*, uint8_t*, hipStream_t) { ++g_entered; return LRC_ERR_INTERNAL; }
int movers_scan_compact(lrc_scene*, lrc_movers*, const double*, uint64_t, const lrc_table*, const float*, double, bool, const lrcnoise::Params*,
                        const lrc_frames*, uint8_t*, uint64_t, uint64_t*, const FlowCompact*) { ++g_entered; return LRC_ERR_INTERNAL; }
// the sensor's records: the two checks of the real check_motion (lidarcast.hip) that the cases below meet
int check_motion(const char* who, const double* m, uint64_t P) {
    for (uint64_t k = 0; k < P; ++k) {
        for (int j = 0; j < 24; ++j)
            if (!std::isfinite(m[k * 24 + j])) return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": record " + std::to_string(k) + " is not finite");
        if (m[k * 24 + 12] < 0.70710678118654752440)
            return fail(LRC_ERR_INVALID_ARG, std::string(who) + ": record " + std::to_string(k) + " rotates by more than pi/2 per sweep");
    }
    return LRC_OK;
}

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s   [%s]\n", __FILE__, __LINE__, #c, g_err.c_str()); ++g_bad; } } while (0)

static bool says(const char* who, const char* what) {
    return g_err.rfind(std::string(who) + ": ", 0) == 0 && g_err.find(what) != std::string::npos;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const char* const DEV = "lrc_scan_noisy_mover_sweeps_dev";
    const char* const CMP = "lrc_scan_noisy_mover_sweeps_compact";

    // handles on the host: nothing below reaches a device function
    lrc_ctx* ctx = new lrc_ctx;
    lrc_ctx* other = new lrc_ctx;
    lrc_scene* room = new lrc_scene;
    lrc_scene* body = new lrc_scene;
    lrc_scene* foreign_body = new lrc_scene;
    room->ctx = body->ctx = ctx;
    foreign_body->ctx = other;
    lrc_movers* set = nullptr;
    lrc_movers* with_room = nullptr;
    lrc_movers* foreign = nullptr;
    lrc_scene* one[1] = {body};
    EXPECT(lrc_movers_create(ctx, one, 1, &set) == LRC_OK && set);
    lrc_scene* two[2] = {body, room};
    EXPECT(lrc_movers_create(ctx, two, 2, &with_room) == LRC_OK && with_room);
    lrc_scene* third[1] = {foreign_body};
    EXPECT(lrc_movers_create(other, third, 1, &foreign) == LRC_OK && foreign);
    // a fire table is a device pointer the refused calls never read: any non-NULL value stands for "the table has one"
    double fire_stands_in = 0.0;
    lrc_table table, foreign_table, empty_table, bare_table;
    table.ctx = ctx; table.n = 600; table.d_fire = &fire_stands_in;
    foreign_table.ctx = other; foreign_table.n = 600; foreign_table.d_fire = &fire_stands_in;
    empty_table.ctx = ctx; empty_table.n = 0; empty_table.d_fire = &fire_stands_in;
    bare_table.ctx = ctx; bare_table.n = 600;

    const uint64_t P = 3, N = 600;
    // the pointers are never read by a refused call beyond what it checks: exactly sized heap arrays, so that a read past them
    // would be seen
    std::vector<double> motion(P * 24, 0.0), dirs(N * 3, 0.0), fire(N, 0.0);
    for (uint64_t k = 0; k < P; ++k) motion[k * 24] = motion[k * 24 + 5] = motion[k * 24 + 10] = motion[k * 24 + 12] = 1.0;
    auto still = [](uint64_t count) {
        std::vector<float> r(count * 24, 0.0f);
        for (uint64_t k = 0; k < count; ++k) r[k * 24] = r[k * 24 + 5] = r[k * 24 + 10] = r[k * 24 + 12] = 1.0f;
        return r;
    };
    const std::vector<float> mr = still(P), mr2 = still(P * 2);
    std::vector<uint64_t> counts(P, 0);
    std::vector<float> t_col(P * N, 0.0f);
    lrc_hits hits{};
    hits.t = t_col.data();
    lrc_frames fr{};
    fr.counts = counts.data();
    const lrc_noise good{7u, 5u, 0.01, 8.7e-5, 0.05};
    uint64_t total = 99;

    auto dev = [&](lrc_scene* s, lrc_movers* m, const lrc_noise* nz, const lrc_hits* out, uint64_t rays = 600) {
        return lrc_scan_noisy_mover_sweeps_dev(s, m, motion.data(), P, dirs.data(), fire.data(), rays,
                                               m == with_room ? mr2.data() : mr.data(), 20.0, nz, out, nullptr, nullptr);
    };
    auto cmp = [&](lrc_scene* s, lrc_movers* m, const lrc_table* tb, const float* records, const lrc_noise* nz, const lrc_frames* out,
                   uint64_t np = 3, const double* sensor = nullptr) {
        total = 99;
        return lrc_scan_noisy_mover_sweeps_compact(s, m, sensor ? sensor : motion.data(), np, tb, records, 20.0, nz, out, nullptr, 0,
                                                   &total);
    };

    // ---- the mover sweep calls' own refusals ----
    EXPECT(dev(nullptr, set, &good, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "NULL scene or output"));
    EXPECT(dev(room, set, &good, nullptr) == LRC_ERR_INVALID_ARG && says(DEV, "NULL scene or output"));
    EXPECT(cmp(nullptr, set, &table, mr.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "NULL scene or output") && total == 0);
    EXPECT(cmp(room, set, &table, mr.data(), &good, nullptr) == LRC_ERR_INVALID_ARG && says(CMP, "NULL scene or output"));
    EXPECT(dev(room, with_room, &good, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "the static scene is one of its own movers"));
    EXPECT(cmp(room, with_room, &table, mr2.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "one of its own movers"));
    EXPECT(dev(room, foreign, &good, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "movers and scene belong to different contexts"));
    EXPECT(cmp(room, foreign, &table, mr.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "different contexts"));
    {
        lrc_hits counted = hits;
        std::vector<uint32_t> tiles((P * N + 63) / 64, 0u);
        counted.tile_count = tiles.data();
        EXPECT(dev(room, set, &good, &counted) == LRC_ERR_INVALID_ARG && says(DEV, "tile_count is not written"));
        EXPECT(dev(room, nullptr, &good, &counted) == LRC_ERR_INVALID_ARG && says(DEV, "tile_count is not written"));
    }
    {
        const float some = 0.0f;
        room->opts.range_noise = &some;
        EXPECT(dev(room, set, &good, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "a range_noise option is set"));
        EXPECT(dev(room, nullptr, &good, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "a range_noise option is set"));
        EXPECT(cmp(room, set, &table, mr.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "a range_noise option is set"));
        EXPECT(cmp(room, nullptr, &table, nullptr, &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "a range_noise option is set"));
        EXPECT(cmp(room, set, &table, mr.data(), &good, &fr, 0) == LRC_ERR_INVALID_ARG && says(CMP, "a range_noise option is set"));
        room->opts.range_noise = nullptr;
    }
    for (lrc_movers* m : {set, (lrc_movers*)nullptr}) {
        EXPECT(lrc_scan_noisy_mover_sweeps_dev(room, m, nullptr, P, dirs.data(), fire.data(), N, mr.data(), 20.0, &good, &hits, nullptr,
                                               nullptr) == LRC_ERR_INVALID_ARG && says(DEV, "motion24, dirs3 or fire is NULL"));
        EXPECT(lrc_scan_noisy_mover_sweeps_dev(room, m, motion.data(), P, nullptr, fire.data(), N, mr.data(), 20.0, &good, &hits, nullptr,
                                               nullptr) == LRC_ERR_INVALID_ARG && says(DEV, "motion24, dirs3 or fire is NULL"));
        EXPECT(lrc_scan_noisy_mover_sweeps_dev(room, m, motion.data(), P, dirs.data(), nullptr, N, mr.data(), 20.0, &good, &hits, nullptr,
                                               nullptr) == LRC_ERR_INVALID_ARG && says(DEV, "motion24, dirs3 or fire is NULL"));
    }
    EXPECT(lrc_scan_noisy_mover_sweeps_dev(room, set, motion.data(), P, dirs.data(), fire.data(), N, nullptr, 20.0, &good, &hits, nullptr,
                                           nullptr) == LRC_ERR_INVALID_ARG && says(DEV, "mover_motion24 is NULL"));
    EXPECT(cmp(room, set, nullptr, mr.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "table is NULL"));
    EXPECT(cmp(room, set, &foreign_table, mr.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "table and scene belong to different contexts"));
    EXPECT(cmp(room, set, &bare_table, mr.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "the table has no fire table"));
    EXPECT(cmp(room, nullptr, &bare_table, nullptr, &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "the table has no fire table"));
    EXPECT(cmp(room, set, &bare_table, mr.data(), &good, &fr, 0) == LRC_ERR_INVALID_ARG && says(CMP, "the table has no fire table"));
    EXPECT(cmp(room, set, &table, nullptr, &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "mover_motion24 is NULL"));
    {
        lrc_frames uncounted{};
        EXPECT(cmp(room, set, &table, mr.data(), &good, &uncounted) == LRC_ERR_INVALID_ARG && says(CMP, "motion24 or counts is NULL"));
        EXPECT(cmp(room, nullptr, &table, nullptr, &good, &uncounted) == LRC_ERR_INVALID_ARG && says(CMP, "motion24 or counts is NULL"));
        // the sensor's records, with and without a set
        std::vector<double> sensor = motion;
        sensor[1 * 24 + 17] = nan;
        EXPECT(cmp(room, set, &table, mr.data(), &good, &fr, 3, sensor.data()) == LRC_ERR_INVALID_ARG && says(CMP, "record 1 is not finite"));
        EXPECT(cmp(room, nullptr, &table, nullptr, &good, &fr, 3, sensor.data()) == LRC_ERR_INVALID_ARG && says(CMP, "record 1 is not finite"));
        sensor = motion;
        sensor[2 * 24 + 12] = 0.5;
        EXPECT(cmp(room, set, &table, mr.data(), &good, &fr, 3, sensor.data()) == LRC_ERR_INVALID_ARG && says(CMP, "record 2 rotates by more than pi/2"));
        // the movers' records
        std::vector<float> bad = mr;
        bad[1 * 24 + 3] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(cmp(room, set, &table, bad.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "mover sweep record 1 has an entry that is not finite"));
        bad = mr;
        bad[2 * 24 + 17] = std::numeric_limits<float>::infinity();
        EXPECT(cmp(room, set, &table, bad.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "mover sweep record 2 has an entry that is not finite"));
        bad = mr;
        bad[2 * 24] += 0x1p-12f;
        EXPECT(cmp(room, set, &table, bad.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "mover sweep record 2 is no rotation"));
        bad = mr;
        bad[0 * 24 + 12] = 0.69f;
        bad[0 * 24 + 15] = 0.72f;
        EXPECT(cmp(room, set, &table, bad.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "mover sweep record 0 rotates by more than pi/2 per sweep"));
    }

    // ---- the model's refusals: what lrc_scan_noisy_sweeps_dev refuses, with and without a set ----
    struct Bad { lrc_noise nz; const char* what; };
    const Bad bads[] = {
        {{7u, 5u, -0.01, 0.0, 0.0}, "range_std must be finite and not negative"}, {{7u, 5u, inf, 0.0, 0.0}, "range_std must be finite"},
        {{7u, 5u, nan, 0.0, 0.0}, "range_std must be finite"}, {{7u, 5u, 0.0, -1e-300, 0.0}, "angle_std must be finite and not negative"},
        {{7u, 5u, 0.0, inf, 0.0}, "angle_std must be finite"}, {{7u, 5u, 0.0, nan, 0.0}, "angle_std must be finite"},
        {{7u, 5u, 0.0, 0.0, 1.0}, "dropout must lie in [0, 1)"}, {{7u, 5u, 0.0, 0.0, -1e-9}, "dropout must lie in [0, 1)"},
        {{7u, 5u, 0.0, 0.0, nan}, "dropout must lie in [0, 1)"}, {{7u, 5u, 0.0, 0.0, inf}, "dropout must lie in [0, 1)"}};
    for (const Bad& b : bads) {
        for (lrc_movers* m : {set, (lrc_movers*)nullptr}) {
            EXPECT(dev(room, m, &b.nz, &hits) == LRC_ERR_INVALID_ARG && says(DEV, b.what));
            EXPECT(dev(room, m, &b.nz, &hits, 0) == LRC_ERR_INVALID_ARG && says(DEV, b.what));          // an empty call too
            EXPECT(cmp(room, m, &table, mr.data(), &b.nz, &fr) == LRC_ERR_INVALID_ARG && says(CMP, b.what) && total == 0);
            EXPECT(cmp(room, m, &table, mr.data(), &b.nz, &fr, 0) == LRC_ERR_INVALID_ARG && says(CMP, b.what));
            EXPECT(cmp(room, m, &empty_table, mr.data(), &b.nz, &fr) == LRC_ERR_INVALID_ARG && says(CMP, b.what));
        }
    }
    for (lrc_movers* m : {set, (lrc_movers*)nullptr}) {
        EXPECT(dev(room, m, nullptr, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "noise is NULL"));
        EXPECT(cmp(room, m, &table, mr.data(), nullptr, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "noise is NULL"));
        EXPECT(cmp(room, m, &empty_table, mr.data(), nullptr, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "noise is NULL"));
    }
    EXPECT(dev(room, set, &good, &hits, 0x100000000ull) == LRC_ERR_INVALID_ARG && says(DEV, "at most 2^32 - 1 rays per pose"));
    EXPECT(dev(room, nullptr, &good, &hits, 0xFFFFFFFFFFFFFFFFull) == LRC_ERR_INVALID_ARG && says(DEV, "at most 2^32 - 1 rays per pose"));
    {
        lrc_table huge;
        huge.ctx = ctx; huge.n = 0x100000000ull; huge.d_fire = &fire_stands_in;
        EXPECT(cmp(room, set, &huge, mr.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "at most 2^32 - 1 rays per pose"));
        EXPECT(cmp(room, nullptr, &huge, nullptr, &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "at most 2^32 - 1 rays per pose"));
    }

    // ---- an empty call with a good model is fine and reaches no device either ----
    EXPECT(cmp(room, set, &table, mr.data(), &good, &fr, 0) == LRC_OK && total == 0);
    EXPECT(cmp(room, set, &empty_table, mr.data(), &good, &fr) == LRC_OK && total == 0);
    EXPECT(cmp(room, nullptr, &empty_table, nullptr, &good, &fr) == LRC_OK);
    const lrc_noise edge{0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull, 0.0, 0.0, 0.99999999999999989};      // the largest dropout below 1
    EXPECT(cmp(room, set, &empty_table, mr.data(), &edge, &fr) == LRC_OK);

    EXPECT(g_entered == 0);          // every refusal came before the unit that launches
    EXPECT(ctx->d_noise_tab == nullptr && set->scratch == nullptr);

    EXPECT(lrc_movers_destroy(set) == LRC_OK && lrc_movers_destroy(with_room) == LRC_OK && lrc_movers_destroy(foreign) == LRC_OK);
    delete room; delete body; delete foreign_body; delete ctx; delete other;
    std::printf(g_bad ? "mover_sweep_noise_host_check: %d FAILED\n" : "mover_sweep_noise_host_check: ok\n", g_bad);
    return g_bad ? 1 : 0;
}
