// mover_noise_host_check.cpp -- stand-alone driver of the host code of the seeded sensor noise under movers
// (csrc/lrc_movers.hip: lrc_scan_noisy_movers_dev, lrc_scan_noisy_movers_compact) for a sanitizer build: every refusal the two
// calls make, on handles that live on the host (a context, scenes, a mover set and a table that no device ever saw), with the
// model's own checks from the real csrc/lrc_noise.hip.  Every refusal must come with the call's name and the offender in the
// message and before the unit that launches is entered (the stubs below count their calls).  Uses no GPU: no call that would
// reach a device function is made.  Build and run from csrc/:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I. -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined ../../tools/mover_noise_host_check.cpp lrc_movers.hip lrc_noise.hip \
//         -o mover_noise_host_check
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
int check_motion(const char*, const double*, uint64_t) { return LRC_OK; }

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s   [%s]\n", __FILE__, __LINE__, #c, g_err.c_str()); ++g_bad; } } while (0)

static bool says(const char* who, const char* what) {
    return g_err.rfind(std::string(who) + ": ", 0) == 0 && g_err.find(what) != std::string::npos;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const char* const DEV = "lrc_scan_noisy_movers_dev";
    const char* const CMP = "lrc_scan_noisy_movers_compact";

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
    lrc_table table, foreign_table, empty_table;
    table.ctx = ctx; table.n = 600;
    foreign_table.ctx = other; foreign_table.n = 600;
    empty_table.ctx = ctx; empty_table.n = 0;

    const uint64_t P = 3, N = 600;
    // the pointers are never read by a refused call: exactly sized heap arrays, so that a read past them would be seen
    std::vector<double> poses(P * 16, 0.0), dirs(N * 3, 0.0);
    std::vector<float> mp(P * 12, 0.0f);
    for (uint64_t k = 0; k < P; ++k) mp[k * 12] = mp[k * 12 + 5] = mp[k * 12 + 10] = 1.0f;
    std::vector<float> mp2(P * 2 * 12, 0.0f);
    for (uint64_t k = 0; k < P * 2; ++k) mp2[k * 12] = mp2[k * 12 + 5] = mp2[k * 12 + 10] = 1.0f;
    std::vector<uint64_t> counts(P, 0);
    std::vector<float> t_col(P * N, 0.0f);
    lrc_hits hits{};
    hits.t = t_col.data();
    lrc_frames fr{};
    fr.counts = counts.data();
    const lrc_noise good{7u, 5u, 0.01, 8.7e-5, 0.05};
    uint64_t total = 99;

    auto dev = [&](lrc_scene* s, lrc_movers* m, const lrc_noise* nz, const lrc_hits* out, uint64_t rays = 600) {
        return lrc_scan_noisy_movers_dev(s, m, poses.data(), P, dirs.data(), rays, m == with_room ? mp2.data() : mp.data(), 20.0, nz, out,
                                         nullptr, nullptr);
    };
    auto cmp = [&](lrc_scene* s, lrc_movers* m, const lrc_table* tb, const float* mover_poses, const lrc_noise* nz, const lrc_frames* out,
                   uint64_t np = 3) {
        total = 99;
        return lrc_scan_noisy_movers_compact(s, m, poses.data(), np, tb, mover_poses, 20.0, nz, out, nullptr, 0, &total);
    };

    // ---- the mover calls' own refusals ----
    EXPECT(dev(nullptr, set, &good, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "NULL scene or output"));
    EXPECT(dev(room, set, &good, nullptr) == LRC_ERR_INVALID_ARG && says(DEV, "NULL scene or output"));
    EXPECT(cmp(nullptr, set, &table, mp.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "NULL scene or output") && total == 0);
    EXPECT(cmp(room, set, &table, mp.data(), &good, nullptr) == LRC_ERR_INVALID_ARG && says(CMP, "NULL scene or output"));
    EXPECT(dev(room, with_room, &good, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "the static scene is one of its own movers"));
    EXPECT(cmp(room, with_room, &table, mp2.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "one of its own movers"));
    EXPECT(dev(room, foreign, &good, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "movers and scene belong to different contexts"));
    EXPECT(cmp(room, foreign, &table, mp.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "different contexts"));
    {
        lrc_hits counted = hits;
        std::vector<uint32_t> tiles((P * N + 63) / 64, 0u);
        counted.tile_count = tiles.data();
        EXPECT(dev(room, set, &good, &counted) == LRC_ERR_INVALID_ARG && says(DEV, "tile_count is not written"));
    }
    {
        const float some = 0.0f;
        room->opts.range_noise = &some;
        EXPECT(dev(room, set, &good, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "a range_noise option is set"));
        EXPECT(dev(room, nullptr, &good, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "a range_noise option is set"));
        EXPECT(cmp(room, set, &table, mp.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "a range_noise option is set"));
        room->opts.range_noise = nullptr;
    }
    EXPECT(lrc_scan_noisy_movers_dev(room, set, nullptr, P, dirs.data(), N, mp.data(), 20.0, &good, &hits, nullptr, nullptr) ==
               LRC_ERR_INVALID_ARG && says(DEV, "poses16 or dirs3 is NULL"));
    EXPECT(lrc_scan_noisy_movers_dev(room, set, poses.data(), P, nullptr, N, mp.data(), 20.0, &good, &hits, nullptr, nullptr) ==
               LRC_ERR_INVALID_ARG && says(DEV, "poses16 or dirs3 is NULL"));
    EXPECT(lrc_scan_noisy_movers_dev(room, set, poses.data(), P, dirs.data(), N, nullptr, 20.0, &good, &hits, nullptr, nullptr) ==
               LRC_ERR_INVALID_ARG && says(DEV, "mover_poses12 is NULL"));
    EXPECT(cmp(room, set, nullptr, mp.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "table is NULL"));
    EXPECT(cmp(room, set, &foreign_table, mp.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "table and scene belong to different contexts"));
    EXPECT(cmp(room, set, &table, nullptr, &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "mover_poses12 is NULL"));
    {
        lrc_frames uncounted{};
        EXPECT(cmp(room, set, &table, mp.data(), &good, &uncounted) == LRC_ERR_INVALID_ARG && says(CMP, "poses16 or counts is NULL"));
        std::vector<float> bad = mp;
        bad[1 * 12 + 3] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(cmp(room, set, &table, bad.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "mover pose 1 has an entry that is not finite"));
        bad = mp;
        bad[2 * 12] += 0x1p-14f;
        EXPECT(cmp(room, set, &table, bad.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "mover pose 2 is no rotation"));
        bad = mp;
        bad[2 * 12 + 7] = std::numeric_limits<float>::infinity();
        EXPECT(cmp(room, set, &table, bad.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "mover pose 2 has an entry that is not finite"));
    }

    // ---- the model's refusals: what lrc_scan_noisy_dev refuses, with and without a set ----
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
            EXPECT(cmp(room, m, &table, mp.data(), &b.nz, &fr) == LRC_ERR_INVALID_ARG && says(CMP, b.what) && total == 0);
        }
        // checked for an empty call too
        EXPECT(cmp(room, set, &table, mp.data(), &b.nz, &fr, 0) == LRC_ERR_INVALID_ARG && says(CMP, b.what));
        EXPECT(cmp(room, set, &empty_table, mp.data(), &b.nz, &fr) == LRC_ERR_INVALID_ARG && says(CMP, b.what));
    }
    EXPECT(dev(room, set, nullptr, &hits) == LRC_ERR_INVALID_ARG && says(DEV, "noise is NULL"));
    EXPECT(cmp(room, set, &table, mp.data(), nullptr, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "noise is NULL"));
    EXPECT(dev(room, set, &good, &hits, 0x100000000ull) == LRC_ERR_INVALID_ARG && says(DEV, "at most 2^32 - 1 rays per pose"));
    EXPECT(dev(room, nullptr, &good, &hits, 0xFFFFFFFFFFFFFFFFull) == LRC_ERR_INVALID_ARG && says(DEV, "at most 2^32 - 1 rays per pose"));
    {
        lrc_table huge;
        huge.ctx = ctx; huge.n = 0x100000000ull;
        EXPECT(cmp(room, set, &huge, mp.data(), &good, &fr) == LRC_ERR_INVALID_ARG && says(CMP, "at most 2^32 - 1 rays per pose"));
    }

    // ---- an empty call with a good model is fine and reaches no device either ----
    EXPECT(cmp(room, set, &table, mp.data(), &good, &fr, 0) == LRC_OK && total == 0);
    EXPECT(cmp(room, set, &empty_table, mp.data(), &good, &fr) == LRC_OK && total == 0);
    EXPECT(cmp(room, nullptr, &empty_table, nullptr, &good, &fr) == LRC_OK);
    const lrc_noise edge{0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull, 0.0, 0.0, 0.99999999999999989};      // the largest dropout below 1
    EXPECT(cmp(room, set, &empty_table, mp.data(), &edge, &fr) == LRC_OK);

    EXPECT(g_entered == 0);          // every refusal came before the unit that launches
    EXPECT(ctx->d_noise_tab == nullptr && set->scratch == nullptr);

    EXPECT(lrc_movers_destroy(set) == LRC_OK && lrc_movers_destroy(with_room) == LRC_OK && lrc_movers_destroy(foreign) == LRC_OK);
    delete room; delete body; delete foreign_body; delete ctx; delete other;
    std::printf(g_bad ? "mover_noise_host_check: %d FAILED\n" : "mover_noise_host_check: ok\n", g_bad);
    return g_bad ? 1 : 0;
}
