// movers_host_check.cpp -- stand-alone driver of the host side of the moving objects (csrc/lrc_movers.hip, csrc/lrc_movers.h)
// for a sanitizer build: lrc_mover_rays, lrc_mover_merge, lrc_mover_sweep_rays and lrc_mover_sweep_normals on random and crafted
// columns in exactly sized heap arrays, checked against a plain restatement of the header's text; the refusals that need no device; and the cull test of the ray kernel
// (lrcmov::culled) against a float64 slab test: a ray that meets the mover's box must never be left out.  Uses no GPU.  The
// units lrc_movers.hip calls into are stubbed below.  Build and run from csrc/:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I. -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined ../../tools/movers_host_check.cpp lrc_movers.hip -o movers_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "lrc_internal.h"

// ---- what lrc_movers.hip expects of the other units ----
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
int movers_scan_dev(lrc_scene*, lrc_movers*, const MoverScan&, const lrc_hits*, uint8_t*, hipStream_t) { return LRC_ERR_INTERNAL; }
int movers_scan_compact(lrc_scene*, lrc_movers*, const double*, uint64_t, const lrc_table*, const float*, double, bool, const lrcnoise::Params*,
                        const lrc_frames*, uint8_t*, uint64_t, uint64_t*, const FlowCompact*) { return LRC_ERR_INTERNAL; }
int check_motion(const char*, const double*, uint64_t) { return LRC_OK; }
int noise_params(lrc_ctx*, const char*, const lrc_noise*, uint64_t, lrcnoise::Params*) { return LRC_ERR_INTERNAL; }
int noise_params_host(const char*, const lrc_noise*, uint64_t, lrcnoise::Params*) { return LRC_ERR_INTERNAL; }

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_bad; } } while (0)

static bool same_bits(const float* a, const float* b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

static void random_pose(std::mt19937& g, float* m) {
    std::uniform_real_distribution<double> u(-3.14, 3.14), c(-8.0, 8.0);
    const double a = u(g), b = u(g), k = u(g);
    const double R[9] = {std::cos(a) * std::cos(b), std::cos(a) * std::sin(b) * std::sin(k) - std::sin(a) * std::cos(k),
                         std::cos(a) * std::sin(b) * std::cos(k) + std::sin(a) * std::sin(k),
                         std::sin(a) * std::cos(b), std::sin(a) * std::sin(b) * std::sin(k) + std::cos(a) * std::cos(k),
                         std::sin(a) * std::sin(b) * std::cos(k) - std::cos(a) * std::sin(k),
                         -std::sin(b), std::cos(b) * std::sin(k), std::cos(b) * std::cos(k)};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m[4 * i + j] = (float)R[3 * i + j];
        m[4 * i + 3] = (float)c(g);
    }
}

int main() {
    std::mt19937 g(20261019u);
    const float inf = std::numeric_limits<float>::infinity();

    // ---- lrc_mover_rays against the header's text ----
    for (int round = 0; round < 50; ++round) {
        const size_t n = 1 + (g() % 3000);
        std::vector<float> rays(n * 6), out(n * 6), want(n * 6);
        std::uniform_real_distribution<float> u(-20.f, 20.f);
        for (float& v : rays) v = u(g);
        float m[12];
        random_pose(g, m);
        EXPECT(lrc_mover_rays(rays.data(), n, m, out.data()) == LRC_OK);
        for (size_t i = 0; i < n; ++i) {
            const float* r = &rays[i * 6];
            const float e[3] = {r[0] - m[3], r[1] - m[7], r[2] - m[11]};
            for (int j = 0; j < 3; ++j) {
                want[i * 6 + j] = (m[j] * e[0] + m[4 + j] * e[1]) + m[8 + j] * e[2];
                want[i * 6 + 3 + j] = (m[j] * r[3] + m[4 + j] * r[4]) + m[8 + j] * r[5];
            }
        }
        EXPECT(same_bits(out.data(), want.data(), n * 6));
    }
    {
        float m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, r[6] = {1, 2, 3, 4, 5, 6}, o[6];
        EXPECT(lrc_mover_rays(r, 1, nullptr, o) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_mover_rays(nullptr, 1, m, o) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_mover_rays(r, 1, m, nullptr) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_mover_rays(nullptr, 0, m, nullptr) == LRC_OK);
        EXPECT(lrc_mover_rays(r, 1, m, o) == LRC_OK && same_bits(r, o, 6));
    }

    // ---- lrc_mover_merge against the header's text: misses, ties with the static scene, ties among movers ----
    for (int round = 0; round < 60; ++round) {
        const size_t n = 1 + (g() % 700);
        const uint32_t M = round < 3 ? (uint32_t)round * 127u + (round == 0) : 1 + (g() % 9);      // 1, 127, 254, then small sets
        std::vector<float> ts(n), ns(n * 3), tm((size_t)M * n), nm((size_t)M * n * 3), p12((size_t)M * 12), ot(n), on(n * 3);
        std::vector<uint8_t> ow(n);
        std::uniform_real_distribution<float> u(0.25f, 9.f), nn(-1.f, 1.f);
        for (size_t i = 0; i < n; ++i) ts[i] = (g() % 5 == 0) ? inf : u(g);
        for (float& v : tm) v = (g() % 3 == 0) ? inf : u(g);
        for (float& v : ns) v = nn(g);
        for (float& v : nm) v = nn(g);
        for (uint32_t m = 0; m < M; ++m) random_pose(g, &p12[(size_t)m * 12]);
        for (size_t i = 0; i < n; i += 7) tm[i] = ts[i];                                     // mover 0 ties with the static scene
        for (size_t i = 0; i < n; i += 11) tm[i] = tm[(size_t)(M - 1) * n + i] = 0.125f;       // the first and the last mover tie
        EXPECT(lrc_mover_merge(n, M, ts.data(), ns.data(), tm.data(), nm.data(), p12.data(), ot.data(), on.data(), ow.data()) == LRC_OK);
        for (size_t i = 0; i < n; ++i) {
            float t = ts[i], w[3] = {ns[i * 3], ns[i * 3 + 1], ns[i * 3 + 2]};
            uint8_t who = 0;
            for (uint32_t m = 0; m < M; ++m) {
                if (!(tm[(size_t)m * n + i] < t)) continue;
                t = tm[(size_t)m * n + i];
                const float* q = &nm[((size_t)m * n + i) * 3];
                const float* R = &p12[(size_t)m * 12];
                for (int j = 0; j < 3; ++j) w[j] = (R[4 * j] * q[0] + R[4 * j + 1] * q[1]) + R[4 * j + 2] * q[2];
                who = (uint8_t)(m + 1);
            }
            EXPECT(same_bits(&ot[i], &t, 1) && same_bits(&on[i * 3], w, 3) && ow[i] == who);
            if (i % 7 == 0 && i % 11 != 0) EXPECT(ow[i] != 1 || tm[i] != ts[i]);
            if (i % 11 == 0) EXPECT(ow[i] == 1 || ts[i] <= 0.125f);
        }
    }
    {
        float t = 1.f, n3[3] = {0, 0, 1}, p12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, ot, on[3];
        uint8_t ow;
        EXPECT(lrc_mover_merge(1, 256, &t, n3, &t, n3, p12, &ot, on, &ow) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_mover_merge(1, 1, nullptr, n3, &t, n3, p12, &ot, on, &ow) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_mover_merge(1, 1, &t, n3, &t, n3, nullptr, &ot, on, &ow) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_mover_merge(1, 0, &t, n3, nullptr, nullptr, nullptr, &ot, on, &ow) == LRC_OK && ow == 0 && ot == 1.f);
        EXPECT(lrc_mover_merge(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == LRC_OK);
    }

    // ---- lrc_mover_sweep_rays / lrc_mover_sweep_normals against the header's text: general, still and one-sided records ----
    for (int round = 0; round < 60; ++round) {
        const size_t n = 1 + (g() % 2000);
        std::vector<float> rays(n * 6), out(n * 6), want(n * 6), n3(n * 3), on(n * 3), wn(n * 3);
        std::vector<double> fire(n);
        std::uniform_real_distribution<float> u(-20.f, 20.f), un(-1.f, 1.f);
        std::uniform_real_distribution<double> uf(0.0, 1.0), ang(-0.78, 0.78), ax(-1.0, 1.0);
        for (float& v : rays) v = u(g);
        for (float& v : n3) v = un(g);
        for (size_t i = 0; i < n; ++i) fire[i] = i % 13 == 0 ? 0.0 : uf(g);
        float r[24] = {0};
        random_pose(g, r);
        r[12] = 1.f;
        if (round % 4 != 1) {                      // a rotation about a random axis (round % 4 == 1: translation only or still)
            const double a = ang(g), x = ax(g), y = ax(g), z = ax(g), l = std::sqrt(x * x + y * y + z * z) + 1e-9;
            r[12] = (float)std::cos(a); r[13] = (float)(std::sin(a) * x / l); r[14] = (float)(std::sin(a) * y / l); r[15] = (float)(std::sin(a) * z / l);
        }
        if (round % 4 != 2 && round % 8 != 1)      // round % 4 == 2: rotation only; round % 8 == 1: the still record
            for (int j = 16; j < 19; ++j) r[j] = u(g) * 0.05f;
        const bool still = r[12] == 1.f && !std::memcmp(&r[13], std::vector<float>(6, 0.f).data(), 24);
        EXPECT(still == (round % 8 == 1));
        EXPECT(lrc_mover_sweep_rays(rays.data(), fire.data(), n, r, out.data()) == LRC_OK);
        EXPECT(lrc_mover_sweep_normals(n3.data(), fire.data(), n, r, on.data()) == LRC_OK);
        for (size_t i = 0; i < n; ++i) {
            const float s = (float)fire[i];
            const float c[3] = {r[3] + s * r[16], r[7] + s * r[17], r[11] + s * r[18]};
            const float qw = (1.0f - s) + s * r[12], ux = s * r[13], uy = s * r[14], uz = s * r[15];
            const float k = 2.0f / (((qw * qw + ux * ux) + uy * uy) + uz * uz);
            auto rot = [&](const float* v, bool inverse, float* o) {
                const float tx = uy * v[2] - uz * v[1], ty = uz * v[0] - ux * v[2], tz = ux * v[1] - uy * v[0];
                const float wx = uy * tz - uz * ty, wy = uz * tx - ux * tz, wz = ux * ty - uy * tx;
                if (inverse) { o[0] = v[0] + k * (wx - qw * tx); o[1] = v[1] + k * (wy - qw * ty); o[2] = v[2] + k * (wz - qw * tz); }
                else { o[0] = v[0] + k * (qw * tx + wx); o[1] = v[1] + k * (qw * ty + wy); o[2] = v[2] + k * (qw * tz + wz); }
            };
            const float* ry = &rays[i * 6];
            float e[3] = {ry[0] - (still ? r[3] : c[0]), ry[1] - (still ? r[7] : c[1]), ry[2] - (still ? r[11] : c[2])}, d[3] = {ry[3], ry[4], ry[5]};
            if (!still) { float t3[3]; rot(e, true, t3); std::memcpy(e, t3, 12); rot(d, true, t3); std::memcpy(d, t3, 12); }
            for (int j = 0; j < 3; ++j) {
                want[i * 6 + j] = (r[j] * e[0] + r[4 + j] * e[1]) + r[8 + j] * e[2];
                want[i * 6 + 3 + j] = (r[j] * d[0] + r[4 + j] * d[1]) + r[8 + j] * d[2];
            }
            const float* q = &n3[i * 3];
            float w[3];
            for (int j = 0; j < 3; ++j) w[j] = (r[4 * j] * q[0] + r[4 * j + 1] * q[1]) + r[4 * j + 2] * q[2];
            if (!still) { float t3[3]; rot(w, false, t3); std::memcpy(w, t3, 12); }
            std::memcpy(&wn[i * 3], w, 12);
        }
        EXPECT(same_bits(out.data(), want.data(), n * 6));
        EXPECT(same_bits(on.data(), wn.data(), n * 3));
    }
    {
        float r[24] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1}, ray[6] = {1, 2, 3, 4, 5, 6}, o[6];
        double f = 0.5;
        EXPECT(lrc_mover_sweep_rays(ray, &f, 1, nullptr, o) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_mover_sweep_rays(ray, nullptr, 1, r, o) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_mover_sweep_rays(nullptr, &f, 1, r, o) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_mover_sweep_rays(nullptr, nullptr, 0, r, nullptr) == LRC_OK);
        EXPECT(lrc_mover_sweep_rays(ray, &f, 1, r, o) == LRC_OK && same_bits(ray, o, 6));
        EXPECT(lrc_mover_sweep_normals(ray, &f, 1, r, nullptr) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_mover_sweep_normals(ray, &f, 1, r, o) == LRC_OK && same_bits(ray, o, 3));
        lrc_hits hits{};
        lrc_frames fr{};
        EXPECT(lrc_scan_mover_sweeps_dev(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 1.0, &hits, nullptr, nullptr) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_scan_mover_sweeps_compact(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1.0, &fr, nullptr, 0, nullptr) == LRC_ERR_INVALID_ARG);
    }

    // ---- refusals that need no device ----
    {
        lrc_movers* set = nullptr;
        lrc_scene* none[1] = {nullptr};
        EXPECT(lrc_movers_create(nullptr, none, 0, &set) == LRC_ERR_INVALID_ARG && g_err.find("[1, 255]") != std::string::npos);
        EXPECT(lrc_movers_create(nullptr, none, 256, &set) == LRC_ERR_INVALID_ARG && g_err.find("[1, 255]") != std::string::npos);
        EXPECT(lrc_movers_create(nullptr, none, 1, &set) == LRC_ERR_INVALID_ARG && set == nullptr);
        EXPECT(lrc_movers_destroy(nullptr) == LRC_OK);
        lrc_hits hits{};
        lrc_frames fr{};
        EXPECT(lrc_scan_movers_dev(nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 1.0, &hits, nullptr, nullptr) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_scan_movers_compact(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1.0, &fr, nullptr, 0, nullptr) == LRC_ERR_INVALID_ARG);
    }

    // ---- the cull never leaves out a ray that meets the box (float64 slab test), at any distance and any direction scale ----
    {
        uint64_t met = 0, left_out = 0, total = 0;
        for (int round = 0; round < 400; ++round) {
            std::uniform_real_distribution<float> ext(0.05f, 2.f), pos(-3.f, 3.f);
            float lo[3], hi[3];
            for (int a = 0; a < 3; ++a) { lo[a] = pos(g); hi[a] = lo[a] + ext(g); }
            const lrcmov::Sphere s = lrcmov::bounding_sphere(lo, hi);
            const float reach = round % 4 == 0 ? 2000.f : round % 4 == 1 ? 60.f : 6.f;
            std::uniform_real_distribution<float> org(-reach, reach), tgt(-0.3f, 1.3f), scale(-6.f, 6.f);
            for (int k = 0; k < 2000; ++k) {
                lrcmov::Vec o{org(g), org(g), org(g)};
                // aimed at a point in or near the box, so that many rays meet it and many graze it
                const float p[3] = {lo[0] + tgt(g) * (hi[0] - lo[0]), lo[1] + tgt(g) * (hi[1] - lo[1]), lo[2] + tgt(g) * (hi[2] - lo[2])};
                const float sc = std::exp2(scale(g)) * (k % 5 == 0 ? -1.f : 1.f);       // some point away from it
                lrcmov::Vec d{(p[0] - o.x) * sc, (p[1] - o.y) * sc, (p[2] - o.z) * sc};
                double tn = 0.0, tf = std::numeric_limits<double>::infinity();
                const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
                bool miss = false;
                for (int a = 0; a < 3; ++a) {
                    if (dd[a] == 0.0) { miss |= oo[a] < lo[a] || oo[a] > hi[a]; continue; }
                    double t0 = (lo[a] - oo[a]) / dd[a], t1 = (hi[a] - oo[a]) / dd[a];
                    if (t0 > t1) std::swap(t0, t1);
                    tn = std::fmax(tn, t0);
                    tf = std::fmin(tf, t1);
                }
                const bool meets = !miss && tn <= tf;
                const bool out = lrcmov::culled(s, o, d);
                ++total;
                met += meets;
                left_out += out;
                EXPECT(!(meets && out));
            }
        }
        std::printf("cull: %llu rays, %llu meet the box, %llu left out\n", (unsigned long long)total, (unsigned long long)met,
                    (unsigned long long)left_out);
        EXPECT(met > total / 10 && left_out > total / 10);
        // what cannot be judged is cast
        const lrcmov::Sphere s = lrcmov::bounding_sphere(std::vector<float>{-1, -1, -1}.data(), std::vector<float>{1, 1, 1}.data());
        EXPECT(!lrcmov::culled(s, lrcmov::Vec{3e30f, 0, 0}, lrcmov::Vec{1, 0, 0}));
        EXPECT(!lrcmov::culled(s, lrcmov::Vec{std::nanf(""), 0, 0}, lrcmov::Vec{1, 0, 0}));
        EXPECT(!lrcmov::culled(s, lrcmov::Vec{5, 0, 0}, lrcmov::Vec{inf, 0, 0}));
        EXPECT(!lrcmov::culled(s, lrcmov::Vec{5, 0, 0}, lrcmov::Vec{0, 0, 0}));
        EXPECT(lrcmov::culled(s, lrcmov::Vec{5, 0, 0}, lrcmov::Vec{1, 0, 0}));          // points away
        EXPECT(lrcmov::culled(s, lrcmov::Vec{5, 5, 0}, lrcmov::Vec{-1, 0, 0}));         // passes beside
        EXPECT(!lrcmov::culled(s, lrcmov::Vec{5, 0, 0}, lrcmov::Vec{-1, 0, 0}));
    }

    std::printf(g_bad ? "movers_host_check: %d FAILED\n" : "movers_host_check: ok\n", g_bad);
    return g_bad ? 1 : 0;
}
