// flow_host_check.cpp -- stand-alone driver of the host side of the scene flow under movers (csrc/lrc_flow.hip, csrc/lrc_flow.h)
// for a sanitizer build: lrc_flow_rays and lrc_flow_status on random and crafted columns in exactly sized heap arrays, checked
// against a plain restatement of the header's text, and the refusals that need no device.  Uses no GPU.  The units lrc_flow.hip and
// lrc_movers.hip call into are stubbed below.  Build and run from csrc/:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I. -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined ../../tools/flow_host_check.cpp lrc_flow.hip lrc_movers.hip -o flow_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "lrc_internal.h"

// ---- what lrc_flow.hip and lrc_movers.hip expect of the other units ----
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
int movers_scan_dev(lrc_scene*, lrc_movers*, const MoverScan&, const lrc_hits*, uint8_t*, hipStream_t) { return LRC_ERR_INTERNAL; }
int movers_scan_compact(lrc_scene*, lrc_movers*, const double*, uint64_t, const lrc_table*, const float*, double, bool, const lrcnoise::Params*,
                        const lrc_frames*, uint8_t*, uint64_t, uint64_t*, const FlowCompact*) { return LRC_ERR_INTERNAL; }
int noise_params(lrc_ctx*, const char*, const lrc_noise*, uint64_t, lrcnoise::Params*) { return LRC_ERR_INTERNAL; }
int noise_params_host(const char*, const lrc_noise*, uint64_t, lrcnoise::Params*) { return LRC_ERR_INTERNAL; }
int check_motion(const char*, const double*, uint64_t) { return LRC_OK; }
int flow_scan_dev(lrc_scene*, lrc_movers*, const lrc_hits*, const uint8_t*, uint64_t, uint64_t, const float*, const FlowNext&, double,
                  float*, uint8_t*, hipStream_t, const FlowPairs*) { return LRC_ERR_INTERNAL; }
DeformMesh deform_mesh(const lrc_deform*) { return DeformMesh{}; }
int flow_scan_compact(lrc_scene*, lrc_movers*, const double*, uint64_t, const lrc_table*, const float*, const FlowNext&, double,
                      const lrc_frames*, uint8_t*, float*, uint8_t*, uint64_t, uint64_t*) { return LRC_ERR_INTERNAL; }

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_bad; } } while (0)

static bool same_bits(const float* a, const float* b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

static void random_pose(std::mt19937& g, float* m) {
    std::uniform_real_distribution<double> u(-3.14, 3.14), c(-6.0, 6.0);
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

// the header's steps 1 to 3 and 6 for one row, written out plainly
struct Row { float flow[3], ray[6], thr; uint8_t keep, status; };
static Row restate(bool live, uint32_t w, uint32_t M, const float* x, const float* A, const float* B, const double* next16,
                   double max_range, double min_range) {
    Row r{};
    if (!live) return r;
    double y[3] = {x[0], x[1], x[2]};
    if (w != 0 && w <= M && std::memcmp(A, B, 48) != 0) {
        const double e[3] = {(double)x[0] - A[3], (double)x[1] - A[7], (double)x[2] - A[11]};
        double q[3];
        for (int j = 0; j < 3; ++j) q[j] = ((double)A[j] * e[0] + (double)A[4 + j] * e[1]) + (double)A[8 + j] * e[2];
        for (int j = 0; j < 3; ++j) y[j] = (((double)B[4 * j] * q[0] + (double)B[4 * j + 1] * q[1]) + (double)B[4 * j + 2] * q[2]) + (double)B[4 * j + 3];
        for (int j = 0; j < 3; ++j) r.flow[j] = (float)(y[j] - (double)x[j]);
    }
    const float y32[3] = {(float)y[0], (float)y[1], (float)y[2]};
    const double c[3] = {next16[3], next16[7], next16[11]};
    const float o[3] = {(float)c[0], (float)c[1], (float)c[2]};
    const float d[3] = {y32[0] - o[0], y32[1] - o[1], y32[2] - o[2]};
    const float L = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const double e[3] = {(double)y32[0] - c[0], (double)y32[1] - c[1], (double)y32[2] - c[2]};
    const double dist = std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    const bool in = dist < max_range && !(min_range > 0.0 && !(dist >= min_range));
    r.status = in ? 1 : 3;
    if (!in) return r;
    r.keep = 1;
    for (int j = 0; j < 3; ++j) { r.ray[j] = o[j]; r.ray[3 + j] = d[j] / L; }
    r.thr = L - 0x1p-12f * (L > 1.0f ? L : 1.0f);
    return r;
}

int main() {
    std::mt19937 g(20261020u);
    const float inf = std::numeric_limits<float>::infinity();

    // ---- lrc_flow_rays against the header's text: random columns, every M the id column can name ----
    for (int round = 0; round < 40; ++round) {
        const uint64_t P = 1 + (g() % 4), N = 1 + (g() % 500), n = P * N;
        const uint32_t M = round == 0 ? 255u : round == 1 ? 0u : 1 + (g() % 6);
        std::vector<float> t(n), x(n * 3), A((size_t)P * M * 12), B((size_t)P * M * 12), flow(n * 3), rays(n * 6), thr(n);
        std::vector<uint8_t> w(n), has(P), keep(n), st(n);
        std::vector<double> next(P * 16, 0.0);
        std::uniform_real_distribution<float> u(-6.f, 6.f);
        std::uniform_real_distribution<double> jit(-1e-4, 1e-4);
        for (uint64_t i = 0; i < n; ++i) {
            t[i] = (g() % 6 == 0) ? inf : 1.0f;
            for (int j = 0; j < 3; ++j) x[i * 3 + j] = u(g);
            w[i] = (uint8_t)(g() % 3 == 0 ? 0 : g() % (M + 2));          // also ids one above M
        }
        for (uint64_t k = 0; k < P * M; ++k) { random_pose(g, &A[k * 12]); random_pose(g, &B[k * 12]); }
        for (uint64_t k = 0; k < P * M; k += 3) std::memcpy(&B[k * 12], &A[k * 12], 48);      // movers that stand still
        for (uint64_t p = 0; p < P; ++p) {
            float m[12];
            random_pose(g, m);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) next[p * 16 + 4 * i + j] = (double)m[4 * i + j] + (j == 3 ? jit(g) : 0.0);
            next[p * 16 + 15] = 1.0;
            has[p] = (uint8_t)(g() % 4 != 0);
        }
        const double min_range = round % 2 ? 2.0 : 0.0;
        const uint8_t* hn = round % 5 == 4 ? nullptr : has.data();
        EXPECT(lrc_flow_rays(t.data(), x.data(), M ? w.data() : nullptr, P, N, M, M ? A.data() : nullptr, M ? B.data() : nullptr,
                             next.data(), hn, 7.0, min_range, flow.data(), rays.data(), keep.data(), thr.data(), st.data()) == LRC_OK);
        for (uint64_t p = 0; p < P; ++p)
            for (uint64_t i = 0; i < N; ++i) {
                const uint64_t k = p * N + i;
                const bool live = t[k] < inf && (!hn || hn[p]);
                const uint32_t id = M ? w[k] : 0;
                const size_t row = id && id <= M ? (p * M + id - 1) * 12 : 0;
                const Row r = restate(live, id, M, &x[k * 3], M ? &A[row] : nullptr, M ? &B[row] : nullptr, &next[p * 16], 7.0, min_range);
                EXPECT(same_bits(&flow[k * 3], r.flow, 3) && same_bits(&rays[k * 6], r.ray, 6) && same_bits(&thr[k], &r.thr, 1));
                EXPECT(keep[k] == r.keep && st[k] == r.status);
            }
    }

    // ---- lrc_flow_status: ranges exactly at thr, one ulp below, misses everywhere ----
    for (int round = 0; round < 30; ++round) {
        const size_t n = 1 + (g() % 900);
        const uint32_t M = round == 0 ? 255u : g() % 5;
        std::vector<float> ts(n), tm((size_t)M * n), thr(n);
        std::vector<uint8_t> st(n), out(n);
        std::uniform_real_distribution<float> u(0.25f, 9.f);
        for (size_t i = 0; i < n; ++i) {
            thr[i] = u(g);
            ts[i] = g() % 3 == 0 ? inf : u(g);
            st[i] = (uint8_t)(g() % 4 == 0 ? (g() % 2 ? 0 : 3) : 1);
            if (i % 5 == 0) ts[i] = thr[i];
        }
        for (float& v : tm) v = g() % 2 ? inf : u(g);
        for (size_t i = 1; M && i < n; i += 5) { ts[i] = inf; for (uint32_t m = 0; m < M; ++m) tm[m * n + i] = inf; tm[(size_t)(M - 1) * n + i] = std::nextafter(thr[i], 0.f); }
        EXPECT(lrc_flow_status(n, M, ts.data(), M ? tm.data() : nullptr, thr.data(), st.data(), out.data()) == LRC_OK);
        for (size_t i = 0; i < n; ++i) {
            float t = ts[i];
            for (uint32_t m = 0; m < M; ++m) if (tm[m * n + i] < t) t = tm[m * n + i];
            EXPECT(out[i] == (st[i] == 1 ? (t < thr[i] ? 2 : 1) : st[i]));
        }
    }

    // ---- refusals that need no device ----
    {
        float t = 1.f, x[3] = {1, 2, 3}, p12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, f[3], r[6], thr;
        double next[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        uint8_t w = 1, keep, st;
        EXPECT(lrc_flow_rays(&t, x, &w, 1, 1, 1, p12, p12, next, nullptr, 9.0, 0.0, f, r, &keep, &thr, &st) == LRC_OK && st == 1 && keep == 1);
        EXPECT(f[0] == 0.f && f[1] == 0.f && f[2] == 0.f && !std::signbit(f[0]));
        EXPECT(lrc_flow_rays(&t, x, &w, 1, 1, 256, p12, p12, next, nullptr, 9.0, 0.0, f, r, &keep, &thr, &st) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_flow_rays(&t, x, nullptr, 1, 1, 1, p12, p12, next, nullptr, 9.0, 0.0, f, r, &keep, &thr, &st) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_flow_rays(&t, x, &w, 1, 1, 1, p12, p12, nullptr, nullptr, 9.0, 0.0, f, r, &keep, &thr, &st) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_flow_rays(&t, x, &w, 1, 1, 1, p12, p12, next, nullptr, 9.0, 0.0, nullptr, r, &keep, &thr, &st) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_flow_rays(nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, 9.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr) == LRC_OK);
        EXPECT(lrc_flow_status(1, 256, &t, &t, &thr, &st, &keep) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_flow_status(1, 1, &t, nullptr, &thr, &st, &keep) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_flow_status(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == LRC_OK);
        lrc_hits hits{};
        lrc_frames fr{};
        EXPECT(lrc_scan_flow_dev(nullptr, nullptr, &hits, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 1.0, nullptr, nullptr, nullptr) == LRC_ERR_INVALID_ARG);
        EXPECT(g_err.find("NULL scene") != std::string::npos);
        EXPECT(lrc_scan_flow_compact(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0, &fr, nullptr, nullptr, nullptr, 0, nullptr) == LRC_ERR_INVALID_ARG);
    }

    std::printf(g_bad ? "flow_host_check: %d FAILED\n" : "flow_host_check: ok\n", g_bad);
    return g_bad ? 1 : 0;
}
