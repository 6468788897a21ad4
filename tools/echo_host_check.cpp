// echo_host_check.cpp -- stand-alone driver of the host side of the beam footprint (csrc/lrc_echo.hip, csrc/lrc_echo.h) for a
// sanitizer build: the beam validation of every entry point and lrc_echo_reduce on crafted and random rows, checked against a
// brute-force restatement.  Uses no GPU.  The units lrc_echo.hip calls into are stubbed below.  Build and run from csrc/:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined ../../tools/echo_host_check.cpp lrc_echo.hip -o echo_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "lrc_internal.h"

// ---- what lrc_echo.hip expects of the other units ----
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
int echo_scan_dev(lrc_scene*, const double*, uint64_t, const double*, uint64_t, const lrcecho::Params&, double, const lrc_hits*,
                  hipStream_t) { return LRC_ERR_INTERNAL; }
int echo_scan_compact(lrc_scene*, const double*, uint64_t, const lrc_table*, const double*, lrcecho::Params, double,
                      const lrc_frames*, uint8_t*, uint64_t, uint64_t*) { return LRC_ERR_INTERNAL; }

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_bad; } } while (0)

// the header's text, the slow way: sort, split, filter, cut
static void brute(const float* t, uint32_t K, uint32_t E, uint32_t mc, float sep, std::vector<int32_t>& rep, std::vector<uint8_t>& w) {
    std::vector<uint32_t> ks;
    for (uint32_t k = 0; k < K; ++k) if (t[k] < std::numeric_limits<float>::infinity()) ks.push_back(k);
    for (size_t a = 0; a < ks.size(); ++a)
        for (size_t b = a + 1; b < ks.size(); ++b)
            if (t[ks[b]] < t[ks[a]] || (t[ks[b]] == t[ks[a]] && ks[b] < ks[a])) std::swap(ks[a], ks[b]);
    std::vector<std::vector<uint32_t>> cl;
    for (size_t m = 0; m < ks.size(); ++m) {
        if (m == 0 || (float)(t[ks[m]] - t[ks[m - 1]]) > sep) cl.emplace_back();
        cl.back().push_back(ks[m]);
    }
    rep.assign(E, -1); w.assign(E, 0);
    uint32_t e = 0;
    for (auto& c : cl) {
        if (c.size() < mc || e >= E) continue;
        uint32_t first = c[0];
        for (uint32_t k : c) first = k < first ? k : first;
        rep[e] = (int32_t)first; w[e] = (uint8_t)c.size(); ++e;
    }
}

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    // validation
    const lrc_beam good{7, 2, 1, 0.05f};
    const lrc_beam bads[] = {{0, 2, 1, 0.05f}, {17, 2, 1, 0.05f}, {7, 0, 1, 0.05f}, {7, 5, 1, 0.05f}, {7, 2, 0, 0.05f}, {7, 2, 8, 0.05f},
                             {7, 2, 1, 0.0f}, {7, 2, 1, -1.0f}, {7, 2, 1, inf}, {7, 2, 1, std::nanf("")}};
    float t16[16] = {};
    int32_t rep4[4]; uint8_t w4[4];
    double off[32] = {};
    lrc_hits hits{}; lrc_frames frames{};
    for (const lrc_beam& b : bads) {
        EXPECT(lrc_echo_reduce(t16, 1, &b, rep4, w4) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_scan_echoes_dev(nullptr, nullptr, 0, nullptr, 0, nullptr, &b, 1.0, &hits, nullptr, nullptr) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_scan_echoes_compact(nullptr, nullptr, 0, nullptr, off, &b, 1.0, &frames, nullptr, 0, nullptr) == LRC_ERR_INVALID_ARG);
        EXPECT(g_err.find("scene") == std::string::npos);
    }
    EXPECT(lrc_echo_reduce(t16, 1, nullptr, rep4, w4) == LRC_ERR_INVALID_ARG);
    EXPECT(lrc_echo_reduce(nullptr, 1, &good, rep4, w4) == LRC_ERR_INVALID_ARG);
    EXPECT(lrc_echo_reduce(nullptr, 0, &good, nullptr, nullptr) == LRC_OK);
    off[13] = std::nan("");
    EXPECT(lrc_scan_echoes_compact(nullptr, nullptr, 0, nullptr, off, &good, 1.0, &frames, nullptr, 0, nullptr) == LRC_ERR_INVALID_ARG);
    EXPECT(g_err.find("non-finite offset") != std::string::npos);
    off[13] = 0.0;
    EXPECT(lrc_scan_echoes_compact(nullptr, nullptr, 0, nullptr, off, &good, 1.0, &frames, nullptr, 0, nullptr) == LRC_ERR_INVALID_ARG);
    EXPECT(g_err.find("NULL scene") != std::string::npos);
    uint32_t word = 0;
    hits.tile_count = &word;
    EXPECT(lrc_scan_echoes_dev(nullptr, nullptr, 0, nullptr, 0, nullptr, &good, 1.0, &hits, nullptr, nullptr) == LRC_ERR_INVALID_ARG);
    EXPECT(g_err.find("tile_count") != std::string::npos);
    // the reduction: exactly sized heap arrays, so that a stray access is the sanitizer's to find
    uint64_t state = 0x9E3779B97F4A7C15ull, beams = 0;
    auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    std::vector<int32_t> wr; std::vector<uint8_t> ww;
    for (uint32_t K = 1; K <= 16; ++K)
        for (uint32_t E = 1; E <= 4; ++E)
            for (uint32_t mc = 1; mc <= K; mc += (K > 4 ? 3 : 1)) {
                const uint64_t B = 200;
                std::vector<float> t(B * K);
                for (uint64_t b = 0; b < B; ++b) {
                    const float base[3] = {0.5f + (rnd() % 1000) * 0.003f, 0.5f + (rnd() % 1000) * 0.003f, 1.5f};
                    for (uint32_t k = 0; k < K; ++k) {
                        const uint64_t r = rnd();
                        float v = base[r % 3] + ((r >> 8) % 5) * 0.0125f * (float)((r >> 16) % 5);
                        if ((r >> 24) % 4 == 0) v = inf;
                        if (b < 3) v = inf;                                  // all misses
                        if (b == 3) v = 1.0f + 0.04f * (float)(K - 1 - k);   // a chain
                        t[b * K + k] = v;
                    }
                }
                std::vector<int32_t> rep(B * E); std::vector<uint8_t> w(B * E);
                const lrc_beam bm{K, E, mc, 0.05f};
                EXPECT(lrc_echo_reduce(t.data(), B, &bm, rep.data(), w.data()) == LRC_OK);
                for (uint64_t b = 0; b < B; ++b) {
                    brute(&t[b * K], K, E, mc, 0.05f, wr, ww);
                    for (uint32_t e = 0; e < E; ++e) { EXPECT(rep[b * E + e] == wr[e]); EXPECT(w[b * E + e] == ww[e]); }
                }
                beams += B;
            }
    std::printf("echo_host_check: %llu beams reduced, %d failures\n", (unsigned long long)beams, g_bad);
    return g_bad ? 1 : 0;
}
