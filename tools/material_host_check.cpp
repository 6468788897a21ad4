// material_host_check.cpp -- stand-alone driver of the host side of the surface materials (csrc/lrc_material.hip,
// csrc/lrc_material.h) for a sanitizer build: the validation of a model and its records at every entry point and
// lrc_material_step on crafted and random segments, checked against a plain restatement of the header's text.  Uses no GPU.
// The units lrc_material.hip calls into are stubbed below.  Build and run from csrc/:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I. -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined ../../tools/material_host_check.cpp lrc_material.hip -o material_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "lrc_internal.h"

// ---- what lrc_material.hip expects of the other units ----
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
int material_scan_dev(lrc_scene*, const double*, uint64_t, const double*, uint64_t, const lrcmat::Params&, double, const lrc_hits*,
                      hipStream_t) { return LRC_ERR_INTERNAL; }
int material_scan_compact(lrc_scene*, const double*, uint64_t, const lrc_table*, lrcmat::Params, double, const lrc_frames*, float*,
                          uint8_t*, float*, uint64_t, uint64_t*) { return LRC_ERR_INTERNAL; }

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_bad; } } while (0)

struct Ray { float o[3], d[3], T, g; uint8_t b, st; float I, s[3]; };

// the header's text, one ray, written without the shared inline functions
static void restate(const lrc_material_model& m, const lrc_material* rec, float t, uint16_t sem, const float* n, Ray& r) {
    if (r.st != 0) return;
    if (!(t < std::numeric_limits<float>::infinity())) { r.st = 2; return; }
    const float nrm = std::sqrt((r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2]);
    const float h[3] = {r.d[0] / nrm, r.d[1] / nrm, r.d[2] / nrm};
    const float pp[3] = {r.o[0] + h[0] * t, r.o[1] + h[1] * t, r.o[2] + h[2] * t};
    const float c = std::fabs(std::fma(h[2], n[2], std::fma(h[1], n[1], h[0] * n[0])));
    r.T = r.T + t;
    lrc_material k{0, 1.0f, 0.0f, 0.0f};
    if (sem < m.num_classes) k = rec[sem];
    if (k.kind == 0 || c >= k.retro_cos) {
        const float I = (r.g * k.albedo) * c;
        if (I < m.min_intensity) { r.st = 2; return; }
        r.st = 1; r.I = I;
        std::memcpy(r.s, pp, sizeof pp);
        return;
    }
    if (r.b == m.max_bounces) { r.st = 2; return; }
    r.b += 1;
    r.g = r.g * k.pass;
    if (k.kind == 2) {
        const float dn = (h[0] * n[0] + h[1] * n[1]) + h[2] * n[2];
        const float s = dn + dn;
        for (int a = 0; a < 3; ++a) r.d[a] = h[a] - s * n[a];
    }
    const float nrm2 = std::sqrt((r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2]);
    for (int a = 0; a < 3; ++a) r.o[a] = pp[a] + (r.d[a] / nrm2) * 0x1p-10f;
    r.T = r.T + 0x1p-10f;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::nanf("");
    // ---- validation: exactly sized heap arrays, so that a stray access is the sanitizer's to find ----
    std::vector<lrc_material> good = {{0, 1.0f, 0.0f, 0.0f}, {1, 0.1f, 0.9f, 0.999f}, {2, 0.05f, 0.95f, 2.0f}};
    const lrc_material_model ok{3, 4, 0.0f, 0};
    const uint64_t n1 = 1;
    std::vector<float> t(n1, 1.0f), nm = {1.0f, 0.0f, 0.0f}, o(3, 0.0f), d = {1.0f, 0.0f, 0.0f}, T(n1, 0.0f), g(n1, 1.0f), I(n1), s(3);
    std::vector<uint16_t> sem(n1, 0);
    std::vector<uint8_t> b(n1, 0), st(n1, 0);
    auto step = [&](const lrc_material_model* m, const lrc_material* rec) {
        st[0] = 0;
        return lrc_material_step(m, rec, n1, t.data(), sem.data(), nm.data(), o.data(), d.data(), T.data(), g.data(), b.data(), st.data(),
                                 I.data(), s.data());
    };
    lrc_material_table* handle = nullptr;
    const lrc_material_model bad_models[] = {{0, 4, 0.0f, 0}, {257, 4, 0.0f, 0}, {3, 9, 0.0f, 0}, {3, 4, -0.1f, 0}, {3, 4, 1.5f, 0},
                                             {3, 4, nan, 0}, {3, 4, inf, 0}};
    for (const lrc_material_model& m : bad_models) {
        std::vector<lrc_material> rec(m.num_classes && m.num_classes <= 256 ? m.num_classes : 1, good[0]);
        EXPECT(step(&m, rec.data()) == LRC_ERR_INVALID_ARG);
        EXPECT(lrc_material_table_create(nullptr, &m, rec.data(), &handle) == LRC_ERR_INVALID_ARG && handle == nullptr);
        EXPECT(g_err.find("context") == std::string::npos);
    }
    const lrc_material bad_records[] = {{3, 1.0f, 0.0f, 0.0f}, {0, 1.5f, 0.0f, 0.0f}, {0, -0.1f, 0.0f, 0.0f}, {0, nan, 0.0f, 0.0f},
                                        {1, 1.0f, 2.0f, 0.0f}, {1, 1.0f, inf, 0.0f}, {1, 1.0f, 0.5f, -0.1f}, {1, 1.0f, 0.5f, nan},
                                        {1, 1.0f, 0.5f, inf}};
    for (const lrc_material& r : bad_records) {
        std::vector<lrc_material> rec = good;
        rec[2] = r;
        EXPECT(step(&ok, rec.data()) == LRC_ERR_INVALID_ARG);
        EXPECT(g_err.find("class 2") != std::string::npos);
        EXPECT(lrc_material_table_create(nullptr, &ok, rec.data(), &handle) == LRC_ERR_INVALID_ARG);
    }
    EXPECT(step(nullptr, good.data()) == LRC_ERR_INVALID_ARG);
    EXPECT(step(&ok, nullptr) == LRC_ERR_INVALID_ARG);
    EXPECT(step(&ok, good.data()) == LRC_OK);
    EXPECT(lrc_material_step(&ok, good.data(), 1, nullptr, sem.data(), nm.data(), o.data(), d.data(), T.data(), g.data(), b.data(),
                             st.data(), I.data(), s.data()) == LRC_ERR_INVALID_ARG);
    EXPECT(lrc_material_step(&ok, good.data(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr) == LRC_OK);
    EXPECT(lrc_material_table_create(nullptr, &ok, good.data(), &handle) == LRC_ERR_INVALID_ARG);
    EXPECT(g_err.find("NULL context") != std::string::npos);
    EXPECT(lrc_material_table_destroy(nullptr) == LRC_OK);
    lrc_hits hits{}; lrc_frames frames{};
    EXPECT(lrc_scan_materials_dev(nullptr, nullptr, 0, nullptr, 0, nullptr, 1.0, &hits, nullptr, nullptr, nullptr) == LRC_ERR_INVALID_ARG);
    EXPECT(g_err.find("materials is NULL") != std::string::npos);
    EXPECT(lrc_scan_materials_compact(nullptr, nullptr, 0, nullptr, nullptr, 1.0, &frames, nullptr, nullptr, nullptr, 0, nullptr) ==
           LRC_ERR_INVALID_ARG);
    EXPECT(g_err.find("materials is NULL") != std::string::npos);

    // ---- the step: random chains of segments against the restatement, every model limit ----
    uint64_t state = 0x9E3779B97F4A7C15ull, steps = 0;
    auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    auto uni = [&]() { return (float)((rnd() >> 40) * (1.0 / 16777216.0)); };      // [0, 1)
    for (uint32_t classes : {1u, 3u, 12u, 256u})
        for (uint32_t mb = 0; mb <= 8; mb += 2)
            for (float mi : {0.0f, 0.3f, 1.0f}) {
                const lrc_material_model m{classes, mb, mi, 0};
                std::vector<lrc_material> rec(classes);
                for (uint32_t k = 0; k < classes; ++k)
                    rec[k] = lrc_material{(uint32_t)(rnd() % 3), uni(), uni(), (rnd() % 4 == 0) ? 2.0f : 0.5f + 0.5f * uni()};
                const uint64_t n = 257;
                std::vector<Ray> want(n);
                std::vector<float> vt(n), vn(3 * n), vo(3 * n), vd(3 * n), vT(n), vg(n), vI(n), vs(3 * n);
                std::vector<uint16_t> vsem(n);
                std::vector<uint8_t> vb(n), vst(n);
                for (uint64_t i = 0; i < n; ++i) {
                    Ray& r = want[i];
                    for (int a = 0; a < 3; ++a) { r.o[a] = 4.0f * uni(); r.d[a] = 2.0f * uni() - 1.0f; }
                    r.d[0] += 0.25f;
                    r.T = 0.0f; r.g = 1.0f; r.b = 0; r.st = (i % 17 == 16) ? 1 : 0; r.I = 0.0f; r.s[0] = r.s[1] = r.s[2] = 0.0f;
                    std::memcpy(&vo[3 * i], r.o, 12); std::memcpy(&vd[3 * i], r.d, 12);
                    vT[i] = r.T; vg[i] = r.g; vb[i] = r.b; vst[i] = r.st; vI[i] = 0.0f; vs[3 * i] = vs[3 * i + 1] = vs[3 * i + 2] = 0.0f;
                }
                for (int seg = 0; seg < 11; ++seg) {
                    for (uint64_t i = 0; i < n; ++i) {
                        vt[i] = (rnd() % 9 == 0) ? inf : 0.05f + 3.0f * uni();
                        vsem[i] = (uint16_t)(rnd() % (classes + 2));
                        float nn[3] = {2.0f * uni() - 1.0f, 2.0f * uni() - 1.0f, 2.0f * uni() - 0.75f};
                        const float len = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
                        for (int a = 0; a < 3; ++a) vn[3 * i + a] = nn[a] / len;
                        restate(m, rec.data(), vt[i], vsem[i], &vn[3 * i], want[i]);
                    }
                    EXPECT(lrc_material_step(&m, rec.data(), n, vt.data(), vsem.data(), vn.data(), vo.data(), vd.data(), vT.data(), vg.data(),
                                             vb.data(), vst.data(), vI.data(), vs.data()) == LRC_OK);
                    for (uint64_t i = 0; i < n; ++i) {
                        const Ray& r = want[i];
                        EXPECT(vst[i] == r.st);
                        if (r.st == 2) continue;          // a ray without a return: its state is not specified further
                        EXPECT(vb[i] == r.b);
                        EXPECT(std::memcmp(&vT[i], &r.T, 4) == 0 && std::memcmp(&vg[i], &r.g, 4) == 0);
                        if (r.st == 1) EXPECT(std::memcmp(&vI[i], &r.I, 4) == 0 && std::memcmp(&vs[3 * i], r.s, 12) == 0);
                        if (r.st == 0) EXPECT(std::memcmp(&vo[3 * i], r.o, 12) == 0 && std::memcmp(&vd[3 * i], r.d, 12) == 0);
                    }
                    steps += n;
                }
                for (uint64_t i = 0; i < n; ++i) EXPECT(vst[i] != 0);      // b <= 8: eleven segments end every chain
            }
    std::printf("material_host_check: %llu segment steps, %d failures\n", (unsigned long long)steps, g_bad);
    return g_bad ? 1 : 0;
}
