// lrc_material.h -- surface materials of lrc_scan_materials_* (include/lidarcast.h "surface materials", DESIGN.md section
// 5j): what the trace kernel needs of a material table (GEN = 7), and ONE segment's step of a ray's chain, written once for
// the host and the kernel.  The kernel calls step() behind every traversal of a pending lane (lidarcast.hip, trace_kernel
// GEN = 7); lrc_material_step calls it on arrays, and the tests compare both with a numpy restatement of the header's text
// over the explicit-ray cast.
//
//   state     (o, d) the segment, T the path length so far (+0), g the gain (1), b the bounces (0)
//   geometry  h = d / |d|, pp = o + h * t, c = |fma(hz, nz, fma(hy, ny, hx * nx))|, T = T + t
//   own       kind == 0 or c >= retro_cos: returns with I = (g * albedo) * c
//   go on     b == max_bounces: no return; else b += 1, g = g * pass, glass d' = d, mirror d' = h - (dn + dn) * n with
//             dn = (hx * nx + hy * ny) + hz * nz; h' = d' / |d'|, o' = pp + h' * skin, T = T + skin
// float32, one rounding per operation (the build is -ffp-contract=off) except the fused c.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LRC_MHD __host__ __device__ __forceinline__
#else
#define LRC_MHD inline
#endif

namespace lrcmat {

constexpr uint32_t kMaxClasses = 256, kMaxBounces = 8;
constexpr uint32_t kDiffuse = 0, kGlass = 1, kMirror = 2;
constexpr float kSkin = 0x1p-10f;      // metres: a continued segment starts this far along its own direction
constexpr int kContinue = 0, kReturn = 1, kNoReturn = 2;

// one class's record: the 16 bytes of an lrc_material
struct Record { uint32_t kind; float albedo, pass, retro_cos; };

// what the trace kernel needs of an lrc_material_table (40 bytes)
struct Params {
    const Record* table;         // device: num_classes records
    uint8_t* bounces;            // device, nullable: b per ray, 0 without a return
    float* surface3;             // device, nullable: the last pp per ray, 0 without a return
    float min_intensity;
    uint32_t num_classes;
    uint32_t max_bounces;
};

struct Seg { float ox, oy, oz, dx, dy, dz, T, g; uint32_t b; };

// T = T + t alone: all that a segment ending on a diffuse surface changes when no output reads I or pp (the kernel's lanes on
// diffuse surfaces in a scan that writes neither intensity nor surface points and has no min_intensity)
LRC_MHD float path_add(float T, float t) { return T + t; }

// One segment whose closest hit lies at t on a surface with unit normal (nx, ny, nz) and record m.  kReturn: I and (px, py,
// pz) are the return's; kNoReturn: the cap; kContinue: s holds the next segment.  (px, py, pz) is pp in every case.
LRC_MHD int step(Seg& s, float t, float nx, float ny, float nz, const Record m, uint32_t max_bounces, float& I, float& px,
                 float& py, float& pz) {
    const float nrm = __builtin_sqrtf((s.dx * s.dx + s.dy * s.dy) + s.dz * s.dz);
    const float hx = s.dx / nrm, hy = s.dy / nrm, hz = s.dz / nrm;
    px = s.ox + hx * t; py = s.oy + hy * t; pz = s.oz + hz * t;
    const float c = __builtin_fabsf(__builtin_fmaf(hz, nz, __builtin_fmaf(hy, ny, hx * nx)));
    s.T = path_add(s.T, t);
    if (m.kind == kDiffuse || c >= m.retro_cos) {
        I = (s.g * m.albedo) * c;
        return kReturn;
    }
    if (s.b == max_bounces) return kNoReturn;
    s.b += 1u;
    s.g = s.g * m.pass;
    if (m.kind == kMirror) {
        const float dn = (hx * nx + hy * ny) + hz * nz;
        const float sd = dn + dn;
        s.dx = hx - sd * nx; s.dy = hy - sd * ny; s.dz = hz - sd * nz;
    }
    const float nrm2 = __builtin_sqrtf((s.dx * s.dx + s.dy * s.dy) + s.dz * s.dz);
    s.ox = px + (s.dx / nrm2) * kSkin; s.oy = py + (s.dy / nrm2) * kSkin; s.oz = pz + (s.dz / nrm2) * kSkin;
    s.T = s.T + kSkin;
    return kContinue;
}

// the record of semantic id `sem`: an id at or above num_classes is diffuse with albedo 1
LRC_MHD Record record_of(const Record* table, uint32_t num_classes, uint32_t sem) {
    if (sem < num_classes) return table[sem];
    return Record{kDiffuse, 1.0f, 0.0f, 0.0f};
}

}  // namespace lrcmat
