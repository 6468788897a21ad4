// lrc_material.h -- surface materials of lrc_scan_materials_* (include/lidarcast.h "surface materials", DESIGN.md section
// 5j): what the trace kernel needs of a material table (kGenMaterials), and ONE segment's step of a ray's chain, written once
// for the host and the kernel.  The kernel's tail (chain_lanes below: trace_kernel<kGenMaterials>, lidarcast.hip) calls step()
// behind every traversal of a pending lane; lrc_material_step calls it on arrays, and the tests compare both with a numpy restatement of the header's text
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
#include "lrc_device.h"
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

#if defined(__HIPCC__)
// The chain of segments of one wave: the tail of trace_kernel<kGenMaterials>, behind the first traversal.  The lane holds its
// ray (o, d) and that ray's closest hit (tbest, best_slot, best_label; best_slot = 0xFFFFFFFF: none).
// Behind every traversal a pending lane looks at its closest hit: the surface returns, the chain is cut at the cap, or the
// ray goes on as a new segment.  While any lane of the wave goes on (ballot) those lanes traverse again -- traverse(): the
// closest hit of the lane's current (o, d) into (tbest, best_slot), over the float32 nodes with the clause tested per triangle
// as the redo route does: continued rays of a wave share no octant -- and the finished lanes idle.  Carried: T, g, b and the
// current (o, d); a finished lane keeps its final slot in best_slot.
// A finished lane needs its segment no longer: its origin's registers keep the surface point and d.x the intensity.
// need_geom (kernel arguments: uniform over the launch): some output reads I or pp.  Where none does, a lane on a diffuse
// surface -- which ends the chain whatever c is -- adds t to T and is done: no normal, no unit direction.
//   P          the kernel's parameter block: mat, out.intensity, slot_label
//   normal     (slot, nx, ny, nz): the unit normal of a triangle slot, as the record carries it
//   write      (touched, T, slot, label, I) -> kept: the fused write-back of the ORIGINAL ray at the total path length, which
//              the kernel forms again in (o, d) where `touched` says that a lane of the wave has overwritten it
// `ray` is the ray's index in the launch, the row of the two outputs that travel beside the record set.
template <class P, class Normal, class Traverse, class Write>
__device__ __forceinline__ void chain_lanes(const P& p, uint64_t ray, lrcdev::V3& o, lrcdev::V3& d, float& tbest,
                                            uint32_t& best_slot, uint32_t best_label, Normal normal, Traverse traverse,
                                            Write write) {
    using lrcdev::V3;
    const bool need_geom = p.out.intensity != nullptr || p.mat.surface3 != nullptr || p.mat.min_intensity > 0.0f;
    float T = 0.0f, g = 1.0f;
    uint32_t b = 0u;
    bool pend = true;
    bool touched = false;      // this lane's (o, d) no longer hold the original ray
    while (true) {
        bool cont = false;
        if (pend && best_slot == 0xFFFFFFFFu) pend = false;      // a miss: no return
        if (pend) {
            const Record m = record_of(p.mat.table, p.mat.num_classes, best_label & 0xFFFFu);
            if (m.kind == kDiffuse && !need_geom) {
                T = path_add(T, tbest);
                pend = false;
            } else {
                float nx, ny, nz, I = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
                touched = true;
                normal(best_slot, nx, ny, nz);
                Seg sg{o.x, o.y, o.z, d.x, d.y, d.z, T, g, b};
                const int r = step(sg, tbest, nx, ny, nz, m, p.mat.max_bounces, I, sx, sy, sz);
                T = sg.T; g = sg.g; b = sg.b;
                if (r == kContinue) {
                    o = V3{sg.ox, sg.oy, sg.oz}; d = V3{sg.dx, sg.dy, sg.dz};
                    tbest = __builtin_inff(); best_slot = 0xFFFFFFFFu;
                    cont = lrcdev::finite_ray(o, d);      // a segment that is not finite is a miss, as for every cast
                } else {
                    pend = false;
                    o = V3{sx, sy, sz}; d.x = I;
                    if (r == kNoReturn) best_slot = 0xFFFFFFFFu;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(cont) == 0ull) break;
        if (cont) traverse();
        // every lane loads its label again, as behind the redo route: it is not held through the traversal
        best_label = best_slot != 0xFFFFFFFFu ? p.slot_label[best_slot] : 0u;
    }
    const float I = d.x, sx = o.x, sy = o.y, sz = o.z;      // of a lane with a return; anything else is not kept
    if (need_geom && best_slot != 0xFFFFFFFFu && I < p.mat.min_intensity) best_slot = 0xFFFFFFFFu;
    const bool kept = write(touched, T, best_slot, best_label, I);
    if (p.mat.bounces) p.mat.bounces[ray] = kept ? (uint8_t)b : (uint8_t)0;
    if (p.mat.surface3) {
        float* q = p.mat.surface3 + ray * 3;
        q[0] = kept ? sx : 0.0f; q[1] = kept ? sy : 0.0f; q[2] = kept ? sz : 0.0f;
    }
}
#endif

}  // namespace lrcmat
