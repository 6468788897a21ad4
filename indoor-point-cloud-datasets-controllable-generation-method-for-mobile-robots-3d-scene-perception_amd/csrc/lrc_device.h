// lrc_device.h -- device-side arithmetic of the ray-cast scan (gfx950 only).
//
// This header fixes the float32 expression trees that define a "hit" (DESIGN.md section 3).
// oracle/lrc_oracle.c restates the same trees in plain C for the CPU; tests compare bit for bit.
// The file is compiled with -ffp-contract=off: every fused multiply-add below is explicit.
//
// Reference semantics being reproduced:
//   * closest hit, two-sided, tnear = 0 exclusive, tfar = +inf, parametric t along the given
//     direction: the contract of open3d RaycastingScene.cast_rays, called at
//     raycast_engine/raycast_engine_cpu.py:51 (Embree's Moeller-Trumbore intersector restated).
//   * p = o + (d/|d|)*t in float32, separate mul and add:   raycast_engine_cpu.py:55-62
//   * range filter and incident angle in float64:            raycast_engine_cpu.py:95-107
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lrc_noise.h"

namespace lrcdev {

#define LRC_DI __device__ __forceinline__
#define LRC_HDI __host__ __device__ __forceinline__     // also compiled for the host: the test hooks call these very functions

constexpr float kTinyDir = 1e-30f;
constexpr float kPadRelLo = 0.999755859375f;     // 1 - 2^-12
constexpr float kPadRelHi = 1.000244140625f;     // 1 + 2^-12
constexpr float kPadAbs   = 1.52587890625e-05f;  // 2^-16
constexpr double kRadToDeg = 57.29577951308232;  // 180/pi, numpy's npy_rad2deg factor

struct V3 { float x, y, z; };

LRC_DI float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
LRC_DI float dot3(V3 a, V3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
LRC_DI V3 cross3(V3 a, V3 b) {
    V3 r;
    r.x = fma_(a.y, b.z, -(a.z * b.y));
    r.y = fma_(a.z, b.x, -(a.x * b.z));
    r.z = fma_(a.x, b.y, -(a.y * b.x));
    return r;
}
LRC_DI V3 sub3(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
LRC_DI float xorsign(float x, uint32_t s) { return __uint_as_float(__float_as_uint(x) ^ s); }
LRC_DI float min2(float a, float b) { return a < b ? a : b; }
LRC_DI float max2(float a, float b) { return a > b ? a : b; }

// Per-ray constants of the slab test.
struct RaySlab { float ix, iy, iz, ox, oy, oz; };   // idir and o*idir

LRC_HDI float safe_inv(float d) {
    float a = __builtin_fabsf(d);
    float s = a < kTinyDir ? __builtin_copysignf(kTinyDir, d) : d;
    return 1.0f / s;
}
LRC_DI RaySlab make_slab(V3 o, V3 d) {
    RaySlab r;
    r.ix = safe_inv(d.x); r.iy = safe_inv(d.y); r.iz = safe_inv(d.z);
    r.ox = o.x * r.ix; r.oy = o.y * r.iy; r.oz = o.z * r.iz;
    return r;
}

// which of lo / hi a ray enters a box through, per axis: bit a set = negative 1/d (safe_inv keeps the sign of d, of a
// zero component too)
LRC_DI uint32_t sign_octant(V3 d) {
    return (__float_as_uint(d.x) >> 31) | ((__float_as_uint(d.y) >> 31) << 1) | ((__float_as_uint(d.z) >> 31) << 2);
}

// Padded entry/exit parameters of the ray against the box [lo,hi].
// Monotone in lo/hi, hence the interval of a box contains the interval of every box inside it.
LRC_DI void slab_interval(const RaySlab& s, float lox, float loy, float loz, float hix, float hiy,
                          float hiz, float& tn, float& tf) {
    float t0x = fma_(lox, s.ix, -s.ox), t1x = fma_(hix, s.ix, -s.ox);
    float t0y = fma_(loy, s.iy, -s.oy), t1y = fma_(hiy, s.iy, -s.oy);
    float t0z = fma_(loz, s.iz, -s.oz), t1z = fma_(hiz, s.iz, -s.oz);
    float nx = min2(t0x, t1x), fx = max2(t0x, t1x);
    float ny = min2(t0y, t1y), fy = max2(t0y, t1y);
    float nz = min2(t0z, t1z), fz = max2(t0z, t1z);
    float n = max2(max2(nx, ny), max2(nz, 0.0f));
    float f = min2(min2(fx, fy), fz);
    tn = fma_(n, kPadRelLo, -kPadAbs);
    tf = fma_(f, kPadRelHi, kPadAbs);
}

// Entry / exit plane of one axis for two boxes, picked on the scalar unit: (n, f) = (hi, lo) if bit B of oct is set
// (negative direction component), else (lo, hi).  Every operand is wave-uniform and lives in SGPRs.  Inline assembly
// because the compiler keeps a loop-invariant condition as a lane mask and selects with v_mov + v_cndmask pairs.
template <int B>
LRC_DI void pick_planes_s(uint32_t oct, float lo0, float hi0, float lo1, float hi1, float& n0, float& f0, float& n1,
                          float& f1) {
    asm("s_bitcmp1_b32 %4, %9\n\t"
        "s_cselect_b32 %0, %6, %5\n\t"
        "s_cselect_b32 %1, %5, %6\n\t"
        "s_cselect_b32 %2, %8, %7\n\t"
        "s_cselect_b32 %3, %7, %8"
        : "=&s"(n0), "=&s"(f0), "=&s"(n1), "=&s"(f1)
        : "s"(oct), "s"(lo0), "s"(hi0), "s"(lo1), "s"(hi1), "n"(B)
        : "scc");
}

// slab_interval of the two children of a wave-uniform node, for the rays of a wave that all point into direction
// octant `oct` (sign_octant of d, wave-uniform): the plane the rays enter / leave through on each axis is picked by the
// sign of d (pick_planes_s) instead of ordered by a min / max.  safe_inv keeps the sign of d, of a zero component too,
// so s.ix has d's sign; for s.ix > 0 and lo <= hi, fma(lo, ix, -ox) <= fma(hi, ix, -ox) by monotone rounding (the
// reverse for ix < 0), and the picked value IS slab_interval's min / max.  Where the two can differ, they differ in
// the sign of a zero only, which the pad FMAs remove: tn and tf are slab_interval's, bit for bit, on every box with
// lo <= hi.  The inverted box of the empty leaf (lo > hi; only a one-leaf mesh has it) is never hit here, as on the per-lane
// v_perm path; it holds no triangle, so no result depends on it.
// c0 / c1: lo x, y, z, hi x, y, z of each child.
LRC_DI void slab_interval2_oct(const RaySlab& s, uint32_t oct, const float* c0, const float* c1, float& tn0, float& tf0,
                               float& tn1, float& tf1) {
    float n0[3], f0[3], n1[3], f1[3];
    pick_planes_s<0>(oct, c0[0], c0[3], c1[0], c1[3], n0[0], f0[0], n1[0], f1[0]);
    pick_planes_s<1>(oct, c0[1], c0[4], c1[1], c1[4], n0[1], f0[1], n1[1], f1[1]);
    pick_planes_s<2>(oct, c0[2], c0[5], c1[2], c1[5], n0[2], f0[2], n1[2], f1[2]);
    auto one = [&](const float* n, const float* f, float& tn, float& tf) {
        const float nx = fma_(n[0], s.ix, -s.ox), fx = fma_(f[0], s.ix, -s.ox);
        const float ny = fma_(n[1], s.iy, -s.oy), fy = fma_(f[1], s.iy, -s.oy);
        const float nz = fma_(n[2], s.iz, -s.oz), fz = fma_(f[2], s.iz, -s.oz);
        const float nn = max2(max2(nx, ny), max2(nz, 0.0f));
        const float ff = min2(min2(fx, fy), fz);
        tn = fma_(nn, kPadRelLo, -kPadAbs);
        tf = fma_(ff, kPadRelHi, kPadAbs);
    };
    one(n0, f0, tn0, tf0);
    one(n1, f1, tn1, tf1);
}

// Ray/triangle test on an edge record (v0, e1 = v0 - v1, e2 = v2 - v0, Ng = cross(e2, e1)); the hit definition of
// DESIGN.md section 3 is tri_mt && box_clause:
//   den = Ng.D != 0,  U = (C x D).e2,  V = (C x D).e1 (sign-corrected), U,V >= 0, U+V <= |den|,
//   T = Ng.C (sign-corrected) > 0,  t = T/|den| finite  [tri_mt: the Moeller-Trumbore conditions, Embree's form]
//   and t inside the padded slab interval of the triangle's own vertex box  [box_clause: the one clause Embree lacks]
// The traversal ranks candidates by tri_mt alone and tests the clause ONCE, on the closest candidate, after the
// traversal: if it passes, that candidate is the definition's closest hit (every triangle passing both tests is a
// candidate too, and pruning by a candidate's t never hides a closer one); if it fails -- never observed -- the ray is
// redone with the clause tested per triangle.  The edges are stored, not formed per test: six subtractions and seven
// registers less in the hot loop; the vertex box the clause needs sits in a side table (slot_box).
LRC_DI bool tri_mt(V3 o, V3 d, V3 v0, V3 e1, V3 e2, V3 ng, float& t_out) {
    V3 c = sub3(v0, o);
    V3 r = cross3(c, d);
    float den = dot3(ng, d);
    float aden = __builtin_fabsf(den);
    uint32_t sgn = __float_as_uint(den) & 0x80000000u;
    float u = xorsign(dot3(r, e2), sgn);
    float v = xorsign(dot3(r, e1), sgn);
    float tt = xorsign(dot3(ng, c), sgn);
    bool ok = (den != 0.0f) & (u >= 0.0f) & (v >= 0.0f) & (u + v <= aden) & (tt > 0.0f);
    if (!ok) return false;
    float t = tt / aden;
    if (!(t < __builtin_inff())) return false;
    t_out = t;
    return true;
}
LRC_DI bool box_clause(const RaySlab& s, float lox, float loy, float loz, float hix, float hiy, float hiz, float t) {
    float tn, tf;
    slab_interval(s, lox, loy, loz, hix, hiy, hiz, tn, tf);
    return (tn <= t) & (t <= tf);
}
// both at once, for callers that test few (ray, triangle) pairs (laboratory kernels): bx = the slot's box, 6 floats
LRC_DI bool tri_hit(V3 o, V3 d, const RaySlab& s, V3 v0, V3 e1, V3 e2, V3 ng, const float* bx, float& t_out) {
    float t;
    if (!tri_mt(o, d, v0, e1, e2, ng, t)) return false;
    if (!box_clause(s, bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], t)) return false;
    t_out = t;
    return true;
}

// A ray takes part in the cast only if its six components are finite (bit test: immune to -fno-honor-nans).  Anything
// else is reported as a miss without touching the tree, so no comparison ever sees a NaN (include/lidarcast.h,
// "finite-ray contract"; the oracle applies the same rule).
LRC_DI bool finite_ray(V3 o, V3 d) {
    const uint32_t m = 0x7F800000u;
    return ((__float_as_uint(o.x) & m) != m) & ((__float_as_uint(o.y) & m) != m) & ((__float_as_uint(o.z) & m) != m) &
           ((__float_as_uint(d.x) & m) != m) & ((__float_as_uint(d.y) & m) != m) & ((__float_as_uint(d.z) & m) != m);
}

// One output of np.dot(directions, R.T): the BLAS kernel accumulates over k from a +0.0 accumulator with fused
// multiply-adds.  The accumulator matters for signed zeros only: (-0.0)*r or 0.0*(-r) alone would be -0.0, dgemm gives
// +0.0 -- and the sign of a zero direction component decides which side of a box plane an in-plane ray is on.
LRC_HDI double dgemm_row(double a, double b, double c, double r0, double r1, double r2) {
    return __builtin_fma(c, r2, __builtin_fma(b, r1, __builtin_fma(a, r0, 0.0)));
}

// Ray (pose, i) of a pose-batched scan: origin = float32(pose[:3,3]); direction = float32(dirs3[i] @ R^T).
// The reference forms the product with np.dot(directions, pose[:3,:3].T) in float64 (lidar/indoor_lidar.py:127-131),
// i.e. BLAS dgemm, whose kernels accumulate over k with fused multiply-adds: out_j = fma(c, R[j][2],
// fma(b, R[j][1], fma(a, R[j][0], +0))).  Reproduced here term for term (dgemm_row), so the float64 product -- and hence the float32
// direction -- is bit-identical for rotated poses too (checked against vectors captured from the reference at
// yaw 0.7, tests/golden/).  c = pose[:3,3] in float64.
LRC_DI void gen_ray(const double* poses16, const double* dirs3, uint64_t pose, uint64_t i, V3& o, V3& d,
                    double& cx, double& cy, double& cz) {
    const double* M = poses16 + pose * 16;
    const double* dv = dirs3 + i * 3;
    const double a = dv[0], b = dv[1], c = dv[2];
    d.x = (float)dgemm_row(a, b, c, M[0], M[1], M[2]);
    d.y = (float)dgemm_row(a, b, c, M[4], M[5], M[6]);
    d.z = (float)dgemm_row(a, b, c, M[8], M[9], M[10]);
    cx = M[3]; cy = M[7]; cz = M[11];
    o.x = (float)cx; o.y = (float)cy; o.z = (float)cz;
}

// Ray (pose, i) of the dual-axis sensor from its noisy scan angles (phi, theta), float64, drawn on the host from the
// seeded stream (lidar/indoor_lidar.py:270-272): d = (cos(theta)cos(phi), cos(theta)sin(phi), sin(theta)), rotated as
// the reference rotates it, ray by ray with numpy's un-fused (d0*R[:,0] + d1*R[:,1]) + d2*R[:,2] (:283-287), then
// narrowed to float32.  Opt-in path: the device's double sin/cos are not guaranteed to round like the host's libm.
LRC_DI void gen_ray_angles(const double* poses16, uint64_t pose, double phi, double theta, V3& o, V3& d,
                           double& cx, double& cy, double& cz) {
    const double* M = poses16 + pose * 16;
    const double ct = cos(theta);
    const double d0 = ct * cos(phi), d1 = ct * sin(phi), d2 = sin(theta);
    d.x = (float)((d0 * M[0] + d1 * M[1]) + d2 * M[2]);
    d.y = (float)((d0 * M[4] + d1 * M[5]) + d2 * M[6]);
    d.z = (float)((d0 * M[8] + d1 * M[9]) + d2 * M[10]);
    cx = M[3]; cy = M[7]; cz = M[11];
    o.x = (float)cx; o.y = (float)cy; o.z = (float)cz;
}

// ---- moving-sensor sweeps (lrc_scan_sweeps_*; include/lidarcast.h "moving-sensor sweeps") ----
// Motion record of sweep k, 24 float64: M[0..11] the start pose's first three rows (as poses16), M[12..15] dq = (w, x, y, z)
// with R_end = R(dq) R_start and w >= cos(pi/4), M[16..18] dc = c_end - c_start, the rest zero.  s = fire[i] in [0, 1).
// Every operation is a separate IEEE float64 operation in exactly this order (the file is built with -ffp-contract=off;
// tests/test_sweep_host.py restates it op for op in numpy):
//   centre   cs_j = s * dc_j;  c_j = (cs_j == 0) ? c0_j : c0_j + cs_j        (the select keeps a -0.0 start centre bit for bit)
//   rotation qw = (1 - s) + s * dq.w;  u = (s * dq.x, s * dq.y, s * dq.z)     (nlerp, never normalised)
//            n = ((qw*qw + ux*ux) + uy*uy) + uz*uz;  k = 2 / n
//            t = u x v:  tx = uy*vz - uz*vy,  ty = uz*vx - ux*vz,  tz = ux*vy - uy*vx
//            w = u x t:  wx = uy*tz - uz*ty,  wy = uz*tx - ux*tz,  wz = ux*ty - uy*tx
//            v'_j = v_j + k * (qw * t_j + w_j)
// v is gen_ray's float64 world direction (dgemm_row): s = 0 adds only signed zeros to it (dgemm_row never yields -0.0), so the
// static ray comes out bit for bit.
LRC_HDI void sweep_centre(const double* M, double s, double& cx, double& cy, double& cz) {
    const double sx = s * M[16], sy = s * M[17], sz = s * M[18];
    cx = sx == 0.0 ? M[3] : M[3] + sx;
    cy = sy == 0.0 ? M[7] : M[7] + sy;
    cz = sz == 0.0 ? M[11] : M[11] + sz;
}

// Ray (k, i) of a moving-sensor sweep: direction = float32(rotate(v, q(s))), origin = float32(c(s)).
LRC_DI void gen_ray_sweep(const double* motion24, const double* dirs3, const double* fire, uint64_t k, uint64_t i, V3& o,
                          V3& d) {
    const double* M = motion24 + k * 24;
    const double* dv = dirs3 + i * 3;
    const double a = dv[0], b = dv[1], c = dv[2];
    const double vx = dgemm_row(a, b, c, M[0], M[1], M[2]);
    const double vy = dgemm_row(a, b, c, M[4], M[5], M[6]);
    const double vz = dgemm_row(a, b, c, M[8], M[9], M[10]);
    const double s = fire[i];
    const double qw = (1.0 - s) + s * M[12];
    const double ux = s * M[13], uy = s * M[14], uz = s * M[15];
    const double n = ((qw * qw + ux * ux) + uy * uy) + uz * uz;
    const double kk = 2.0 / n;
    const double tx = uy * vz - uz * vy, ty = uz * vx - ux * vz, tz = ux * vy - uy * vx;
    const double wx = uy * tz - uz * ty, wy = uz * tx - ux * tz, wz = ux * ty - uy * tx;
    d.x = (float)(vx + kk * (qw * tx + wx));
    d.y = (float)(vy + kk * (qw * ty + wy));
    d.z = (float)(vz + kk * (qw * tz + wz));
    double cx, cy, cz;
    sweep_centre(M, s, cx, cy, cz);
    o.x = (float)cx; o.y = (float)cy; o.z = (float)cz;
}

// ---- seeded sensor noise (lrc_scan_noisy_*; include/lidarcast.h "seeded sensor noise") ----------
// Ray (pose, i) of a noisy scan: gen_ray with the table row jittered in the sensor frame BEFORE the dgemm chain
// (lrc_noise.h jitter_row; dp = angle_std * z(w1), dt = angle_std * z(w2), the float32 variates widened), and
// live = false for a ray the dropout word drops (w3 < drop_thr): never cast, reported as a miss.  The words are the Philox
// block of (seed, first_frame + pose, i).  Zero parameters skip their step (kernel arguments: wave-uniform), so a row passes
// through bit for bit when angle_std == 0.
LRC_DI void gen_ray_noisy(const double* poses16, const double* dirs3, const lrcnoise::Params& np, uint64_t pose, uint64_t i,
                          V3& o, V3& d, double& cx, double& cy, double& cz, bool& live) {
    const double* M = poses16 + pose * 16;
    const double* dv = dirs3 + i * 3;
    double a = dv[0], b = dv[1], c = dv[2];
    if (np.angle_std != 0.0 || np.drop_thr != 0u) {
        const lrcnoise::Words w = lrcnoise::ray_words(np.seed, np.first_frame + pose, (uint32_t)i);
        if (np.drop_thr != 0u) live = w.w3 >= np.drop_thr;
        if (np.angle_std != 0.0) {
            const double dp = np.angle_std * (double)lrcnoise::normal_of(w.w1, np.tab);
            const double dt = np.angle_std * (double)lrcnoise::normal_of(w.w2, np.tab);
            lrcnoise::jitter_row(a, b, c, dp, dt);
        }
    }
    d.x = (float)dgemm_row(a, b, c, M[0], M[1], M[2]);
    d.y = (float)dgemm_row(a, b, c, M[4], M[5], M[6]);
    d.z = (float)dgemm_row(a, b, c, M[8], M[9], M[10]);
    cx = M[3]; cy = M[7]; cz = M[11];
    o.x = (float)cx; o.y = (float)cy; o.z = (float)cz;
}
// The range draw of ray (frame, i): t' = t + range_std * z(w0), a float32 multiply then an add.
LRC_DI float noisy_range(const lrcnoise::Params& np, uint64_t frame, uint32_t i, float t) {
    const lrcnoise::Words w = lrcnoise::ray_words(np.seed, frame, i);
    return t + np.range_std * lrcnoise::normal_of(w.w0, np.tab);
}

// ---- noisy moving-sensor sweeps (lrc_scan_noisy_sweeps_*; include/lidarcast.h "noisy moving-sensor sweeps") ----
// Ray (k, i) of a noisy sweep: the two generators above, one behind the other.  The jitter acts on the float64 table row in FRONT
// of the dgemm chain, the sweep on the float64 world direction BEHIND it; every step a separate float64 operation in this order:
//   words     w = ray_words(seed, first_frame + k, i), formed only if angle_std != 0 or drop_thr != 0; drop_thr != 0 and
//             w3 < drop_thr: live = false (never cast, reported as a miss)                                    [gen_ray_noisy]
//   jitter    angle_std != 0: jitter_row(a, b, c, angle_std * z(w1), angle_std * z(w2)); an h == 0 row passes through  [gen_ray_noisy]
//   static    v = dgemm_row(row, R_start) from motion24[k]
//   sweep     s = fire[i]: v' = rotate(v, q(s)), origin = float32(c(s)) with the -0.0-keeping select            [gen_ray_sweep]
// The range draw (noisy_range) and the filter centre (sweep_centre) are formed again behind the traversal.  Zero parameters skip
// their step (kernel arguments: wave-uniform): the all-zero model is gen_ray_sweep bit for bit; s = 0, or a record whose end is
// its start, adds signed zeros only to gen_ray_noisy's direction.  Also compiled for the host: lrc_noisy_sweep_rays is this text.
LRC_HDI void gen_ray_noisy_sweep(const double* motion24, const double* dirs3, const double* fire, const lrcnoise::Params& np,
                                 uint64_t k, uint64_t i, V3& o, V3& d, bool& live) {
    const double* M = motion24 + k * 24;
    const double* dv = dirs3 + i * 3;
    double a = dv[0], b = dv[1], c = dv[2];
    if (np.angle_std != 0.0 || np.drop_thr != 0u) {
        const lrcnoise::Words w = lrcnoise::ray_words(np.seed, np.first_frame + k, (uint32_t)i);
        if (np.drop_thr != 0u) live = w.w3 >= np.drop_thr;
        if (np.angle_std != 0.0) {
            const double dp = np.angle_std * (double)lrcnoise::normal_of(w.w1, np.tab);
            const double dt = np.angle_std * (double)lrcnoise::normal_of(w.w2, np.tab);
            lrcnoise::jitter_row(a, b, c, dp, dt);
        }
    }
    const double vx = dgemm_row(a, b, c, M[0], M[1], M[2]);
    const double vy = dgemm_row(a, b, c, M[4], M[5], M[6]);
    const double vz = dgemm_row(a, b, c, M[8], M[9], M[10]);
    const double s = fire[i];
    const double qw = (1.0 - s) + s * M[12];
    const double ux = s * M[13], uy = s * M[14], uz = s * M[15];
    const double n = ((qw * qw + ux * ux) + uy * uy) + uz * uz;
    const double kk = 2.0 / n;
    const double tx = uy * vz - uz * vy, ty = uz * vx - ux * vz, tz = ux * vy - uy * vx;
    const double wx = uy * tz - uz * ty, wy = uz * tx - ux * tz, wz = ux * ty - uy * tx;
    d.x = (float)(vx + kk * (qw * tx + wx));
    d.y = (float)(vy + kk * (qw * ty + wy));
    d.z = (float)(vz + kk * (qw * tz + wz));
    double cx, cy, cz;
    sweep_centre(M, s, cx, cy, cz);
    o.x = (float)cx; o.y = (float)cy; o.z = (float)cz;
}

// ---- beam footprint (lrc_scan_echoes_*; include/lidarcast.h "beam footprint and multi-echo returns") ----
// Sub-ray k of beam (pose, i): gen_ray with the table row moved by the offset (du, dv) = offsets2[k] in the sensor frame BEFORE
// the dgemm chain.  One float64 operation per step: h = sqrt(a*a + b*b), dp = du / h (du is an arc: the footprint stays round
// at high elevation), dt = dv, then lrc_noise.h jitter_row(a, b, c, dp, dt).  A zero offset passes the row through bit for bit
// (the sub-ray is gen_ray's ray), and so does a row with h == 0 for every offset.
LRC_DI void gen_ray_beam(const double* poses16, const double* dirs3, const double* offsets2, uint64_t pose, uint64_t i,
                         uint32_t k, V3& o, V3& d, double& cx, double& cy, double& cz) {
    const double* M = poses16 + pose * 16;
    const double* dv = dirs3 + i * 3;
    double a = dv[0], b = dv[1], c = dv[2];
    const double du = offsets2[2 * k], dt = offsets2[2 * k + 1];
    if (du != 0.0 || dt != 0.0) {
        const double h = __builtin_sqrt(a * a + b * b);
        if (h != 0.0) {
            const double dp = du / h;
            lrcnoise::jitter_row(a, b, c, dp, dt);
        }
    }
    d.x = (float)dgemm_row(a, b, c, M[0], M[1], M[2]);
    d.y = (float)dgemm_row(a, b, c, M[4], M[5], M[6]);
    d.z = (float)dgemm_row(a, b, c, M[8], M[9], M[10]);
    cx = M[3]; cy = M[7]; cz = M[11];
    o.x = (float)cx; o.y = (float)cy; o.z = (float)cz;
}

// d/|d| : numpy float32, one rounding per operation (reference: raycast_engine_cpu.py:57-60).  The one expression behind
// hit_point and the ray table of a prepared pipeline submit (ray_row below).
LRC_HDI V3 unit_dir(V3 d) {
    const float nrm = __builtin_sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
    return V3{d.x / nrm, d.y / nrm, d.z / nrm};
}
// p = o + (d/|d|)*t : numpy float32, one rounding per operation (reference: raycast_engine_cpu.py:57-62).
// h receives the normalised direction.
LRC_DI void hit_point(V3 o, V3 d, float t, V3& h, V3& pt) {
    h = unit_dir(d);
    pt.x = o.x + h.x * t; pt.y = o.y + h.y * t; pt.z = o.z + h.z * t;
}

// ---- ray table of a prepared pipeline submit -------------------------------------------------------
// What a ray of a pose-batched scan owes to the table row and the pose's ROTATION alone, formed once per row for the rotation
// block R (row major, 9 float64) by the functions the trace kernel itself calls per ray: d = float32(row . R^T) (gen_ray's
// dgemm_row chain), inv = safe_inv(d) (the slab constants before the scene's scaling) and h = d / |d| (hit_point's unit
// direction).  A pose whose rotation block has the same 72 bytes gets the same d, inv and h, bit for bit.
struct RayRow { V3 d, inv, h; };
LRC_HDI RayRow ray_row(const double* R, double a, double b, double c) {
    RayRow r;
    r.d.x = (float)dgemm_row(a, b, c, R[0], R[1], R[2]);
    r.d.y = (float)dgemm_row(a, b, c, R[3], R[4], R[5]);
    r.d.z = (float)dgemm_row(a, b, c, R[6], R[7], R[8]);
    r.inv = V3{safe_inv(r.d.x), safe_inv(r.d.y), safe_inv(r.d.z)};
    r.h = unit_dir(r.d);
    return r;
}
// The packed output row (x, y, z, label bits) of a ray of a prepared submit from what its 12-byte record and the submit's table
// hold: p = o + h * t, numpy float32, one rounding per operation (multiply, then add: the file is built with -ffp-contract=off),
// o the pose record's float32 origin and h the table row's unit vector.  The write-back of the trace (for its range filter) and
// every consumer of a record set (the scatters, the expansion for lrc_pipe_records) form the point here, so they cannot drift.
struct PairRow { float x, y, z; uint32_t label; };
LRC_HDI PairRow pair_row(V3 o, V3 h, float t, uint32_t label) {
    return PairRow{o.x + h.x * t, o.y + h.y * t, o.z + h.z * t, label};
}

// ---- two-line tiles of the scan pipeline ----------------------------------------------------------
// A pose of tpp tiles of 64 rays, its rays in scan lines of W = 64 * wt consecutive table rows.  Tile u of the pose does not
// take 64 consecutive rays of one line (11.25 degrees x 0 for the benchmark sensor) but 32 consecutive columns of two adjacent
// lines (5.6 x 1.1 degrees): the wave's rays stay together for more of the descent.  With g = u / (2 wt) the line pair and
// c0 = (u % (2 wt)) * 32 the first column, lanes 0-31 take ray (2g) W + c0 + lane and lanes 32-63 ray (2g + 1) W + c0 + lane - 32.
// The 2 wt tiles of pair g cover its 2 W rays exactly once (2 wt column blocks of 32, two lines each); tiles past the last
// whole pair (an odd last line, or rays behind the last whole line when W does not divide the pose) keep the 1-D mapping, which
// covers exactly their own 64 rays.  So the mapping is a bijection of the pose's rays for ANY wt: a width that is not the
// table's costs coherence, never a byte.  wt = 0: 1-D tiles.  Each half of a wave is half of a 1-D tile: rays
// 64 t + 32 h ... + 31 of 1-D tile t, whose keep mask it fills as one 32-bit word.
//
// Line-group tiles generalise this to 64 / L columns of L adjacent lines, L in {1, 2, 4}.  `grp` packs the grouping: bit 31
// set = groups of four lines where there are four, bits 0-30 = split, the first line whose elevation sign differs from line
// 0's (0, or anything not below the number of whole lines: no split).  Lines [0, split) and [split, H) are grouped each from
// its own start, so that no group holds lines of both signs (a wave of both points into two direction octants and walks
// the float32 nodes): groups of 4 (bit 31), then one group of 2 if 2 or 3 lines remain (without bit 31: groups of 2 all the
// way), then 1-D tiles for an odd last line.  A group of L lines starting at line a owns tiles [a wt, (a + L) wt) and rays
// [a W, (a + L) W); its tile r takes columns [r 64 / L, (r + 1) 64 / L) of each of its lines, lanes [j 64 / L, (j + 1) 64 / L)
// line a + j: every ray of the group once.  Groups, odd lines and the tiles behind the last whole line partition the pose's
// tiles and, range for range, its rays: a bijection for ANY (wt, tpp, grp).  grp = 0 is the two-line mapping above.  Each
// quarter of a wave is a quarter of a 1-D tile: rays 64 t + 16 q ... + 15, 16 bits of tile t's keep mask.
// One division (the tile's line); whether a group is whole is decided by products against the run's last tile -- the
// mapping runs twice per wave, in front of and behind the traversal, and a scalar division costs some twenty instructions.
LRC_HDI uint32_t tile_ray(uint32_t u, uint32_t lane, uint32_t wt, uint32_t tpp, uint32_t grp = 0u) {
    if (wt == 0u) return u * 64u + lane;
    const uint32_t line = u / wt, c = u - line * wt;          // this tile's line as a 1-D tile, its place in the line
    const uint32_t s = grp & 0x7FFFFFFFu;
    const uint64_t sw = (uint64_t)s * wt;
    // the run of lines of one sign this tile lies in: first line l0, tiles end at `lim` (s beyond the whole lines: one run)
    const uint32_t l0 = line < s ? 0u : s;
    const uint32_t lim = (line < s && sw < tpp) ? (uint32_t)sw : tpp;
    const uint32_t k = line - l0;
    const uint32_t b4 = (grp >> 31) != 0u ? (k & ~3u) : 0u;   // first line (in the run) of the would-be group of four, ...
    if ((grp >> 31) != 0u && (l0 + b4 + 4u) * wt <= lim)
        return ((l0 + b4 + (lane >> 4)) * wt) * 64u + ((k & 3u) * wt + c) * 16u + (lane & 15u);
    const uint32_t b2 = b4 + ((k - b4) & ~1u);                // ... of the would-be pair behind the run's groups of four
    if ((l0 + b2 + 2u) * wt <= lim)
        return ((l0 + b2 + (lane >> 5)) * wt) * 64u + (((k - b4) & 1u) * wt + c) * 32u + (lane & 31u);
    return u * 64u + lane;
}
// the grouping word for `lines` (4: groups of four; anything else: of two) lines per tile and a split line
LRC_HDI uint32_t line_group_for(uint32_t split, uint32_t lines) {
    return (split > 0x7FFFFFFFu ? 0u : split) | (lines == 4u ? 0x80000000u : 0u);
}
// lines per tile the mapping above yields at its widest for (wt, tpp, grp): 4, 2, or 1 (no group at all)
LRC_HDI uint32_t tile_lines_of(uint32_t wt, uint32_t tpp, uint32_t grp) {
    if (wt == 0u) return 1u;
    const uint32_t hf = tpp / wt;
    uint32_t s = grp & 0x7FFFFFFFu;
    if (s >= hf) s = 0u;
    const uint32_t a = s, b = hf - s, m = a > b ? a : b;
    return ((grp >> 31) != 0u && m >= 4u) ? 4u : (m >= 2u ? 2u : 1u);
}
// the line width (in tiles) a pipeline uses for a table of N rays whose lines are W rays long: whole tiles per line, whole
// lines per pose, at least one pair -- else 1-D tiles (0)
LRC_HDI uint32_t line_tiles_for(uint64_t W, uint64_t N) {
    if (W == 0 || W % 64u != 0 || N % W != 0 || N / W < 2u || N > 0xFFFFFFFFull) return 0u;
    return (uint32_t)(W / 64u);
}

// ---- range filter without the float64 square root ----------------------------------------------------------------------
// The reference keeps a return when dist < R with dist = sqrt(s), s = (ex*ex + ey*ey) + ez*ez, all float64 (raycast_engine_cpu.py:
// 95-107).  The square root is only there to be compared, and it is correctly rounded and monotone, so away from R*R the
// comparison can be made on s itself.  With u = 2^-53 (a float64 rounding is off by at most a factor 1 +- u):
//   lo = fl(fl(R*R) * (1 - 2^-48)) <= R^2 (1 + u)^2 (1 - 2^-48) < R^2 (1 - 2^-52)^2.  For s < lo the exact root is below
//        R (1 - 2^-52) <= pred(R) (neighbouring float64 are at most 2^-52 relative apart), and rounding is monotone:
//        fl(sqrt(s)) <= pred(R) < R -- kept, as the reference keeps it.
//   hi = fl(fl(R*R) * (1 + 2^-48)) >= R^2 (1 - u)^2 (1 + 2^-48) > R^2.  For s > hi the exact root is above R, so
//        fl(sqrt(s)) >= R -- dropped, as the reference drops it.
// s in [lo, hi] (about 2^-47 relative: a few tens of ulp either side of R*R) is decided by the square root itself, as before.
// The bounds are formed in the kernel from the launch's max_range (four wave-uniform operations: the trace kernel's argument
// block has no room for two more doubles without the register allocation changing, and the host test hook calls the same
// function); fast = 0 (R not positive and finite, or R*R outside the normal range with room to spare) sends every ray to the
// square root.  A NaN s is in no class that keeps it, with or without the root.
struct RangeBand { double lo, hi; int fast; };
LRC_HDI RangeBand range_band(double R) {
    RangeBand b{0.0, 0.0, 0};
    if (!(R >= 0x1p-500) || !(R <= 0x1p500)) return b;
    const double r2 = R * R;
    b.lo = r2 * (1.0 - 0x1p-48);
    b.hi = r2 * (1.0 + 0x1p-48);
    b.fast = 1;
    return b;
}
LRC_HDI bool range_in_band(double s, double lo, double hi) { return (s >= lo) & (s <= hi); }   // the square root decides
LRC_HDI bool range_below(double s, double lo) { return s < lo; }                               // outside the band: kept iff below

}  // namespace lrcdev
