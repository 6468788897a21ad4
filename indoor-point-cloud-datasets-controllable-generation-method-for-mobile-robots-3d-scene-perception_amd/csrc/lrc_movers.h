// lrc_movers.h -- rigid movers of lrc_scan_movers_* (include/lidarcast.h "moving objects"): the three
// pieces of arithmetic the mover kernels of lidarcast.hip and the host functions lrc_mover_rays / lrc_mover_merge share,
// written once for both.  Below them: the per-ray mover pose of lrc_scan_mover_sweeps_* (DESIGN.md section 5n).
//
//   pose12    the row-major 3 x 4 [R | c] from object to world: R[i][j] = m[4 i + j], c_i = m[4 i + 3]
//   to_object e = o - c; o'_j = (R[0][j] * e_x + R[1][j] * e_y) + R[2][j] * e_z; d'_j the same expression on d
//   takes     a mover's range replaces the running winner's only when it is SMALLER as float32: the static scene, which
//             starts the chain, wins an exact tie over every mover, and the smaller m wins among movers
//   to_world  n_j = (R[j][0] * n_x + R[j][1] * n_y) + R[j][2] * n_z, not renormalised
//   culled    a ray that cannot meet the mover's bounding sphere (see below): weaker than the traversal's root-box test
// float32, one rounding per operation (the build is -ffp-contract=off), nothing fused.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LRC_VHD __host__ __device__ __forceinline__
#else
#define LRC_VHD inline
#endif

namespace lrcmov {

constexpr uint32_t kMaxMovers = 255;
constexpr double kOrthoTol = 0x1p-16;      // max |R^T R - I| a host-checked pose may have (float64)

struct Vec { float x, y, z; };

// R^T v, the rotation part of world -> object
LRC_VHD Vec rot_to_object(const float* m, Vec v) {
    return Vec{(m[0] * v.x + m[4] * v.y) + m[8] * v.z,
               (m[1] * v.x + m[5] * v.y) + m[9] * v.z,
               (m[2] * v.x + m[6] * v.y) + m[10] * v.z};
}

// step 2 of the header: the world ray (o, d) in the mover's frame
LRC_VHD void to_object(const float* m, Vec o, Vec d, Vec& oo, Vec& od) {
    const Vec e{o.x - m[3], o.y - m[7], o.z - m[11]};
    oo = rot_to_object(m, e);
    od = rot_to_object(m, d);
}

// R n: the mover record's normal in the world
LRC_VHD Vec to_world(const float* m, Vec n) {
    return Vec{(m[0] * n.x + m[1] * n.y) + m[2] * n.z,
               (m[4] * n.x + m[5] * n.y) + m[6] * n.z,
               (m[8] * n.x + m[9] * n.y) + m[10] * n.z};
}

// step 3: does a mover's range replace the running winner's?  (a miss is +inf on both sides and never does)
LRC_VHD bool takes(float t_mover, float t_winner) { return t_mover < t_winner; }

// The bounding sphere of a mover's box [lo, hi] in its own frame, enlarged: radius = half diagonal * (1 + 2^-6) + 2^-10.
// The margin is six orders of magnitude above the rounding of the test below and of the triangle test, so a ray the test
// leaves out lies clear of the box by a distance no float32 hit can bridge.
struct Sphere { float cx, cy, cz, r2; };

inline Sphere bounding_sphere(const float* lo, const float* hi) {
    const double hx = 0.5 * ((double)hi[0] - lo[0]), hy = 0.5 * ((double)hi[1] - lo[1]), hz = 0.5 * ((double)hi[2] - lo[2]);
    double r = __builtin_sqrt(hx * hx + hy * hy + hz * hz);
    r = r * (1.0 + 0x1p-6) + 0x1p-10;
    return Sphere{(float)(0.5 * ((double)hi[0] + lo[0])), (float)(0.5 * ((double)hi[1] + lo[1])),
                  (float)(0.5 * ((double)hi[2] + lo[2])), (float)(r * r)};
}

// bit test (immune to -fno-honor-nans): neither an infinity nor a NaN
LRC_VHD bool finite_bits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}

// true: the object-frame ray (o, d) is left out of the mover's cast.  Either its line passes the sphere's centre at more
// than the radius (|e x d|^2 > (r^2 + 2^-10 |e|^2) |d|^2: the second term covers the cancellation in the cross product, whose
// error grows with the distance |e| of the origin), or it starts outside the sphere and points away from the centre.  A ray
// whose squares overflow (or are NaN) cannot be judged and is cast.  The traversal's own root-box test fails for every ray
// this one leaves out: the box lies inside the sphere, with the margin above.
LRC_VHD bool culled(const Sphere s, Vec o, Vec d) {
    const Vec e{s.cx - o.x, s.cy - o.y, s.cz - o.z};
    const float kx = e.y * d.z - e.z * d.y, ky = e.z * d.x - e.x * d.z, kz = e.x * d.y - e.y * d.x;
    const float k2 = (kx * kx + ky * ky) + kz * kz;
    const float d2 = (d.x * d.x + d.y * d.y) + d.z * d.z;
    const float e2 = (e.x * e.x + e.y * e.y) + e.z * e.z;
    const float ed = (e.x * d.x + e.y * d.y) + e.z * d.z;
    const bool beside = k2 > (s.r2 + 0x1p-10f * e2) * d2;
    const bool behind = (ed < 0.0f) & (e2 > s.r2);
    return (beside | behind) & finite_bits(k2) & finite_bits(d2) & finite_bits(e2);
}

// What the ray kernel needs of one mover of a call (lidarcast.hip, mover_rays_kernel<SWEEP, NOISY>; flow_object_rays_kernel).
struct RayPass {
    const float* records;      // device: the mover poses (P, M, 12), under SWEEP the mover sweep records (P, M, 24) below;
                               // NULL: the static pass, the world ray itself is formed and stored, nothing culled
    uint32_t M, m;
    Sphere sphere;
};

// ---- movers under moving-sensor sweeps (lrc_scan_mover_sweeps_*; include/lidarcast.h "movers under moving-sensor sweeps",
// DESIGN.md section 5n) -----------------------------------------------------------------------------------------------------
// Mover sweep record of (sweep, mover), 24 float32: r[0..11] the START pose12, r[12..15] dq = (w, x, y, z) with
// R_end = R(dq) R_start and w >= cos(pi/4), r[16..18] dc = c_end - c_start, the rest zero.  Ray i fires at s = (float)fire[i] and
// meets the mover at its pose at s.  Every operation is a separate IEEE float32 operation in exactly this order (nothing fused;
// tests/mover_sweep_restate.py restates it op for op in numpy):
//   pose at s   c_j = c0_j + s * dc_j                                                 (a product, then a sum)
//               qw = (1 - s) + s * dq.w;  u = (s * dq.x, s * dq.y, s * dq.z)          (nlerp, never normalised)
//               n = ((qw*qw + ux*ux) + uy*uy) + uz*uz;  k = 2 / n
//   cross       t = u x v:  tx = uy*vz - uz*vy,  ty = uz*vx - ux*vz,  tz = ux*vy - uy*vx
//               w = u x t:  wx = uy*tz - uz*ty,  wy = uz*tx - ux*tz,  wz = ux*ty - uy*tx
//   forward     R(q) v:    v'_j = v_j + k * (qw * t_j + w_j)                          (gen_ray_sweep's form, in float32)
//   inverse     R(q)^T v:  v'_j = v_j + k * (w_j - qw * t_j)                          (the conjugate: u -> -u flips t, keeps w)
//   to_object_at  e = o - c (three subtractions);  o' = rot_to_object(R_start, inverse(e));  d' = rot_to_object(R_start, inverse(d))
//   to_world_at   n' = forward(to_world(R_start, n)), not renormalised
// A STILL record -- r[12] has the bits of 1.0f and r[13..18] are all +0.0f, tested on the seven words -- takes to_object /
// to_world with r[0..11] instead, so a mover that stands still through a sweep gives the bits of lrc_scan_movers_*.  (A -0.0 among
// the six words is no still record: it takes the general path, whose result then differs from the still one in signed zeros only.)
struct At { float cx, cy, cz, qw, ux, uy, uz, k; };

LRC_VHD bool still(const float* r) {
    uint32_t w[7];
    __builtin_memcpy(w, r + 12, 28);
    return (w[0] == 0x3F800000u) & ((w[1] | w[2] | w[3] | w[4] | w[5] | w[6]) == 0u);
}

LRC_VHD At pose_at(const float* r, float s) {
    At a;
    a.cx = r[3] + s * r[16];
    a.cy = r[7] + s * r[17];
    a.cz = r[11] + s * r[18];
    a.qw = (1.0f - s) + s * r[12];
    a.ux = s * r[13]; a.uy = s * r[14]; a.uz = s * r[15];
    const float n = ((a.qw * a.qw + a.ux * a.ux) + a.uy * a.uy) + a.uz * a.uz;
    a.k = 2.0f / n;
    return a;
}

// R(q) v (inverse == false) or R(q)^T v (inverse == true)
LRC_VHD Vec rot_at(const At& a, Vec v, bool inverse) {
    const float tx = a.uy * v.z - a.uz * v.y, ty = a.uz * v.x - a.ux * v.z, tz = a.ux * v.y - a.uy * v.x;
    const float wx = a.uy * tz - a.uz * ty, wy = a.uz * tx - a.ux * tz, wz = a.ux * ty - a.uy * tx;
    if (inverse) return Vec{v.x + a.k * (wx - a.qw * tx), v.y + a.k * (wy - a.qw * ty), v.z + a.k * (wz - a.qw * tz)};
    return Vec{v.x + a.k * (a.qw * tx + wx), v.y + a.k * (a.qw * ty + wy), v.z + a.k * (a.qw * tz + wz)};
}

// the world ray (o, d) in the frame the mover of record r has at s
LRC_VHD void to_object_at(const float* r, float s, Vec o, Vec d, Vec& oo, Vec& od) {
    if (still(r)) { to_object(r, o, d, oo, od); return; }
    const At a = pose_at(r, s);
    const Vec e{o.x - a.cx, o.y - a.cy, o.z - a.cz};
    oo = rot_to_object(r, rot_at(a, e, true));
    od = rot_to_object(r, rot_at(a, d, true));
}

// the mover record's normal in the world, by the pose the mover of record r has at s
LRC_VHD Vec to_world_at(const float* r, float s, Vec n) {
    if (still(r)) return to_world(r, n);
    return rot_at(pose_at(r, s), to_world(r, n), false);
}

}  // namespace lrcmov
