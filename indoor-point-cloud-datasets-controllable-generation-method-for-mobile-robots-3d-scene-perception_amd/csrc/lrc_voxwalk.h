// lrc_voxwalk.h -- the voxel walk of one segment, host and device: the one definition of the grid, the walk and its limits for
// the static grid (lrc_voxgrid.hip) and the frame slots (lrc_voxseq.hip, section 5u).  Both walk kernels
// and the host step lrc_voxseq_walk are compiled from these very functions; tests/voxgrid_restate.py restates them in numpy.
//
//   Grid    origin g (3 float64), voxel size s (float64 > 0), dims (nx, ny, nz), nx*ny*nz <= 2^31 - 1.  The voxel of a
//           float64 point x is i_a = floor((x_a - g_a) / s) (an f64 subtract, then an f64 divide, then floor); it is
//           inside iff 0 <= i < n on every axis; linear index (i*ny + j)*nz + k (C order, z fastest).
//   Walk    float64, no contraction, the float32 o and e widened exactly: a = voxel(o), b = voxel(e), D = e - o.  Per axis with
//           b_a != a_a: n_a = |b_a - a_a|, step_a = sign(b_a - a_a), tMax_a = ((g_a + (a_a + 1)*s) - o_a) / D_a stepping
//           up, ((g_a + a_a*s) - o_a) / D_a stepping down, tDelta_a = s / |D_a|; axes with n_a = 0 take no part.  Visit a;
//           while any n_a > 0: take the axis with the smallest tMax among those with n_a > 0 (ties x, then y, then z),
//           step it, tMax_a += tDelta_a, n_a -= 1, visit the new voxel.  The walk ends in b (Manhattan + 1 voxels).
//           Every visited in-grid voxel except b goes to the sink (its FREE bit); a == b carves nothing.
//   Limits  a segment whose o or e is not finite, whose voxel coordinates leave [-2^31, 2^31), or whose walk is 2^24 or
//           more steps long is REJECTED: nothing goes to the sink and it has no end voxel.
#ifndef LRC_VOXWALK_H
#define LRC_VOXWALK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace lrcwalk {

#define LRC_WALK_HD __host__ __device__ inline

constexpr int64_t kMaxWalk = 1ll << 24;             // steps per segment (the Manhattan distance) refused
constexpr double kCoordLimit = 2147483648.0;        // voxel coordinates in [-2^31, 2^31)

struct Grid {
    double gx, gy, gz, s;
    int32_t nx, ny, nz;
    uint32_t V;
};

enum { kWalkRejected = -1, kWalkNoEnd = 0, kWalkEnd = 1 };

LRC_WALK_HD bool finite_f(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7F800000u) != 0x7F800000u; }

// voxel coordinate of one axis; false when it leaves [-2^31, 2^31) (x, g finite, s > 0: no NaN here)
LRC_WALK_HD bool vox_coord(double x, double g, double s, int32_t& out) {
    const double f = __builtin_floor((x - g) / s);
    if (!(f >= -kCoordLimit && f < kCoordLimit)) return false;
    out = (int32_t)f;                                // exact: an integer in int32's range
    return true;
}

// the rest of the walk is outside the grid on this axis: c is past the grid in the direction of travel (or the axis does
// not move and c is outside)
LRC_WALK_HD bool gone(int32_t c, int32_t step, int32_t n) { return (step >= 0 && c >= n) || (step <= 0 && c < 0); }

LRC_WALK_HD bool in_grid(const Grid& g, int32_t c0, int32_t c1, int32_t c2) {
    return (uint32_t)c0 < (uint32_t)g.nx && (uint32_t)c1 < (uint32_t)g.ny && (uint32_t)c2 < (uint32_t)g.nz;
}

LRC_WALK_HD uint32_t linear(const Grid& g, int32_t c0, int32_t c1, int32_t c2) {
    return ((uint32_t)c0 * (uint32_t)g.ny + (uint32_t)c1) * (uint32_t)g.nz + (uint32_t)c2;
}

// Walk o -> e.  sink.add(idx) receives every visited in-grid voxel except b, in walk order, then sink.flush() once (a walk
// that is rejected or never enters the grid calls neither).  The walk stops early once it
// has left the grid on an axis in that axis' direction of travel: no later voxel, b included, can be inside again.
// Returns kWalkRejected (limits: nothing was added; b3 is b when only the length was refused, else untouched), kWalkEnd (b
// is in the grid, end_idx its linear index) or kWalkNoEnd.  b3 receives b whenever the coordinates are in range.
template <class Sink>
LRC_WALK_HD int walk_segment(const Grid& g, float ox_, float oy_, float oz_, float ex_, float ey_, float ez_, Sink& sink,
                             uint32_t& end_idx, int32_t* b3) {
    if (!(finite_f(ox_) && finite_f(oy_) && finite_f(oz_) && finite_f(ex_) && finite_f(ey_) && finite_f(ez_)))
        return kWalkRejected;
    const double ox = ox_, oy = oy_, oz = oz_, ex = ex_, ey = ey_, ez = ez_;
    int32_t a0, a1, a2, b0, b1, b2;
    if (!(vox_coord(ox, g.gx, g.s, a0) && vox_coord(oy, g.gy, g.s, a1) && vox_coord(oz, g.gz, g.s, a2) &&
          vox_coord(ex, g.gx, g.s, b0) && vox_coord(ey, g.gy, g.s, b1) && vox_coord(ez, g.gz, g.s, b2)))
        return kWalkRejected;
    b3[0] = b0; b3[1] = b1; b3[2] = b2;
    const int64_t d0 = (int64_t)b0 - a0, d1 = (int64_t)b1 - a1, d2 = (int64_t)b2 - a2;
    const int64_t m0 = d0 < 0 ? -d0 : d0, m1 = d1 < 0 ? -d1 : d1, m2 = d2 < 0 ? -d2 : d2;
    if (m0 + m1 + m2 >= kMaxWalk) return kWalkRejected;
    int32_t n0 = (int32_t)m0, n1 = (int32_t)m1, n2 = (int32_t)m2;
    const int32_t s0 = d0 > 0 ? 1 : (d0 < 0 ? -1 : 0);
    const int32_t s1 = d1 > 0 ? 1 : (d1 < 0 ? -1 : 0);
    const int32_t s2 = d2 > 0 ? 1 : (d2 < 0 ? -1 : 0);
    int32_t c0 = a0, c1 = a1, c2 = a2;
    if (gone(c0, s0, g.nx) || gone(c1, s1, g.ny) || gone(c2, s2, g.nz)) return kWalkNoEnd;     // never enters
    const double D0 = ex - ox, D1 = ey - oy, D2 = ez - oz;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0;
    if (s0) {
        t0 = ((g.gx + ((double)a0 + (s0 > 0 ? 1.0 : 0.0)) * g.s) - ox) / D0;
        q0 = g.s / __builtin_fabs(D0);
    }
    if (s1) {
        t1 = ((g.gy + ((double)a1 + (s1 > 0 ? 1.0 : 0.0)) * g.s) - oy) / D1;
        q1 = g.s / __builtin_fabs(D1);
    }
    if (s2) {
        t2 = ((g.gz + ((double)a2 + (s2 > 0 ? 1.0 : 0.0)) * g.s) - oz) / D2;
        q2 = g.s / __builtin_fabs(D2);
    }
    bool inside = true;
    while (n0 + n1 + n2 > 0) {
        if (in_grid(g, c0, c1, c2)) sink.add(linear(g, c0, c1, c2));
        bool out;
        if (n0 > 0 && (n1 == 0 || t0 <= t1) && (n2 == 0 || t0 <= t2)) {
            c0 += s0; t0 = t0 + q0; --n0;
            out = gone(c0, s0, g.nx);
        } else if (n1 > 0 && (n2 == 0 || t1 <= t2)) {
            c1 += s1; t1 = t1 + q1; --n1;
            out = gone(c1, s1, g.ny);
        } else {
            c2 += s2; t2 = t2 + q2; --n2;
            out = gone(c2, s2, g.nz);
        }
        if (out) {
            inside = false;
            break;
        }
    }
    sink.flush();           // here, not in the caller: after the return the sink's state would be carried through every exit
    // the walk ended in b (or left the grid for good: b is outside then)
    if (!(inside && in_grid(g, c0, c1, c2))) return kWalkNoEnd;
    end_idx = linear(g, c0, c1, c2);
    return kWalkEnd;
}

// Free bits of one ray on the device: consecutive voxels in one bitset word (steps along z, the fastest axis) are gathered
// into one mask; a word is written when the walk leaves it (and by flush() after the walk), with a plain load
// first and an atomicOr only when a bit is still clear -- all rays of a pose start in the sensor's voxel, and after the first
// wave those words are set.  (An L1-bypassing check load measured 2x slower: the plain load's stale answer costs at most an
// idempotent atomic.)
struct FreeSink {
    uint32_t* __restrict__ bits;                     // first word of the grid's (the frame slot's) bitset
    uint32_t w = 0xFFFFFFFFu, m = 0;
    __device__ void flush() {
        if (m && (bits[w] & m) != m) atomicOr(&bits[w], m);
    }
    __device__ void add(uint32_t idx) {
        const uint32_t nw = idx >> 5;
        if (nw != w) {
            flush();
            w = nw;
            m = 0;
        }
        m |= 1u << (idx & 31u);
    }
};

}  // namespace lrcwalk

#endif  // LRC_VOXWALK_H
