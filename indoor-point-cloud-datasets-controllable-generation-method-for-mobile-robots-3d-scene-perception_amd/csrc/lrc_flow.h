// lrc_flow.h -- scene flow under rigid movers (include/lidarcast.h "scene flow"): the arithmetic the flow
// kernels of lidarcast.hip and the host functions lrc_flow_rays / lrc_flow_status share, written once for both.
//
//   target    where the surface under a point x of mover w (pose A when scanned, pose B next) will be: y = R_B (R_A^T (x - c_A)) + c_B
//             in float64, one rounding per operation, nothing fused (the build is -ffp-contract=off); y = x for the room (w = 0),
//             for a mover whose two poses have the same 48 bytes, and for a mover id above M (no such pose row)
//   ray       flow3 = float32(y - x); the line of sight from the next sensor origin o to y32 = float32(y): d = y32 - o,
//             L = |d|, h = d / L in float32; thr = L - 2^-12 max(L, 1); the range test of the scan's filter on y32
//   judge     occluded iff the nearest range met along (o, h) is below thr, as float32
// and, for deforming movers (section 5p, shared by nonrigid_target_kernel and lrc_nonrigid_flow_rays):
//   nonrigid_ray   the target of a row on a deforming triangle (rest, displace, world), then the line of sight (sight)
#pragma once
#include "lrc_movers.h"

namespace lrcflow {

constexpr uint8_t kNone = 0;           // no return, or the frame has no next
constexpr uint8_t kVisible = 1;        // in range and nothing in front of it
constexpr uint8_t kOccluded = 2;
constexpr uint8_t kOutOfRange = 3;     // not cast
constexpr float kMargin = 0x1p-12f;    // relative to max(L, 1): the product with it is exact

// the two poses of a mover are the same 48 bytes: it stands still, whatever the bytes say
LRC_VHD bool same_pose(const float* a, const float* b) {
    bool same = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        uint32_t u, v;
        __builtin_memcpy(&u, a + k, 4);
        __builtin_memcpy(&v, b + k, 4);
        same &= u == v;
    }
    return same;
}

// step 1 of the header for a moved point: float64, three subtractions, R_A^T, R_B, three additions
LRC_VHD void target(const float* x, const float* A, const float* B, double* y) {
    const double ex = (double)x[0] - (double)A[3], ey = (double)x[1] - (double)A[7], ez = (double)x[2] - (double)A[11];
    double q[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = ((double)A[j] * ex + (double)A[4 + j] * ey) + (double)A[8 + j] * ez;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        y[j] = (((double)B[4 * j] * q[0] + (double)B[4 * j + 1] * q[1]) + (double)B[4 * j + 2] * q[2]) + (double)B[4 * j + 3];
}

// What steps 1 to 3 give for one row: the flow, the line of sight and the preliminary status (kVisible: to be cast and judged).
struct Ray {
    float flow[3];
    lrcmov::Vec o, h;
    float thr;
    uint8_t status;
};

// `live`: the row has a return and its frame a next one.  `moved`: A and B are the row's own pose pair and differ (the caller
// has looked at w and at the bytes).  next16: the next sensor pose, row-major 4 x 4 float64.
LRC_VHD Ray ray(bool live, bool moved, const float* x, const float* A, const float* B, const double* next16, double max_range,
                double min_range) {
    Ray r{};
    r.status = kNone;
    if (!live) return r;
    double y[3] = {(double)x[0], (double)x[1], (double)x[2]};
    if (moved) {
        target(x, A, B, y);
#pragma unroll
        for (int j = 0; j < 3; ++j) r.flow[j] = (float)(y[j] - (double)x[j]);
    }
    const float y32[3] = {(float)y[0], (float)y[1], (float)y[2]};
    const double cx = next16[3], cy = next16[7], cz = next16[11];
    r.o = lrcmov::Vec{(float)cx, (float)cy, (float)cz};
    const float dx = y32[0] - r.o.x, dy = y32[1] - r.o.y, dz = y32[2] - r.o.z;
    const float L = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
    r.h = lrcmov::Vec{dx / L, dy / L, dz / L};
    r.thr = L - kMargin * (L > 1.0f ? L : 1.0f);
    // the scan's range filter (write_back): the float64 distance of the float32 point from the float64 centre
    const double ex = (double)y32[0] - cx, ey = (double)y32[1] - cy, ez = (double)y32[2] - cz;
    const double dist = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);
    bool in = dist < max_range;
    if (min_range > 0.0) in = in & (dist >= min_range);
    r.status = in ? kVisible : kOutOfRange;
    return r;
}

// step 5: the running minimum of the static scene's and the movers' ranges against the row's threshold
LRC_VHD float nearer(float t, float t_min) { return t < t_min ? t : t_min; }
LRC_VHD uint8_t judge(float t_min, float thr) { return t_min < thr ? kOccluded : kVisible; }

// ---- non-rigid flow (include/lidarcast.h "non-rigid scene flow") ------------------------------------------
// The target of a row that lies on a deforming triangle: the point goes into the mover's frame (rest = the first half of
// target), is given the triangle's vertex displacements from shape A to shape B, interpolated at its barycentric coordinates in
// shape A, and leaves the frame at the next pose (world = the second half of target).  A triangle whose three vertices keep
// their bits gives z = q with no addition, hence the bytes of target.
constexpr uint32_t kMaxPairs = 16;     // surface pairs per call: they travel in the kernel arguments

LRC_VHD void rest(const float* x, const float* A, double* q) {
    const double ex = (double)x[0] - (double)A[3], ey = (double)x[1] - (double)A[7], ez = (double)x[2] - (double)A[11];
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = ((double)A[j] * ex + (double)A[4 + j] * ey) + (double)A[8 + j] * ez;
}

LRC_VHD void world(const double* z, const float* B, double* y) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
        y[j] = (((double)B[4 * j] * z[0] + (double)B[4 * j + 1] * z[1]) + (double)B[4 * j + 2] * z[2]) + (double)B[4 * j + 3];
}

LRC_VHD double dot3(const double* p, const double* q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

// va9 / vb9: the three vertices of the row's triangle in shape A and in shape B.  Returns whether any of the nine displacement
// components differs from zero; z = q exactly when none does.  No clamp of (u, v): a point a rounding outside its triangle is
// extrapolated.  A triangle without area (den <= 0, or NaN) takes the displacement of its first vertex.
LRC_VHD bool displace(const double* q, const float* va9, const float* vb9, double* z) {
    double a[9], D[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) a[k] = (double)va9[k];
    const double e1[3] = {a[3] - a[0], a[4] - a[1], a[5] - a[2]};
    const double e2[3] = {a[6] - a[0], a[7] - a[1], a[8] - a[2]};
    const double r[3] = {q[0] - a[0], q[1] - a[1], q[2] - a[2]};
    const double d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), r1 = dot3(r, e1), r2 = dot3(r, e2);
    const double den = d11 * d22 - d12 * d12;
    double u = 0.0, v = 0.0;
    if (den > 0.0) {
        u = (d22 * r1 - d12 * r2) / den;
        v = (d11 * r2 - d12 * r1) / den;
    }
    const double s = (1.0 - u) - v;
    bool bent = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        D[k] = (double)vb9[k] - a[k];
        bent |= !(D[k] == 0.0);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) z[c] = bent ? q[c] + ((s * D[c] + u * D[3 + c]) + v * D[6 + c]) : q[c];
    return bent;
}

// steps 2 to 3 of section 5m from a target y on, as `ray` has them: the line of sight, thr and the range test
LRC_VHD void sight(Ray& r, const double* y, const double* next16, double max_range, double min_range) {
    const float y32[3] = {(float)y[0], (float)y[1], (float)y[2]};
    const double cx = next16[3], cy = next16[7], cz = next16[11];
    r.o = lrcmov::Vec{(float)cx, (float)cy, (float)cz};
    const float dx = y32[0] - r.o.x, dy = y32[1] - r.o.y, dz = y32[2] - r.o.z;
    const float L = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
    r.h = lrcmov::Vec{dx / L, dy / L, dz / L};
    r.thr = L - kMargin * (L > 1.0f ? L : 1.0f);
    const double ex = (double)y32[0] - cx, ey = (double)y32[1] - cy, ez = (double)y32[2] - cz;
    const double dist = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);
    bool in = dist < max_range;
    if (min_range > 0.0) in = in & (dist >= min_range);
    r.status = in ? kVisible : kOutOfRange;
}

// `ray` for a live row with a surface pair: A and B are the row's own pose pair.  y = x and +0 flow if and only if the two poses
// have the same 48 bytes AND no vertex of the triangle moves.
LRC_VHD Ray nonrigid_ray(const float* x, const float* A, const float* B, const float* va9, const float* vb9, const double* next16,
                         double max_range, double min_range) {
    Ray r{};
    double q[3], z[3], y[3] = {(double)x[0], (double)x[1], (double)x[2]};
    rest(x, A, q);
    const bool bent = displace(q, va9, vb9, z);
    if (bent || !same_pose(A, B)) {
        world(z, B, y);
#pragma unroll
        for (int j = 0; j < 3; ++j) r.flow[j] = (float)(y[j] - (double)x[j]);
    }
    sight(r, y, next16, max_range, min_range);
    return r;
}

}  // namespace lrcflow
