// lrc_flow.h -- scene flow under rigid movers (include/lidarcast.h "scene flow"): the arithmetic the flow
// kernels of lidarcast.hip and the host functions lrc_flow_rays / lrc_flow_status share, written once for both.
//
//   target    where the surface under a point x of mover w (pose A when scanned, pose B next) will be: y = R_B (R_A^T (x - c_A)) + c_B
//             in float64, one rounding per operation, nothing fused (the build is -ffp-contract=off); y = x for the room (w = 0),
//             for a mover whose two poses have the same 48 bytes, and for a mover id above M (no such pose row)
//   ray       flow3 = float32(y - x); the line of sight from the next sensor origin o to y32 = float32(y): d = y32 - o,
//             L = |d|, h = d / L in float32; thr = L - 2^-12 max(L, 1); the range test of the scan's filter on y32
//   judge     occluded iff the nearest range met along (o, h) is below thr, as float32
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

}  // namespace lrcflow
