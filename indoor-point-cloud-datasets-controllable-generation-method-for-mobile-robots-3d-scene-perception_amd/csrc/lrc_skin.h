// lrc_skin.h -- skinned deforming movers (include/lidarcast.h "skinned deforming movers"): the arithmetic
// the kernel of lrc_skin.hip, the host pass of lrc_deform_create_skinned and lrc_skin_apply share, written once for all three.
//
//   bone pose  12 float32, the row-major 3 x 4 [A | c] of lrc_movers.h's pose12: any affine map, no orthonormality demanded
//   vertex     rest position (x, y, z), idx[4] (uint8 bone indices) and wgt[4] (float32 weights); an unused influence carries
//              weight +0 and any valid bone index
//   skin1      all four influences, always, in index order.  With m = bones + 12 * idx[j]:
//                  p_j.i = ((m[4i] * x + m[4i+1] * y) + m[4i+2] * z) + m[4i+3]
//                  v.i   = ((wgt0 * p_0.i + wgt1 * p_1.i) + wgt2 * p_2.i) + wgt3 * p_3.i
// A shape (k0, k1, w) is lrcdef::blend1(skin1 under pose k0, skin1 under pose k1, w) per coordinate; for w == 0, w == 1 or
// k0 == k1 it is skin1 under the one pose and nothing is blended.
// float32, one rounding per operation (the build is -ffp-contract=off), nothing fused.
#pragma once
#include <stdint.h>

#include "lrc_deform.h"

namespace lrcskin {

constexpr uint32_t kMaxBones = 255;

// coordinate i of the rest position (x, y, z) under the bone pose m
LRC_THD float bone1(const float* m, int i, float x, float y, float z) {
    return ((m[4 * i] * x + m[4 * i + 1] * y) + m[4 * i + 2] * z) + m[4 * i + 3];
}

// bones: a pose's table of 12-float bone poses; idx, wgt: the vertex's four influences; p: its rest position; out: 3 floats
LRC_THD void skin1(const float* bones, const uint8_t* idx, const float* wgt, const float* p, float* out) {
    const float* m0 = bones + 12 * (uint32_t)idx[0];
    const float* m1 = bones + 12 * (uint32_t)idx[1];
    const float* m2 = bones + 12 * (uint32_t)idx[2];
    const float* m3 = bones + 12 * (uint32_t)idx[3];
    for (int i = 0; i < 3; ++i) {
        const float p0 = bone1(m0, i, p[0], p[1], p[2]);
        const float p1 = bone1(m1, i, p[0], p[1], p[2]);
        const float p2 = bone1(m2, i, p[0], p[1], p[2]);
        const float p3 = bone1(m3, i, p[0], p[1], p[2]);
        out[i] = ((wgt[0] * p0 + wgt[1] * p1) + wgt[2] * p2) + wgt[3] * p3;
    }
}

}  // namespace lrcskin
