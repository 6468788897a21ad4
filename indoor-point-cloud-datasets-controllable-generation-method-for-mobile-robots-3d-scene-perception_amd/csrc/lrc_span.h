// lrc_span.h -- animated movers under sweeps (include/lidarcast.h "animated movers under sweeps"): the
// arithmetic the kernels of lrc_span.hip and the host functions lrc_span_vertices / lrc_deform_span_refit share, written once
// for both.  A SPAN is a deformable between two shapes A and B: ray i of a sweep, fired at s = (float)fire[i], meets the
// triangles of the shape span_vertex(A, B, s).
//
//   span_vertex  one coordinate of the shape at s: a where s == 0 or a and b have the same bits, b where s == 1, else
//                lrcdef::blend1(a, b, s).  The three copies are the rule blend1 asks of its callers (-0 + 0 is +0): a shape that
//                does not change keeps its vertices bit for bit.  blend1 clamps into [min(a, b), max(a, b)], so every value lies
//                between its two ends exactly.
//   slot_span    one leaf slot from the vertices of both shapes: the slot's vertex record (v0, v1, v2 of A, then of B: 18
//                floats, gathered once so that a leaf test reads consecutive bytes) and its span box, tmin / tmax of the
//                triangle's vertex boxes at A and at B (lrctri::tri_record's own boxes, the builders' total order)
// float32, one rounding per operation (the build is -ffp-contract=off), nothing fused.
#pragma once
#include <stdint.h>

#include "lrc_deform.h"

namespace lrcspan {

constexpr int kRecFloats = 20;      // per slot: 18 floats and two of padding, five 16-byte loads

LRC_THD float span_vertex(float a, float b, float s) {
    uint32_t ua, ub;
    __builtin_memcpy(&ua, &a, 4);
    __builtin_memcpy(&ub, &b, 4);
    if (s == 0.0f || ua == ub) return a;
    if (s == 1.0f) return b;
    return lrcdef::blend1(a, b, s);
}

// rec18: nullable
LRC_THD void slot_span(const float* va3, const float* vb3, const uint32_t* tris3, uint32_t prim, float* rec18, float* box6) {
    float v[18];
    for (int c = 0; c < 3; ++c) {
        const uint64_t i = 3 * (uint64_t)tris3[3 * (uint64_t)prim + c];
        for (int k = 0; k < 3; ++k) { v[3 * c + k] = va3[i + k]; v[9 + 3 * c + k] = vb3[i + k]; }
    }
    float ra[12], ba[6], bb[6];
    lrctri::tri_record(v, v + 3, v + 6, ra, ba);
    lrctri::tri_record(v + 9, v + 12, v + 15, ra, bb);
    for (int k = 0; k < 3; ++k) { box6[k] = lrctri::tmin(ba[k], bb[k]); box6[3 + k] = lrctri::tmax(ba[3 + k], bb[3 + k]); }
    if (rec18)
        for (int k = 0; k < 18; ++k) rec18[k] = v[k];
}

}  // namespace lrcspan
