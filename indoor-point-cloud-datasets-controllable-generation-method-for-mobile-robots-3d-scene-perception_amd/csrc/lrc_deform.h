// lrc_deform.h -- deforming movers (include/lidarcast.h "deforming movers"): the arithmetic the kernels
// of lrc_deform.hip and the host functions lrc_deform_blend / lrc_deform_refit share, written once for both.
//
//   blend1     one coordinate of a blended vertex: v = a + w * (b - a), then clamped into [min(a, b), max(a, b)], so a blended
//              vertex lies in the union box of its two keyframes exactly (no argument about ulps).  The caller copies the
//              bits of a keyframe for w == 0, w == 1 and k0 == k1 and never calls this then.
//   slot_refit the 48-byte record and the slot box of one leaf slot from the current vertices (lrc_trirec.h: the builders'
//              own expressions)
//   node_refit both child boxes of one inner node: a leaf child's box is the min / max over its <= 4 slot boxes, an inner
//              child's box the min / max of that node's two boxes, in the builders' total order (-0 below +0); an empty leaf
//              (count 0: the sibling of a wrapped single leaf) keeps its box.  References are not touched.
// float32, one rounding per operation (the build is -ffp-contract=off), nothing fused.
#pragma once
#include <stdint.h>

#include "lrc_trirec.h"

namespace lrcdef {

LRC_THD float blend1(float a, float b, float w) {
    float v = a + w * (b - a);
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    v = v < lo ? lo : v;
    v = v > hi ? hi : v;
    return v;
}

LRC_THD void slot_refit(const float* verts3, const uint32_t* tris3, uint32_t prim, float* rec12, float* box6) {
    const float* v0 = verts3 + 3 * (uint64_t)tris3[3 * (uint64_t)prim];
    const float* v1 = verts3 + 3 * (uint64_t)tris3[3 * (uint64_t)prim + 1];
    const float* v2 = verts3 + 3 * (uint64_t)tris3[3 * (uint64_t)prim + 2];
    lrctri::tri_record(v0, v1, v2, rec12, box6);
}

// node: the 16 floats of one inner node (read: references, written: the twelve box planes); nodes: the whole array, of which
// only nodes of a smaller height are read
LRC_THD void node_refit(float* node, const float* nodes, const float* slot_box) {
    for (int c = 0; c < 2; ++c) {
        int32_t ref;
        __builtin_memcpy(&ref, &node[12 + c], 4);
        int lo[3], hi[3];
        if (ref < 0) {
            const uint32_t code = (uint32_t)(~ref), first = code >> 3, cnt = code & 7u;
            if (cnt == 0) continue;
            const float* b = slot_box + 6 * (uint64_t)first;
            for (int k = 0; k < 3; ++k) { lo[k] = lrctri::enc(b[k]); hi[k] = lrctri::enc(b[3 + k]); }
            for (uint32_t s = 1; s < cnt; ++s)
                for (int k = 0; k < 3; ++k) {
                    lo[k] = lrctri::imin(lo[k], lrctri::enc(b[6 * s + k]));
                    hi[k] = lrctri::imax(hi[k], lrctri::enc(b[6 * s + 3 + k]));
                }
        } else {
            const float* ch = nodes + 16 * (uint64_t)ref;
            for (int k = 0; k < 3; ++k) {
                lo[k] = lrctri::imin(lrctri::enc(ch[k]), lrctri::enc(ch[6 + k]));
                hi[k] = lrctri::imax(lrctri::enc(ch[3 + k]), lrctri::enc(ch[9 + k]));
            }
        }
        for (int k = 0; k < 3; ++k) { node[6 * c + k] = lrctri::dec(lo[k]); node[6 * c + 3 + k] = lrctri::dec(hi[k]); }
    }
}

}  // namespace lrcdef
