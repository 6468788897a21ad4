"""The numpy restatement of the deforming movers' arithmetic (include/lidarcast.h "deforming movers"),
shared by tests/test_deform_host.py and tests/test_deform_gpu.py: the blend, the builders' total order on float32 (-0 below
+0), the 48-byte triangle record, the slot box, and the box invariant of a tree in the documented node layout."""
import numpy as np

from helpers import assert_bit_equal, bits

F = np.float32


def blend_restate(a, b, w):
    a, b, w = np.asarray(a, F), np.asarray(b, F), F(w)
    if w == 0:
        return a.copy()
    if w == 1:
        return b.copy()
    v = (a + (w * (b - a)).astype(F)).astype(F)
    lo, hi = np.where(a < b, a, b), np.where(a < b, b, a)
    v = np.where(v < lo, lo, v)
    return np.where(v > hi, hi, v).astype(F)


def enc(x):
    i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
    return np.where(i < 0, i ^ 0x7FFFFFFF, i)


def tmin(x, axis=0):
    """min in the builders' total order (-0 below +0), bits kept."""
    x = np.ascontiguousarray(x, F)
    return np.take_along_axis(x, np.expand_dims(np.argmin(enc(x), axis), axis), axis).squeeze(axis)


def tmax(x, axis=0):
    x = np.ascontiguousarray(x, F)
    return np.take_along_axis(x, np.expand_dims(np.argmax(enc(x), axis), axis), axis).squeeze(axis)


def leaf_ref(first, count):
    return np.int32(~np.int64(first * 8 + count))


def set_refs(node, r0, r1):
    node[12:14] = np.array([r0, r1], np.int32).view(F)


def verts_below(nodes, slot_prim, tris, ref, verts):
    """Every vertex (rows) of every triangle below child reference ``ref``."""
    ref = int(ref)
    if ref < 0:
        code = ~ref
        first, cnt = code >> 3, code & 7
        return verts[tris[slot_prim[first:first + cnt]].reshape(-1)]
    r = nodes[ref, 12:14].view(np.int32)
    return np.concatenate([verts_below(nodes, slot_prim, tris, r[0], verts), verts_below(nodes, slot_prim, tris, r[1], verts)], 0)


def check_box_invariant(nodes, slot_prim, tris, verts, what):
    """Every child box is the exact min / max, in the total order, of the vertices below it; an empty leaf's box is zero."""
    refs = nodes[:, 12:14].view(np.int32)
    for i in range(len(nodes)):
        for c in range(2):
            box = nodes[i, 6 * c:6 * c + 6]
            if refs[i, c] < 0 and (~int(refs[i, c]) & 7) == 0:
                assert not bits(box).any(), f"{what}: empty leaf of node {i} has a box"
                continue
            pts = verts_below(nodes, slot_prim, tris, refs[i, c], verts)
            assert_bit_equal(box[:3], tmin(pts), f"{what}: node {i} child {c} lo")
            assert_bit_equal(box[3:], tmax(pts), f"{what}: node {i} child {c} hi")


def records_restate(slot_prim, tris, verts):
    v0, v1, v2 = (verts[tris[slot_prim, k]] for k in range(3))
    e1, e2 = (v0 - v1).astype(F), (v2 - v0).astype(F)

    def fma_cross(j, k):            # fma(e2_j, e1_k, -(e2_k * e1_j)): the product rounded once, the fma exact in float64
        p = (e2[:, k] * e1[:, j]).astype(F)
        return (e2[:, j].astype(np.float64) * e1[:, k].astype(np.float64) - p.astype(np.float64)).astype(F)

    ng = np.stack([fma_cross(1, 2), fma_cross(2, 0), fma_cross(0, 1)], 1)
    return np.concatenate([v0, e1, e2, ng], 1).astype(F)


def slot_boxes_restate(slot_prim, tris, verts):
    tv = verts[tris[slot_prim]]          # (S, 3, 3)
    return np.concatenate([tmin(tv, 1), tmax(tv, 1)], 1)
