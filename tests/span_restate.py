"""The numpy restatement of the animated movers under sweeps (include/lidarcast.h "animated movers under sweeps"; DESIGN.md section
5s), shared by tests/test_span_host.py and tests/test_span_gpu.py.  Written from the header's text: span_vertex per coordinate, the
span box of a leaf slot, the box invariant of a tree refitted to two shapes, the composition of a sweep scan whose animated
movers are cast per firing fraction on a fresh mesh of the blended vertices, and the float64 witness of the physical check (the
distance of a world point from triangle ``prim`` of the shape and pose at the point's own firing fraction)."""
import numpy as np

import mover_sweep_restate as ms
from deform_restate import blend_restate, tmax, tmin, verts_below
from helpers import assert_bit_equal, bits

F = np.float32


def span_vertices_restate(a, b, s):
    """a where s == 0 or the bits agree, b where s == 1, else the blend: v = a + s * (b - a), clamped into [min, max]"""
    a, b, s = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F), F(s)
    if s == 0:
        return a.copy()
    if s == 1:
        return np.where(bits(a) == bits(b), a, b).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        v = (a + (s * (b - a)).astype(F)).astype(F)
    lo, hi = np.where(a < b, a, b), np.where(a < b, b, a)
    v = np.where(v < lo, lo, v)
    v = np.where(v > hi, hi, v).astype(F)
    return np.where(bits(a) == bits(b), a, v).astype(F)


def span_boxes_restate(slot_prim, tris, va, vb):
    """per slot the min / max, in the builders' total order, over its triangle's three vertices in both shapes"""
    tv = np.concatenate([va[tris[slot_prim]], vb[tris[slot_prim]]], 1)          # (S, 6, 3)
    return np.concatenate([tmin(tv, 1), tmax(tv, 1)], 1)


def check_span_invariant(nodes, before, slot_prim, tris, va, vb, what):
    """Every child box is the exact min / max, in the total order, over both shapes' vertices below it; an empty leaf keeps the
    box it had in ``before``."""
    refs = nodes[:, 12:14].view(np.int32)
    for i in range(len(nodes)):
        for c in range(2):
            box = nodes[i, 6 * c:6 * c + 6]
            if refs[i, c] < 0 and (~int(refs[i, c]) & 7) == 0:
                assert_bit_equal(box, before[i, 6 * c:6 * c + 6], f"{what}: the empty leaf of node {i}")
                continue
            pts = np.concatenate([verts_below(nodes, slot_prim, tris, refs[i, c], va),
                                  verts_below(nodes, slot_prim, tris, refs[i, c], vb)], 0)
            assert_bit_equal(box[:3], tmin(pts), f"{what}: node {i} child {c} lo")
            assert_bit_equal(box[3:], tmax(pts), f"{what}: node {i} child {c} hi")


def fraction_cast(cast_of_vertices, va, vb, fire):
    """A "cast these rays" function for ONE sweep of an animated mover: the rays (one per entry of ``fire``) are grouped by
    float32(fire) and each group is cast by ``cast_of_vertices(span_vertices(va, vb, s))(rays)``, a cast on a fresh mesh."""
    from lidarcast import deform
    s32 = np.asarray(fire, np.float64).astype(F)

    def cast(rays):
        rays = np.ascontiguousarray(rays, F)
        out = None
        for s in np.unique(s32):
            idx = np.flatnonzero(s32 == s)
            part = cast_of_vertices(deform.span_vertices(va, vb, s))(rays[idx])
            if out is None:
                out = {k: np.zeros((len(rays),) + np.asarray(v).shape[1:], np.asarray(v).dtype) for k, v in part.items()}
            for k, v in part.items():
                out[k][idx] = v
        return out
    return cast


def compose_sweeps(cast_static, casts_of_sweep, rays, centres, fire, records, N, max_range, **kw):
    """mover_sweep_restate.compose_host sweep by sweep: ``casts_of_sweep(p)`` gives the M cast functions of sweep p (an animated
    mover's is a ``fraction_cast`` of that sweep's two shapes).  Same return value: (records over all P * N rays, winners)."""
    P = len(rays) // N
    outs, wins = [], []
    for p in range(P):
        sl = slice(p * N, (p + 1) * N)
        o, w = ms.compose_host(cast_static, casts_of_sweep(p), rays[sl], centres[sl], fire, records[p:p + 1], N, max_range, **kw)
        outs.append(o)
        wins.append(w)
    cat = lambda ds: {k: np.concatenate([d[k] for d in ds]) for k in ds[0]}
    return cat(outs), cat(wins)


def _point_triangle_distance(p, a, b, c):
    """float64 distance of point p from triangle abc (Ericson's closest point)"""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return np.linalg.norm(ap)
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return np.linalg.norm(bp)
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return np.linalg.norm(ap - ab * (d1 / (d1 - d3)))
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return np.linalg.norm(cp)
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return np.linalg.norm(ap - ac * (d2 / (d2 - d6)))
    va = d3 * d6 - d5 * d4
    if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        return np.linalg.norm(p - (b + w * (c - b)))
    den = 1.0 / (va + vb + vc)
    return np.linalg.norm(p - (a + ab * (vb * den) + ac * (vc * den)))


def triangle_distance(points, prim, s, rec, tris, va, vb):
    """The float64 witness: the distance of each world point from triangle ``prim`` of the shape at its own s -- the exact
    linear blend of the two float32 shapes -- in the mover's frame by the pose the record gives at s (the centre c0 + s dc, the
    rotation R(q(s) / |q(s)|) R_start)."""
    r = np.asarray(rec, np.float64).reshape(24)
    p = np.asarray(points, np.float64)
    s = np.asarray(s, np.float64)
    A, B = np.asarray(va, np.float64), np.asarray(vb, np.float64)
    R0 = r[:12].reshape(3, 4)[:, :3]
    out = np.empty(len(p))
    for i in range(len(p)):
        q = np.array([(1.0 - s[i]) + s[i] * r[12], s[i] * r[13], s[i] * r[14], s[i] * r[15]])
        w, x, y, z = q / np.linalg.norm(q)
        Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        local = (Rq @ R0).T @ (p[i] - (r[[3, 7, 11]] + s[i] * r[16:19]))
        tri = tris[int(prim[i])]
        v = A[tri] + s[i] * (B[tri] - A[tri])
        out[i] = _point_triangle_distance(local, v[0], v[1], v[2])
    return out
