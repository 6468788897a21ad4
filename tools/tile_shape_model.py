#!/usr/bin/env python3
"""tools/tile_shape_model.py [scene] [pose ...] -- CPU lock-step model of the trace kernel's wave for different tile shapes.

Per-ray work does not depend on how rays are grouped into waves; how long a wave runs in lock step, and how often all its
live lanes want the same node (the scalar-fetch step), does.  The model walks a binned-SAH BVH (<= 4 triangles per leaf; NOT
the product builder's tree) with the kernel's while-while schedule: all lanes of a wave that are at an inner node step
together (near child first, the far one pushed, pruned by the closest hit so far), until none is; then every lane tests its
leaf, two triangle records per round; then every lane pops.  A step is uniform when all live lanes are at the same node.
Rays: the C3 table (32 x 2048) at the given poses of the bench trajectory (default 0 21 42 63).  No GPU, numpy only.

Output per tile shape (columns x lines x poses): uniform / divergent steps and leaf rounds per wave, lane use of the node
steps, waves whose rays point into more than one octant, and modelled vector instructions and per-lane vector loads per wave
(28 / 42 / 110 instructions -- the counts of the compiled product kernel -- and 0 / 2 / 6 loads per uniform step / divergent
step / leaf round).  "16x4 split" is the pipeline's grouping (csrc/lrc_device.h, tile_ray): lines above and below the horizon
grouped separately, by fours, then a pair, then an odd line.  The shapes that span two poses (rejected: DESIGN.md section 10)
pair each given pose with the one MODEL_POSE_STRIDE (default 1 = 4.8 cm) further along the bench trajectory."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import bench  # noqa: E402  (puts the package on sys.path)
from lidarcast import synth  # noqa: E402
from lidar import IndoorLidar  # noqa: E402

BINS, MAX_LEAF = 16, 4


def build_bvh(v, t):
    """Binned SAH over triangle centroids, iterative; returns child boxes (n,2,6), children (n,2) (leaf: ~(first << 3 | cnt)),
    and the triangle order."""
    tri = v[t]
    lo, hi = tri.min(1), tri.max(1)
    cen = (lo + hi) * 0.5
    order = np.arange(len(t))
    boxes, kids = [], []
    out_tris = []

    def area(a, b):
        d = np.maximum(b - a, 0.0)
        return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]

    def leaf(ids):
        first = len(out_tris)
        out_tris.extend(ids.tolist())
        return ~((first << 3) | len(ids))

    def split(ids):
        c = cen[ids]
        cl, ch = c.min(0), c.max(0)
        best = (np.inf, 0, None)
        for ax in range(3):
            if ch[ax] <= cl[ax]:
                continue
            b = np.minimum(((c[:, ax] - cl[ax]) / (ch[ax] - cl[ax]) * BINS).astype(np.int64), BINS - 1)
            cnt = np.bincount(b, minlength=BINS)
            blo = np.full((BINS, 3), np.inf)
            bhi = np.full((BINS, 3), -np.inf)
            np.minimum.at(blo, b, lo[ids])
            np.maximum.at(bhi, b, hi[ids])
            llo, lhi = np.minimum.accumulate(blo), np.maximum.accumulate(bhi)
            rlo, rhi = np.minimum.accumulate(blo[::-1])[::-1], np.maximum.accumulate(bhi[::-1])[::-1]
            nl = np.cumsum(cnt)
            cost = area(llo[:-1], lhi[:-1]) * nl[:-1] + area(rlo[1:], rhi[1:]) * (len(ids) - nl[:-1])
            cost[(nl[:-1] == 0) | (nl[:-1] == len(ids))] = np.inf
            k = int(np.argmin(cost))
            if cost[k] < best[0]:
                best = (cost[k], ax, b <= k)
        if best[2] is None:
            m = np.zeros(len(ids), bool)
            m[:len(ids) // 2] = True
            return m
        return best[2]

    # node 0 = root; explicit stack of (node index, ids)
    boxes.append(None)
    kids.append(None)
    work = [(0, order)]
    while work:
        ni, ids = work.pop()
        m = split(ids)
        sides = (ids[m], ids[~m])
        nb, nk = np.zeros((2, 6)), [0, 0]
        for s, sid in enumerate(sides):
            nb[s, :3], nb[s, 3:] = lo[sid].min(0), hi[sid].max(0)
            if len(sid) <= MAX_LEAF:
                nk[s] = leaf(sid)
            else:
                boxes.append(None)
                kids.append(None)
                nk[s] = len(boxes) - 1
                work.append((nk[s], sid))
        boxes[ni], kids[ni] = nb, nk
    return np.array(boxes), np.array(kids, dtype=np.int64), np.array(out_tris, dtype=np.int64)


def lockstep(o, d, groups, boxes, kids, tv, depth=64):
    """groups: (waves, 64) ray indices.  Returns per wave: uniform steps, divergent steps, leaf rounds, and per ray node steps."""
    W = groups.shape[0]
    ray = groups.reshape(-1)
    o, d = o[ray], d[ray]
    n = len(ray)
    wave = np.repeat(np.arange(W), 64)
    inv = 1.0 / np.where(np.abs(d) < 1e-30, np.copysign(1e-30, d), d)
    ref = np.zeros(n, np.int64)
    EMPTY = np.iinfo(np.int64).min
    sp = np.zeros(n, np.int64)
    stack = np.zeros((n, depth), np.int64)
    tbest = np.full(n, np.inf)
    done = np.zeros(n, bool)
    uni, div, rounds = np.zeros(W, np.int64), np.zeros(W, np.int64), np.zeros(W, np.int64)
    steps = np.zeros(n, np.int64)
    v0, e1, e2 = tv[:, 0], tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    while not done.all():
        inner = ~done & (ref >= 0)
        winner = np.zeros(W, bool)
        winner[wave[inner]] = True
        if inner.any():
            a = np.flatnonzero(inner)
            r = ref[a]
            # uniform: all live lanes of the wave at one node
            wmin = np.full(W, np.iinfo(np.int64).max)
            wmax = np.full(W, -1)
            np.minimum.at(wmin, wave[a], r)
            np.maximum.at(wmax, wave[a], r)
            u = winner & (wmin == wmax)
            uni += u
            div += winner & ~u
            steps[a] += 1
            b = boxes[r]                                              # (m, 2, 6)
            t0 = (b[:, :, :3] - o[a, None]) * inv[a, None]
            t1 = (b[:, :, 3:] - o[a, None]) * inv[a, None]
            tn = np.maximum(np.minimum(t0, t1).max(2), 0.0)
            tf = np.maximum(t0, t1).min(2)
            hit = (tn <= tf) & (tn <= tbest[a, None])
            k = kids[r]
            both = hit[:, 0] & hit[:, 1]
            first0 = tn[:, 0] <= tn[:, 1]
            nxt = np.where(hit[:, 0], k[:, 0], k[:, 1])
            nxt = np.where(both, np.where(first0, k[:, 0], k[:, 1]), nxt)
            far = np.where(first0, k[:, 1], k[:, 0])
            pb = a[both]
            stack[pb, sp[pb]] = far[both]
            sp[pb] += 1
            none = ~hit[:, 0] & ~hit[:, 1]
            pn = a[none]
            can = sp[pn] > 0
            sp[pn[can]] -= 1
            nxt[none] = EMPTY
            nn = np.flatnonzero(none)
            nxt[nn[can]] = stack[pn[can], sp[pn[can]]]
            ref[a] = nxt
        # waves with no lane at an inner node: the leaf phase, then every lane pops
        lw = ~winner
        lanes = np.flatnonzero(lw[wave] & ~done)
        if len(lanes):
            lr = ref[lanes]
            real = lr != EMPTY
            enc = np.where(real, ~lr, 0)
            first, cnt = enc >> 3, np.where(real, enc & 7, 0)
            wr = np.zeros(W, np.int64)
            np.maximum.at(wr, wave[lanes], (cnt + 1) // 2)
            rounds += wr
            for j in range(MAX_LEAF):
                m = cnt > j
                if not m.any():
                    break
                li, ti = lanes[m], first[m] + j
                p = np.cross(d[li], e2[ti])
                det = (e1[ti] * p).sum(1)
                ok = np.abs(det) > 0
                idet = 1.0 / np.where(ok, det, 1.0)
                s = o[li] - v0[ti]
                uu = (s * p).sum(1) * idet
                q = np.cross(s, e1[ti])
                vv = (d[li] * q).sum(1) * idet
                tt = (e2[ti] * q).sum(1) * idet
                ok &= (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (tt > 0) & (tt < tbest[li])
                tbest[li[ok]] = tt[ok]
            can = sp[lanes] > 0
            done[lanes[~can]] = True
            pl = lanes[can]
            sp[pl] -= 1
            ref[pl] = stack[pl, sp[pl]]
    return uni, div, rounds, steps


def groups_for(P, H, Wd, cols, lines):
    """(waves, 64) ray indices of tiles of cols x lines (cols * lines == 64) over P poses of H lines x Wd columns."""
    idx = np.arange(P * H * Wd).reshape(P, H // lines, lines, Wd // cols, cols)
    return idx.transpose(0, 1, 3, 2, 4).reshape(-1, 64)


def groups_split(P, H, Wd, lines, split):
    """The pipeline's line groups: runs [0, split) and [split, H) cut into groups of `lines` (4: then a pair, then an odd line)."""
    tiles = []
    for a, b in (((0, split), (split, H)) if 0 < split < H else ((0, H),)):
        line = a
        while line < b:
            g = 4 if (lines == 4 and b - line >= 4) else (2 if (lines >= 2 and b - line >= 2) else 1)
            tiles.append((np.arange(g * Wd).reshape(g, g * Wd // 64, 64 // g).transpose(1, 0, 2) + line * Wd).reshape(-1, 64))
            line += g
    one = np.concatenate(tiles)
    return (one[None] + (np.arange(P) * H * Wd)[:, None, None]).reshape(-1, 64)


def groups_pose_span(P, H, Wd, cols, lines):
    """Tiles of cols x lines x 2 adjacent poses (cols * lines * 2 == 64): poses (0, 1), (2, 3), ..."""
    idx = np.arange(P * H * Wd).reshape(P // 2, 2, H // lines, lines, Wd // cols, cols)
    return idx.transpose(0, 2, 4, 1, 3, 5).reshape(-1, 64)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else bench.SCENE
    sel = [int(a) for a in sys.argv[2:]] or [0, 21, 42, 63]
    mesh = synth.make_scene(name)
    v, t = np.asarray(mesh.vertices, np.float64), np.asarray(mesh.triangles, np.int64)
    print(f"scene {name}: {len(t)} triangles; building the model's tree ...", flush=True)
    boxes, kids, order = build_bvh(v, t)
    tv = v[t[order]]
    sensor = bench.c3_sensor()
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    stride = int(os.environ.get("MODEL_POSE_STRIDE", "1"))
    span = os.environ.get("MODEL_POSE_SPAN", "0") == "1"      # also the shapes over two poses: every pose with its partner
    if span:
        sel = [q for s_ in sel for q in (min(s_, 63 - stride), min(s_, 63 - stride) + stride)]
    poses = bench.c3_poses(0, 1)[sel]
    H, Wd = 32, len(dirs) // 32
    o = np.repeat(poses[:, :3, 3].astype(np.float32).astype(np.float64), len(dirs), axis=0)
    d = np.concatenate([(dirs @ p[:3, :3].T).astype(np.float32).astype(np.float64) for p in poses])
    octant = (d[:, 0] < 0) | ((d[:, 1] < 0) << 1) | ((d[:, 2] < 0) << 2)
    print("tile   uniform/wave  divergent/wave  leaf rounds/wave  lane use  mixed octants  model VALU/wave  vector loads/wave  node steps/ray")
    z = dirs[::Wd, 2]
    split = int(np.argmax((z < 0) != (z[0] < 0)))
    shapes = [("64x1", lambda: groups_for(len(poses), H, Wd, 64, 1)), ("32x2", lambda: groups_for(len(poses), H, Wd, 32, 2)),
              ("16x4", lambda: groups_for(len(poses), H, Wd, 16, 4)),
              (f"16x4 split {split}", lambda: groups_split(len(poses), H, Wd, 4, split))]
    if span:
        shapes += [("16x2x2", lambda: groups_pose_span(len(poses), H, Wd, 16, 2)), ("8x4x2", lambda: groups_pose_span(len(poses), H, Wd, 8, 4))]
    for label, make in shapes:
        g = make()
        uni, div, rounds, steps = lockstep(o, d, g, boxes, kids, tv)
        per_wave_steps = steps[np.arange(g.size)].reshape(-1, 64)
        use = per_wave_steps.sum() / ((uni + div).sum() * 64.0)
        mixed = (octant[g].min(1) != octant[g].max(1)).mean()
        valu = 28 * uni.mean() + 42 * div.mean() + 110 * rounds.mean()
        loads = 2 * div.mean() + 6 * rounds.mean()
        print(f"{label:14s} {uni.mean():12.1f} {div.mean():15.1f} {rounds.mean():17.2f} {use:9.3f} {mixed:13.2%} {valu:16.0f} "
              f"{loads:18.0f} {steps.mean():15.1f}", flush=True)


if __name__ == "__main__":
    main()
