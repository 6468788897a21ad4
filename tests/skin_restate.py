"""The skinning arithmetic of csrc/lrc_skin.h restated in numpy, op for op (float32 arrays: one rounding per operation), and the
rigs the skin tests share.  A plain helper of tests/test_skin_host.py and tests/test_skin_gpu.py."""
import numpy as np

F = np.float32


def skin_restate(rest, idx, wgt, bones):
    """With m = bones[idx[j]]: p_j.i = ((m[4i] x + m[4i+1] y) + m[4i+2] z) + m[4i+3], all four influences in index order;
    v.i = ((w0 p_0.i + w1 p_1.i) + w2 p_2.i) + w3 p_3.i."""
    rest, wgt, bones = np.asarray(rest, F), np.asarray(wgt, F), np.asarray(bones, F).reshape(-1, 12)
    m = bones[np.asarray(idx, np.int64)]                      # (V, 4, 12)
    x, y, z = rest[:, 0:1], rest[:, 1:2], rest[:, 2:3]
    out = np.empty((len(rest), 3), F)
    for i in range(3):
        p = ((m[:, :, 4 * i] * x + m[:, :, 4 * i + 1] * y) + m[:, :, 4 * i + 2] * z) + m[:, :, 4 * i + 3]
        assert p.dtype == F
        out[:, i] = ((wgt[:, 0] * p[:, 0] + wgt[:, 1] * p[:, 1]) + wgt[:, 2] * p[:, 2]) + wgt[:, 3] * p[:, 3]
    return out


def affine_poses(rng, K, B, spread=0.2, shift=0.3):
    """(K, B, 12) float32 affine maps near the identity: no two alike, none orthonormal."""
    p = np.zeros((K, B, 3, 4))
    p[..., :3] = np.eye(3) + rng.normal(0.0, spread, (K, B, 3, 3))
    p[..., 3] = rng.normal(0.0, shift, (K, B, 3))
    return p.reshape(K, B, 12).astype(F)


def random_influences(rng, V, B, counts=(1, 2, 3, 4)):
    """(V, 4) uint8 indices below B and (V, 4) float32 weights: row v has counts[v % len(counts)] non-zero weights in its first
    places, the rest +0, and sums to 1 within a few float32 ulps."""
    idx = rng.integers(0, B, (V, 4)).astype(np.uint8)
    w = rng.uniform(0.1, 1.0, (V, 4))
    n = np.asarray(counts)[np.arange(V) % len(counts)]
    w[np.arange(4)[None, :] >= n[:, None]] = 0.0
    w /= w.sum(1, keepdims=True)
    return idx, w.astype(F)


def strip_mesh(V):
    """A bent zig-zag triangle strip of V vertices (V - 2 triangles) along x: (rest (V, 3) float32, triangles int32)."""
    i = np.arange(V)
    rest = np.stack([(5.0 / V) * i, (i % 2) * 0.5, 0.3 * np.sin(28.0 / V * i)], 1).astype(F)
    t = np.array([(j, j + 1, j + 2) if j % 2 == 0 else (j + 1, j, j + 2) for j in range(V - 2)], np.int32)
    return rest, t


def rig(name):
    """{rest, tris, idx, wgt, poses, sem, ins} of a named rig: "walker", "walker_smooth", "tetra" (B = 1: the wrapped single
    leaf), "strip<V>" (B = 3, K = 3, random four-influence weights), "strip<V>b255" (B = 255, K = 2) and "strip<V>k64"."""
    from lidarcast import synth
    rng = np.random.default_rng(23)
    if name in ("walker", "walker_smooth"):
        m = synth.make_walker_rig(smooth=0.08 if name == "walker_smooth" else 0.0, instance=1001)
        return dict(rest=m.vertices.astype(F), tris=np.asarray(m.triangles, np.int32), idx=m.bone_index, wgt=m.bone_weight,
                    poses=m.poses12, sem=m.triangle_sem, ins=m.triangle_ins)
    if name == "tetra":
        rest = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64) - 0.25).astype(F)
        t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
        idx, wgt = np.zeros((4, 4), np.uint8), np.tile(np.array([1, 0, 0, 0], F), (4, 1))
        poses = affine_poses(rng, 3, 1)
    else:
        body = name[5:]
        if body.endswith("b255"):
            V, B, K = int(body[:-4]), 255, 2
        elif body.endswith("k64"):
            V, B, K = int(body[:-3]), 3, 64
        else:
            V, B, K = int(body), 3, 3
        rest, t = strip_mesh(V)
        idx, wgt = random_influences(rng, V, B)
        if B == 255:
            idx[:255, 1] = np.arange(255)              # every bone of the largest table is read, the last one included
        poses = affine_poses(rng, K, B)
    return dict(rest=rest, tris=t, idx=idx, wgt=wgt, poses=poses, sem=np.full(len(t), 12, np.uint16),
                ins=(np.arange(len(t)) % 7 + 1).astype(np.uint16))
