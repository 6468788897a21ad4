"""numpy restatement of dynamic occupancy (csrc/lrc_voxseq.hip, include/lidarcast.h "dynamic occupancy").

The grid, the walk, the limits, the keys and the sem / ins vote are ``voxgrid_restate``'s, imported, not copied.  Added here:

Slots.  A sequence is F frame slots of one grid.  Ray (p, i), entry r = p*N + i, contributes iff t[r] is finite; its slot
is f = frame_of_pose[p].  A pose with f >= F contributes nothing and its returned rays are counted as ``skipped``.

Segments.  o = origins[p] (origin_per_ray False) or origins[r] (True), e = point3[r], both float32; labels sem[r], ins[r];
mover id mover[r] (None: all zero).

STATIC_ONLY.  A returned ray with mover id != 0 carves its free voxels as usual but records no return.

Mover vote, independent of the sem / ins vote: mover[v] = the most frequent mover id among all of v's returns, ties to the
smallest; mover_returns[v] = the number of v's returns with id != 0.

Outputs: per slot the sparse dict, state and counts of ``voxgrid_restate.finalize`` plus ``mover`` / ``mover_returns`` and the
slot's rejected rays; one sparse list ascending by (slot, idx) with ``frame_offsets``; ``skipped``.
"""
import numpy as np

import voxgrid_restate as vr


def mover_vote(idx, mover):
    """(idx ascending, mover, mover_returns) from per-return (idx, mover id)."""
    idx = np.asarray(idx, np.int64)
    mover = np.asarray(mover, np.int64)
    if len(idx) == 0:
        z = np.zeros(0, np.int64)
        return z, z, z
    out_idx, out_m, out_n = [], [], []
    for v in np.unique(idx):
        ids, c = np.unique(mover[idx == v], return_counts=True)      # ascending ids
        out_idx.append(v)
        out_m.append(ids[np.argmax(c)])                              # first maximum = smallest id
        out_n.append(c[ids != 0].sum())
    return np.array(out_idx), np.array(out_m), np.array(out_n)


def sequence_from_records(origins, origin_per_ray, frame_of_pose, t, point3, sem, ins, mover, F, origin, s, dims,
                          min_returns=1, static_only=False):
    """The whole definition.  origins (P, 3) or (P*N, 3) float32, frame_of_pose (P,), t (P*N,), point3 (P*N, 3), sem / ins
    (P*N,), mover (P*N,) or None.  Returns {"frames": [per-slot dict], "frame_offsets", "idx", "sem", "ins", "returns",
    "mover", "mover_returns", "state" (F, V), "counts" (F, 6) in the order of lrc_voxgrid_counts, "skipped", "free" (F, V)}."""
    dims = tuple(int(x) for x in dims)
    V = dims[0] * dims[1] * dims[2]
    t = np.asarray(t, np.float32).reshape(-1)
    fop = np.asarray(frame_of_pose, np.int64).reshape(-1)
    P = len(fop)
    N = len(t) // P
    assert P * N == len(t)
    e = np.asarray(point3, np.float32).reshape(-1, 3)
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    o = o if origin_per_ray else np.repeat(o, N, axis=0)
    assert len(o) == len(t) and len(e) == len(t)
    sem = np.asarray(sem, np.uint16).reshape(-1)
    ins = np.asarray(ins, np.uint16).reshape(-1)
    mv = np.zeros(len(t), np.uint8) if mover is None else np.asarray(mover, np.uint8).reshape(-1)
    slot = np.repeat(fop, N)
    returned = np.isfinite(t)
    skipped = int((returned & (slot >= F)).sum())
    labels = sem.astype(np.uint32) | (ins.astype(np.uint32) << 16)
    frames, cols = [], {k: [] for k in ("idx", "sem", "ins", "returns", "mover", "mover_returns")}
    offsets = [0]
    for f in range(F):
        sel = np.flatnonzero(returned & (slot == f))
        free, end, ok, _ = vr.walk(o[sel], e[sel], origin, s, dims)
        rec = ok & vr.inside(end, dims)
        if static_only:
            rec &= mv[sel] == 0
        ki = vr.linear(end[rec], dims)
        lab = labels[sel][rec]
        sparse, state, counts = vr.finalize(free, ki, (lab & 0xFFFF).astype(np.int64), (lab >> 16).astype(np.int64), dims,
                                            min_returns)
        mi, mm, mn = mover_vote(ki, mv[sel][rec])
        assert np.array_equal(mi, sparse["idx"].astype(np.int64))
        sparse["mover"] = mm.astype(np.uint8)
        sparse["mover_returns"] = mn.astype(np.uint32)
        counts["rejected_rays"] = int((~ok).sum())
        frames.append({"sparse": sparse, "state": state, "counts": counts, "free": free})
        for k in cols:
            cols[k].append(sparse[k])
        offsets.append(offsets[-1] + len(sparse["idx"]))
    out = {k: np.concatenate(v) for k, v in cols.items()}
    out["frames"] = frames
    out["frame_offsets"] = np.array(offsets, np.uint64)
    out["state"] = np.stack([fr["state"] for fr in frames])
    out["free"] = np.stack([fr["free"] for fr in frames])
    out["counts"] = np.array([[c["num_sparse"], c["free"], c["occupied"], c["unknown"], c["rejected_rays"], c["returns"]]
                              for c in (fr["counts"] for fr in frames)], np.uint64)
    out["skipped"] = skipped
    return out


def pack_bits(free, V):
    """(F, V) bool -> (F * ceil(V/32),) uint32, each slot starting on a word boundary, least significant bit first."""
    free = np.asarray(free, bool).reshape(-1, V)
    W = (V + 31) // 32
    pad = np.zeros((free.shape[0], W * 32), bool)
    pad[:, :V] = free
    return np.packbits(pad.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def hostile_segments(seed=5, n=4096, origin=(-0.5, 0.25, -1.0), s=0.25, dims=(5, 7, 33)):
    """The segment set of the voxseq tests on dims (5, 7, 33) (V = 1155 is no multiple of 32 and z crosses a word): random
    segments in and around the grid, then starts outside, a == b, axis-parallel segments, segments through voxel corners
    (exact ties), a NaN end and coordinates beyond 2^31 voxels.  Returns (o, e) float32 (n, 3)."""
    rng = np.random.default_rng(seed)
    g = np.asarray(origin, np.float64)
    ext = np.asarray(dims, np.float64) * s
    o = (g + rng.uniform(-0.2, 1.2, (n, 3)) * ext).astype(np.float32)
    e = (g + rng.uniform(-0.2, 1.2, (n, 3)) * ext).astype(np.float32)
    k = 0
    # starts well outside the grid, ends inside
    o[k:k + 64] = (g + rng.uniform(-3.0, -1.0, (64, 3)) * ext).astype(np.float32); k += 64
    # a == b: the end in the start's voxel, and the very same point
    e[k:k + 32] = o[k:k + 32]; k += 32
    c = np.floor((o[k:k + 32].astype(np.float64) - g) / s)
    o[k:k + 32] = (g + (c + 0.25) * s).astype(np.float32)
    e[k:k + 32] = (g + (c + 0.75) * s).astype(np.float32); k += 32
    # axis-parallel segments, both directions
    for ax in range(3):
        e[k:k + 48] = o[k:k + 48]
        e[k:k + 48, ax] = (g[ax] + rng.uniform(-0.2, 1.2, 48) * ext[ax]).astype(np.float32); k += 48
    # through voxel corners: origin and voxel size are dyadic, so every product is exact -> exact ties on two or three axes
    ci = rng.integers(-1, 8, (96, 3)).astype(np.float64)
    di = rng.integers(1, 6, (96, 1)).astype(np.float64) * rng.choice([-1.0, 1.0], (96, 3))
    di[32:64, 2] = 0.0                                  # ties on x and y only
    o[k:k + 96] = (g + (ci + 0.5) * s).astype(np.float32)
    e[k:k + 96] = (g + (ci + 0.5 + di) * s).astype(np.float32); k += 96
    # NaN / inf ends and starts
    e[k, 1] = np.nan; k += 1
    e[k, 0] = np.inf; k += 1
    o[k, 2] = np.nan; k += 1
    # coordinates beyond 2^31 voxels (and a walk of 2^24 steps or more)
    e[k] = (3.0e9 * s, 0.0, 0.0); k += 1
    o[k] = (0.0, -3.0e9 * s, 0.0); k += 1
    e[k] = (g[0] + 2.0 ** 25 * s, 0.3, 0.3); k += 1
    assert k < n
    return o, e


# ---- the analytic mover scene of the voxseq tests --------------------------------------------------------------------------------

def box_mesh(lo, hi, sem, ins):
    """A closed 12-triangle axis-aligned box as a ``lidarcast.synth.TriangleMesh`` with one label on every triangle."""
    from lidarcast import synth
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float64)
    t = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], np.int32)
    return synth.TriangleMesh(vertices=v, triangles=t, triangle_sem=np.full(12, sem, np.uint16),
                              triangle_ins=np.full(12, ins, np.uint16))


def sphere_dirs(n):
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    r = np.sqrt(1 - z * z)
    phi = i * np.pi * (3 - np.sqrt(5))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def analytic_scene():
    """A closed 4 x 4 x 3 m box room (sem 2, ins 7) and a 0.5 m cube mover (sem 13, ins 1001) around its own origin; voxel 0.1
    with the grid origin at -0.25, so every multiple of 0.1 is a voxel CENTRE:
    the walls, the sensor, the cube's faces and the two hit points on the +x axis all sit at voxel centres, nothing the
    assertions look at lies on a voxel face.  Row 0 of the table is exactly +x, then 1023 sphere directions.  Two frames, the
    sensor at (1.0, 2.2, 1.5) in both: frame 0 has the cube's near face on the +x axis 1 m from the sensor (centre (2.25, 2.35,
    1.55): the axis ray meets the face off its diagonal), frame 1 has the cube 1.5 m to the side (y = 0.85).  The axis ray
    meets the wall x = 4 at (4.0, 2.2, 1.5), off that wall's diagonals."""
    room = box_mesh((0, 0, 0), (4, 4, 3), 2, 7)
    cube = box_mesh((-0.25,) * 3, (0.25,) * 3, 13, 1001)
    pose = np.eye(4)
    pose[:3, 3] = (1.0, 2.2, 1.5)
    poses = np.stack([pose, pose])
    mp = np.zeros((2, 1, 3, 4), np.float32)
    mp[:, 0, :, :3] = np.eye(3)
    mp[0, 0, :, 3] = (2.25, 2.35, 1.55)
    mp[1, 0, :, 3] = (2.25, 0.85, 1.55)
    dirs = np.concatenate([[[1.0, 0.0, 0.0]], sphere_dirs(1023)])
    return {"room": room, "cube": cube, "poses": poses, "mover_poses": mp.reshape(2, 1, 12), "dirs": dirs,
            "origin": (-0.25, -0.25, -0.25), "voxel": 0.1, "dims": (45, 45, 35), "max_range": 20.0}


def axis_voxels(sc):
    """Linear indices of the +x axis voxels of ``analytic_scene``: (between sensor and cube, the cube's near-face voxel, behind
    the cube up to the wall, the wall voxel).  The sensor's own voxel is left out (a == b for nothing, but it is not 'between')."""
    dims = sc["dims"]
    g, s = np.asarray(sc["origin"]), sc["voxel"]
    j, k = int(np.floor((2.2 - g[1]) / s)), int(np.floor((1.5 - g[2]) / s))
    ix = lambda x: int(np.floor((x - g[0]) / s))          # noqa: E731
    lin = lambda i: (i * dims[1] + j) * dims[2] + k      # noqa: E731
    sensor, near, wall = ix(1.0), ix(2.0), ix(4.0)
    return ([lin(i) for i in range(sensor + 1, near)], lin(near), [lin(i) for i in range(near + 1, wall)], lin(wall))


def assert_axis(sc, state, sparse_of, static_state, static_sparse):
    """The assertions of the analytic scene.  ``state`` (2, V) per-frame states, ``sparse_of(f)`` -> {idx: (sem, ins, mover)} of
    frame f's sparse entries, and the same for the static map."""
    between, near, behind, wall = axis_voxels(sc)
    assert len(between) == 9 and len(behind) == 19
    for f in (0, 1):
        assert (state[f][between] == vr.FREE).all(), f                          # between sensor and cube: free in both frames
    assert state[0][near] == vr.OCCUPIED and sparse_of(0)[near] == (13, 1001, 1)   # the near face: the mover, in frame 0
    assert state[1][near] == vr.FREE                                             # ... and free once it stepped aside
    assert (state[0][behind] == vr.UNKNOWN).all()                                # the cube's shadow
    assert (state[1][behind] == vr.FREE).all()
    assert state[0][wall] == vr.UNKNOWN                                          # the wall in the shadow
    assert state[1][wall] == vr.OCCUPIED and sparse_of(1)[wall] == (2, 7, 0)
    assert static_state[near] != vr.OCCUPIED and static_state[wall] == vr.OCCUPIED
    assert near not in static_sparse and static_sparse[wall] == (2, 7, 0)


def analytic_records_on_cpu(sc):
    """The records of the analytic scene without a GPU: the oracle casts the room and, through lrc_mover_rays, the cube in its
    own frame; lrc_mover_merge picks the winner; the end point is o + (d/|d|) * t in float32.  Returns the dict
    ``sequence_from_records`` takes (origins, t, point3, sem, ins, mover)."""
    from lidarcast import movers
    from oracle.c_oracle import OracleMesh
    room, cube = sc["room"], sc["cube"]
    om_room = OracleMesh(room.vertices, room.triangles).build()
    om_cube = OracleMesh(cube.vertices, cube.triangles).build()
    d = sc["dirs"].astype(np.float32)
    d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    N = len(d)
    out = {k: [] for k in ("t", "point3", "sem", "ins", "mover")}
    origins = sc["poses"][:, :3, 3].astype(np.float32)
    for p in range(len(sc["poses"])):
        rays = np.concatenate([np.repeat(origins[p][None], N, 0), d], 1).astype(np.float32)
        ts, _ = om_room.cast(rays)
        tm, _ = om_cube.cast(movers.rays(rays, sc["mover_poses"][p, 0]))
        z3 = np.zeros((N, 3), np.float32)
        t, _, who = movers.merge(ts, z3, tm[None], z3[None], sc["mover_poses"][p])
        hit = np.isfinite(t)
        out["t"].append(t)
        out["point3"].append(np.where(hit[:, None], rays[:, :3] + d * np.where(hit, t, 0)[:, None], 0).astype(np.float32))
        out["sem"].append(np.where(hit, np.where(who == 1, 13, 2), 0).astype(np.uint16))
        out["ins"].append(np.where(hit, np.where(who == 1, 1001, 7), 0).astype(np.uint16))
        out["mover"].append(np.where(hit, who, 0).astype(np.uint8))
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["origins"] = origins
    return out
