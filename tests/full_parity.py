"""What a WHOLE scan must return, stated with the oracle alone, and one comparator that says where a difference sits.

The sampled full-size tests compared a handful of poses ray by ray; a fault that depends on where a tile sits in the launch
(the tile-group remap, the leading workgroups that scatter an earlier scan's rows, a pose whose tiles straddle a super
tile, the last partial tile group) can hide in the poses nobody looked at.  ``expected_scan`` casts every ray of every pose
in ONE ``OracleMesh.cast`` call and applies the reference's post-processing (oracle/np_oracle.py: float32 hit point from
the normalised direction, strict float64 range filter around the pose's centre) to all of them at once;
``assert_scan_equal`` compares every array bit for bit and names the first differing pose, tile and lane.

Only oracle/ and numpy compute here (the rays of a sensor come from the package's host generator, lidar.create_lidar, the
restated reference generator that np_oracle.lidar_intersect_mesh itself calls).  tests/test_full_parity_host.py pins the
result against np_oracle.lidar_intersect_mesh pose by pose and against OracleMesh.brute, and shows that the comparator sees
each kind of defect.  Everything is a pure function of its arguments."""
import functools

import numpy as np

MISS = 0xFFFFFFFF
RECORDS = ("t", "prim", "point3", "normal3", "sem", "ins")      # the fixed-stride records, (P*N, ...) each
CLOUD = ("counts", "rows")                                      # per-pose kept counts, compacted (x, y, z, label) rows
_DTYPES = {"t": np.float32, "prim": np.uint32, "point3": np.float32, "normal3": np.float32, "sem": np.uint16,
           "ins": np.uint16, "counts": np.int64, "rows": np.float32}
THREADS = 16


def sensor_rays(sensor, poses):
    """(P*N, 6) float32 world rays of a multi-line sensor at P poses, pose after pose, and the (P, 3) float64 centres."""
    from lidar import create_lidar
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    rays = np.concatenate([create_lidar(sensor, m).get_rays() for m in poses])
    return rays, poses[:, :3, 3].copy()


def pack_labels(sem, ins):
    """sem | ins << 16 as the float32 bit pattern the 16-byte rows carry in their fourth column."""
    return (np.asarray(sem).astype(np.uint32) | (np.asarray(ins).astype(np.uint32) << 16)).view(np.float32)


def expected_scan(om, rays, centres, max_range, num_poses, tri_sem=None, tri_ins=None, threads=THREADS):
    """Everything a scan of ``num_poses`` poses x N rays must return.

    om        an oracle.c_oracle.OracleMesh (its tree is built once and kept)
    rays      (P*N, 6) float32, pose after pose
    centres   range-filter centres, float64: (P, 3) one per pose, or (P*N, 3) one per ray (moving-sensor sweeps)
    tri_sem / tri_ins   per-triangle labels (None: zeros)

    Returns a dict: P, N; the records t (+inf on a miss or beyond range), prim (0xFFFFFFFF there), point3, normal3, sem,
    ins (all zero there), flat over P*N rays; keep (P*N,) bool; counts (P,) int64; rows (K, 4) float32 in pose order."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    P = int(num_poses)
    n = len(rays)
    assert rays.ndim == 2 and rays.shape[1] == 6 and P > 0 and n % P == 0, (rays.shape, P)
    N = n // P
    cen = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    assert len(cen) in (P, n), (len(cen), P, n)
    if len(cen) == P and N != 1:
        cen = np.repeat(cen, N, axis=0)
    t, prim = om.cast(rays, threads=threads)
    hit = t != np.inf                                                 # raycast_engine_cpu.py:54
    o, d = rays[:, :3], rays[:, 3:]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)                  # :57  float32
    point = np.zeros_like(o)
    point[hit] = o[hit] + d[hit] * t[hit, None]                       # :60-62  mul then add, float32
    dist = np.linalg.norm(point - cen, axis=1)                        # :95-96  float64
    keep = hit & (dist < float(max_range))                            # :97  strict
    del dist, cen, d
    t = np.where(keep, t, np.float32(np.inf)).astype(np.float32)
    prim = np.where(keep, prim, np.uint32(MISS)).astype(np.uint32)
    point[~keep] = 0.0
    normal = om.normals(prim)                                         # zero for a miss
    sem = np.zeros(n, np.uint16)
    ins = np.zeros(n, np.uint16)
    k = prim[keep]
    if tri_sem is not None:
        sem[keep] = np.asarray(tri_sem, dtype=np.uint16)[k]
    if tri_ins is not None:
        ins[keep] = np.asarray(tri_ins, dtype=np.uint16)[k]
    rows = np.empty((int(keep.sum()), 4), np.float32)
    rows[:, :3] = point[keep]
    rows[:, 3] = pack_labels(sem[keep], ins[keep])
    return {"P": P, "N": N, "t": t, "prim": prim, "point3": point, "normal3": normal, "sem": sem, "ins": ins,
            "keep": keep, "counts": keep.reshape(P, N).sum(1).astype(np.int64), "rows": rows}


def expected_sensor_scan(om, mesh, sensor, poses, max_range=None, threads=THREADS):
    """``expected_scan`` for a multi-line sensor at ``poses`` over ``mesh`` (its per-triangle labels, when it has them)."""
    rays, cen = sensor_rays(sensor, poses)
    return expected_scan(om, rays, cen, sensor.max_range if max_range is None else max_range, len(cen),
                         getattr(mesh, "triangle_sem", None), getattr(mesh, "triangle_ins", None), threads)


def frames(want):
    """Per pose (surviving ray indices, points, sem, ins): what the frame-producing entry points return for pose p."""
    P, N = want["P"], want["N"]
    ends = np.cumsum(want["counts"])
    keep = want["keep"].reshape(P, N)
    for p in range(P):
        r = want["rows"][ends[p] - want["counts"][p]:ends[p]]
        lab = r[:, 3].copy().view(np.uint32)
        yield np.flatnonzero(keep[p]), r[:, :3], (lab & 0xFFFF).astype(np.uint16), (lab >> 16).astype(np.uint16)


# ---- the comparator -------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _where(i, N):
    i = int(i)
    return f"pose {i // N}, tile {(i % N) // 64} of the pose (tile {i // 64} of the scan), lane {i % 64} (ray {i % N})"


def differences(got, want, fields):
    """(number of rays that differ, list of messages).  A ray differs when any compared record field of it differs, or a
    compacted row made from it does, or -- counted against the pose's first ray -- its pose's count does."""
    P, N = want["P"], want["N"]
    n = P * N
    bad = np.zeros(n, bool)
    msgs = []
    for f in fields:
        if f not in _DTYPES:
            raise KeyError(f"unknown field {f!r}")
        if f not in got:
            raise KeyError(f"the result under test has no {f!r}")
        g, w = np.asarray(got[f]), want[f]
        if g.dtype != _DTYPES[f]:
            msgs.append(f"{f}: dtype {g.dtype}, expected {np.dtype(_DTYPES[f])}")
            bad[:] = True
            continue
        if f in RECORDS:
            if g.size != w.size:
                msgs.append(f"{f}: {g.size} values, expected {w.size}")
                bad[:] = True
                continue
            ne = _bits(g).reshape(n, -1) != _bits(w).reshape(n, -1)
            ne = ne.any(1)
            if ne.any():
                i = int(np.argmax(ne))
                msgs.append(f"{f}: {int(ne.sum())} of {n} rays differ; first at {_where(i, N)}: "
                            f"got {g.reshape(n, -1)[i].tolist()}, expected {w.reshape(n, -1)[i].tolist()}")
                bad |= ne
        elif f == "counts":
            g = g.reshape(-1)
            if g.shape != w.shape:
                msgs.append(f"counts: {g.size} poses, expected {P}")
                bad[:] = True
                continue
            ne = g != w
            if ne.any():
                p = int(np.argmax(ne))
                msgs.append(f"counts: {int(ne.sum())} of {P} poses differ; first at pose {p}: got {int(g[p])}, "
                            f"expected {int(w[p])}")
                bad[np.flatnonzero(ne) * N] = True
        else:                                   # rows: the first K against the oracle's, whatever follows against `fill`
            K = len(w)
            g = g.reshape(-1, 4)
            if len(g) < K:
                msgs.append(f"rows: {len(g)} rows, expected at least {K}")
                bad[:] = True
                continue
            ne = (_bits(g[:K]) != _bits(w)).any(1)
            if ne.any():
                src = np.flatnonzero(want["keep"])             # row r was made from ray src[r]
                r = int(np.argmax(ne))
                msgs.append(f"rows: {int(ne.sum())} of {K} kept rows differ; first at row {r}, made from "
                            f"{_where(src[r], N)}: got {_bits(g[r]).tolist()}, expected {_bits(w[r]).tolist()} (bits)")
                bad[src[ne]] = True
            if len(g) > K:
                if "fill" not in got:
                    raise KeyError("rows beyond the kept ones need got['fill'], the value the buffer was filled with")
                touched = (_bits(g[K:]) != _bits(np.float32(got["fill"]))).any(1)
                if touched.any():
                    r = K + int(np.argmax(touched))
                    msgs.append(f"rows: {int(touched.sum())} rows beyond the {K} kept ones were written; first at row {r}")
                    bad[min(r, n - 1)] = True
    return int(bad.sum()), msgs


def assert_scan_equal(got, want, what, fields=RECORDS + CLOUD):
    """Bit equality of every field in ``fields`` between the result under test and ``expected_scan``'s.  ``got`` holds the
    same keys (records flat or (P, N, ...); ``rows`` may be the caller's whole buffer, then ``got['fill']`` is the value it
    was filled with and the rows beyond the kept ones must still hold it).  Returns the number of rays compared."""
    n_bad, msgs = differences(got, want, fields)
    assert not msgs, f"{what}: {n_bad} of {want['P'] * want['N']} rays differ\n  " + "\n  ".join(msgs)
    return want["P"] * want["N"]


def report(what, want, differ=0, rays=None):
    """The one line every full-size comparison prints: rays compared, kept share, rays that differ."""
    n = want["P"] * want["N"] if rays is None else rays
    line = f"[full parity] {what}: rays compared {n}, kept share {want['keep'].mean():.5f}, rays that differ {differ}"
    print("\n" + line)
    return line


# ---- shared full-size fixtures (computed once per process) ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_and_oracle(name):
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    mesh = synth.make_scene(name)
    return mesh, OracleMesh(mesh.vertices, mesh.triangles).build()


@functools.lru_cache(maxsize=1)
def c3_expected():
    """BASELINE config C3: bench.SCENE, bench.c3_sensor(), bench.c3_poses(0, 1) -- all 64 x 65 536 rays."""
    import bench
    mesh, om = scene_and_oracle(bench.SCENE)
    return expected_sensor_scan(om, mesh, bench.c3_sensor(), bench.c3_poses(0, 1))
