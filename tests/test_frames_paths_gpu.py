"""-m gpu: every frame column, through every copy path of frames_finish (csrc/lidarcast.hip), for every ray generator.

frames_finish has one small-call path (one stream, worst-case copies, one synchronisation) and a chunked path whose chunks
are graded (4/32, 16/32, 32/32 of the poses), four equal ones, one per pose, or a single one.  Each shape below is the
smallest that selects its path; the number of trace launches the call makes (lrc_scene_get_counters) shows that it did.
All seven compacted columns and all four per-pose statistics are asked for at once and compared bit for bit with the
fixed-stride records of the same scan (lrc_scan_poses, or the generator's *_dev entry point) compacted in numpy with the
keep rule of tests/full_parity.py (a record is kept when its t is not +inf); the statistics with np.mean / np.std over
the segments of tests/stats_shapes.py, as tests/test_stats_shapes_gpu.py does."""
import ctypes as C

import numpy as np
import pytest

import stats_shapes as ss
from helpers import assert_bit_equal, pose, table_rays

pytestmark = pytest.mark.gpu

COLUMNS = ("point3", "sem", "ins", "incident_deg", "index", "xyzl", "range_origin")
WANT = COLUMNS + ("range_origin_stats", "incident_stats")
RECORDS = ("t", "point3", "sem", "ins", "incident_deg")
STATS = ("range_origin_mean", "range_origin_std", "incident_mean", "incident_std")

# name: (P, lines, width, extra rows of the table, trace launches of the call).  48 bytes per row with all seven columns.
SHAPES = {
    "one_stream": (3, 16, 256, 0, 1),           # P * N * 48 <= 4 MB
    "equal4": (4, 64, 4096, 0, 4),              # P * N = 2^20, P < 8: four equal chunks
    "graded": (8, 32, 4096, 0, 3),              # P * N = 2^20, P >= 8: poses [0, 1), [1, 4), [4, 8)
    "per_pose": (2, 128, 4096, 0, 2),           # P * N = 2^20, P < 4: one pose per chunk
    "odd_single": (8, 32, 4096, 1, 1),          # N = 131073: P * N >= 2^20 but N % 64 != 0: a single chunk
}
GENERATORS = ("poses", "table", "grid", "sweeps", "noisy", "angles", "rays")
CASES = [("poses", s) for s in SHAPES] + [(g, s) for g in GENERATORS[1:] for s in ("one_stream", "graded")]
ROOM = (4.0, 3.0, 2.5)
MAX_RANGE = 2.2          # cuts the far walls off: every pose keeps a part of its rays, none all of them


@pytest.fixture(scope="module")
def room():
    import lidarcast
    from lidarcast import synth
    mesh = synth.make_room(size=ROOM, num_boxes=4, seed=5, cell=0.05)
    ctx = lidarcast.Context(0)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    yield scene
    scene.close()
    ctx.close()


def _poses(P):
    return np.stack([pose(1.2 + 1.6 * i / max(P - 1, 1), 1.5 + 0.1 * (i % 3), 1.1, 0.4 * i) for i in range(P)])


def _table(lines, width, extra):
    from lidar import IndoorLidar
    d = IndoorLidar.directions_from_vertical_degrees(list(np.linspace(25.0, -35.0, lines)), width)
    return np.ascontiguousarray(np.concatenate([d, d[:extra]]), dtype=np.float64)


def _mask(P, N, seed):
    return np.random.default_rng([seed, P, N]).random((P, N)) < 0.8


def _dev_records(n, launch):
    import torch
    from lidarcast import DeviceHits
    hits = DeviceHits(n, "cuda", want=RECORDS)
    launch(hits, lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    torch.cuda.synchronize()
    out = {k: hits[k].cpu().numpy() for k in RECORDS}
    out["sem"], out["ins"] = out["sem"].view(np.uint16), out["ins"].view(np.uint16)
    return out


def _inputs(gen, shape):
    P, lines, width, extra, _ = SHAPES[shape]
    poses, dirs = _poses(P), _table(lines, width, extra)
    N = len(dirs)
    a = {"P": P, "N": N, "poses": poses, "dirs": dirs}
    if gen == "grid":
        a["grid"] = (lines, width, np.pi, -2 * np.pi / width)
    if gen == "sweeps":
        from lidarcast import motion_records
        ends = np.stack([pose(m[0, 3] + 0.04, m[1, 3] - 0.02, m[2, 3], 0.4 * i + 0.08) for i, m in enumerate(poses)])
        a["motion"], a["fire"] = motion_records(poses, ends), (np.arange(N) % width) / width
    if gen == "noisy":
        from lidarcast.noise import NoiseModel
        a["model"] = NoiseModel(seed=0xC0FFEE123456789, range_std=0.02, angle_std=0.002, dropout=0.05, first_frame=5)
    if gen == "angles":
        rng = np.random.default_rng([11, P, N])
        a["angles"] = np.stack([rng.uniform(0.0, 2 * np.pi, (P, N)), rng.uniform(-0.6, 0.45, (P, N))], axis=2)
        a["keep"] = _mask(P, N, 12)
    if gen == "rays":
        rays, cen = table_rays(dirs, poses)
        a["rays"], a["centers"], a["keep"] = rays.reshape(P, N, 6), cen, _mask(P, N, 13)
    return a


def _records(scene, gen, a):
    """The fixed-stride records of the scan, and the host-side keep mask (None: every ray is cast)."""
    P, N, n = a["P"], a["N"], a["P"] * a["N"]
    p16 = a["poses"].reshape(P, 16)
    if gen in ("poses", "table", "grid"):
        return scene.scan_poses(a["poses"], a["dirs"], MAX_RANGE, want=RECORDS), None
    if gen == "sweeps":
        return _dev_records(n, lambda h, up: scene.scan_sweeps_dev(up(a["motion"]), up(a["dirs"]), up(a["fire"]), h, MAX_RANGE)), None
    if gen == "noisy":
        return _dev_records(n, lambda h, up: scene.scan_noisy_dev(up(p16), up(a["dirs"]), h, MAX_RANGE, a["model"])), None
    if gen == "angles":
        k8 = a["keep"].view(np.uint8)
        return _dev_records(n, lambda h, up: scene.scan_angles_dev(up(p16), up(a["angles"]), up(k8), h, MAX_RANGE)), None
    off = np.arange(0, n + 1, N, dtype=np.uint64)        # rays: the explicit-ray cast has no mask, the host applies it
    return scene.cast_segments(a["rays"].reshape(-1, 6), off, a["centers"], MAX_RANGE, want=RECORDS), a["keep"]


def _host_frames(rec, mask, P, N):
    """What the frame-producing entry point must return: the records compacted on the host."""
    keep = (rec["t"] != np.inf).reshape(P, N)
    if mask is not None:
        keep &= mask
    sel = keep.reshape(-1)
    pts = rec["point3"][sel]
    counts = keep.sum(1).astype(np.int64)
    out = {"counts": counts, "total": int(counts.sum()), "point3": pts, "sem": rec["sem"][sel], "ins": rec["ins"][sel],
           "incident_deg": rec["incident_deg"][sel], "index": np.nonzero(keep)[1].astype(np.uint32),
           "range_origin": np.linalg.norm(pts, axis=1)}
    xyzl = np.empty((len(pts), 4), np.float32)
    xyzl[:, :3] = pts
    xyzl[:, 3] = (out["sem"].astype(np.uint32) | (out["ins"].astype(np.uint32) << 16)).view(np.float32)
    out["xyzl"] = xyzl
    off = ss.offsets(counts)
    for col, v in (("range_origin", out["range_origin"]), ("incident", out["incident_deg"])):
        for kind, fn in (("mean", np.mean), ("std", np.std)):
            out[f"{col}_{kind}"] = np.array([fn(v[off[i]:off[i + 1]]) if counts[i] else 0 for i in range(P)], dtype=v.dtype)
    return out


_REFERENCES = {}


def _reference(scene, gen, shape):
    """(inputs, expected frames) of a case: computed once, shared by the tests of the case, never written to."""
    slot = _REFERENCES.setdefault((gen, shape), {})
    if not slot:
        a = _inputs(gen, shape)
        rec, mask = _records(scene, gen, a)
        slot["a"], slot["want"] = a, _host_frames(rec, mask, a["P"], a["N"])
        for v in slot["want"].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return slot["a"], slot["want"]


def _compact(scene, gen, a, capacity=None):
    if gen == "poses":
        return scene.scan_poses_compact(a["poses"], a["dirs"], MAX_RANGE, want=WANT, capacity=capacity)
    if gen == "grid":
        return scene.scan_poses_compact(a["poses"], a["dirs"], MAX_RANGE, want=WANT, capacity=capacity, grid=a["grid"])
    if gen == "angles":
        return scene.scan_angles_compact(a["poses"], a["angles"], a["keep"], MAX_RANGE, want=WANT, capacity=capacity)
    if gen == "rays":
        return scene.scan_rays_compact(a["rays"], a["keep"], a["centers"], MAX_RANGE, want=WANT, capacity=capacity)
    from lidarcast import DirectionTable
    table = DirectionTable(scene.ctx, a["dirs"], a.get("fire"))
    try:
        if gen == "table":
            return scene.scan_poses_compact(a["poses"], table, MAX_RANGE, want=WANT, capacity=capacity)
        if gen == "sweeps":
            return scene.scan_sweeps_compact(a["motion"], table, None, MAX_RANGE, want=WANT, capacity=capacity)
        return scene.scan_noisy_compact(a["poses"], table, MAX_RANGE, a["model"], want=WANT, capacity=capacity)
    finally:
        table.close()


@pytest.mark.parametrize("gen,shape", CASES, ids=[f"{g}-{s}" for g, s in CASES])
def test_every_column_on_every_path(room, gen, shape):
    a, want = _reference(room, gen, shape)
    P, N = a["P"], a["N"]
    before = room.counters()[0]
    fr = _compact(room, gen, a)
    launches = room.counters()[0] - before
    share = want["total"] / (P * N)
    print(f"\n[frames paths] {gen} {shape}: P {P} N {N}, kept {want['total']} ({share:.3f}), trace launches {launches}")
    assert share >= 0.30
    assert 0 < want["counts"].min() and want["counts"].max() < N           # the compaction moves rows in every pose
    assert launches == SHAPES[shape][4], "the call did not take the path this shape is meant to select"
    assert fr["total"] == want["total"] and fr["counts"].tolist() == want["counts"].tolist()
    for k in COLUMNS + STATS:
        assert_bit_equal(fr[k], want[k], f"{gen} {shape}: {k}")


@pytest.mark.parametrize("shape", ["graded", "one_stream"])
def test_capacity_one_row_short(room, shape):
    """Capacity K - 1 for a scan that keeps K rows: LRC_ERR_INVALID_ARG with the size needed, in the message and in
    out_total.  (The small shape leaves the one-stream path as soon as capacity < P * N -- that path copies worst-case
    lengths -- and fails in the single-chunk path with the same text.)"""
    import lidarcast
    from lidarcast import _capi
    a, want = _reference(room, "poses", shape)
    P, N, K = a["P"], a["N"], want["total"]
    fr, counts, bufs, cap = room._frames_begin(P, P * N, WANT, K - 1)
    poses = np.ascontiguousarray(a["poses"], dtype=np.float64).reshape(-1, 16)
    total = C.c_uint64(0)
    lib = lidarcast.load()
    rc = lib.lrc_scan_poses_compact(room._h, poses.ctypes.data_as(C.c_void_p), P, a["dirs"].ctypes.data_as(C.c_void_p), N,
                                    float(MAX_RANGE), C.byref(fr), cap, C.byref(total))
    assert rc == _capi.LRC_ERR_INVALID_ARG
    assert lib.lrc_last_error().decode() == f"frame buffers too small: capacity {K - 1} rows, the scan kept {K}"
    assert total.value == K
    assert counts.astype(np.int64).tolist() == want["counts"].tolist()
    # the same buffers with one row more hold the whole scan
    fr2 = room.scan_poses_compact(a["poses"], a["dirs"], MAX_RANGE, want=WANT, capacity=K)
    assert fr2["total"] == K
    assert_bit_equal(fr2["xyzl"], want["xyzl"], f"{shape}: xyzl at capacity K")
