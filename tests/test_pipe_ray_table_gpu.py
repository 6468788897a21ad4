"""-m gpu: prepared submits of the scan pipeline.  A fused lrc_pipe_submit builds a ray table per submit (per table row the
float32 direction, its guarded reciprocal and its unit vector for the rotation of pose 0; per pose whether its rotation block
is pose 0's bit for bit) and the tracing waves of such poses load it instead of forming every ray in float64.  None of it may
change a byte: every case compares rows and counts of lrc_pipe_submit with lrc_scan_poses_dev + lrc_compact_dev and the
expanded lrc_pipe_records with the serial record, bit for bit, with the table switched on and off (lrc_pipe_set_ray_table).
The table itself is read back through a test hook: its per-pose flags must be what the poses' rotations say, and its rows
the library's host compilation of the same function (which tests/test_ray_table_host.py holds against numpy)."""
import ctypes as C

import numpy as np
import pytest

from helpers import bits, pose, sensor_small

pytestmark = pytest.mark.gpu

RECORD = (("t", 4), ("prim", 4), ("normal3", 12), ("point3", 12), ("sem", 2), ("ins", 2), ("tile_count", None))


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    c = lidarcast.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(ctx):
    """The room of tests/test_pipe_two_line_gpu.py, and the same room without its ceiling and the upper part of its walls."""
    import lidarcast
    from lidarcast import synth
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=7, cell=0.04)
    v, t = np.asarray(mesh.vertices), np.asarray(mesh.triangles)
    low = v[t][:, :, 2].max(axis=1) < 1.3
    assert 0 < low.sum() < len(t)
    return {"room": lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins),
            "open_room": lidarcast.Scene(ctx, v, np.ascontiguousarray(t[low]), np.asarray(mesh.triangle_sem)[low],
                                         np.asarray(mesh.triangle_ins)[low])}


def _table(name):
    """8 lines x 128 (16 tiles per pose: groups of four lines and a split at the horizon), 3 lines x 64 (a pair and an odd
    line), and 192 rows without a line structure (1-D tiles)."""
    from lidar import IndoorLidar
    if name == "flat192":
        d = np.random.default_rng(5).normal(size=(192, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True)
    lines, width = {"8x128": (8, 128), "3x64": (3, 64)}[name]
    return IndoorLidar(sensor_small(lines=lines, width=width), np.eye(4)).sensor_directions()


TABLES = ("8x128", "3x64", "flat192")
SCENES = ("room", "open_room")
LINE_TILES = {"8x128": 2, "3x64": 1, "flat192": 0}


def _poses(yaws, rng):
    return np.stack([pose(0.6 + 2.8 * rng.random(), 0.6 + 1.8 * rng.random(), 0.5 + 1.5 * rng.random(), yaw=y)
                     for y in yaws]).reshape(len(yaws), 16)


def _dev_bytes(ptr, nbytes):
    import torch
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(buf.data_ptr()), C.c_void_p(int(ptr)), nbytes, 3) == 0      # device to device
    return buf.cpu().numpy().tobytes()


def _hook(pipe, name, restype):
    import lidarcast
    fn = getattr(lidarcast.load(), name)
    fn.argtypes, fn.restype = [C.c_void_p], restype
    return fn(pipe._h)


def _host_rows(R, dirs):
    import lidarcast
    fn = lidarcast.load().lrc_internal_ray_table_rows
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p], None
    R = np.ascontiguousarray(R, dtype=np.float64)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)
    out = np.empty((len(dirs), 9), dtype=np.float32)
    fn(R.ctypes.data, dirs.ctypes.data, len(dirs), out.ctypes.data)
    return out


def _same_bits(a, b, what):
    """Bit for bit; a NaN (a table row with a NaN component: never cast) only has to be a NaN in the same place."""
    na = np.isnan(a)
    assert np.array_equal(na, np.isnan(b)), what
    assert not ((bits(a) != bits(b)) & ~na).any(), what


def _check_table(pipe, poses16, dirs):
    """The table the last submit's launch carried: flags, origins and centres per pose, rows for pose 0's rotation."""
    ptr = _hook(pipe, "lrc_internal_pipe_ray_table", C.c_void_p)
    assert ptr, "the launch carried no ray table"
    P, N = len(poses16), len(dirs)
    raw = _dev_bytes(ptr, N * 48 + P * 64)
    m = poses16.reshape(P, 4, 4)
    rot = np.ascontiguousarray(m[:, :3, :3]).view(np.uint64).reshape(P, 9)
    want_same = (rot == rot[0]).all(axis=1)
    rec = np.frombuffer(raw, dtype=np.uint8, offset=N * 48).reshape(P, 64)
    same = rec[:, 24:28].copy().view(np.uint32)[:, 0]         # RayPose: centre (3 float64), flag, origin (3 float32)
    assert np.array_equal(same, want_same.astype(np.uint32)), (same, want_same)
    _same_bits(rec[:, 0:24].copy().view(np.float64), np.ascontiguousarray(m[:, :3, 3]), "centres")
    _same_bits(rec[:, 28:40].copy().view(np.float32), m[:, :3, 3].astype(np.float32), "origins")
    di = np.frombuffer(raw, dtype=np.float32, count=N * 8).reshape(N, 2, 4)
    h = np.frombuffer(raw, dtype=np.float32, offset=N * 32, count=N * 4).reshape(N, 4)
    want = _host_rows(m[0, :3, :3], dirs)
    with np.errstate(invalid="ignore"):
        _same_bits(di[:, 0, :3], want[:, 0:3], "table rows: d")
        _same_bits(di[:, 1, :3], want[:, 3:6], "table rows: inv")
        _same_bits(h[:, :3], want[:, 6:9], "table rows: h")
    return want_same


def _reference(scene, d_poses, d_dirs, P, N, max_range, st):
    import torch
    import lidarcast
    from lidarcast._capi import LrcCompactIO
    dev = d_dirs.device
    hits = lidarcast.DeviceHits(P * N, dev, want=tuple(n for n, _ in RECORD))
    rows = torch.full((P * N, 4), -7.0, dtype=torch.float32, device=dev)
    counts = torch.full((P,), -1, dtype=torch.int64, device=dev)
    io = LrcCompactIO()
    io.t, io.point3, io.sem, io.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
    io.tile_count = hits["tile_count"].data_ptr()
    io.out_xyzl, io.counts = rows.data_ptr(), counts.data_ptr()
    scene.scan_poses_dev(d_poses, d_dirs, hits, max_range, st)
    scene.ctx.compact_dev(P, N, io, st)
    torch.cuda.synchronize()
    return hits, rows, counts


def _check_records(pipe, ticket, hits, n):
    import torch
    rec = pipe.records(ticket)
    for name, width in RECORD:
        nbytes = 4 * ((n + 63) // 64) if width is None else n * width
        ref = hits[name].view(torch.uint8).flatten()[:nbytes].cpu().numpy().tobytes()
        assert _dev_bytes(getattr(rec, name), nbytes) == ref, f"records differ: {name}"


def _run(scene, batches, max_range, want_tiles=None):
    """batches: (poses (P, 16), table (N, 3)) per submit, submitted back to back without a wait on ONE device table buffer:
    where a batch's table differs from the one before, the buffer is overwritten in place (behind the trace that still reads
    it).  The serial reference of every batch is computed once, first; then the pipeline runs with the ray table on and
    off.  Returns per batch (reference hits, pose flags of the table if it was the last submit else None)."""
    import torch
    import lidarcast
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    N = len(batches[0][1])
    assert N % 64 == 0 and all(len(d) == N for _, d in batches)
    d_tab = torch.empty((N, 3), dtype=torch.float64, device=dev)
    d_poses = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p, _ in batches]
    refs = []
    for (p, dirs), dp in zip(batches, d_poses):
        d_tab.copy_(torch.from_numpy(np.ascontiguousarray(dirs)))
        refs.append(_reference(scene, dp, d_tab, len(p), N, max_range, st))
    flags = None
    for switch in (1, 0):
        pipe = lidarcast.ScanPipe(scene, max(len(p) for p, _ in batches), N)
        pipe.set_ray_table(switch)
        outs, ticket, current = [], 0, None
        for (p, dirs), dp in zip(batches, d_poses):
            if current is None or current is not dirs:
                if ticket:
                    pipe.trace_done(ticket, st)          # the edit must not overtake the trace that reads the table
                d_tab.copy_(torch.from_numpy(np.ascontiguousarray(dirs)))
                current = dirs
            rows = torch.full((len(p) * N, 4), -7.0, dtype=torch.float32, device=dev)
            counts = torch.full((len(p),), -1, dtype=torch.int64, device=dev)
            ticket = pipe.submit(dp, d_tab, max_range, out_rows_t=rows, counts_t=counts, stream=st)
            outs.append((ticket, rows, counts))
            if want_tiles is not None:
                assert _hook(pipe, "lrc_internal_pipe_line_tiles", C.c_uint32) == want_tiles
        pipe.wait(st)
        torch.cuda.synchronize()
        if switch:
            flags = _check_table(pipe, batches[-1][0], batches[-1][1])
        else:
            assert not _hook(pipe, "lrc_internal_pipe_ray_table", C.c_void_p)
        for i, ((ticket, rows, counts), (hits, ref_rows, ref_counts)) in enumerate(zip(outs, refs)):
            what = f"ray table {switch}, submit {i}"
            assert torch.equal(counts, ref_counts), what + ": per-pose counts differ"
            kk = int(ref_counts.sum().item())
            assert torch.equal(rows[:kk].view(torch.int32), ref_rows[:kk].view(torch.int32)), what + ": rows differ"
            assert bool((rows[kk:] == -7.0).all()), what + ": rows beyond the kept ones were touched"
            if i >= len(outs) - 4:
                _check_records(pipe, ticket, hits, len(batches[i][0]) * N)
        pipe.close()
    return refs, flags


def _kept(refs):
    return sum(int(c.sum().item()) for _, _, c in refs)


grid = pytest.mark.parametrize("scene_name,table", [(s, t) for s in SCENES for t in TABLES])


@grid
@pytest.mark.parametrize("yaw", [0.0, 0.7])
def test_one_rotation_for_all_poses(scenes, scene_name, table, yaw):
    """Cases 1 and 2: every pose at yaw 0, every pose at yaw 0.7; three submits, so that rows also ride in a later launch."""
    rng = np.random.default_rng(1)
    dirs = _table(table)
    refs, flags = _run(scenes[scene_name], [(_poses([yaw] * 4, rng), dirs) for _ in range(3)], 20.0, LINE_TILES[table])
    assert flags.all() and _kept(refs) > 0


@grid
def test_single_pose(scenes, scene_name, table):
    """Case 3: P = 1."""
    refs, flags = _run(scenes[scene_name], [(_poses([0.4], np.random.default_rng(2)), _table(table))], 20.0)
    assert flags.tolist() == [True] and _kept(refs) > 0


@grid
def test_fast_and_slow_waves_in_one_launch(scenes, scene_name, table):
    """Case 4: yaws 0, 0.7, 0, 0.7, 0."""
    refs, flags = _run(scenes[scene_name], [(_poses([0, 0.7, 0, 0.7, 0], np.random.default_rng(3)), _table(table))], 20.0)
    assert flags.tolist() == [True, False, True, False, True] and _kept(refs) > 0


@grid
def test_only_pose_0_has_its_rotation(scenes, scene_name, table):
    """Case 5: pose 0 at yaw 0.3, all others at yaw 0: every wave but pose 0's falls back."""
    refs, flags = _run(scenes[scene_name], [(_poses([0.3, 0, 0, 0], np.random.default_rng(4)), _table(table))], 20.0)
    assert flags.tolist() == [True, False, False, False] and _kept(refs) > 0


@grid
def test_a_zero_of_the_other_sign_is_another_rotation(scenes, scene_name, table):
    """Case 6: rotation blocks equal to pose 0's but for the sign of one zero entry.  They fall back (the flags say so), and
    the bytes are the serial step's either way."""
    p = _poses([0.0] * 4, np.random.default_rng(5)).reshape(4, 4, 4)
    assert p[0, 0, 2] == 0.0 and not np.signbit(p[0, 0, 2]) and p[0, 0, 1] == 0.0
    p[1, 0, 2] = -0.0
    p[2, 0, 1] = -p[0, 0, 1]          # whichever zero helpers.pose left there, the other one
    p[3, 2, 0] = -0.0
    refs, flags = _run(scenes[scene_name], [(p.reshape(4, 16), _table(table))], 20.0)
    assert flags.tolist() == [True, False, False, False] and _kept(refs) > 0


@grid
def test_three_submits_without_a_wait_ragged_pose_counts(scenes, scene_name, table):
    """Case 7: yaw 0, then 0.5, then 0, with 3, 1 and 4 poses."""
    rng = np.random.default_rng(6)
    dirs = _table(table)
    refs, flags = _run(scenes[scene_name], [(_poses([0.0] * 3, rng), dirs), (_poses([0.5], rng), dirs), (_poses([0.0] * 4, rng), dirs)],
                       20.0)
    assert flags.all() and _kept(refs) > 0


@pytest.mark.parametrize("scene_name", SCENES)
def test_table_edited_in_place_and_replaced_at_the_same_address(scenes, scene_name):
    """Case 8: between two submits two rows of the table are swapped and one column is negated, in place; then a different
    table is written to the same address.  Every submit's rows follow the content it was submitted with."""
    rng = np.random.default_rng(7)
    a = _table("8x128")
    b = a.copy()
    b[[5, 700]] = b[[700, 5]]
    b[:, 1] = -b[:, 1]
    c = np.ascontiguousarray(_table("8x128")[::-1] * np.array([1.0, -1.0, 1.0]))
    c[:, 2] += 0.01
    assert not np.array_equal(a, b) and not np.array_equal(b, c)
    p = _poses([0.2] * 3, rng)          # the same poses every time: what differs between the submits is the table alone
    batches = [(p, a), (p, b), (p, c), (p, a)]
    refs, flags = _run(scenes[scene_name], batches, 20.0)
    assert flags.all() and _kept(refs) > 0
    # every edit is visible in the results: the ranges of consecutive submits differ, and the first table gives its ranges again
    ts = [r[0]["t"].cpu().numpy() for r in refs]
    assert all(not np.array_equal(ts[i], ts[i + 1]) for i in range(3)) and np.array_equal(ts[0], ts[3])


@pytest.mark.parametrize("scene_name", SCENES)
@pytest.mark.parametrize("yaw", [0.0, 0.7])
def test_rows_with_zero_and_non_finite_components(scenes, scene_name, yaw):
    """Case 9: rows with exact zero components of both signs, axis-aligned rows, a row with a NaN and one with an Inf
    component.  The non-finite rays are reported as misses, as the serial scan reports them."""
    dirs = _table("8x128").copy()
    special = {3: (1.0, 0.0, 0.0), 64: (0.0, -1.0, 0.0), 130: (0.0, 0.0, 1.0), 131: (-0.0, -0.0, -1.0), 200: (0.6, -0.0, 0.8),
               333: (-0.0, 0.6, -0.8), 513: (0.0, 0.0, 0.0), 640: (np.nan, 0.5, 0.5), 641: (0.5, np.inf, 0.5), 1023: (-np.inf, 0.0, 0.0)}
    for i, v in special.items():
        dirs[i] = v
    refs, flags = _run(scenes[scene_name], [(_poses([yaw, yaw, 0.7, yaw], np.random.default_rng(8)), dirs)], 20.0)
    assert flags.tolist() == [True, True, yaw == 0.7, True]
    t = refs[0][0]["t"].cpu().numpy().reshape(4, -1)
    assert np.isinf(t[:, [640, 641, 1023]]).all() and _kept(refs) > 0


@grid
def test_max_range_taken_from_the_scan(scenes, scene_name, table):
    """Case 10: max_range is the exact float64 distance of one of the scan's own returns, so some hits fall outside it and
    at least one lies within ulps of it (tests/test_range_band_gpu.py); numpy's `sqrt(s) < max_range` decides what is kept."""
    import torch
    scene = scenes[scene_name]
    p = _poses([0.0, 0.0, 0.7, 0.0], np.random.default_rng(9))
    dirs = _table(table)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    hits, _, _ = _reference(scene, torch.from_numpy(p).to(dev), torch.from_numpy(np.ascontiguousarray(dirs)).to(dev), 4, len(dirs),
                            1e6, st)
    t = hits["t"].cpu().numpy().reshape(4, -1)
    pts = hits["point3"].cpu().numpy().reshape(4, -1, 3)
    hit = t != np.inf
    e = pts.astype(np.float64) - p.reshape(4, 4, 4)[:, None, :3, 3]
    s = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    dist = np.sqrt(s)
    R = float(np.quantile(dist[hit], 0.5, method="nearest"))
    assert int((hit & (np.abs(s - R * R) <= R * R * 2.0 ** -48)).sum()) >= 1
    refs, flags = _run(scene, [(p, dirs)], R)
    assert flags.tolist() == [True, True, False, True]
    kept = refs[0][0]["t"].cpu().numpy().reshape(4, -1) != np.inf
    want = hit & (dist < R)
    assert np.array_equal(kept, want) and 0 < want.sum() < hit.sum()
