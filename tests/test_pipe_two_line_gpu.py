"""-m gpu: two-line tiles of the scan pipeline (lrc_pipe_submit regroups the rays of a pose into waves of 32 columns x 2
adjacent scan lines, csrc/lrc_device.h tile_ray) against lrc_scan_poses_dev + lrc_compact_dev, bit for bit: rows, counts
and the expanded records (tile_count included, which the scan pass now forms from the keep masks).  The line width is
detected from the table, hinted right, hinted wrong, or absent; none of it may change a byte."""
import ctypes as C

import numpy as np
import pytest

from helpers import pose, sensor_small

pytestmark = pytest.mark.gpu

RECORD = (("t", 4), ("prim", 4), ("normal3", 12), ("point3", 12), ("sem", 2), ("ins", 2), ("tile_count", None))


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    c = lidarcast.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def room(ctx):
    import lidarcast
    from lidarcast import synth
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=7, cell=0.04)
    return lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)


@pytest.fixture(scope="module")
def open_room(ctx):
    """The same room without its ceiling and the upper part of its walls: rays above the horizon miss."""
    import lidarcast
    from lidarcast import synth
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=7, cell=0.04)
    v, t = np.asarray(mesh.vertices), np.asarray(mesh.triangles)
    low = v[t][:, :, 2].max(axis=1) < 1.3
    assert 0 < low.sum() < len(t)
    return lidarcast.Scene(ctx, v, np.ascontiguousarray(t[low]), np.asarray(mesh.triangle_sem)[low],
                           np.asarray(mesh.triangle_ins)[low])


def _dev_bytes(ptr, nbytes):
    import torch
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(buf.data_ptr()), C.c_void_p(int(ptr)), nbytes, 3) == 0      # device to device
    return buf.cpu().numpy().tobytes()


def _table(lines, width):
    from lidar import IndoorLidar
    return IndoorLidar(sensor_small(lines=lines, width=width), np.eye(4)).sensor_directions()


def _poses(P, rng):
    return np.stack([pose(0.6 + 2.8 * rng.random(), 0.6 + 1.8 * rng.random(), 0.5 + 1.5 * rng.random(), yaw=rng.uniform(-3, 3))
                     for _ in range(P)]).reshape(P, 16)


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


def _line_tiles(pipe):
    """The line width (in tiles) the last submit's trace launch ran with: the regrouping is byte-neutral by design, so only
    the library can say whether it happened."""
    import lidarcast
    fn = lidarcast.load().lrc_internal_pipe_line_tiles
    fn.argtypes, fn.restype = [C.c_void_p], C.c_uint32
    return int(fn(pipe._h))


def _run(scene, dirs, max_range, P=4, submits=6, hints=(None,), seed=0, want_tiles=None):
    """`submits` batches back to back, the line-width hint changed between them as `hints` says (None: leave it);
    every batch's rows and counts, and the records of the last four, against the two-call reference; want_tiles: the line
    width in tiles each submit must have run with.  Returns the number of kept rays and of 64-ray tiles whose keep mask is
    partial in both 32-bit halves."""
    import torch
    import lidarcast
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    N = len(dirs)
    assert N % 64 == 0
    d_dirs = torch.from_numpy(np.ascontiguousarray(dirs)).to(dev)
    rng = np.random.default_rng(seed)
    pipe = lidarcast.ScanPipe(scene, P, N)
    subs = []
    for b in range(submits):
        hint = hints[b % len(hints)]
        if hint is not None:
            pipe.set_line_width(hint)
        d_poses = torch.from_numpy(_poses(P, rng)).to(dev)
        rows = torch.full((P * N, 4), -7.0, dtype=torch.float32, device=dev)
        counts = torch.full((P,), -1, dtype=torch.int64, device=dev)
        ticket = pipe.submit(d_poses, d_dirs, max_range, out_rows_t=rows, counts_t=counts, stream=st)
        subs.append((d_poses, ticket, rows, counts))
        if want_tiles is not None:
            assert _line_tiles(pipe) == want_tiles[b % len(want_tiles)], (b, hint, _line_tiles(pipe))
    pipe.wait(st)
    torch.cuda.synchronize()
    kept = both_partial = 0
    for i, (d_poses, ticket, rows, counts) in enumerate(subs):
        hits, ref_rows, ref_counts = _reference(scene, d_poses, d_dirs, P, N, max_range, st)
        assert torch.equal(counts, ref_counts), f"submit {i}: per-pose counts differ"
        kk = int(ref_counts.sum().item())
        assert torch.equal(rows[:kk].view(torch.int32), ref_rows[:kk].view(torch.int32)), f"submit {i}: rows differ"
        assert bool((rows[kk:] == -7.0).all()), f"submit {i}: rows beyond the kept ones were touched"
        if i >= len(subs) - 4:
            _check_records(pipe, ticket, hits, P * N)
        kept += kk
        k = (hits["t"].cpu().numpy() != np.inf).reshape(-1, 2, 32).sum(axis=2)
        both_partial += int(((k > 0) & (k < 32)).all(axis=1).sum())
    pipe.close()
    return kept, both_partial


def test_benchmark_table_detected_width(room):
    """The C3 table (32 lines x 2048): the width is detected; 64 tiles per line pair."""
    import bench
    from lidar import IndoorLidar
    k = bench.c3_sensor()
    dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
    assert len(dirs) == 32 * 2048 and len(np.unique(dirs[:2048, 2])) == 1 and dirs[2048, 2] != dirs[0, 2]
    kept, _ = _run(room, dirs, k.max_range, P=3, submits=5, seed=1, want_tiles=(32,))
    assert kept > 0


def test_three_line_table_keeps_its_last_line_one_dimensional(room):
    kept, _ = _run(room, _table(3, 256), 20.0, P=5, submits=6, seed=2, want_tiles=(4,))
    assert kept > 0


def test_table_without_line_structure(room):
    """Random directions, N % 64 == 0: no run of equal z, the waves take 64 consecutive rays."""
    rng = np.random.default_rng(5)
    d = rng.normal(size=(64 * 37, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kept, _ = _run(room, d, 20.0, P=4, submits=5, seed=3, want_tiles=(0,))
    assert kept > 0


def test_wrong_and_useless_hints_change_nothing(room):
    """8 lines x 512: hinted as 128 and 1024 (wrong multiples of 64 that divide the pose), 192 and 100 (do not: 1-D tiles),
    the true 512, and back to automatic -- changed from submit to submit on one pipeline."""
    kept, _ = _run(room, _table(8, 512), 20.0, P=4, submits=9, hints=(128, 1024, 192, 100, 512, 0, 2048, 64, None), seed=4,
                   want_tiles=(2, 16, 0, 0, 8, 8, 32, 1, 1))
    assert kept > 0


def test_many_misses_give_masks_partial_in_both_halves(open_room):
    """Open room and a short max_range: rays miss or are dropped by the range filter in patches, so keep masks whose two
    32-bit halves -- written by two different waves -- are both partial occur, and tiles with no kept ray."""
    kept, both_partial = _run(open_room, _table(16, 512), 1.6, P=6, submits=6, seed=6, want_tiles=(8,))
    assert 0 < kept < 6 * 6 * 16 * 512
    assert both_partial > 0


def test_records_of_a_two_line_submit_equal_the_serial_records(room):
    """lrc_pipe_records right after a single two-line submit (no later submit, no flush in between): all seven arrays of
    the record, tile_count included, equal lrc_scan_poses_dev's."""
    import torch
    import lidarcast
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    dirs = _table(6, 320)
    P, N = 3, len(dirs)
    d_dirs = torch.from_numpy(dirs).to(dev)
    d_poses = torch.from_numpy(_poses(P, np.random.default_rng(8))).to(dev)
    pipe = lidarcast.ScanPipe(room, P, N)
    pipe.set_line_width(320)
    rows = torch.zeros((P * N, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros((P,), dtype=torch.int64, device=dev)
    ticket = pipe.submit(d_poses, d_dirs, 3.0, out_rows_t=rows, counts_t=counts, stream=st)
    assert _line_tiles(pipe) == 5
    hits, ref_rows, ref_counts = _reference(room, d_poses, d_dirs, P, N, 3.0, st)
    _check_records(pipe, ticket, hits, P * N)
    pipe.wait(st)
    torch.cuda.synchronize()
    assert torch.equal(counts, ref_counts)
    kk = int(ref_counts.sum().item())
    assert torch.equal(rows[:kk].view(torch.int32), ref_rows[:kk].view(torch.int32))
    pipe.close()
