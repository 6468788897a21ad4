"""-m gpu: line-group tiles of the scan pipeline (lrc_pipe_submit regroups the rays of a pose into waves of 64 / L columns
x L adjacent scan lines that stay on one side of the horizon, csrc/lrc_device.h tile_ray) against lrc_scan_poses_dev +
lrc_compact_dev and against the CPU oracle, bit for bit: rows, per-pose counts and the expanded records (tile_count
included, which the scan pass forms from keep masks that four waves fill).  3 poses of H x 128 rays, H = 8, 9, 10, the
zero-elevation crossing inside a would-be group of four, on a group edge, or absent; each with 0 (automatic), 1, 2 and 4
lines per tile and with a wrong line width; three submits between waits, so that rows leave both through the leading
scatter of a later launch and through lrc_pipe_wait.  None of it may change a byte; the library says what it ran with."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bit_equal
from test_pipe_two_line_gpu import _check_records, _line_tiles, _poses, _reference

pytestmark = pytest.mark.gpu

W, P, SUBMITS, MAX_RANGE = 128, 3, 3, 20.0
# elevations in degrees, top line first: (name, crossing for H lines)
CROSSING = {
    "inside": lambda H: 2,        # lines 0-1 above the horizon: a group of four from line 0 would straddle it
    "edge": lambda H: 4,          # four lines above: the first group of four ends at the crossing
    "absent": lambda H: H,        # every line above
}
# (lines asked for, line width hinted): automatic, 1-D, pairs, fours, and a width that is not the table's
CONFIGS = ((0, None), (1, None), (2, None), (4, None), (0, 64))


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
    from oracle.c_oracle import OracleMesh
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=7, cell=0.04)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    return scene, OracleMesh(mesh.vertices, mesh.triangles).build()


def _sensor(H, split, width=W):
    from lidar import Indoor8LineLidarIntrinsics
    up = list(np.linspace(22.0, 3.0, split))
    down = list(np.linspace(-4.0, -30.0, H - split))
    return Indoor8LineLidarIntrinsics(vertical_res=H, horizontal_res=width, max_range=MAX_RANGE, vertical_degrees=up + down)


def _hook(pipe, name):
    import lidarcast
    fn = getattr(lidarcast.load(), name)
    fn.argtypes, fn.restype = [C.c_void_p], C.c_uint32
    return int(fn(pipe._h))


def _widest(H, split, lines):
    """Lines per tile of the widest group the rule forms: runs [0, split) and [split, H), fours, then a pair, then 1-D."""
    runs = (split, H - split) if 0 < split < H else (H,)
    if lines == 1 or max(runs) < 2:
        return 1
    return 4 if lines == 4 and max(runs) >= 4 else 2


def _oracle_rows(om, sensor, poses16):
    """Per pose the oracle's kept points (float32 rows) and their count."""
    from lidar import create_lidar
    from oracle import np_oracle
    out = []
    for m in poses16.reshape(-1, 4, 4):
        pts, _ = np_oracle.lidar_intersect_mesh(om, create_lidar(sensor, m), threads=4)
        out.append(np.ascontiguousarray(pts, dtype=np.float32))
    return out


@pytest.mark.parametrize("H", [8, 9, 10])
@pytest.mark.parametrize("crossing", ["inside", "edge", "absent"])
def test_every_grouping_gives_the_serial_and_the_oracle_bytes(room, H, crossing):
    import torch
    import lidarcast
    from lidar import IndoorLidar
    scene, om = room
    split = CROSSING[crossing](H)
    sensor = _sensor(H, split)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    N = len(dirs)
    assert N == H * W
    z = dirs[::W, 2]
    assert len(np.unique(dirs[:W, 2])) == 1 and dirs[W, 2] != dirs[0, 2]
    assert int(np.argmax((z < 0) != (z[0] < 0))) == (split if split < H else 0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    d_dirs = torch.from_numpy(np.ascontiguousarray(dirs)).to(dev)
    rng = np.random.default_rng(100 * H + split)
    poses = [_poses(P, rng) for _ in range(SUBMITS)]
    d_poses = [torch.from_numpy(p).to(dev) for p in poses]
    # the references, once: the two serial calls per batch, and the oracle per pose
    refs = [_reference(scene, dp, d_dirs, P, N, MAX_RANGE, st) for dp in d_poses]
    for b, (hits, ref_rows, ref_counts) in enumerate(refs):
        want = _oracle_rows(om, sensor, poses[b])
        assert [len(w) for w in want] == ref_counts.cpu().tolist(), f"batch {b}: serial counts differ from the oracle"
        kk = int(ref_counts.sum().item())
        assert_bit_equal(ref_rows[:kk, :3].cpu().numpy(), np.concatenate(want), f"batch {b}: serial rows against the oracle")
    for lines, hint in CONFIGS:
        pipe = lidarcast.ScanPipe(scene, P, N)
        pipe.set_tile_lines(lines)
        if hint is not None:
            pipe.set_line_width(hint)
        subs = []
        for b in range(SUBMITS):
            rows = torch.full((P * N, 4), -7.0, dtype=torch.float32, device=dev)
            counts = torch.full((P,), -1, dtype=torch.int64, device=dev)
            ticket = pipe.submit(d_poses[b], d_dirs, MAX_RANGE, out_rows_t=rows, counts_t=counts, stream=st)
            subs.append((ticket, rows, counts))
            got = (_line_tiles(pipe), _hook(pipe, "lrc_internal_pipe_tile_lines"), _hook(pipe, "lrc_internal_pipe_line_group"))
            if hint is not None:      # lines of 64 rays, twice as many, no split known: fours
                assert got == (hint // 64, 4, 0x80000000), (lines, hint, got)
            elif lines == 1:
                assert got[:2] == (0, 1), (lines, got)
            else:
                word = (split if split < H else H) | (0x80000000 if lines in (0, 4) else 0)
                assert got == (W // 64, _widest(H, split, 4 if lines == 0 else lines), word), (lines, got)
        pipe.wait(st)
        torch.cuda.synchronize()
        for b, (ticket, rows, counts) in enumerate(subs):
            hits, ref_rows, ref_counts = refs[b]
            what = f"lines {lines}, hint {hint}, submit {b}"
            assert torch.equal(counts, ref_counts), f"{what}: per-pose counts differ"
            kk = int(ref_counts.sum().item())
            assert kk > 0
            assert torch.equal(rows[:kk].view(torch.int32), ref_rows[:kk].view(torch.int32)), f"{what}: rows differ"
            assert bool((rows[kk:] == -7.0).all()), f"{what}: rows beyond the kept ones were touched"
            _check_records(pipe, ticket, hits, P * N)
        pipe.close()


def test_lines_that_are_not_whole_tiles_keep_one_dimensional_tiles(room):
    """8 lines x 96: rays_per_pose % 64 == 0 but a line is one tile and a half -- no width is usable, whatever is asked for."""
    import torch
    import lidarcast
    from lidar import IndoorLidar
    scene, _ = room
    dirs = IndoorLidar(_sensor(8, 2, width=96), np.eye(4)).sensor_directions()
    N = len(dirs)
    assert N % 64 == 0
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    d_dirs = torch.from_numpy(np.ascontiguousarray(dirs)).to(dev)
    d_poses = torch.from_numpy(_poses(P, np.random.default_rng(3))).to(dev)
    hits, ref_rows, ref_counts = _reference(scene, d_poses, d_dirs, P, N, MAX_RANGE, st)
    pipe = lidarcast.ScanPipe(scene, P, N)
    for lines in (0, 4):
        pipe.set_tile_lines(lines)
        rows = torch.full((P * N, 4), -7.0, dtype=torch.float32, device=dev)
        counts = torch.full((P,), -1, dtype=torch.int64, device=dev)
        ticket = pipe.submit(d_poses, d_dirs, MAX_RANGE, out_rows_t=rows, counts_t=counts, stream=st)
        assert (_line_tiles(pipe), _hook(pipe, "lrc_internal_pipe_tile_lines")) == (0, 1)
        pipe.wait(st)
        torch.cuda.synchronize()
        assert torch.equal(counts, ref_counts)
        kk = int(ref_counts.sum().item())
        assert torch.equal(rows[:kk].view(torch.int32), ref_rows[:kk].view(torch.int32))
        _check_records(pipe, ticket, hits, P * N)
    pipe.close()


def test_a_line_count_outside_0_1_2_4_is_refused(room):
    import lidarcast
    scene, _ = room
    pipe = lidarcast.ScanPipe(scene, 1, 128)
    with pytest.raises(Exception):
        pipe.set_tile_lines(3)
    pipe.close()
