"""-m gpu: 12-byte lean records of the scan pipeline.  A fused lrc_pipe_submit stores per ray (t, label, slot); the output row
of a tile whose wave took the submit's ray table is formed where it is consumed -- in the leading workgroups of the launch two
submits later, in lrc_pipe_wait's plain scatter, in the expansion behind lrc_pipe_records -- from the record, the table row's
unit vector and the pose record's origin, out of the table the pipeline keeps per record set.  Tiles whose pose turns against
pose 0, and every tile of a submit without a table, keep a stored row.  None of it may change a byte: every case compares rows
(or the separate columns), per-pose counts and, through ScanPipe.records, all record columns with lrc_scan_poses_dev +
lrc_compact_dev on the same inputs, bit for bit.

Shapes: tables of 4 lines x 64 (four tiles per pose: the scatter's groups of four tiles lie in one pose), 3 x 128 (six tiles:
groups straddle two poses, the odd last line keeps 1-D tiles), 1 x 64 (one tile per pose: every group goes tile by tile) and
8 x 128 (sixteen tiles, line-group tiles of four lines); 1, 2 and 5 poses."""
import ctypes as C

import numpy as np
import pytest

from helpers import pose, sensor_small

pytestmark = pytest.mark.gpu

RECORD = (("t", 4), ("prim", 4), ("normal3", 12), ("point3", 12), ("sem", 2), ("ins", 2), ("tile_count", None))
TABLES = {"4x64": (4, 64), "3x128": (3, 128), "1x64": (1, 64), "8x128": (8, 128)}
FAR = 20.0


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    c = lidarcast.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene(ctx):
    """The small room of the other pipeline tests."""
    import lidarcast
    from lidarcast import synth
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=7, cell=0.04)
    return lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)


def _table(name):
    from lidar import IndoorLidar
    lines, width = TABLES[name]
    return IndoorLidar(sensor_small(lines=lines, width=width), np.eye(4)).sensor_directions()


def _poses(yaws, seed):
    rng = np.random.default_rng(seed)
    return np.stack([pose(0.6 + 2.8 * rng.random(), 0.6 + 1.8 * rng.random(), 0.5 + 1.5 * rng.random(), yaw=y)
                     for y in yaws]).reshape(len(yaws), 16)


def _dev_bytes(ptr, nbytes):
    import torch
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(buf.data_ptr()), C.c_void_p(int(ptr)), nbytes, 3) == 0      # device to device
    return buf.cpu().numpy().tobytes()


class Out:
    """The caller's output buffers of one submit (or of the serial reference), filled with sentinels."""

    def __init__(self, P, N, columns, dev):
        import torch
        n = P * N
        self.columns = columns
        self.counts = torch.full((P,), -1, dtype=torch.int64, device=dev)
        if columns:
            self.point3 = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
            self.sem = torch.full((n,), 0x7A7A, dtype=torch.int16, device=dev)
            self.ins = torch.full((n,), 0x7B7B, dtype=torch.int16, device=dev)
            self.index = torch.full((n,), 0x7C7C7C7C, dtype=torch.int32, device=dev)
        else:
            self.rows = torch.full((n, 4), -7.0, dtype=torch.float32, device=dev)

    def fill(self, io):
        io.counts = self.counts.data_ptr()
        if self.columns:
            io.out_point3, io.out_sem, io.out_ins = self.point3.data_ptr(), self.sem.data_ptr(), self.ins.data_ptr()
            io.out_index = self.index.data_ptr()
        else:
            io.out_xyzl = self.rows.data_ptr()
        return io

    def arrays(self):
        import torch
        names = ("point3", "sem", "ins", "index") if self.columns else ("rows",)
        return {n: getattr(self, n).view(torch.uint8).cpu().numpy().reshape(getattr(self, n).shape[0], -1) for n in names}


_REFS = {}


def _reference(scene, poses16, dirs, max_range, columns):
    """lrc_scan_poses_dev + lrc_compact_dev of one batch: (record columns as bytes, output arrays, counts), computed once per
    distinct input and shared by the cases."""
    import torch
    import lidarcast
    from lidarcast._capi import LrcCompactIO
    key = (poses16.tobytes(), dirs.tobytes(), float(max_range), bool(columns))
    if key in _REFS:
        return _REFS[key]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    P, N = len(poses16), len(dirs)
    hits = lidarcast.DeviceHits(P * N, dev, want=tuple(n for n, _ in RECORD))
    out = Out(P, N, columns, dev)
    io = LrcCompactIO()
    io.t, io.point3, io.sem, io.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
    io.tile_count = hits["tile_count"].data_ptr()
    out.fill(io)
    scene.scan_poses_dev(torch.from_numpy(np.ascontiguousarray(poses16)).to(dev), torch.from_numpy(np.ascontiguousarray(dirs)).to(dev),
                         hits, max_range, st)
    scene.ctx.compact_dev(P, N, io, st)
    torch.cuda.synchronize()
    rec = {}
    for name, width in RECORD:
        nbytes = 4 * ((P * N + 63) // 64) if width is None else P * N * width
        rec[name] = hits[name].view(torch.uint8).flatten()[:nbytes].cpu().numpy().tobytes()
    _REFS[key] = (rec, out.arrays(), out.counts.cpu().numpy())
    return _REFS[key]


def _check_records(pipe, ticket, ref_rec, what):
    rec = pipe.records(ticket)
    for name, _ in RECORD:
        assert _dev_bytes(getattr(rec, name), len(ref_rec[name])) == ref_rec[name], f"{what}: records differ: {name}"


def _check_out(out, ref, what):
    _, ref_arrays, ref_counts = ref
    assert np.array_equal(out.counts.cpu().numpy(), ref_counts), what + ": per-pose counts differ"
    kk = int(ref_counts.sum())
    for name, got in out.arrays().items():
        assert np.array_equal(got[:kk], ref_arrays[name][:kk]), f"{what}: {name} differ"
        assert np.array_equal(got[kk:], ref_arrays[name][kk:]), f"{what}: {name} beyond the kept ones were touched"
    return kk


def _run(scene, dirs, batches, max_range=FAR, switch=1, columns=False, wait_after=(), records="after"):
    """batches: (P, 16) poses per submit, on one table.  wait_after: indices of submits behind which lrc_pipe_wait is called
    (one always follows the last).  records: "before" = the records of the last four submits are asked for in front of the last
    wait (rows still pending), "after" = behind it, with the caller's pose and table tensors overwritten with zeros first.
    Returns the number of rows kept in all submits."""
    import torch
    import lidarcast
    from lidarcast._capi import LrcCompactIO
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    N = len(dirs)
    refs = [_reference(scene, p, dirs, max_range, columns) for p in batches]
    d_tab = torch.from_numpy(np.ascontiguousarray(dirs)).to(dev)
    d_poses = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in batches]
    pipe = lidarcast.ScanPipe(scene, max(len(p) for p in batches), N)
    try:
        pipe.set_ray_table(switch)
        outs, tickets = [], []
        for i, (p, dp) in enumerate(zip(batches, d_poses)):
            out = Out(len(p), N, columns, dev)
            tickets.append(pipe.submit(dp, d_tab, max_range, io=out.fill(LrcCompactIO()), stream=st))
            outs.append(out)
            if i in wait_after:
                pipe.wait(st)
        last4 = list(range(max(0, len(batches) - 4), len(batches)))
        if records == "before":
            for i in reversed(last4):
                _check_records(pipe, tickets[i], refs[i][0], f"submit {i}, before the wait")
        pipe.wait(st)
        torch.cuda.synchronize()
        if records == "after":
            d_tab.zero_()
            for dp in d_poses:
                dp.zero_()
            torch.cuda.synchronize()
            for i in last4:
                _check_records(pipe, tickets[i], refs[i][0], f"submit {i}, after the wait, inputs zeroed")
        return sum(_check_out(out, ref, f"submit {i}") for i, (out, ref) in enumerate(zip(outs, refs)))
    finally:
        pipe.close()


YAWS = {"same": lambda P: [0.3] * P,                       # every tile in the record form
        "pose2": lambda P: [0.0, 0.0, 0.7, 0.0, 0.0][:P],  # a row-form pose between record-form poses
        "pose0": lambda P: [0.3] + [0.0] * (P - 1)}        # pose 0 alone has its rotation: every other pose in the row form
CASES = [(k, P) for k in ("same",) for P in (1, 2, 5)] + [("pose2", 5), ("pose0", 2), ("pose0", 5)]
tables = pytest.mark.parametrize("table", list(TABLES))
cases = pytest.mark.parametrize("kind,P", CASES)
outputs = pytest.mark.parametrize("columns", [False, True], ids=["rows", "columns"])


def _batches(kind, P, n, seed=0):
    return [_poses(YAWS[kind](P), 100 * seed + 10 * P + i) for i in range(n)]


@tables
@cases
@outputs
def test_four_submits_without_a_wait(scene, table, kind, P, columns):
    """The rows of submits 0 and 1 ride in the launches of submits 2 and 3, those of 2 and 3 leave with the plain kernel; the
    records of all four are asked for while rows are pending, and, in a second pipeline, behind the wait with the caller's
    inputs zeroed."""
    dirs = _table(table)
    b = _batches(kind, P, 4)
    assert _run(scene, dirs, b, columns=columns, records="before") > 0
    assert _run(scene, dirs, b, columns=columns, records="after") > 0


@tables
@pytest.mark.parametrize("P", [1, 2, 5])
@outputs
def test_table_switched_off(scene, table, P, columns):
    """set_ray_table(0): every tile of every submit in the row form."""
    assert _run(scene, _table(table), _batches("same", P, 3), switch=0, columns=columns) > 0


@tables
@cases
def test_a_third_of_the_rays_out_of_range(scene, table, kind, P):
    """max_range at the 2/3 quantile of the returns' ranges: masks neither full nor empty, records of dropped rays."""
    dirs = _table(table)
    b = _batches(kind, P, 3, seed=1)
    rec, _, _ = _reference(scene, np.concatenate(b), dirs, 1e6, False)
    t = np.frombuffer(rec["t"], np.float32)
    R = float(np.quantile(t[np.isfinite(t)], 2.0 / 3.0))
    kept = _run(scene, dirs, b, max_range=R)
    assert 0.5 * np.isfinite(t).sum() < kept < 0.8 * np.isfinite(t).sum()


@tables
@pytest.mark.parametrize("kind", ["same", "pose2"])
@outputs
def test_fewer_poses_into_a_set_that_held_more(scene, table, kind, columns):
    """Submits 4 to 7 write 2, 1, 3 and 1 poses into the sets (and tables) that held 5."""
    b = _batches(kind, 5, 4, seed=2) + [_poses(YAWS[kind](5)[:P], 300 + P + i) for i, P in enumerate((2, 1, 3, 1))]
    assert _run(scene, _table(table), b, columns=columns) > 0


@tables
@pytest.mark.parametrize("submits", [1, 2])
@pytest.mark.parametrize("kind,P,switch", [("same", 1, 1), ("same", 5, 1), ("pose0", 5, 1), ("pose2", 5, 1), ("same", 2, 0)])
@outputs
def test_wait_after_one_and_after_two_submits(scene, table, submits, kind, P, switch, columns):
    """The plain-kernel drain of record-form and of row-form tiles, then the pipeline goes on: two more submits and a wait."""
    b = _batches(kind, P, submits + 2, seed=3)
    assert _run(scene, _table(table), b, switch=switch, columns=columns, wait_after=(submits - 1,)) > 0


def test_the_record_form_is_what_ran(scene):
    """The cases above mean what they say: with the table on, the launch of the last submit carried one (the hook returns it),
    and its pose flags say which poses' tiles are in the record form."""
    import torch
    import lidarcast
    lib = lidarcast.load()
    lib.lrc_internal_pipe_ray_table.argtypes, lib.lrc_internal_pipe_ray_table.restype = [C.c_void_p], C.c_void_p
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    dirs = _table("4x64")
    N = len(dirs)
    d_tab = torch.from_numpy(np.ascontiguousarray(dirs)).to(dev)
    pipe = lidarcast.ScanPipe(scene, 5, N)
    try:
        seen = []
        for kind in ("same", "pose2", "pose0", "same", "pose2"):      # five submits: the fifth uses the first's set and table
            p = torch.from_numpy(_poses(YAWS[kind](5), 7)).to(dev)
            rows = torch.empty((5 * N, 4), dtype=torch.float32, device=dev)
            pipe.submit(p, d_tab, FAR, out_rows_t=rows, stream=st)
            ptr = lib.lrc_internal_pipe_ray_table(pipe._h)
            assert ptr
            seen.append(ptr)
            pipe.wait(st)
            torch.cuda.synchronize()
            flags = np.frombuffer(_dev_bytes(ptr + N * 48, 5 * 64), np.uint32).reshape(5, 16)[:, 6]
            want = {"same": [1, 1, 1, 1, 1], "pose2": [1, 1, 0, 1, 1], "pose0": [1, 0, 0, 0, 0]}[kind]
            assert flags.tolist() == want, (kind, flags)
        assert len(set(seen[:4])) == 4 and seen[4] == seen[0], "one table per record set"
        pipe.set_ray_table(0)
        pipe.submit(p, d_tab, FAR, out_rows_t=rows, stream=st)
        assert not lib.lrc_internal_pipe_ray_table(pipe._h)
        pipe.wait(st)
        torch.cuda.synchronize()
    finally:
        pipe.close()
