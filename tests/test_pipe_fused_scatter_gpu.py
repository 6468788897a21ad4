"""-m gpu: where the scan pipeline scatters the rows of a submit -- in the leading workgroups of the trace launch two submits
later, or in lrc_pipe_wait -- must not show in the result.  Rows and per-pose counts against lrc_scan_poses_dev +
lrc_compact_dev, bit for bit: equal batches, ragged sequences (the earlier batch larger than, equal to and smaller than the
launch that carries its rows), tile counts that are no multiple of a leading workgroup's eight, a wait in the middle, a single
submit, other output kinds between rows-only submits, rows without counts, an open scene whose tiles are partly and wholly
empty, three rotating output buffers reused across waits.  Written for the fused scatter of profiles/pipe_fused_scatter.txt
(tools/pipe_fused_scatter.patch passes it in all three placements); kept for the streaming scatter that was merged instead."""
import numpy as np
import pytest

from helpers import pose, sensor_small

pytestmark = pytest.mark.gpu

FILL = -7.0


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
    m = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=11, cell=0.04)
    return lidarcast.Scene(ctx, m.vertices, m.triangles, m.triangle_sem, m.triangle_ins)


@pytest.fixture(scope="module")
def open_room(ctx):
    """The same kind of room with every triangle beyond x = 1.8 m taken away: rays that leave through the opening hit
    nothing, so keep masks are not all ones and whole tiles are empty."""
    import lidarcast
    from lidarcast import synth
    m = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=12, cell=0.04)
    near = m.vertices[m.triangles].mean(axis=1)[:, 0] < 1.8
    return lidarcast.Scene(ctx, m.vertices, np.ascontiguousarray(m.triangles[near]),
                           np.ascontiguousarray(m.triangle_sem[near]), np.ascontiguousarray(m.triangle_ins[near]))


class Rig:
    """One sensor on one scene: the pipeline under test and the two-call reference on the caller's stream."""

    def __init__(self, scene, lines, width, max_poses, seed, max_range=20.0):
        import torch
        import lidarcast
        from lidar import IndoorLidar
        self.scene = scene
        self.k = sensor_small(lines=lines, width=width, max_range=max_range)
        dirs = IndoorLidar(self.k, np.eye(4)).sensor_directions()
        self.N, self.max_poses = len(dirs), max_poses
        assert self.N % 64 == 0
        self.dev = torch.device("cuda", 0)
        self.d_dirs = torch.from_numpy(dirs).to(self.dev)
        self.rng = np.random.default_rng(seed)
        self.st = torch.cuda.current_stream().cuda_stream
        self.pipe = lidarcast.ScanPipe(scene, max_poses, self.N)

    def poses(self, P):
        import torch
        p = np.stack([pose(0.6 + 2.8 * self.rng.random(), 0.6 + 1.8 * self.rng.random(), 0.5 + 1.5 * self.rng.random(),
                           yaw=self.rng.uniform(-3, 3)) for _ in range(P)])
        return torch.from_numpy(p.reshape(P, 16)).to(self.dev)

    def buffers(self, P, every_kind=False):
        import torch
        n = P * self.N
        o = {"rows": torch.full((n, 4), FILL, dtype=torch.float32, device=self.dev),
             "counts": torch.full((P,), -1, dtype=torch.int64, device=self.dev)}
        if every_kind:
            o.update(p3=torch.zeros((n, 3), dtype=torch.float32, device=self.dev),
                     sem=torch.zeros(n, dtype=torch.int16, device=self.dev),
                     ins=torch.zeros(n, dtype=torch.int16, device=self.dev),
                     idx=torch.zeros(n, dtype=torch.int32, device=self.dev),
                     rng=torch.zeros(n, dtype=torch.float32, device=self.dev))
        return o

    def io_of(self, o, with_counts=True):
        from lidarcast._capi import LrcCompactIO
        io = LrcCompactIO()
        io.out_xyzl = o["rows"].data_ptr()
        if with_counts:
            io.counts = o["counts"].data_ptr()
        if "p3" in o:
            io.out_point3, io.out_sem, io.out_ins = o["p3"].data_ptr(), o["sem"].data_ptr(), o["ins"].data_ptr()
            io.out_index, io.out_range_origin = o["idx"].data_ptr(), o["rng"].data_ptr()
        return io

    def submit(self, d_poses, o, with_counts=True):
        return self.pipe.submit(d_poses, self.d_dirs, self.k.max_range, io=self.io_of(o, with_counts), stream=self.st)

    def reference(self, d_poses, every_kind=False):
        import torch
        import lidarcast
        P = d_poses.shape[0]
        hits = lidarcast.DeviceHits(P * self.N, self.dev, want=("t", "prim", "normal3", "point3", "sem", "ins", "tile_count"))
        o = self.buffers(P, every_kind)
        io = self.io_of(o)
        io.t, io.point3, io.sem, io.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
        io.tile_count = hits["tile_count"].data_ptr()
        self.scene.scan_poses_dev(d_poses, self.d_dirs, hits, self.k.max_range, self.st)
        self.scene.ctx.compact_dev(P, self.N, io, self.st)
        torch.cuda.synchronize()
        return o, hits["tile_count"][: P * self.N // 64].clone()

    def check(self, got, ref, with_counts=True, what=""):
        import torch
        if with_counts:
            assert torch.equal(got["counts"], ref["counts"]), f"per-pose counts differ {what}"
        kk = int(ref["counts"].sum().item())
        assert torch.equal(got["rows"][:kk].view(torch.int32), ref["rows"][:kk].view(torch.int32)), f"rows differ {what}"
        assert bool((got["rows"][kk:] == FILL).all()), f"rows beyond the kept ones were touched {what}"
        for name in ("p3", "sem", "ins", "idx", "rng"):
            if name in ref:
                a, b = got[name][:kk], ref[name][:kk]
                if a.dtype == torch.float32:
                    a, b = a.view(torch.int32), b.view(torch.int32)
                assert torch.equal(a, b), f"{name} {what}"
        return kk


def _sequence(rig, plan):
    """plan: pose counts, "wait", or (pose count, "every") for a submit that asks for every output kind.  Every submit has
    buffers of its own; all are compared after the final wait."""
    import torch
    subs = []
    for step in plan:
        if step == "wait":
            rig.pipe.wait(rig.st)
            continue
        P, every = (step[0], True) if isinstance(step, tuple) else (step, False)
        d_poses = rig.poses(P)
        o = rig.buffers(P, every)
        rig.submit(d_poses, o)
        subs.append((d_poses, every, o))
    rig.pipe.wait(rig.st)
    torch.cuda.synchronize()
    kept = 0
    for i, (d_poses, every, o) in enumerate(subs):
        ref, _ = rig.reference(d_poses, every)
        kept += rig.check(o, ref, what=f"(submit {i}, {d_poses.shape[0]} poses)")
    return kept


def test_equal_batches(room):
    rig = Rig(room, lines=8, width=512, max_poses=6, seed=1)
    assert _sequence(rig, [6] * 7) > 0
    rig.pipe.close()


def test_ragged_batches(room):
    """The earlier batch larger than (64 -> 3 two submits on, 64 -> 1), equal to and smaller than (3 -> 17, 1 -> 64) the
    launch that carries its rows."""
    rig = Rig(room, lines=4, width=256, max_poses=64, seed=2)
    assert _sequence(rig, [64, 3, 64, 1, 17, 64, 2, 64, 64, 5]) > 0
    rig.pipe.close()


def test_tile_count_not_a_multiple_of_the_leading_tile_group(room):
    """64 rays per pose: one tile per pose, so the number of tiles of a batch is any number, also one that is not a multiple
    of the tiles a leading workgroup takes."""
    rig = Rig(room, lines=1, width=64, max_poses=40, seed=3)
    assert rig.N == 64
    assert _sequence(rig, [13, 3, 9, 40, 11, 1, 40, 7, 21]) > 0
    rig.pipe.close()


def test_one_pose_pipeline(room):
    rig = Rig(room, lines=8, width=512, max_poses=1, seed=4)
    assert _sequence(rig, [1] * 6) > 0
    rig.pipe.close()


def test_wait_in_the_middle(room):
    rig = Rig(room, lines=4, width=256, max_poses=9, seed=5)
    assert _sequence(rig, [9, 4, 9, "wait", 9, "wait", 2, 9, 9, 9, "wait", "wait", 3]) > 0
    rig.pipe.close()


def test_single_submit_then_wait(room):
    rig = Rig(room, lines=8, width=512, max_poses=5, seed=6)
    assert _sequence(rig, [5]) > 0
    assert _sequence(rig, [3]) > 0          # and the pipe goes on after it
    rig.pipe.close()


def test_other_output_kinds_between_rows_only_submits(room):
    rig = Rig(room, lines=4, width=256, max_poses=7, seed=7)
    assert _sequence(rig, [7, (7, "every"), 7, 7, (3, "every"), (7, "every"), 5, 7, 7]) > 0
    rig.pipe.close()


def test_rows_without_counts(room):
    """No per-pose counts asked for: the leading workgroups are sized by the tiles alone and the count buffer stays untouched."""
    import torch
    rig = Rig(room, lines=4, width=256, max_poses=8, seed=8)
    subs = []
    for P in (8, 8, 8, 5, 8, 8):
        d_poses = rig.poses(P)
        o = rig.buffers(P)
        rig.submit(d_poses, o, with_counts=False)
        subs.append((d_poses, o))
    rig.pipe.wait(rig.st)
    torch.cuda.synchronize()
    for i, (d_poses, o) in enumerate(subs):
        ref, _ = rig.reference(d_poses)
        rig.check(o, ref, with_counts=False, what=f"(submit {i})")
        assert bool((o["counts"] == -1).all())
    rig.pipe.close()


def test_open_scene_with_empty_and_partial_tiles(open_room):
    import torch
    rig = Rig(open_room, lines=8, width=512, max_poses=12, seed=9)
    d_probe = rig.poses(12)
    _, tc = rig.reference(d_probe)
    assert int((tc == 0).sum()) > 0 and int(((tc > 0) & (tc < 64)).sum()) > 0 and int((tc == 64).sum()) > 0, \
        "the scene must give empty, partial and full tiles"
    kept = _sequence(rig, [12, 12, 5, 12, 12, 1, 12])
    assert 0 < kept < (12 * 5 + 6) * rig.N
    rig.pipe.close()


def test_three_rotating_buffers_reused_across_waits(open_room):
    """The caller's pattern: three row / count buffers in rotation, a wait every few submits, the buffers of a submit read
    after the wait that follows it and then reused."""
    import torch
    rig = Rig(open_room, lines=8, width=512, max_poses=10, seed=10)
    bufs = [rig.buffers(10) for _ in range(3)]
    inflight = []
    checked = 0
    for i in range(14):
        P = (10, 10, 4, 10)[i % 4]
        d_poses = rig.poses(P)
        o = bufs[i % 3]
        o["rows"].fill_(FILL)
        o["counts"].fill_(-1)
        rig.submit(d_poses, o)
        inflight.append((i, d_poses, o))
        if len(inflight) == 3 or i == 13:
            rig.pipe.wait(rig.st)
            torch.cuda.synchronize()
            for j, d_p, oo in inflight:
                ref, _ = rig.reference(d_p)
                n = d_p.shape[0]
                got = {"rows": oo["rows"][: n * rig.N], "counts": oo["counts"][:n]}
                rig.check(got, ref, what=f"(submit {j})")
                checked += 1
            inflight = []
    assert checked == 14
    rig.pipe.close()
