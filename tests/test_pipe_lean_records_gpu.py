"""-m gpu: the scan pipeline's lean record sets (lrc_pipe_submit with rays_per_pose % 64 == 0 writes per ray only the packed
row and (t, slot); lrc_pipe_records expands them into the 36-byte record on demand) against lrc_scan_poses_dev +
lrc_compact_dev, bit for bit, where test_scan_pipeline_equals_scan_plus_compaction does not reach: rays dropped by the
range filter (min_range, a short max_range), range noise, records read after later submits, the full-record fallback,
and sharded and plain submits on one pipe."""
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
def scene(ctx):
    import lidarcast
    from lidarcast import synth
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=7, cell=0.04)
    s = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    yield s
    s.reset_options()


def _dev_bytes(ptr, nbytes):
    import torch
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(buf.data_ptr()), C.c_void_p(int(ptr)), nbytes, 3) == 0      # device to device
    return buf.cpu().numpy().tobytes()


class Setup:
    def __init__(self, scene, lines, width, max_range, P, seed):
        import torch
        from lidar import IndoorLidar
        self.k = sensor_small(lines=lines, width=width, max_range=max_range)
        dirs = IndoorLidar(self.k, np.eye(4)).sensor_directions()
        self.N, self.P = len(dirs), P
        self.dev = torch.device("cuda", 0)
        self.d_dirs = torch.from_numpy(dirs).to(self.dev)
        self.rng = np.random.default_rng(seed)
        self.scene = scene
        self.st = torch.cuda.current_stream().cuda_stream

    def poses(self):
        import torch
        p = np.stack([pose(0.6 + 2.8 * self.rng.random(), 0.6 + 1.8 * self.rng.random(), 0.5 + 1.5 * self.rng.random(),
                           yaw=self.rng.uniform(-3, 3)) for _ in range(self.P)])
        return torch.from_numpy(p.reshape(self.P, 16)).to(self.dev)

    def outputs(self, every_kind):
        """The caller's buffers of one submit: rows and counts, plus every other output kind when asked."""
        import torch
        from lidarcast._capi import LrcCompactIO
        n = self.P * self.N
        o = {"rows": torch.full((n, 4), -7.0, dtype=torch.float32, device=self.dev),
             "counts": torch.full((self.P,), -1, dtype=torch.int64, device=self.dev)}
        if every_kind:
            o.update(p3=torch.zeros((n, 3), dtype=torch.float32, device=self.dev),
                     sem=torch.zeros(n, dtype=torch.int16, device=self.dev),
                     ins=torch.zeros(n, dtype=torch.int16, device=self.dev),
                     idx=torch.zeros(n, dtype=torch.int32, device=self.dev),
                     rng=torch.zeros(n, dtype=torch.float32, device=self.dev))
        io = LrcCompactIO()
        io.out_xyzl, io.counts = o["rows"].data_ptr(), o["counts"].data_ptr()
        if every_kind:
            io.out_point3, io.out_sem, io.out_ins = o["p3"].data_ptr(), o["sem"].data_ptr(), o["ins"].data_ptr()
            io.out_index, io.out_range_origin = o["idx"].data_ptr(), o["rng"].data_ptr()
        return o, io

    def reference(self, d_poses, every_kind):
        """The same batch through lrc_scan_poses_dev + lrc_compact_dev on one stream: records and outputs."""
        import torch
        import lidarcast
        hits = lidarcast.DeviceHits(self.P * self.N, self.dev, want=tuple(n for n, _ in RECORD))
        o, io = self.outputs(every_kind)
        io.t, io.point3, io.sem, io.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
        io.tile_count = hits["tile_count"].data_ptr()
        self.scene.scan_poses_dev(d_poses, self.d_dirs, hits, self.k.max_range, self.st)
        self.scene.ctx.compact_dev(self.P, self.N, io, self.st)
        torch.cuda.synchronize()
        return hits, o

    def check_outputs(self, got, ref):
        import torch
        assert torch.equal(got["counts"], ref["counts"]), "per-pose counts differ"
        kk = int(ref["counts"].sum().item())
        assert torch.equal(got["rows"][:kk].view(torch.int32), ref["rows"][:kk].view(torch.int32)), "rows differ"
        assert bool((got["rows"][kk:] == -7.0).all()), "rows beyond the kept ones were touched"
        for name in ("p3", "sem", "ins", "idx", "rng"):
            if name in ref:
                a, b = got[name][:kk], ref[name][:kk]
                if a.dtype == torch.float32:
                    a, b = a.view(torch.int32), b.view(torch.int32)
                assert torch.equal(a, b), name
        return kk

    def check_records(self, pipe, ticket, hits, skip=()):
        n = self.P * self.N
        rec = pipe.records(ticket)
        for name, width in RECORD:
            if name in skip:
                continue
            nbytes = 4 * ((n + 63) // 64) if width is None else n * width
            ref = hits[name].view(__import__("torch").uint8).flatten()[:nbytes].cpu().numpy().tobytes()
            assert _dev_bytes(getattr(rec, name), nbytes) == ref, f"records differ: {name}"


def _run(scene, s, sizes_every_kind, records_lag=2):
    """Submits back to back; the records of each submit are read `records_lag` submits later (inside the four-set window)
    and again after the flush; rows, counts and every output kind against the two-call reference."""
    import torch
    import lidarcast
    pipe = lidarcast.ScanPipe(scene, s.P, s.N)
    subs = []
    for b, every in enumerate(sizes_every_kind):
        d_poses = s.poses()
        o, io = s.outputs(every)
        ticket = pipe.submit(d_poses, s.d_dirs, s.k.max_range, io=io, stream=s.st)
        subs.append((d_poses, every, ticket, o))
        if b >= records_lag:              # a lean set read after later submits: the expansion sits behind its own trace
            d_p, ev, t_, _ = subs[b - records_lag]
            torch.cuda.synchronize()
            hits, _ = s.reference(d_p, ev)
            s.check_records(pipe, t_, hits)
    pipe.wait(s.st)
    torch.cuda.synchronize()
    kept = 0
    for i, (d_poses, every, ticket, o) in enumerate(subs):
        hits, ref = s.reference(d_poses, every)
        kept += s.check_outputs(o, ref)
        if i >= len(subs) - 4:            # still inside the window: the same bytes when read again
            s.check_records(pipe, ticket, hits)
    with pytest.raises(ValueError):
        pipe.records(subs[-5][2])         # rotated out
    pipe.close()
    return kept


def test_lean_pipe_with_range_filter_drops(scene):
    """min_range and a short max_range drop hits whose triangle was found: the lean row and the keep mask must
    carry the filter's decision, not the hit's."""
    s = Setup(scene, lines=8, width=512, max_range=2.5, P=5, seed=1)
    scene.set_options(min_range=0.9)
    try:
        kept = _run(scene, s, [False, True, False, True, False, False, True])
    finally:
        scene.reset_options()
    assert 0 < kept < 7 * s.P * s.N


def test_lean_pipe_with_range_noise(scene):
    """Device range noise (one entry per ray of a call): the lean aux word carries t after the noise, and rays the noise
    makes non-positive are dropped."""
    import torch
    s = Setup(scene, lines=4, width=256, max_range=20.0, P=6, seed=2)
    g = torch.Generator(device="cpu").manual_seed(5)
    noise = (torch.randn(s.P * s.N, generator=g) * 0.05).to(torch.float32)
    noise[::97] = -50.0                   # a few returns pushed behind the sensor
    d_noise = noise.to(s.dev)
    scene.set_options(min_range=0.3, range_noise=(d_noise.data_ptr(), d_noise.numel()))
    try:
        _run(scene, s, [True, False, False, True, False, True], records_lag=3)
    finally:
        scene.reset_options()


def test_full_record_fallback_unchanged(scene):
    """rays_per_pose % 64 != 0: the pipeline keeps the complete record and the scan + compaction per stream."""
    s = Setup(scene, lines=3, width=100, max_range=3.0, P=4, seed=3)
    assert s.N % 64 != 0
    scene.set_options(min_range=0.5)
    try:
        _run(scene, s, [False, True, False, True, False])
    finally:
        scene.reset_options()


def test_sharded_and_plain_submits_on_one_pipe(scene):
    """A sharded submit (complete records, ids into the caller's send slab) between plain ones on the same pipe, the
    pending rows flushed around it: plain rows and lean records stay exact, the send slab carries the ids of the
    reference records."""
    import torch
    import lidarcast
    s = Setup(scene, lines=8, width=512, max_range=20.0, P=3, seed=4)
    pipe = lidarcast.ScanPipe(scene, s.P, s.N)
    n = s.P * s.N
    send_prim = torch.full((n,), -1, dtype=torch.int32, device=s.dev)
    send_tc = torch.full(((n + 63) // 64,), -1, dtype=torch.int32, device=s.dev)
    plan = ["plain", "plain", "flush", "sharded", "plain", "plain", "flush", "plain", "sharded", "flush"]
    subs = []
    for step in plan:
        if step == "flush":
            pipe.wait(s.st)
            continue
        d_poses = s.poses()
        if step == "plain":
            o, io = s.outputs(len(subs) % 2 == 1)
            subs.append(("plain", d_poses, pipe.submit(d_poses, s.d_dirs, s.k.max_range, io=io, stream=s.st), o))
        else:
            t_ = pipe.submit_sharded(d_poses, s.d_dirs, s.k.max_range, send_prim, send_tc, stream=s.st)
            torch.cuda.synchronize()
            hits, _ = s.reference(d_poses, False)
            assert torch.equal(send_prim, hits["prim"].view(torch.int32)), "send slab ids differ"
            assert torch.equal(send_tc, hits["tile_count"].view(torch.int32)), "send slab keep counts differ"
            subs.append(("sharded", d_poses, t_, None))
    torch.cuda.synchronize()
    for i, (kind, d_poses, ticket, o) in enumerate(subs):
        if kind != "plain":
            continue
        every = "p3" in o
        hits, ref = s.reference(d_poses, every)
        s.check_outputs(o, ref)
        if len(subs) - i <= 4:
            s.check_records(pipe, ticket, hits)
    pipe.close()
