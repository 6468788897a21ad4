"""-m gpu: the scan pipeline (lrc_pipe_*) at the shapes and schedules bench.py does not use, against the plain path --
lrc_scan_poses_dev + lrc_compact_dev of the same poses on one stream -- bit for bit: rows as int32, per-pose counts, rows
beyond the kept ones untouched.

A tile is 64 rays of one pose, a super tile 1024 tiles; tps = N / 64 tiles per pose.  The cases reach:
  * tps that does not divide 1024 (a pose's tiles straddle a super-tile boundary), tps = 1, and N > 65536 (one pose spans
    several super tiles) -- local and sharded, own slab first / middle / last;
  * more than 64 super tiles in a local submit (super_prefix_wave's loop), more than 256 in a gathered scan (the grid-stride
    loop of compact_scan_kernel behind lrc_pipe_scan_gathered), more than 512 in lrc_compact_dev (compact_base_kernel);
  * assembly lags L = (ticket of the submit that carries it) - own_ticket of 1, 2, 3 and the rejected 4, lrc_pipe_assemble at
    distances d = pp->ticket - own_ticket of 0 to 3 and the rejected 4;
  * a direction table edited in place, or freed and allocated again, between sharded steps;
  * the laboratory build (-DLRC_VARIANTS) through the pipeline.

Cases (nsuper: super tiles of one local submit / of the gathered scan of all W ranks):
  off-grid, local and W = 3   N 384 tps 6 P 200, N 960 tps 15 P 80, N 1920 tps 30 P 40, N 64 tps 1 P 1100: nsuper 2 / 4;
                              N 98304 tps 1536 P 3: nsuper 5 / 14
  large                       local C3 N 65536 tps 1024 P 80: 80; gathered W 4 P 80 at N 65536: 320;
                              lrc_compact_dev 5 x 7 000 003 (unaligned): 535, 3 x 11 534 400 (tile counts handed in): 529
  lags                        N 1920 tps 30 P 40 W 3: nsuper 2 / 4
  direction tables            N 4096 tps 64 P 5 W 3: nsuper 1 / 1"""
import os

import numpy as np
import pytest

from helpers import pose, sensor_32x2048, sensor_small

pytestmark = pytest.mark.gpu

# N: (lines, width, max poses).  P is chosen so that a submit has more than 1024 tiles, i.e. a pose straddles a boundary.
OFF_GRID = {384: (3, 128, 200),        # tps 6:    1200 tiles, pose 170 holds tiles 1020..1025
            960: (5, 192, 80),         # tps 15:   1200 tiles, pose 68 holds tiles 1020..1034
            1920: (30, 64, 40),        # tps 30:   1200 tiles, pose 34 holds tiles 1020..1049
            64: (1, 64, 1100),         # tps 1:    1100 tiles, 1100 per-pose counts
            98304: (3, 32768, 3)}      # tps 1536: 4608 tiles, every pose spans two or three super tiles


def nsuper(tiles):
    return (tiles + 1023) // 1024


def shape_id(N):
    lines, width, P = OFF_GRID[N]
    return f"N{N}-tps{N // 64}-P{P}-nsuper{nsuper(P * N // 64)}"


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
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.04)
    return lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)


def directions(sensor):
    from lidar import IndoorLidar
    return IndoorLidar(sensor, np.eye(4)).sensor_directions()


def random_poses(rng, P):
    import torch
    p = np.stack([pose(0.6 + 2.8 * rng.random(), 0.6 + 1.8 * rng.random(), 0.5 + 1.5 * rng.random(),
                       yaw=rng.uniform(-3, 3)) for _ in range(P)])
    return torch.from_numpy(p.reshape(P, 16)).to("cuda")


class Reference:
    """The plain path: lrc_scan_poses_dev into fixed-stride records, lrc_compact_dev into rows and counts."""

    WANT = ("t", "prim", "normal3", "point3", "sem", "ins", "tile_count")

    def __init__(self, scene, max_rays):
        import lidarcast
        self.scene = scene
        self.hits = lidarcast.DeviceHits(max_rays, "cuda", want=self.WANT)

    def run(self, d_poses, d_dirs, max_range, every_kind=False):
        import torch
        P, N = d_poses.shape[0], d_dirs.shape[0]
        st = torch.cuda.current_stream().cuda_stream
        o, io = outputs(P, N, every_kind)
        h = self.hits
        io.t, io.point3, io.sem, io.ins = (h[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
        io.tile_count = h["tile_count"].data_ptr()
        self.scene.scan_poses_dev(d_poses, d_dirs, h, max_range, st)
        self.scene.ctx.compact_dev(P, N, io, st)
        torch.cuda.synchronize()
        return o


def outputs(P, N, every_kind):
    """The caller's buffers of one scan: rows (-7 where nothing is written) and counts, plus every other output kind."""
    import torch
    from lidarcast._capi import LrcCompactIO
    n = P * N
    o = {"rows": torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda"),
         "counts": torch.full((P,), -1, dtype=torch.int64, device="cuda")}
    io = LrcCompactIO()
    io.out_xyzl, io.counts = o["rows"].data_ptr(), o["counts"].data_ptr()
    if every_kind:
        o.update(p3=torch.zeros((n, 3), dtype=torch.float32, device="cuda"),
                 sem=torch.zeros(n, dtype=torch.int16, device="cuda"),
                 ins=torch.zeros(n, dtype=torch.int16, device="cuda"),
                 idx=torch.zeros(n, dtype=torch.int32, device="cuda"),
                 rng=torch.zeros(n, dtype=torch.float32, device="cuda"))
        io.out_point3, io.out_sem, io.out_ins = o["p3"].data_ptr(), o["sem"].data_ptr(), o["ins"].data_ptr()
        io.out_index, io.out_range_origin = o["idx"].data_ptr(), o["rng"].data_ptr()
    return o, io


def assert_same_outputs(got, ref, what):
    import torch
    assert torch.equal(got["counts"], ref["counts"]), f"{what}: per-pose counts differ"
    kept = int(ref["counts"].sum().item())
    ne = got["rows"][:kept].view(torch.int32) != ref["rows"][:kept].view(torch.int32)
    assert not bool(ne.any()), f"{what}: {int(ne.any(1).sum())} of {kept} rows differ"
    assert bool((got["rows"][kept:] == -7.0).all()), f"{what}: rows beyond the kept ones were touched"
    for name in ("p3", "sem", "ins", "idx", "rng"):
        if name in ref:
            a, b = got[name][:kept], ref[name][:kept]
            if a.dtype == torch.float32:
                a, b = a.view(torch.int32), b.view(torch.int32)
            assert torch.equal(a, b), f"{what}: {name} differs"
    return kept


def _dev_bytes(ptr, nbytes):
    import ctypes as C
    import torch
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(buf.data_ptr()), C.c_void_p(int(ptr)), nbytes, 3) == 0      # device to device
    return buf


def run_local(scene, sensor, max_poses, sizes, seed):
    """lrc_pipe_submit back to back with `sizes` poses per submit (every other one asks for every output kind: the per-tile
    scatter; the others for rows only: the multi-tile one), one flush at the end.  Rows, counts and -- for the submits still
    inside the four-set window -- the records expanded from the lean sets, against the plain path."""
    import torch
    import lidarcast
    rng = np.random.default_rng(seed)
    d_dirs = torch.from_numpy(directions(sensor)).to("cuda")
    N = d_dirs.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    pipe = lidarcast.ScanPipe(scene, max_poses, N)
    subs = []
    for b, P in enumerate(sizes):
        d_poses = random_poses(rng, P)
        o, io = outputs(P, N, every_kind=b % 2 == 1)
        subs.append((d_poses, o, pipe.submit(d_poses, d_dirs, sensor.max_range, io=io, stream=st)))
    pipe.wait(st)
    torch.cuda.synchronize()
    ref = Reference(scene, max_poses * N)
    kept = 0
    for b, (d_poses, o, ticket) in enumerate(subs):
        r = ref.run(d_poses, d_dirs, sensor.max_range, every_kind="p3" in o)
        kept += assert_same_outputs(o, r, f"submit {b} of {sizes[b]} poses")
        if b >= len(subs) - 4:
            rec = pipe.records(ticket)
            n = sizes[b] * N
            for name, width in (("t", 4), ("prim", 4), ("normal3", 12), ("point3", 12), ("sem", 2), ("ins", 2)):
                want = ref.hits[name].view(torch.uint8).flatten()[:n * width]
                assert torch.equal(_dev_bytes(getattr(rec, name), n * width), want), f"records of submit {b}: {name}"
    pipe.close()
    return kept


class OneRank:                 # PrimGather only asks the process group for its size when sizing the receive view
    @staticmethod
    def get_world_size(group=None):
        return 1


class Sharded:
    """W ranks emulated on one GPU, as in test_sharded_scan_pipeline_assembles_the_scene_cloud: this rank (slab `own`) traces
    its pose block with lrc_pipe_submit_sharded; the "collective" -- a copy of its send slab plus scans of the other ranks'
    poses into their slabs, on a communication stream behind lrc_pipe_trace_done -- fills one of `lag + 1` gather buffers;
    lrc_pipe_scan_gathered into scan slot step % 2.  run() assembles step j in the launch of step j + lag (via "carry"), or
    with lrc_pipe_assemble just before that submit (via "assemble": d = lag - 1)."""

    def __init__(self, scene, sensor, P, W, own, lag, seed=11):
        import torch
        import lidarcast
        from lidarcast.distributed import PrimGather
        self.scene, self.sensor, self.P, self.W, self.own, self.lag = scene, sensor, P, W, own, lag
        self.dirs_host = directions(sensor)            # what d_dirs holds (the reference's table of a step)
        self.d_dirs = torch.from_numpy(self.dirs_host).to("cuda")
        self.N = N = self.d_dirs.shape[0]
        self.pipe = lidarcast.ScanPipe(scene, P, N)
        self.gathers = [PrimGather(P, N, OneRank, "cuda", world=W) for _ in range(max(lag, 2) + 1)]
        self.tl = lidarcast.DeviceHits(0, "cuda", want=())
        self.main = torch.cuda.current_stream()
        self.comm = torch.cuda.Stream()
        self.rng = np.random.default_rng(seed)
        self.steps = []        # per step: poses of all ranks, cloud, counts, own ticket, the table as traced, scanned event

    def job(self, j):
        from lidarcast import ScanPipe
        s, g = self.steps[j], self.gathers[j % len(self.gathers)]
        return ScanPipe.gathered(s["poses"], g.all_prims, g.all_tile_counts, self.P, g.stride_bytes, self.own, s["ticket"],
                                 s["cloud"], s["counts"], scan_slot=j % 2)

    def poses_of_step(self, j):
        """(W * P, 16) device poses of all ranks for step j, slab after slab (a subclass may hand in poses of its own)."""
        return random_poses(self.rng, self.W * self.P)

    def trace(self, carry=None):
        """One step: the own submit (carrying the assembly of step `carry`), then the collective of its slabs."""
        import torch
        j = len(self.steps)
        P, W, N, own = self.P, self.W, self.N, self.own
        all_poses = self.poses_of_step(j)
        self.steps.append({"poses": all_poses, "dirs": self.dirs_host,
                           "cloud": torch.full((W * P * N, 4), -7.0, dtype=torch.float32, device="cuda"),
                           "counts": torch.full((W * P,), -1, dtype=torch.int64, device="cuda"), "scanned": None})
        g = self.gathers[j % len(self.gathers)]
        asm = None
        if carry is not None:
            self.main.wait_event(self.steps[carry]["scanned"])
            asm = self.job(carry)
        ticket = self.pipe.submit_sharded(all_poses[own * P:(own + 1) * P], self.d_dirs, self.sensor.max_range, g.prim,
                                          g.tile_count, assemble=asm, stream=self.main.cuda_stream)
        self.steps[j]["ticket"] = ticket
        self.pipe.trace_done(ticket, self.comm.cuda_stream)
        with torch.cuda.stream(self.comm):
            g.all_slabs[own * g.words:(own + 1) * g.words].copy_(g.slab)
            for v in range(W):
                if v != own:
                    self.tl.struct.prim = g.all_slabs[v * g.words:].data_ptr()
                    self.tl.struct.tile_count = g.all_slabs[v * g.words + g.n:].data_ptr()
                    self.scene.scan_poses_dev(all_poses[v * P:(v + 1) * P], self.d_dirs, self.tl, self.sensor.max_range,
                                              self.comm.cuda_stream)
        return j

    def scan(self, j):
        import torch
        with torch.cuda.stream(self.comm):
            self.pipe.scan_gathered(self.d_dirs, self.job(j), self.comm.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(self.comm)
        self.steps[j]["scanned"] = ev

    def assemble(self, j):
        self.main.wait_event(self.steps[j]["scanned"])
        self.pipe.assemble(self.d_dirs, self.job(j), self.main.cuda_stream)

    def run(self, steps, via="carry", before_step=None):
        """`steps` steps; the scan of step j is enqueued behind the collective of step j + max(0, lag - 2), so that scan slot
        j % 2 is free again (its previous assembly has been enqueued); the last `lag` steps are assembled at the end."""
        delay = max(0, self.lag - 2)
        for s in range(steps):
            if before_step:
                before_step(self, s)
            j = s - self.lag
            if via == "assemble" and j >= 0:
                self.assemble(j)
            self.trace(carry=j if via == "carry" and j >= 0 else None)
            if s - delay >= 0:
                self.scan(s - delay)
        for j in range(max(0, steps - self.lag), steps):
            if self.steps[j]["scanned"] is None:
                self.comm.wait_stream(self.main)       # the slot's previous assembly first
                self.scan(j)
            self.assemble(j)
        self.finish()

    def finish(self):
        import torch
        self.pipe.wait(self.main.cuda_stream)
        torch.cuda.synchronize()

    def check(self):
        import torch
        W, P, N = self.W, self.P, self.N
        ref = Reference(self.scene, W * P * N)
        for j, s in enumerate(self.steps):
            r = ref.run(s["poses"], torch.from_numpy(s["dirs"]).to("cuda"), self.sensor.max_range)
            kept = assert_same_outputs({"rows": s["cloud"], "counts": s["counts"]}, r, f"step {j}")
            assert 0 < kept
        self.pipe.close()


# ---- 1. off-grid fused shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", list(OFF_GRID), ids=shape_id)
def test_local_pipe_off_grid_shapes(scene, N):
    """One pipe, submits of max_poses, 1 and in-between poses: segment_count and the two lean scatters where a pose's tiles
    straddle a super tile (tps does not divide 1024), with one tile per pose, and with poses longer than a super tile."""
    lines, width, P = OFF_GRID[N]
    sensor = sensor_small(lines=lines, width=width, max_range=3.0)
    sizes = [P, 1, P, P // 2 + 1, 1, P - 1, P]
    assert run_local(scene, sensor, P, sizes, seed=N) > 0


@pytest.mark.parametrize("own", [0, 1, 2], ids=["own-first", "own-middle", "own-last"])
@pytest.mark.parametrize("N", list(OFF_GRID), ids=shape_id)
def test_sharded_pipe_off_grid_shapes(scene, N, own):
    """W = 3, lag 2: rebuild_counts, rebuild_tiles and the own rows' scatter at gathered offsets where poses straddle super
    tiles (the gathered scan has 3 * P * tps tiles)."""
    lines, width, P = OFF_GRID[N]
    r = Sharded(scene, sensor_small(lines=lines, width=width, max_range=3.0), P, W=3, own=own, lag=2, seed=N + own)
    r.run(steps=4)
    r.check()


# ---- 2. large scans -------------------------------------------------------------------------------------------------------
def test_local_pipe_more_than_64_super_tiles(scene):
    """The C3 sensor (65 536 rays per pose, 1024 tiles) at P = 80: 80 super tiles, so super_prefix_wave loops twice."""
    sensor = sensor_32x2048()
    assert nsuper(80 * 1024) == 80
    assert run_local(scene, sensor, 80, [80, 80, 37, 80], seed=64) > 0


def test_gathered_scan_more_than_256_super_tiles(scene):
    """W = 4 ranks of P = 80 poses at 65 536 rays: 327 680 gathered tiles, 320 super tiles -- more than the 256 waves
    lrc_pipe_scan_gathered gives compact_scan_kernel, whose grid-stride loop therefore runs twice."""
    r = Sharded(scene, sensor_32x2048(), 80, W=4, own=2, lag=2, seed=256)
    assert nsuper(4 * 80 * 1024) == 320
    r.run(steps=3)
    r.check()


@pytest.mark.parametrize("nseg,seg_len,handed_counts", [(5, 7_000_003, False), (3, 11_534_400, True)],
                         ids=["nsuper535-counted", "nsuper529-tile-counts"])
def test_compaction_more_than_512_super_tiles(ctx, nseg, seg_len, handed_counts):
    """lrc_compact_dev over more than 512 super tiles (> 33.5 M entries): the bases come from compact_base_kernel instead of
    being summed inline.  Reference: torch's boolean-mask selection (stable) on the same device tensors."""
    import torch
    from lidarcast._capi import LrcCompactIO
    n = nseg * seg_len
    tps = (seg_len + 63) // 64
    assert nsuper(nseg * tps) > 512
    g = torch.Generator(device="cuda").manual_seed(seg_len)
    t = torch.rand(n, generator=g, device="cuda") * 10
    t[torch.rand(n, generator=g, device="cuda") < 0.37] = float("inf")
    p3 = torch.randn((n, 3), generator=g, device="cuda")
    sem = torch.randint(0, 13, (n,), generator=g, device="cuda", dtype=torch.int16)
    ins = torch.randint(-32768, 32767, (n,), generator=g, device="cuda", dtype=torch.int16)
    rows = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((nseg,), -1, dtype=torch.int64, device="cuda")
    io = LrcCompactIO()
    io.t, io.point3, io.sem, io.ins = t.data_ptr(), p3.data_ptr(), sem.data_ptr(), ins.data_ptr()
    io.out_xyzl, io.out_index, io.counts = rows.data_ptr(), idx.data_ptr(), counts.data_ptr()
    keep = torch.isfinite(t)
    if handed_counts:                  # seg_len % 64 == 0: the per-tile keep counts come from the caller (as from a scan)
        assert seg_len % 64 == 0
        tile_count = keep.view(-1, 64).sum(1, dtype=torch.int32)
        io.tile_count = tile_count.data_ptr()
    ctx.compact_dev(nseg, seg_len, io, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(counts, keep.view(nseg, seg_len).sum(1))
    kept = int(keep.sum().item())
    label = (sem.long() & 0xFFFF) | ((ins.long() & 0xFFFF) << 16)          # uint32 bits as int32
    label = torch.where(label >= 2 ** 31, label - 2 ** 32, label).to(torch.int32)
    want = torch.cat([p3.view(torch.int32), label[:, None]], 1)[keep]
    assert torch.equal(rows[:kept].view(torch.int32), want), "rows differ"
    assert bool((rows[kept:] == -7.0).all()), "rows beyond the kept ones were touched"
    pos = torch.arange(seg_len, dtype=torch.int32, device="cuda").repeat(nseg)
    assert torch.equal(idx[:kept], pos[keep]), "indices differ"
    assert bool((idx[kept:] == -1).all())


# ---- 3. assembly lags -----------------------------------------------------------------------------------------------------
LAG_SENSOR = dict(lines=30, width=64, max_range=3.0)      # N = 1920, tps 30; 3 ranks of 40 poses: 3600 gathered tiles


@pytest.mark.parametrize("lag", [1, 2, 3])
def test_sharded_assembly_lags(scene, lag):
    """The assembly of step j carried by the submit of step j + lag: lag 1 and 3 run it in a launch on the other trace stream
    than the one that rewrites the own records four submits later."""
    r = Sharded(scene, sensor_small(**LAG_SENSOR), 40, W=3, own=1, lag=lag, seed=100 + lag)
    r.run(steps=8)
    r.check()


@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_assemble_distances(scene, d):
    """lrc_pipe_assemble of step j called when d = pp->ticket - own_ticket further submits have been made."""
    r = Sharded(scene, sensor_small(**LAG_SENSOR), 40, W=3, own=0, lag=d + 1, seed=200 + d)
    r.run(steps=7, via="assemble")
    r.check()


def test_lag_4_is_rejected(scene):
    """A submit may not carry the assembly of the submit four tickets before it (its own trace would rewrite the records the
    assembly reads: check_gathered let pp->ticket - own_ticket == 3 through), nor may lrc_pipe_assemble or
    lrc_pipe_scan_gathered reach back four submits: ValueError, raised on the host before anything is enqueued.  The same
    pipe then goes on at lag 3 and d = 3, and every step it assembled is exact."""
    r = Sharded(scene, sensor_small(**LAG_SENSOR), 40, W=3, own=2, lag=4, seed=300)
    for _ in range(4):                 # tickets 1..4, nothing carried
        r.trace()
    r.scan(0)
    r.scan(1)
    r.main.wait_event(r.steps[0]["scanned"])
    with pytest.raises(ValueError):    # would be ticket 5 carrying ticket 1: lag 4
        r.pipe.submit_sharded(r.steps[0]["poses"][:r.P], r.d_dirs, r.sensor.max_range, r.gathers[4].prim,
                              r.gathers[4].tile_count, assemble=r.job(0), stream=r.main.cuda_stream)
    r.assemble(0)                      # d = 3
    r.trace(carry=1)                   # ticket 5 carries ticket 2: lag 3
    r.trace()                          # ticket 6
    with pytest.raises(ValueError):    # ticket 2 is four submits back: d = 4
        r.pipe.assemble(r.d_dirs, r.job(1), r.main.cuda_stream)
    with pytest.raises(ValueError):
        r.pipe.scan_gathered(r.d_dirs, r.job(1), r.comm.cuda_stream)
    r.comm.wait_stream(r.main)         # scan slot 0: step 0's assembly first
    r.scan(2)
    r.main.wait_event(r.steps[2]["scanned"])
    with pytest.raises(ValueError):    # would be ticket 7 carrying ticket 3: lag 4
        r.pipe.submit_sharded(r.steps[2]["poses"][:r.P], r.d_dirs, r.sensor.max_range, r.gathers[2].prim,
                              r.gathers[2].tile_count, assemble=r.job(2), stream=r.main.cuda_stream)
    r.assemble(2)                      # d = 3
    for j in (3, 4, 5):
        r.comm.wait_stream(r.main)
        r.scan(j)
        r.assemble(j)
    r.finish()
    r.check()


# ---- 4. direction table changes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["in-place", "reallocated"])
def test_direction_table_changes_between_sharded_steps(scene, how):
    """The table of the run changes twice (8 x 512 -> 16 x 256 -> 8 x 512 lines, the same N), edited in place or freed and
    allocated again (torch's allocator may hand back the same address).  The other ranks' rows of every step must be rebuilt
    along the table that step was traced with: lrc_pipe_scan_gathered transposes the table it is given on every call."""
    import torch
    a = directions(sensor_small(lines=8, width=512, max_range=3.0))
    b = directions(sensor_small(lines=16, width=256, max_range=3.0))
    assert a.shape == b.shape and not np.array_equal(a, b)
    r = Sharded(scene, sensor_small(lines=8, width=512, max_range=3.0), 5, W=3, own=1, lag=2, seed=400)
    reused = []

    def change(r, s):
        if s not in (3, 6):
            return
        torch.cuda.synchronize()       # nothing reads the old contents any more (lidarcast.h: inputs of a submit)
        r.dirs_host = b if s == 3 else a
        new = torch.from_numpy(r.dirs_host)
        if how == "in-place":
            r.d_dirs.copy_(new)
        else:
            old = r.d_dirs.data_ptr()
            r.d_dirs = None
            r.d_dirs = new.to("cuda")
            reused.append(r.d_dirs.data_ptr() == old)

    r.run(steps=8, before_step=change)
    assert [s["dirs"] is b for s in r.steps] == [False] * 3 + [True] * 3 + [False] * 2
    r.check()


# ---- 5. the laboratory build ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"LRC_LEAFW": "1"}], ids=["lab-default", "lab-leafw1"])
def test_pipeline_in_the_laboratory_build(env):
    """This file (but this test), the two pipeline tests of test_parity_gpu.py and test_pipe_lean_records_gpu.py in a child
    process that loads the laboratory build (LRC_LIB): its default dispatch (four-wide quantised nodes) and LRC_LEAFW=1.
    A pipelined launch there must take the product dispatch, whose grid holds the leading workgroups."""
    import re
    import subprocess
    import sys
    import __graft_entry__ as entry
    from conftest import REPO
    tests = os.path.join(REPO, "tests")
    parity = os.path.join(tests, "test_parity_gpu.py")
    args = [os.path.join(tests, "test_pipe_edges_gpu.py"), parity + "::test_scan_pipeline_equals_scan_plus_compaction",
            parity + "::test_sharded_scan_pipeline_assembles_the_scene_cloud", os.path.join(tests, "test_pipe_lean_records_gpu.py")]
    r = subprocess.run([sys.executable, "-m", "pytest", *args, "-q", "-x", "-m", "gpu", "-k", "not laboratory"],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, LRC_LIB=entry.LAB_LIB, **env), cwd=REPO)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0 and re.search(r"\d+ passed", r.stdout), tail
    assert not re.search(r"\d+ (failed|skipped|errors?)\b", r.stdout), tail
