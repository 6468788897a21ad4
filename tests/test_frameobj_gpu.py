"""-m gpu: per-frame object annotations (csrc/lrc_frameobj.hip) against the numpy restatement (tests/frameobj_restate.py),
bit for bit: the static object table, accumulation of synthetic records, order and chunking, a real scan through the
engine, the box property, and the refusals."""
import numpy as np
import pytest

import coverage_restate as CR
import frameobj_restate as R
from helpers import assert_bit_equal, pose, random_soup, sensor_small

pytestmark = pytest.mark.gpu

FIELDS = ("returns", "seen_tris", "seen_q", "vmin", "vmax")


@pytest.fixture(scope="module")
def eng():
    from raycast_engine import RaycastEngineGPU
    return RaycastEngineGPU()


@pytest.fixture(scope="module")
def ctx(eng):
    return eng.ctx


@pytest.fixture(scope="module")
def room():
    from lidarcast import synth
    m = synth.make_room(size=(3, 3, 2.5), num_boxes=3, seed=5, cell=0.1)
    return m, R.object_table(m.vertices, m.triangles, m.triangle_sem, m.triangle_ins)


@pytest.fixture(scope="module")
def soup():
    """600 triangles, every pair its own instance: 300 objects, more than the workgroup's LDS table has rows."""
    v, f = random_soup(600, seed=3, extent=2.0, size=0.3)
    sem = np.full(600, 8, np.uint16)
    ins = (np.arange(600) // 2 + 1).astype(np.uint16)
    return (v, f, sem, ins), R.object_table(v, f, sem, ins)


def _fo(ctx, mesh, F, labels=True):
    from lidarcast import FrameObjects
    if isinstance(mesh, tuple):
        v, f, sem, ins = mesh
    else:
        v, f, sem, ins = mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins
    return FrameObjects(ctx, v, f, sem if labels else None, ins if labels else None, num_frames=F)


def _dev(a, torch_dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").view(torch_dtype)


def _acc(fo, rec, poses, N, first_frame=0, sl=None):
    import torch
    t, prim, pts = rec
    a, b = (0, len(poses)) if sl is None else sl
    fo.accumulate_dev(_dev(t[a * N:b * N], torch.float32), _dev(prim[a * N:b * N], torch.int32),
                      _dev(pts[a * N:b * N], torch.float32), poses[a:b], N, first_frame=first_frame)


def _same(res, want, what=""):
    for name in FIELDS:
        assert_bit_equal(getattr(res, name), want[name], f"{what}{name}")
    assert res.rejected_rays == want["rejected_rays"], what


# ---- 1. static table ---------------------------------------------------------------------------------------------------
def _check_table(fo, tab):
    key, cnt, tq, wmin, wmax = fo.objects()
    assert key.dtype == np.uint32 and np.array_equal(key, tab["key"])
    assert np.array_equal(cnt, tab["tri_count"]) and cnt.dtype == np.uint32
    assert np.array_equal(tq, tab["total_q"]) and tq.dtype == np.uint64
    assert_bit_equal(wmin, tab["wmin"], "wmin")
    assert_bit_equal(wmax, tab["wmax"], "wmax")


def test_static_table_room(ctx, room):
    from lidarcast import SurfaceCoverage
    m, tab = room
    assert len(m.triangles) == 12310 and len(tab["key"]) == 9
    q = CR.area_q(m.vertices, m.triangles)
    cov = SurfaceCoverage(ctx, m.vertices, m.triangles, m.triangle_sem)
    assert np.array_equal(cov.area_q(), q)                       # the shared area function left coverage's table as it was
    assert np.array_equal(tab["q"], q)
    fo = _fo(ctx, m, 2)
    assert (fo.num_triangles, fo.num_frames, fo.num_objects, fo.words_per_frame) == (12310, 2, 9, (12310 + 31) // 32)
    _check_table(fo, tab)
    v = np.asarray(m.vertices, np.float64)
    f = np.asarray(m.triangles)
    for k in range(9):                                           # the table against plain numpy, object by object
        sel = tab["obj"] == k
        assert int(fo.objects()[2][k]) == sum(int(x) for x in q[sel])
        assert np.array_equal(fo.objects()[3][k], v[f[sel].reshape(-1)].min(0))
        assert np.array_equal(fo.objects()[4][k], v[f[sel].reshape(-1)].max(0))
    r = fo.export()                                              # a fresh object: zeros and +-inf
    assert not r.returns.any() and not r.seen_tris.any() and not r.seen_q.any()
    assert (r.vmin == np.inf).all() and (r.vmax == -np.inf).all() and r.rejected_rays == 0


def test_static_table_without_labels_and_many_objects(ctx, room, soup):
    m, _ = room
    fo = _fo(ctx, m, 1, labels=False)
    assert fo.num_objects == 1
    _check_table(fo, R.object_table(m.vertices, m.triangles))
    sm, stab = soup
    fo = _fo(ctx, sm, 1)
    assert fo.num_objects == 300
    _check_table(fo, stab)


# ---- 2. synthetic records ----------------------------------------------------------------------------------------------
def _poses9():
    yaws = (0.0, 0.7, -2.0)
    rng = np.random.default_rng(11)
    ps = []
    for p in range(9):
        c = rng.uniform(0.3, 2.2, 3)
        if p % 3 == 0:
            c[p // 3] = 0.0                                      # a translation coordinate of exactly zero
        ps.append(pose(c[0], c[1], c[2], yaws[p % 3]))
    return np.stack(ps)


def _synthetic(seed, poses, N, T):
    """Records as tests/test_coverage_gpu.py::_synthetic draws them, plus the point rows."""
    P = len(poses)
    rng = np.random.default_rng(seed)
    prim = rng.integers(0, T, P * N).astype(np.uint32)
    runs = rng.random(P * N) < 0.7                                   # long runs of equal prims
    for i in range(1, P * N):
        if runs[i]:
            prim[i] = prim[i - 1]
    t = rng.uniform(0.1, 5, P * N).astype(np.float32)
    t[rng.random(P * N) < 0.1] = np.inf                             # range-filtered: valid prim, t = inf
    miss = rng.random(P * N) < 0.1
    t[miss] = np.inf
    prim[miss] = R.INVALID
    prim[rng.random(P * N) < 0.01] = R.INVALID                       # invalid prim with a finite t: ignored
    big = rng.choice(P * N, 5, replace=False)
    prim[big] = np.array([T, T + 1, T + 31, 2 * T, 0x7FFFFFFF], np.uint32)   # prim >= T with whatever t
    pts = rng.uniform(-0.2, 3.2, (P * N, 3)).astype(np.float32)
    # coordinates equal to the pose translation's, with either sign of zero where that is zero
    c32 = np.repeat(poses[:, :3, 3], N, axis=0).astype(np.float32)
    same = rng.random((P * N, 3)) < 0.05
    sign = np.where(rng.random((P * N, 3)) < 0.5, np.float32(-1.0), np.float32(1.0))
    pts[same] = (c32 * sign)[same]
    ok = np.isfinite(t) & (prim.astype(np.int64) < T)
    pts[~ok] = np.nan                                               # rows of rays that do not return must not be read
    bad = rng.choice(np.flatnonzero(ok), 3, replace=False)
    pts[bad, [0, 1, 2]] = [np.inf, -np.inf, np.inf]                  # three returned rows with an inf coordinate
    return t, prim, pts


@pytest.fixture(scope="module")
def room_records(room):
    m, tab = room
    poses = _poses9()
    rec = _synthetic(0, poses, 3000, len(m.triangles))
    return poses, rec, R.restate(tab, *rec, poses, 3000)


def test_synthetic_records_equal_restatement(ctx, room, room_records):
    m, tab = room
    poses, rec, want = room_records
    assert want["rejected_rays"] == 3 and want["returns"].sum() > 15000
    fo = _fo(ctx, m, 9)
    _acc(fo, rec, poses, 3000)
    _same(fo.export(), want)


def test_hand_made_records_on_the_device(ctx):
    """The six rays of frameobj_restate.hand_made_case: ignored rays, one triangle hit twice, the sign of a zero
    extreme, an object without a return."""
    mesh, M, rec = R.hand_made_case()
    fo = _fo(ctx, mesh, 1)
    assert fo.objects()[0].tolist() == [7 | 1 << 16, 8 | 2 << 16]
    assert fo.objects()[2].tolist() == [(1 << 31) + (1 << 32), (1 << 31) + (1 << 33)]
    _acc(fo, rec, M[None], 6)
    r = fo.export()
    for name, dt in zip(FIELDS, (np.uint32, np.uint32, np.uint64, np.float64, np.float64)):
        assert_bit_equal(getattr(r, name), np.array(R.HAND_MADE_RESULT[name], dt), name)
    assert r.rejected_rays == 0


def test_synthetic_records_many_objects_odd_width(ctx, soup):
    sm, stab = soup
    poses = _poses9()
    rec = _synthetic(1, poses, 250, 600)                             # N = 250: no multiple of 64
    want = R.restate(stab, *rec, poses, 250)
    hit = [np.flatnonzero(r) for r in want["returns"]]               # dozens of objects per frame, and in every frame
    assert min(len(h) for h in hit) > 40                             # two that share a row of the 128-row LDS table
    assert all(len(np.unique(h % 128)) < len(h) for h in hit)
    fo = _fo(ctx, sm, 9)
    _acc(fo, rec, poses, 250)
    _same(fo.export(), want)


# ---- 3. order and chunking ---------------------------------------------------------------------------------------------
def test_order_chunking_doubling_reset(ctx, room, room_records):
    m, tab = room
    poses, rec, want = room_records
    N = 3000
    fo = _fo(ctx, m, 9)
    for a, b in ((0, 2), (2, 7), (7, 9)):
        _acc(fo, rec, poses, N, first_frame=a, sl=(a, b))
    _same(fo.export(), want, "chunks: ")
    rev = _fo(ctx, m, 9)
    for p in range(8, -1, -1):
        _acc(rev, rec, poses, N, first_frame=p, sl=(p, p + 1))
    r_rev = rev.export()
    _same(r_rev, want, "reverse: ")
    _acc(fo, rec, poses, N)                                          # the same frames again
    twice = fo.export()
    assert np.array_equal(twice.returns, 2 * want["returns"]) and twice.rejected_rays == 6
    for name in FIELDS[1:]:
        assert_bit_equal(getattr(twice, name), want[name], f"second accumulation: {name}")
    fo.reset()
    z = fo.export()
    assert not z.returns.any() and not z.seen_tris.any() and not z.seen_q.any() and z.rejected_rays == 0
    assert (z.vmin == np.inf).all() and (z.vmax == -np.inf).all()
    _acc(fo, rec, poses, N)                                          # a second run gives identical bytes
    again = fo.export()
    for name in FIELDS:
        assert getattr(again, name).tobytes() == getattr(r_rev, name).tobytes(), name


# ---- 4. a real scan ----------------------------------------------------------------------------------------------------
SCAN_POSES = np.stack([pose(0.5, 1.5, 1.0, 0.0), pose(1.5, 1.5, 0.4, 0.7), pose(2.6, 1.45, 1.0, -2.0)])


def test_engine_frame_objects_equal_restatement_of_the_scan(eng, room):
    m, tab = room
    k = sensor_small(lines=5, width=50, max_range=2.2)
    res = eng.frame_objects(k, SCAN_POSES, m)
    rec, n = eng.scan_poses(k, SCAN_POSES, m, want=("t", "prim", "point3"))
    assert n == 250
    t, prim, pts = rec["t"].reshape(-1), rec["prim"].reshape(-1), rec["point3"].reshape(-1, 3).copy()
    # the room is closed, so every ray hits: the rays without a return are the range-filtered ones (the scan's records
    # carry t = inf for them, with or without the triangle id)
    assert (~np.isfinite(t)).reshape(3, -1).sum(1).tolist() == [41, 3, 35]
    pts[~np.isfinite(t)] = np.nan
    want = R.restate(tab, t, prim, pts, SCAN_POSES, n)
    _same(res, want)
    assert np.array_equal(res.key, tab["key"]) and np.array_equal(res.total_q, tab["total_q"])
    o9 = int(np.flatnonzero(res.ins == 9)[0])
    assert res.returns[1, o9] == 0 and res.returns[0, o9] > 0         # zero rows and filled rows both occur
    assert res.returns[:, o9].tolist() == [10, 0, 6]
    ceiling = np.flatnonzero(res.sem == 0)
    assert len(ceiling) and not res.returns[:, ceiling].any()
    assert (res.vmin[1, o9] == np.inf).all() and (res.vmax[1, o9] == -np.inf).all()
    # chunked scanning gives the same bytes
    res2 = eng.frame_objects(k, SCAN_POSES, m, chunk_poses=2)
    for name in FIELDS:
        assert getattr(res2, name).tobytes() == getattr(res, name).tobytes(), name


# ---- 5. property -------------------------------------------------------------------------------------------------------
def test_visible_boxes_lie_inside_the_rotated_world_boxes(eng):
    """Every return lies on its object's surface, so the visible box lies inside the sensor-frame AABB of the eight
    rotated corners of the object's world AABB.  Slack 1e-4 m: about 30 times the 2.8e-6 m the README records as the
    worst distance of a hit point to the double-precision witness; float32 point rounding at <= 25 m is below 2e-6."""
    from lidarcast import synth
    m = synth.make_room(size=(3, 3, 2.5), num_boxes=3, seed=5, cell=0.1, jitter=0)
    k = sensor_small(lines=5, width=50, max_range=20.0)
    res = eng.frame_objects(k, SCAN_POSES, m)
    assert (res.returns > 0).sum() >= 12
    corners = np.stack([np.where([(i >> a) & 1 for a in range(3)], res.wmax, res.wmin) for i in range(8)], 1)  # (K, 8, 3)
    for f, M in enumerate(SCAN_POSES):
        s = R.sensor_coords(M, corners.reshape(-1, 3).astype(np.float64)).reshape(-1, 8, 3)
        lo, hi = s.min(1), s.max(1)
        seen = res.returns[f] > 0
        assert (res.vmin[f][seen] >= lo[seen] - 1e-4).all() and (res.vmax[f][seen] <= hi[seen] + 1e-4).all()
        assert (res.vmin[f][seen] <= res.vmax[f][seen]).all()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(eng, ctx, room, room_records):
    import ctypes as C
    import lidarcast
    import torch
    from lidar import DualAxisLidarIntrinsics
    from lidarcast import FrameObjects
    m, _ = room
    poses, rec, _ = room_records
    fo = _fo(ctx, m, 4)
    with pytest.raises(ValueError):
        _acc(fo, rec, poses, 3000, first_frame=2, sl=(0, 3))          # first_frame + P > F
    with pytest.raises(ValueError):
        _acc(fo, rec, poses, 3000, first_frame=5, sl=(0, 1))
    lib = lidarcast.load()
    tt = _dev(rec[0][:3000], torch.float32)
    pt = _dev(poses[:1].reshape(-1, 16), torch.float64)
    vp = C.c_void_p
    for nul in range(4):                                              # NULL poses / t / prim / point3
        a = [vp(pt.data_ptr()), vp(tt.data_ptr()), vp(tt.data_ptr()), vp(tt.data_ptr())]
        a[nul] = None
        rc = lib.lrc_frameobj_accumulate_dev(fo._h, a[0], 1, 1000, a[1], a[2], a[3], 0, None)
        assert rc == lidarcast._capi.LRC_ERR_INVALID_ARG, nul
    r = fo.export()
    assert not r.returns.any() and r.rejected_rays == 0              # nothing was launched
    v, f = random_soup(4097, seed=1)
    ins = np.arange(4097).astype(np.uint16)
    with pytest.raises(ValueError, match="4096"):
        FrameObjects(ctx, v, f, None, ins)
    assert FrameObjects(ctx, v[:3 * 4096], f[:4096], None, ins[:4096]).num_objects == 4096
    bad = np.array(m.vertices, np.float64)
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        FrameObjects(ctx, bad, m.triangles)
    with pytest.raises(ValueError):
        FrameObjects(ctx, m.vertices, m.triangles, num_frames=0)
    with pytest.raises(NotImplementedError):
        eng.frame_objects(DualAxisLidarIntrinsics.create_blk2go_dual_axis(), np.eye(4)[None], m)
