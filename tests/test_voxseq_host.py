"""CPU: dynamic occupancy without a GPU -- the host step lrc_voxseq_walk (compiled from the inline functions the walk kernel
calls, csrc/lrc_voxwalk.h) against tests/voxgrid_restate.walk bit for bit on a hostile segment set, the restatement's own
additions (slots, STATIC_ONLY, the mover vote, skipped) against hand answers, the refusals of create and of
export_dynamic_occupancy that need no device, and the new symbols against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import voxgrid_restate as VR
import voxseq_restate as SR
from conftest import REPO

ORIGIN, S, DIMS = (-0.5, 0.25, -1.0), 0.25, (5, 7, 33)
V = DIMS[0] * DIMS[1] * DIMS[2]

NEW = ("lrc_voxseq_create", "lrc_voxseq_destroy", "lrc_voxseq_get_info", "lrc_voxseq_reset", "lrc_voxseq_accumulate_dev",
       "lrc_voxseq_finalize", "lrc_voxseq_finalize_dev", "lrc_voxseq_export_bits", "lrc_voxseq_walk")


@pytest.fixture(scope="module")
def segments():
    o, e = SR.hostile_segments(origin=ORIGIN, s=S, dims=DIMS)
    free, end, ok, visited = VR.walk(o, e, ORIGIN, S, DIMS)
    return o, e, free, end, ok, visited


def test_the_segment_set_holds_what_it_promises(segments):
    o, e, free, end, ok, visited = segments
    assert len(o) == 4096 and V == 1155 and V % 32 != 0
    a = VR.voxel_of(o.astype(np.float64), ORIGIN, S)
    fin = np.isfinite(o).all(1) & np.isfinite(e).all(1)
    assert (~VR.inside(a[ok].astype(np.int64), DIMS)).sum() >= 64                      # starts outside the grid
    assert (ok & (visited == 1)).sum() >= 64                                            # a == b
    d = (e - o)[fin]
    assert ((d != 0).sum(1) == 1).sum() >= 3 * 40                                       # axis-parallel
    assert np.isnan(e).any() and np.isinf(e).any() and np.isnan(o).any()
    assert (~ok).sum() == 6 and (~ok[fin]).sum() == 3                                   # three beyond 2^31 voxels or 2^24 steps
    # exact ties: segments whose first crossings coincide on two or three axes
    D = (e.astype(np.float64) - o.astype(np.float64))
    with np.errstate(all="ignore"):
        b = VR.voxel_of(e.astype(np.float64), ORIGIN, S)
        plane = np.asarray(ORIGIN) + (a + (b > a)) * S
        tmax = np.where(b != a, (plane - o) / D, np.inf)
    ties = ok & (((tmax[:, 0] == tmax[:, 1]) & np.isfinite(tmax[:, 0])) | ((tmax[:, 1] == tmax[:, 2]) & np.isfinite(tmax[:, 1])))
    assert ties.sum() >= 64
    assert free.any()


def test_host_walk_matches_the_restated_walk_bit_for_bit(segments):
    from lidarcast import voxseq
    o, e, free, end, ok, _ = segments
    bits, b, rejected = voxseq.walk(o, e, ORIGIN, S, DIMS)
    assert bits.dtype == np.uint32 and len(bits) == (V + 31) // 32
    assert np.array_equal(bits, SR.pack_bits(free, V))
    assert np.array_equal(rejected, ~ok)
    assert np.array_equal(b, end) and b.dtype == np.int64
    # the 4096 segments together set nearly every bit, so the special segments are also compared one at a time
    for r in np.r_[0:40, 60:70, 100:110, 128:140, 176:186, 224:236, 272:380, 4000:4010]:
        w, _, _ = voxseq.walk(o[r:r + 1], e[r:r + 1], ORIGIN, S, DIMS)
        f1, _, _, _ = VR.walk(o[r:r + 1], e[r:r + 1], ORIGIN, S, DIMS)
        assert np.array_equal(w, SR.pack_bits(f1, V)), r


def test_host_walk_on_hand_answers():
    from lidarcast import voxseq
    bits, b, rej = voxseq.walk([[0.5, 0.5, 0.5]], [[2.5, 2.5, 2.5]], (0, 0, 0), 1.0, (3, 3, 3))
    want = {(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1)}                      # ties x, then y, then z
    got = {tuple(int(x) for x in np.unravel_index(v, (3, 3, 3))) for v in range(27) if bits[v >> 5] >> (v & 31) & 1}
    assert got == want and list(b[0]) == [2, 2, 2] and not rej[0]
    bits, b, rej = voxseq.walk([[0.2, 0.2, 0.2]], [[0.7, 0.6, 0.9]], (0, 0, 0), 1.0, (3, 3, 3))     # a == b carves nothing
    assert not bits.any() and list(b[0]) == [0, 0, 0]
    with pytest.raises(ValueError):
        voxseq.walk([[0, 0, 0]], [[1, 1, 1]], (0, 0, 0), 0.0, (3, 3, 3))


def test_restatement_slots_static_only_and_mover_vote():
    dims, F = (10, 3, 3), 3
    org = np.float32([[0.5, 1.5, 1.5], [0.5, 0.5, 0.5], [0.5, 1.5, 1.5]])                          # three poses, two rays each
    p3 = np.float32([[4.5, 1.5, 1.5], [4.5, 1.5, 1.5], [2.5, 0.5, 0.5], [0, 0, 0], [6.5, 1.5, 1.5], [6.5, 1.5, 1.5]])
    t = np.float32([4, 4, 2, np.inf, 6, 6])
    sem, ins = np.uint16([13, 1, 2, 0, 5, 5]), np.uint16([7, 0, 0, 0, 1, 1])
    mover = np.uint8([2, 0, 0, 0, 1, 1])
    r = SR.sequence_from_records(org, False, [1, 0, 9], t, p3, sem, ins, mover, F, (0, 0, 0), 1.0, dims)
    assert r["skipped"] == 2 and list(r["frame_offsets"]) == [0, 1, 2, 2]
    v41 = (4 * 3 + 1) * 3 + 1
    assert list(r["idx"]) == [(2 * 3 + 0) * 3 + 0, v41]
    # slot 1, voxel (4,1,1): one return off mover 2 (sem 13), one off the room (sem 1): sem ties to 1, mover ties to 0
    assert list(r["sem"]) == [2, 1] and list(r["mover"]) == [0, 0] and list(r["mover_returns"]) == [0, 1]
    assert list(r["returns"]) == [1, 2]
    assert r["state"][1].reshape(dims)[:4, 1, 1].tolist() == [VR.FREE] * 4 and r["state"][2].max() == VR.UNKNOWN
    assert r["counts"][1].tolist() == [1, 4, 1, 90 - 5, 0, 2]
    s = SR.sequence_from_records(org, False, [1, 0, 9], t, p3, sem, ins, mover, F, (0, 0, 0), 1.0, dims, static_only=True)
    assert list(s["returns"]) == [1, 1] and list(s["sem"]) == [2, 1] and list(s["mover_returns"]) == [0, 0]
    assert np.array_equal(s["free"], r["free"])                                                     # a mover's ray still carves
    # per-ray origins repeated give the per-pose result
    q = SR.sequence_from_records(np.repeat(org, 2, 0), True, [1, 0, 9], t, p3, sem, ins, mover, F, (0, 0, 0), 1.0, dims)
    for k in ("idx", "sem", "ins", "returns", "mover", "mover_returns", "state", "counts", "frame_offsets"):
        assert np.array_equal(q[k], r[k]), k
    # a majority for the mover
    r2 = SR.sequence_from_records(org[:1], False, [0], np.float32([4, 4, 4]), np.float32([[4.5, 1.5, 1.5]] * 3),
                                  np.uint16([13, 13, 1]), np.uint16([7, 7, 0]), np.uint8([3, 3, 0]), 1, (0, 0, 0), 1.0, dims)
    assert list(r2["mover"]) == [3] and list(r2["mover_returns"]) == [2] and list(r2["sem"]) == [13] and list(r2["ins"]) == [7]


def test_new_symbols_load_and_match_the_header():
    from lidarcast import _capi
    lib = _capi.load()
    header = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    width = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double, "int": C.c_int}
    for name in NEW:
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
        args = [a.strip() for a in re.search(rf"\bint {name}\((.*?)\);", src, re.S).group(1).split(",")]
        got = getattr(lib, name).argtypes
        assert len(got) == len(args), (name, args)
        for a, g in zip(args, got):
            if "*" in a:
                assert g is C.c_void_p or issubclass(g, C._Pointer), (name, a, g)
            else:
                assert g is width[a.split()[0]], (name, a, g)
    assert C.sizeof(_capi.LrcVoxseqInfo) == 96 and "/* 96 bytes */" in header
    assert C.sizeof(_capi.LrcVoxseqOut) == 80 and "/* 80 bytes */" in header
    fields = re.search(r"typedef struct lrc_voxseq_out \{(.*?)\} lrc_voxseq_out;", src, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in _capi.LrcVoxseqOut._fields_]
    fields = re.search(r"typedef struct lrc_voxseq_info \{(.*?)\} lrc_voxseq_info;", src, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[3\])?;", fields) == [f[0] for f in _capi.LrcVoxseqInfo._fields_]
    assert re.search(r"#define LRC_VOXSEQ_STATIC_ONLY 1u", header)
    from lidarcast import voxseq
    assert voxseq.STATIC_ONLY == 1
    assert "voted separately" in header                 # sem / ins and mover can name different surfaces


def test_creation_refusals_need_no_device():
    from lidarcast import _capi, voxseq
    lib = _capi.load()
    E = _capi.LRC_ERR_INVALID_ARG
    h = C.c_void_p()
    g = (C.c_double * 3)(0, 0, 0)
    d = (C.c_int64 * 3)(4, 4, 4)
    fake = C.c_void_p(1)                                 # never dereferenced: the argument checks come first
    assert lib.lrc_voxseq_create(None, g, 0.1, d, 1, C.byref(h)) == E and b"NULL" in lib.lrc_last_error()
    assert lib.lrc_voxseq_create(fake, g, 0.1, d, 0, C.byref(h)) == E and b"num_frames must be >= 1" in lib.lrc_last_error()
    assert lib.lrc_voxseq_create(fake, g, 0.0, d, 1, C.byref(h)) == E and b"voxel_size" in lib.lrc_last_error()
    assert lib.lrc_voxseq_create(fake, g, float("nan"), d, 1, C.byref(h)) == E
    assert lib.lrc_voxseq_create(fake, (C.c_double * 3)(0, float("inf"), 0), 0.1, d, 1, C.byref(h)) == E
    assert lib.lrc_voxseq_create(fake, g, 0.1, (C.c_int64 * 3)(4, 0, 4), 1, C.byref(h)) == E
    assert lib.lrc_voxseq_create(fake, g, 0.1, (C.c_int64 * 3)(1 << 11, 1 << 10, 1 << 10), 1, C.byref(h)) == E
    assert b"2^31 - 1" in lib.lrc_last_error()
    # 64 voxels = 2 words per slot: F * 64 <= 2^31 - 1 holds for F = 2^25 - 1 and fails for 2^25
    assert lib.lrc_voxseq_create(fake, g, 0.1, d, 1 << 25, C.byref(h)) == E and b"num_frames * 32" in lib.lrc_last_error()
    # 65 voxels = 3 words per slot: the padded size counts
    d65 = (C.c_int64 * 3)(5, 13, 1)
    assert lib.lrc_voxseq_create(fake, g, 0.1, d65, (0x7FFFFFFF // 96) + 1, C.byref(h)) == E
    assert h.value is None
    assert lib.lrc_voxseq_create(fake, g, 0.1, d, 1, None) == E
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        voxseq.check_frames(1 << 25, (4, 4, 4))
    assert voxseq.check_frames((1 << 25) - 1, (4, 4, 4)) == (1 << 25) - 1
    assert voxseq.check_frames(0x7FFFFFFF // 96, (5, 13, 1)) == 0x7FFFFFFF // 96
    for bad in (0, -1, 1.5, "x", None):
        with pytest.raises(ValueError):
            voxseq.check_frames(bad, (4, 4, 4))
    # accumulate and finalize refuse a NULL object before anything else
    assert lib.lrc_voxseq_accumulate_dev(None, None, 0, 1, 1, None, 0, None, None, 0, None) == E
    assert lib.lrc_voxseq_finalize_dev(None, 1, None, 0, None) == E
    assert lib.lrc_voxseq_destroy(None) == 0


def sim_with(config):
    import s3dis_simulator
    sim = s3dis_simulator.S3DISSimulator.__new__(s3dis_simulator.S3DISSimulator)      # no engine is built
    sim.config = config
    sim.scene = object()
    return sim


MOVERS = {"period": 0.1, "objects": [{"mesh": "pedestrian", "semantic": 13, "instance": 1001, "path": [[0.0, 1.8, 2.6, 0.0, 20.0]]}]}


class _Group:
    """stands for a multi-rank process group: the simulator asks no more of it before it refuses"""


def test_export_dynamic_occupancy_refusals(monkeypatch):
    from lidar import DualAxisLidarIntrinsics, Indoor8LineLidarIntrinsics
    for key, cfg, named in (("motion", {"speed": 1.0}, "the motion key"),
                            ("motion", {"speed": 1.0, "movers": MOVERS}, "the motion.movers key"),
                            ("noise", {"seed": 1}, "the noise key"), ("beam", {"divergence_mrad": 3.0}, "the beam key"),
                            ("materials", {"classes": {}}, "the materials key")):
        sim = sim_with({key: cfg})
        sim.lidar_config = Indoor8LineLidarIntrinsics.create_standard_8line()
        with pytest.raises(NotImplementedError, match=named):
            sim.export_dynamic_occupancy([], "unused")
    sim = sim_with({"movers": MOVERS})
    sim.lidar_config = DualAxisLidarIntrinsics()
    with pytest.raises(NotImplementedError, match="dual-axis sensor"):
        sim.export_dynamic_occupancy([], "unused")
    sim.lidar_config = Indoor8LineLidarIntrinsics.create_standard_8line()
    import lidarcast.distributed as dist
    monkeypatch.setattr(dist, "active_group", lambda g: (object(), _Group()))
    with pytest.raises(NotImplementedError, match="multi-rank process group"):
        sim.export_dynamic_occupancy([], "unused")
    monkeypatch.undo()
    sim.scene = None
    with pytest.raises(ValueError, match="Scene not loaded"):
        sim.export_dynamic_occupancy([], "unused")
    # the single-grid export keeps refusing the movers key
    with pytest.raises(NotImplementedError, match="movers key"):
        sim_with({"movers": MOVERS}).export_occupancy_grid([], "unused")


def sparse_dict(idx, sem, ins, mover):
    return {int(i): (int(s), int(n), int(m)) for i, s, n, m in zip(idx, sem, ins, mover)}


def test_analytic_mover_scene_on_the_cpu():
    """The expectations of the GPU test's analytic scene, confirmed without a GPU: the oracle's casts, lrc_mover_rays and
    lrc_mover_merge give the records, the restatement the grids."""
    sc = SR.analytic_scene()
    rec = SR.analytic_records_on_cpu(sc)
    assert np.isfinite(rec["t"]).all()                                 # a closed room: every ray returns
    assert rec["mover"][0] == 1 and rec["mover"][1024] == 0           # the axis ray: the cube in frame 0, the wall in frame 1
    assert np.array_equal(rec["point3"][0], np.float32([2.0, 2.2, 1.5])) and np.array_equal(rec["point3"][1024], np.float32([4.0, 2.2, 1.5]))
    args = (rec["t"], rec["point3"], rec["sem"], rec["ins"], rec["mover"])
    r = SR.sequence_from_records(rec["origins"], False, [0, 1], *args, 2, sc["origin"], sc["voxel"], sc["dims"])
    s = SR.sequence_from_records(rec["origins"], False, [0, 0], *args, 1, sc["origin"], sc["voxel"], sc["dims"], static_only=True)
    fr = [r["frames"][f]["sparse"] for f in (0, 1)]
    st = s["frames"][0]["sparse"]
    SR.assert_axis(sc, r["state"], lambda f: sparse_dict(fr[f]["idx"], fr[f]["sem"], fr[f]["ins"], fr[f]["mover"]),
                   s["state"][0], sparse_dict(st["idx"], st["sem"], st["ins"], st["mover"]))
    assert (r["mover_returns"] > 0).sum() > 10 and s["mover_returns"].sum() == 0
    assert r["counts"][:, 4].sum() == 0 and r["skipped"] == 0
