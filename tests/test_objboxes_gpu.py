"""GPU: per-object outlier filter and boxes (lidarcast.object_boxes / object_boxes_dev, csrc/lrc_objboxes.hip) against
lrc_cloud_preprocess run on each object alone (bit for bit), against the float64 restatement of tests/objbox_restate.py,
and end to end through s3dis_bbox_visualizer on a synthetic area.  Parity with Open3D itself is not pinned."""
import io
import json
from contextlib import redirect_stdout
from pathlib import Path

import numpy as np
import pytest

import objbox_restate

pytestmark = pytest.mark.gpu
K = 20


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


def _objects(seed=3):
    """Hundreds of objects: sizes 1, k-1, k, k+1, thousands and one of 10^6 rows, 3-decimal rounding (coincident
    rows), scattered outliers, and two objects interleaved in the same region of space."""
    rng = np.random.default_rng(seed)
    objs = []
    sizes = [0, 1, K - 1, K, K + 1, 2, 37, 5000, 3000] + list(rng.integers(1, 400, 300)) + [1_000_000]
    for j, m in enumerate(sizes):
        m = int(m)
        c = rng.uniform(0, 30, 3)
        kind = j % 3
        if kind == 0:                      # a sheet (surface-like), rounded
            p = c + np.stack([rng.random(m) * 1.5, rng.random(m) * 0.8, np.zeros(m) + rng.random(m) * 0.002], 1)
        elif kind == 1:                    # a box surface
            p = c + rng.random((m, 3)) * 0.6
            ax = rng.integers(0, 3, m)
            p[np.arange(m), ax] = c[ax] + np.round(rng.random(m)) * 0.6
        else:                              # a dense blob with coincident rows
            p = c + rng.normal(0, 0.05, (m, 3))
        out = rng.random(m) < 0.02
        p[out] += rng.normal(0, 0.5, (int(out.sum()), 3))
        objs.append(np.round(p, 3))
    a = np.round(rng.random((4000, 3)), 3)            # interleaved pair: same region, every other row
    objs.append(a[0::2])
    objs.append(a[1::2] + 0.0005)
    return objs


def _concat(objs):
    off = np.concatenate([[0], np.cumsum([len(o) for o in objs])]).astype(np.int64)
    return np.concatenate(objs, axis=0), off


@pytest.fixture(scope="module")
def area_objs():
    return _objects()


@pytest.fixture(scope="module")
def result(ctx, area_objs):
    import lidarcast
    pts, off = _concat(area_objs)
    return lidarcast.object_boxes(ctx, pts, off, k=K, std_ratio=2.0, return_rows=True)


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def test_bit_identical_to_preprocess_per_object(ctx, area_objs, result):
    import lidarcast
    _, off = _concat(area_objs)
    b = result.boxes
    assert b["num_points"].tolist() == [len(o) for o in area_objs]
    for s, p in enumerate(area_objs):
        avg = result.avg[off[s]:off[s + 1]]
        keep = result.keep[off[s]:off[s + 1]].astype(bool)
        if len(p) < K:
            assert b["filtered"][s] == 0 and (avg == -1.0).all() and keep.all(), s
            assert b["mean"][s] == 0.0 and b["threshold"][s] == np.inf
            continue
        r = lidarcast.preprocess_cloud(ctx, p, remove_outliers=True, nb_neighbors=K, std_ratio=2.0,
                                       estimate_normals=False)
        assert b["filtered"][s] == 1
        assert np.array_equal(_bits(avg), _bits(r.avg)), s
        assert np.array_equal(np.flatnonzero(keep), r.kept.astype(np.int64)), s
        assert _bits(b["mean"][s]) == _bits(r.mean) and _bits(b["threshold"][s]) == _bits(r.threshold), s
        assert np.array_equal(result.kept_rows(s).astype(np.int64) - off[s], r.kept.astype(np.int64)), s


def test_against_the_restatement(area_objs, result):
    _, off = _concat(area_objs)
    b = result.boxes
    for s, p in enumerate(area_objs):
        avg, keep, mean, thr, filtered = objbox_restate.restate_object(p, K, 2.0)
        assert np.array_equal(_bits(result.avg[off[s]:off[s + 1]]), _bits(avg)), s
        assert np.array_equal(result.keep[off[s]:off[s + 1]].astype(bool), keep), s
        assert bool(b["filtered"][s]) == filtered and int(b["num_kept"][s]) == int(keep.sum())
        if filtered and len(p) > 1:
            assert _bits(b["mean"][s]) == _bits(mean) and _bits(b["threshold"][s]) == _bits(thr), s
        if keep.any():
            assert np.array_equal(_bits(b["min3"][s]), _bits(p[keep].min(0)))
            assert np.array_equal(_bits(b["max3"][s]), _bits(p[keep].max(0)))
        else:
            assert (b["min3"][s] == np.inf).all() and (b["max3"][s] == -np.inf).all()


def test_invariant_to_cell_size_and_object_order(ctx, area_objs, result):
    import lidarcast
    small = [o for o in area_objs if len(o) < 100_000]
    pts, off = _concat(small)
    ref = lidarcast.object_boxes(ctx, pts, off, k=K, return_rows=True)
    for cs in (0.005, 0.5, 50.0):
        r = lidarcast.object_boxes(ctx, pts, off, k=K, cell_size=cs, return_rows=True)
        assert r.boxes.tobytes() == ref.boxes.tobytes(), cs
        assert r.avg.tobytes() == ref.avg.tobytes() and r.keep.tobytes() == ref.keep.tobytes(), cs
        assert np.array_equal(r.kept, ref.kept)
    perm = np.random.default_rng(0).permutation(len(small))
    pts2, off2 = _concat([small[i] for i in perm])
    r2 = lidarcast.object_boxes(ctx, pts2, off2, k=K, return_rows=True)
    assert r2.boxes.tobytes() == ref.boxes[perm].tobytes()
    for j, i in enumerate(perm):
        assert r2.avg[off2[j]:off2[j + 1]].tobytes() == ref.avg[off[i]:off[i + 1]].tobytes()


def test_device_entry_matches_host_entry(ctx, area_objs):
    import torch
    import lidarcast
    small = [o for o in area_objs if len(o) < 100_000]
    pts, off = _concat(small)
    h = lidarcast.object_boxes(ctx, pts, off, k=K, return_rows=True)
    d = lidarcast.object_boxes_dev(ctx, torch.from_numpy(pts).cuda(), off, k=K, return_rows=True)
    assert d.boxes.tobytes() == h.boxes.tobytes()
    assert d.avg.cpu().numpy().tobytes() == h.avg.tobytes() and d.keep.cpu().numpy().tobytes() == h.keep.tobytes()
    assert np.array_equal(d.kept.cpu().numpy().astype(np.uint32), h.kept)


def test_invalid_arguments(ctx):
    import lidarcast
    p = np.random.default_rng(1).random((100, 3))
    for off in ([0, 60, 50, 100], [1, 50, 100], [0, 50, 99], [0, 50, 101]):
        with pytest.raises(ValueError, match="offsets"):
            lidarcast.object_boxes(ctx, p, off)
    for k in (0, 33):
        with pytest.raises(ValueError, match="k"):
            lidarcast.object_boxes(ctx, p, [0, 100], k=k)
    with pytest.raises(ValueError, match="std_ratio"):
        lidarcast.object_boxes(ctx, p, [0, 100], std_ratio=float("nan"))
    from lidarcast import _capi
    import ctypes as C
    off = np.array([0, 1 << 31], np.uint64)
    rc = _capi.load().lrc_object_boxes(ctx._h, p.ctypes.data, 1 << 31, off.ctypes.data, 1, 20, 2.0, 0.0,
                                       np.zeros(1, lidarcast.OBJBOX_DTYPE).ctypes.data, None, None, None)
    assert rc == _capi.LRC_ERR_INVALID_ARG                  # n >= 2^31: refused on the host, nothing is read
    big = np.zeros(2, np.uint64)
    rc = _capi.load().lrc_object_boxes(ctx._h, p.ctypes.data, 0, big.ctypes.data, 1 << 31, 20, 2.0, 0.0,
                                       np.zeros(1, lidarcast.OBJBOX_DTYPE).ctypes.data, None, None, None)
    assert rc == _capi.LRC_ERR_INVALID_ARG
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[77, 2] = bad
        with pytest.raises(ValueError, match="non-finite"):
            lidarcast.object_boxes(ctx, q, [0, 10, 100])
    del C
    r = lidarcast.object_boxes(ctx, np.zeros((0, 3)), [0, 0, 0])
    assert r.boxes["num_points"].tolist() == [0, 0] and (r.boxes["min3"] == np.inf).all()


def test_process_area_and_main_match_the_host_flow(ctx, tmp_path, monkeypatch):
    from lidarcast import synth
    import s3dis_bbox_visualizer as mod
    synth.make_s3dis_area(tmp_path / "data", "Area_5", num_rooms=7, seed=2, density=1500.0, num_boxes=5, small_objects=6)
    area = tmp_path / "data" / "Area_5"

    def run(where, restated):
        d = tmp_path / where
        d.mkdir()
        monkeypatch.chdir(d)
        if restated:
            monkeypatch.setattr(mod.S3DISBBoxVisualizer, "filter_objects",
                                lambda self, ps, k=20, std_ratio=2.0: objbox_restate.restate_filter_objects(ps, k, std_ratio))
        np.random.seed(4)
        with redirect_stdout(io.StringIO()):
            assert mod.S3DISBBoxVisualizer(ctx=ctx).process_area(area) == []
            mod.main(["--data_root", str(tmp_path / "data"), "--area_name", "Area_5", "--room_name", "office_1"])
        rng = np.random.random(3).tolist()
        files = {str(f.relative_to(d)): f.read_bytes() for f in sorted(d.rglob("*.json"))}
        monkeypatch.undo()
        return files, rng

    dev, rng_dev = run("dev", False)
    host, rng_host = run("host", True)
    assert rng_dev == rng_host
    assert len(dev) == 7 and dev == host
    assert sum(len(json.loads(v)["annotations"]) for v in dev.values()) > 7
    assert Path(tmp_path / "dev").exists()


def test_remove_outliers_returns_the_kept_rows(ctx, area_objs):
    from s3dis_bbox_visualizer import S3DISBBoxVisualizer
    v = S3DISBBoxVisualizer(ctx=ctx)
    for p in (area_objs[3], area_objs[7], area_objs[2]):         # k rows, thousands, k - 1 (returned untouched)
        c = np.full((len(p), 3), 0.5)
        got_p, got_c = v.remove_outliers(p, c)
        want_p, want_c = objbox_restate.restate_remove_outliers(p, c)
        assert np.array_equal(got_p, want_p) and np.array_equal(got_c, want_c)
        assert v.remove_outliers(p)[1] is None
