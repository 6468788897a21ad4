"""GPU: annotation boxes (lidarcast.object_boxes / object_boxes_dev, csrc/lrc_objboxes.hip) on the inputs of
tests/box_edges.py, bit for bit against its restatement: signed coordinates and denormal extremes (the negative branch of
the order keys), zero extremes of both signs (the zrow path), every list length of ob_knn_kernel, offset tables with empty
objects and more than 65535 objects (the stride loops of the (object, chunk) launches), the reduction chunk boundaries,
degenerate objects (each branch of the cell rule) and wavefronts that mix filtered and unfiltered objects.  Every case runs
through the host entry at cell_size 0 and two more sizes and through the device entry: all four give the same bytes.
tests/test_box_edges_host.py shows that these inputs hold the edges and that wrong restatements change the bytes."""
import numpy as np
import pytest

import box_edges as BE

pytestmark = pytest.mark.gpu
CASES = BE.object_cases()
_BRUTE = {}


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


def _host(ctx, pts, off, k, cell_size=0.0):
    import lidarcast
    r = lidarcast.object_boxes(ctx, pts, off, k=k, std_ratio=BE.STD_RATIO, cell_size=cell_size, return_rows=True)
    return r.boxes, r.avg, r.keep, r.kept


def _dev(ctx, pts, off, k):
    import torch
    import lidarcast
    r = lidarcast.object_boxes_dev(ctx, torch.from_numpy(pts).cuda(), off, k=k, std_ratio=BE.STD_RATIO, return_rows=True)
    return r.boxes, r.avg.cpu().numpy(), r.keep.cpu().numpy(), r.kept.cpu().numpy().view(np.uint32)


def _blob(out):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)


def _check(got, want):
    import lidarcast
    assert lidarcast.OBJBOX_DTYPE == BE.OBJBOX
    assert np.array_equal(BE.bits(got[1]), BE.bits(want[1])), "avg differs from the restatement"
    assert np.array_equal(got[2], want[2]), "keep differs from the restatement"
    assert np.array_equal(got[3], want[3]), "kept rows differ from the restatement"
    assert BE.same(got[0], want[0]) is None, BE.same(got[0], want[0])


@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_the_restatement_at_every_cell_size_and_entry(ctx, name):
    objs, k, cells = CASES[name]
    pts, off = BE.concat(objs)
    want = BE.expected_objects(pts, off, k, cache=_BRUTE)
    got = _host(ctx, pts, off, k)
    _check(got, want)
    ref = _blob(got)
    for cs in cells:
        assert _blob(_host(ctx, pts, off, k, cs)) == ref, f"cell_size {cs} changes the bytes"
    assert _blob(_dev(ctx, pts, off, k)) == ref, "the device entry differs from the host entry"
    b = got[0]
    if name == "k01":                              # the only neighbour is the row itself: avg 0, every filtered row removed
        f = b["filtered"] == 1
        assert f.sum() == 5 and (b["num_kept"][f] == 0).all() and (got[1][got[1] != -1.0] == 0.0).all()
        one = np.flatnonzero(b["num_points"] == 1)[0]          # m = 1, k = 1: 0 / 0 under the root
        assert b["mean"][one] == 0.0 and np.isnan(b["threshold"][one])
        assert (b["min3"][one] == np.inf).all() and (b["max3"][one] == -np.inf).all()
    if name == "k02":                              # equal_avg_object: avg == threshold removes, <= would keep
        assert b["num_points"][-1] == 256 and b["num_kept"][-1] == 0 and b["mean"][-1] == b["threshold"][-1] == 0.125
    if name == "deg_identical":
        assert b["num_kept"][0] == 0 and b["mean"][0] == 0.0 and b["threshold"][0] == 0.0
        assert (b["min3"][0] == np.inf).all() and (b["max3"][0] == -np.inf).all()


@pytest.mark.parametrize("S", [65535, 65536, 65540])
def test_more_objects_than_one_grid_row(ctx, S):
    pts, off, edges = BE.many_objects(S)
    assert len(off) == S + 1 and edges["rows"] < 70_000
    want = BE.expected_objects(pts, off, 20)
    got = _host(ctx, pts, off, 20)
    _check(got, want)
    assert (got[0]["filtered"][edges["filtered"]] == 1).all() and (got[0]["num_points"][edges["empty"]] == 0).all()
    assert _blob(_dev(ctx, pts, off, 20)) == _blob(got), "the device entry differs from the host entry"
