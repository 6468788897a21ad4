"""GPU: detection boxes (lidarcast.instance_boxes / instance_boxes_dev, csrc/lrc_boxes.hip) on the inputs of
tests/box_edges.py, bit for bit against its restatement -- mean and threshold included, in box_stats_kernel's own order
(lanes strided by 256, then the tree): signed coordinates, zero extremes of both signs (numpy's rule: the last kept zero
row gives the sign), the class list at its limits, instance sizes around min_points, k and the 256-lane stride, every list
length, more than 65535 segments, degenerate instances.  Every case runs through the host entry at cell_size 0 and two
more sizes and through the device entry: all four give the same bytes."""
import numpy as np
import pytest

import box_edges as BE

pytestmark = pytest.mark.gpu
CASES = BE.instance_cases()
_BRUTE = {}


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


def _host(ctx, p, sem, ins, classes, min_points, k, cell_size=0.0):
    import lidarcast
    return lidarcast.instance_boxes(ctx, p, sem, ins, classes, min_points=min_points, k=k, std_ratio=BE.STD_RATIO,
                                    cell_size=cell_size, return_rows=True)


def _dev(ctx, p, sem, ins, classes, min_points, k):
    import torch
    import lidarcast
    rows = np.empty((len(p), 4), np.float32)
    rows[:, :3] = p
    rows[:, 3] = (sem.astype(np.uint32) | (ins.astype(np.uint32) << 16)).view(np.float32)
    b, avg, keep = lidarcast.instance_boxes_dev(ctx, torch.from_numpy(rows).cuda(), classes, min_points=min_points, k=k,
                                                std_ratio=BE.STD_RATIO, return_rows=True,
                                                stream=torch.cuda.current_stream().cuda_stream)
    return b, avg.cpu().numpy(), keep.cpu().numpy()


def _blob(out):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)


def _check(got, want):
    import lidarcast
    assert lidarcast.BOX_DTYPE == BE.BOX
    assert np.array_equal(BE.bits(got[1]), BE.bits(want[1])), "avg differs from the restatement"
    assert np.array_equal(got[2], want[2]), "keep differs from the restatement"
    assert BE.same(got[0], want[0]) is None, BE.same(got[0], want[0])


@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_the_restatement_at_every_cell_size_and_entry(ctx, name):
    p, sem, ins, classes, min_points, k, cells = CASES[name]
    want = BE.expected_instances(p, sem, ins, classes, min_points, k, cache=_BRUTE)
    got = _host(ctx, p, sem, ins, classes, min_points, k)
    _check(got, want)
    ref = _blob(got)
    for cs in cells:
        assert _blob(_host(ctx, p, sem, ins, classes, min_points, k, cs)) == ref, f"cell_size {cs} changes the bytes"
    assert _blob(_dev(ctx, p, sem, ins, classes, min_points, k)) == ref, "the device entry differs from the host entry"
    b = got[0]
    if name == "every_row_ignored":
        assert len(b) == 0 and (got[1] == -1.0).all() and not got[2].any()
    if name == "signed":
        assert {0, 0xFFFF} <= set(b["sem"].tolist()) and {1, 65535} <= set(b["ins"].tolist()) and 9 not in b["sem"]
    if name == "sizes_mp1_k1":                     # n = 1, k = 1: filtered, 0 / 0 under the root
        one = np.flatnonzero(b["num_points"] == 1)[0]
        assert b["filtered"][one] == 1 and b["num_kept"][one] == 0 and b["mean"][one] == 0.0
        assert np.isnan(b["threshold"][one]) and (b["min3"][one] == np.inf).all() and (b["max3"][one] == -np.inf).all()
        assert (b["num_kept"] == 0).all()
    if name == "k02":
        j = np.flatnonzero(b["num_points"] == 256)[0]
        assert b["num_kept"][j] == 0 and b["mean"][j] == b["threshold"][j] == 0.125
    if name == "deg_identical":
        assert b["num_kept"][0] == 0 and b["mean"][0] == 0.0 and b["threshold"][0] == 0.0
        assert (b["min3"][0] == np.inf).all() and (b["max3"][0] == -np.inf).all()


def test_more_segments_than_65535_workgroups(ctx):
    p, sem, ins, classes, big = BE.many_segments()
    want = BE.expected_instances(p, sem, ins, classes, 1, 20)
    got = _host(ctx, p, sem, ins, classes, 1, 20)
    _check(got, want)
    b = got[0]
    assert len(b) == 64 * 1100 > 65535
    where = [0, int(np.flatnonzero((b["sem"] == big[1][0]) & (b["ins"] == big[1][1]))[0]), len(b) - 1]
    assert [(int(b["sem"][j]), int(b["ins"][j])) for j in where] == big
    assert (b["num_points"][where] == 40).all() and (b["filtered"][where] == 1).all() and b["filtered"].sum() == 3
    assert _blob(_dev(ctx, p, sem, ins, classes, 1, 20)) == _blob(got), "the device entry differs from the host entry"


def test_sixty_five_classes_are_refused(ctx):
    import lidarcast
    p, sem, ins = CASES["64_classes"][:3]
    with pytest.raises(ValueError, match="64 classes"):
        lidarcast.instance_boxes(ctx, p, sem, ins, list(range(65)))
