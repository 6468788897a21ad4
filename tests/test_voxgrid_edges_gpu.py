"""-m gpu: the static semantic occupancy grid (csrc/lrc_voxgrid.hip) against the numpy restatement on the hostile ray set
of tests/voxgrid_restate.py, bit for bit: rejected rays of every kind, exact ties on two and three axes, walks that never
start, the 2^24 boundary pair, hostile labels, waves of misses only and of rejected rays only, grids of one voxel and
with V = 2^k - 1 and 2^k, launches of 1 to 257 rays, the key buffer's growth paths, finalize between accumulates, reset.
tests/test_voxgrid_coverage_edges_host.py shows on the CPU that the set holds these kinds and that wrong tie rules, limits
and votes change the expected output."""
import ctypes as C

import numpy as np
import pytest

import voxgrid_restate as R
from test_voxgrid_gpu import _assert_equal, _rows_of
from voxseq_restate import pack_bits

pytestmark = pytest.mark.gpu

G, S = R.HOSTILE_ORIGIN, R.HOSTILE_S
MAIN = R.HOSTILE_DIMS[0]


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


def _upload(b):
    import torch
    P = len(b["poses"])
    return (torch.from_numpy(np.ascontiguousarray(b["poses"], np.float64).reshape(P, 16)).cuda(),
            torch.from_numpy(np.ascontiguousarray(b["dirs"], np.float64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(b["t_label"]).view(np.int32)).cuda())


def _host_finalize(vg, min_returns):
    """lrc_voxgrid_finalize, the host form: (idx, sem, ins, returns, state, the six counts)."""
    from lidarcast._capi import LrcVoxgridCounts, check
    n = max(1, int(vg.info().sparse_bound))
    idx, ret = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    sem, ins = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    state = np.zeros(vg.num_voxels, np.uint8)
    c = LrcVoxgridCounts()
    check(vg._lib.lrc_voxgrid_finalize(vg._h, int(min_returns), idx.ctypes.data, sem.ctypes.data, ins.ctypes.data,
                                       ret.ctypes.data, n, state.ctypes.data, C.byref(c)), "lrc_voxgrid_finalize")
    k = int(c.num_sparse)
    return idx[:k], sem[:k], ins[:k], ret[:k], state, (k, int(c.num_free), int(c.num_occupied), int(c.num_unknown),
                                                      int(c.rejected_rays), int(c.returns))


def _check(vg, blocks, dims, min_returns=(1,), long=True):
    """Everything finalize and free_bits report against the restatement of the returned rays of ``blocks``."""
    o, e, lab = R.returned_segments(blocks)
    V = int(np.prod(dims))
    free, _, _, _ = (R.walk_long if long else R.walk)(o, e, G, S, dims)
    assert np.array_equal(vg.free_bits(), pack_bits(free, V))
    top = 0
    for mr in min_returns:
        mr = top + 1 if mr == "above" else mr
        sp, st, c = (R.grid_from_rays_long if long else R.grid_from_rays)(o, e, lab, G, S, dims, min_returns=mr)
        top = max(top, int(sp["returns"].max()) if len(sp["returns"]) else 0)
        res = vg.finalize(min_returns=mr)
        _assert_equal(res, sp, st, c)
        six = (c["num_sparse"], c["free"], c["occupied"], c["unknown"], c["rejected_rays"], c["returns"])
        idx, sem, ins, ret, state, got = _host_finalize(vg, mr)
        assert got == six, (mr, got, six)
        assert np.array_equal(idx, sp["idx"]) and np.array_equal(sem, sp["sem"]) and np.array_equal(ins, sp["ins"])
        assert np.array_equal(ret, sp["returns"]) and np.array_equal(state, st)
        if mr == top + 1:
            assert c["occupied"] == 0 and res.num_occupied == 0
    return res


@pytest.mark.parametrize("dims", R.HOSTILE_DIMS)
def test_hostile_rays_bit_equal_to_restatement(ctx, dims):
    from lidarcast import OccupancyGrid
    blocks = R.hostile_rays(G, S, dims)
    vg = OccupancyGrid(ctx, G, S, dims)
    up = []
    for b in blocks:
        # the device forms o and e from (poses, dirs, t) as numpy restates them: asserted once, on the scene cloud's rows
        with np.errstate(over="ignore"):
            o, e, lab, dev = _rows_of(ctx, b["poses"], b["dirs"], b["t_label"])
        keep = np.isfinite(b["t"])
        assert np.array_equal(e.view(np.uint32), b["e"][keep].view(np.uint32))
        assert np.array_equal(o.view(np.uint32), b["o"][keep].view(np.uint32))
        assert np.array_equal(lab, b["t_label"][keep, 1])
        up.append(dev)
    for b, dev in zip(blocks, up):                      # block by block: a union of all rays would hide more
        vg.reset()
        vg.accumulate_dev(*dev)
        _check(vg, [b], dims)
    vg.reset()
    for dev in up:
        vg.accumulate_dev(*dev)
    res = _check(vg, blocks, dims, min_returns=(1, 2, 3, "above"))
    V = int(np.prod(dims))
    assert res.rejected_rays >= 8 and {0, V - 1} <= set(res.idx.tolist())
    vg.close()


@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("one_pose", [True, False])
def test_launch_edges(ctx, total, one_pose):
    """One pose row with N = total, and the same rays as ``total`` poses with N = 1."""
    from lidarcast import OccupancyGrid
    pose, dirs, tl = R.launch_edge_rays(G, S, MAIN)
    b = {"poses": pose, "dirs": dirs[:total], "t_label": tl[:total], "t": tl[:total, 0].view(np.float32)}
    b["o"], b["e"] = R.segments_of(pose, b["dirs"], b["t"])
    vg = OccupancyGrid(ctx, G, S, MAIN)
    if one_pose:
        vg.accumulate_dev(*_upload(b))
    else:                                              # N = 1: every ray a pose of its own, all along table row 0
        rng = np.random.default_rng(8)
        poses = np.repeat(pose, total, axis=0)
        poses[:, :3, 3] = np.asarray(G) + rng.uniform(-0.1, 1.1, (total, 3)) * np.asarray(MAIN) * S
        b = {"poses": poses, "dirs": dirs[:1], "t_label": tl[:total], "t": tl[:total, 0].view(np.float32)}
        b["o"], b["e"] = R.segments_of(poses, b["dirs"], b["t"])
        vg.accumulate_dev(*_upload(b))
    assert int(vg.info().reserved_keys) == total
    _check(vg, [b], MAIN, min_returns=(1, 2), long=False)
    vg.close()


def test_growth_order_and_reset(ctx):
    """Chunks of 3, 2, 40 and 45 poses into one grid: the first call allocates the key buffer, the second fits into twice
    the capacity (it doubles), the third needs more than double, the fourth doubles again; finalize after the second
    and the fourth chunk (the second call regrows the finalize scratch); reset, then the first chunk alone."""
    from lidarcast import OccupancyGrid
    blk = R.growth_rays(G, S, MAIN)
    V = int(np.prod(MAIN))
    vg = OccupancyGrid(ctx, G, S, MAIN)
    assert int(vg.info().reserved_keys) == 0 and int(vg.info().sparse_bound) == 0
    assert int(vg.info().num_voxels) == V and int(vg.info().words) == (V + 31) // 32
    edges = [0, 3, 5, 45, 90]
    for j in range(4):
        vg.accumulate_dev(*_upload(R.chunk(blk, edges[j], edges[j + 1])))
        rays = R.RAYS_PER_POSE * edges[j + 1]
        info = vg.info()                               # every ray reserves a key slot; sparse_bound = min(V, reserved)
        assert int(info.reserved_keys) == rays and int(info.sparse_bound) == min(V, rays)
        if j in (1, 3):
            a = _check(vg, [R.chunk(blk, 0, edges[j + 1])], MAIN, min_returns=(1, 2, 3), long=False)
            b = vg.finalize(min_returns=3)             # twice in a row: identical
            assert np.array_equal(a.idx, b.idx) and np.array_equal(a.sem, b.sem) and np.array_equal(a.ins, b.ins)
            assert np.array_equal(a.returns, b.returns) and np.array_equal(a.state, b.state)
            assert (a.num_free, a.num_occupied, a.num_unknown, a.rejected_rays) == \
                (b.num_free, b.num_occupied, b.num_unknown, b.rejected_rays)
            assert a.rejected_rays > 0 and len(a.idx) > 0
    vg.reset()
    assert int(vg.info().reserved_keys) == 0
    vg.accumulate_dev(*_upload(R.chunk(blk, 0, 3)))
    assert int(vg.info().reserved_keys) == 21
    _check(vg, [R.chunk(blk, 0, 3)], MAIN, min_returns=(1, 2), long=False)      # no key of the 90 poses survives
    vg.close()
