"""-m gpu: lrcecho::reduce_lanes -- the tail of trace_kernel<kGenEchoes> -- on crafted rows, through the device test hook
lrc_internal_echo_lanes_dev (lidarcast.echo.reduce_lanes_dev), against tests/echo_restate.py.

A scan puts in front of the reduction only what a traversal returns; the hook puts the rows of tests/echo_rows.py there: every
row over a six-letter alphabet built around one separation for K = 1..5, seeded rows over a longer alphabet for K = 6..16, and
the rows of tests/test_echo_host.py.  Every K in 1..16 runs with every E in 1..4 and min_count in {1, min(2, K), K}, and every
row set stands at every group position of a wave: 64 / G copies in one launch, copy s behind as many filler beams (all-miss and
all-tie in turn) as put its first beam at position s of a wave, the launch ending in a partial wave.  All four columns are
compared by integer equality or by bits: rep and weight as returned, range the representative's t, label beam * K + rep, an
empty slot -1 / +inf / weight 0.  The restatement is computed once per (K, min_count) with four slots -- slot e does not depend
on the slots behind it, so E slots are its first E columns (tests/test_echo_rows_host.py holds lrc_echo_reduce to the same) --
and tiled."""
import ctypes as C
import functools

import numpy as np
import pytest

import echo_restate as er
import echo_rows as rows
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    c = lidarcast.Context(0)
    yield c
    c.close()


def _beam(K, E, min_count, separation):
    from lidarcast._capi import LrcBeam
    b = LrcBeam()
    b.subrays, b.max_echoes, b.min_count, b.separation = K, E, min_count, separation
    return b


def group_of(K, E):
    g = 1
    while g < max(K, E):
        g *= 2
    return g


@functools.lru_cache(maxsize=None)
def restated(K, min_count):
    """The row set of K behind its two filler rows (all-miss, all-tie), its restatement with four slots, and its profile."""
    t = np.concatenate([rows.fillers(2, K), rows.row_set(K)])
    rep, weight = er.reduce_rows(t, 4, min_count, rows.SEP)
    for a in (t, rep, weight):
        a.setflags(write=False)
    return t, rep, weight


@functools.lru_cache(maxsize=None)
def profile(K):
    return rows.profile(rows.row_set(K), rows.SEP)


def tiled(n, W):
    """Row numbers (into filler rows 0, 1 and set rows 2 .. n + 1) of one launch: W copies of the set, copy s behind the fewest
    fillers that put its first beam at position s (mod W) of a wave, and one more filler where the total would be even.
    Returns (row numbers, first beam of every copy)."""
    src, starts = [], []
    cur = 0
    for s in range(W):
        pad = (s - cur) % W
        src.append(np.arange(pad) % 2)
        cur += pad
        starts.append(cur)
        src.append(2 + np.arange(n))
        cur += n
    if cur % 2 == 0:
        src.append(np.array([1]))
        cur += 1
    return np.concatenate(src), np.array(starts)


def run_rows(ctx, t, rep4, weight4, src, K, E, min_count, separation, what):
    """One launch over rows t[src]; the restatement (rep4, weight4: rows of t, four slots) tiled the same way."""
    from lidarcast import echo
    t_all = np.ascontiguousarray(t[src])
    got = echo.reduce_lanes_dev(ctx, t_all, _beam(K, E, min_count, separation))
    rep, weight = rep4[src][:, :E], weight4[src][:, :E]
    assert got["rep"].dtype == np.int32 and np.array_equal(got["rep"], rep), \
        f"{what}: rep, first differing beam {np.argwhere((got['rep'] != rep).any(axis=1))[:1].tolist()}"
    assert got["weight"].dtype == np.uint8 and np.array_equal(got["weight"], weight), \
        f"{what}: weight, first differing beam {np.argwhere((got['weight'] != weight).any(axis=1))[:1].tolist()}"
    has = rep >= 0
    beam = np.arange(len(src))[:, None]
    want_range = np.where(has, t_all[beam, np.where(has, rep, 0)], np.float32(np.inf)).astype(np.float32)
    assert_bit_equal(got["range"], want_range, f"{what}: range")
    want_label = (beam * K + rep).astype(np.uint32)
    assert np.array_equal(got["label"][has], want_label[has]), f"{what}: label"
    assert (weight[~has] == 0).all() and (weight[has] >= min_count).all()            # what an empty slot is, in the restatement
    return got


@pytest.mark.parametrize("K", range(1, 17))
def test_row_set_at_every_group_position(ctx, K):
    n = len(rows.row_set(K))
    prof = profile(K)
    odd_totals = {}
    for min_count in sorted({1, min(2, K), K}):
        t, rep4, weight4 = restated(K, min_count)
        for E in (1, 2, 3, 4):
            G = group_of(K, E)
            W = 64 // G
            src, starts = tiled(n, W)
            assert (starts % W == np.arange(W)).all() and (src[starts] == 2).all()
            assert len(src) % 2 == 1 and (len(src) * G) % 64 != 0                 # the last wave is partial
            assert len(src) <= (rows.RANDOM_ROWS + 4 + 64) * 64
            odd_totals[G] = len(src)
            # the set holds what the case is for
            count = rows.kinds(prof, E, min_count)
            for kind, possible in rows.possible_kinds(K, E, min_count).items():
                assert (count[kind] > 0) == possible, (K, E, min_count, kind, count)
            assert count["all_miss"] >= 1
            run_rows(ctx, t, rep4, weight4, src, K, E, min_count, rows.SEP, f"K={K} E={E} min_count={min_count} G={G}")
    assert set(odd_totals) == {group_of(K, E) for E in (1, 2, 3, 4)}


def test_every_group_size_runs():
    assert {group_of(K, E) for K in range(1, 17) for E in (1, 2, 3, 4)} == {1, 2, 4, 8, 16}
    assert group_of(1, 1) == 1 and group_of(2, 1) == group_of(1, 2) == 2 and group_of(3, 4) == 4 and group_of(16, 1) == 16


def test_crafted_host_rows_at_every_group_position(ctx):
    """The rows tests/test_echo_host.py gives lrc_echo_reduce, with the results recorded for them."""
    for c in rows.CRAFTED:
        K = c.t.shape[1]
        t = np.concatenate([rows.fillers(2, K), c.t])
        rep4, weight4 = er.reduce_rows(t, 4, c.min_count, c.separation)
        assert rep4[2, :c.E].tolist() == c.rep[0] and weight4[2, :c.E].tolist() == c.weight[0], c
        W = 64 // group_of(K, c.E)
        src, starts = tiled(1, W)
        got = run_rows(ctx, t, rep4, weight4, src, K, c.E, c.min_count, c.separation, repr(c))
        assert got["rep"][starts].tolist() == c.rep * W and got["weight"][starts].tolist() == c.weight * W, c


def test_hostile_values_behind_a_miss(ctx):
    """NaN takes no part (it is not < +inf), -0.0 ties with 0.0, and the largest finite float is a hit far from everything."""
    big = np.finfo(np.float32).max
    t = np.array([[np.nan, 1.0, np.nan, 1.25], [-0.0, 0.0, big, np.inf], [big, big, 0.0, np.nan]], np.float32)
    t = np.concatenate([rows.fillers(2, 4), t])
    for min_count in (1, 2):
        rep4, weight4 = er.reduce_rows(t, 4, min_count, rows.SEP)
        for E in (1, 2, 4):
            src, _ = tiled(3, 64 // 4)
            run_rows(ctx, t, rep4, weight4, src, 4, E, min_count, rows.SEP, f"hostile E={E} min_count={min_count}")
    rep, w = er.reduce_rows(t[2:], 2, 1, rows.SEP)
    assert rep.tolist() == [[1, -1], [0, 2], [2, 0]] and w.tolist() == [[2, 0], [2, 1], [1, 2]]


def test_refusals_and_the_empty_call(ctx):
    import torch
    from lidarcast import _capi, echo
    lib = _capi.load()
    fn = lib.lrc_internal_echo_lanes_dev
    t = torch.zeros((1, 16), dtype=torch.float32, device="cuda")
    rep, lab = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    rng = torch.zeros(4, dtype=torch.float32, device="cuda")
    w = torch.zeros(4, dtype=torch.uint8, device="cuda")
    args = (t.data_ptr(), 1)
    outs = (rep.data_ptr(), rng.data_ptr(), lab.data_ptr(), w.data_ptr(), None)
    bad = [dict(K=0), dict(K=17), dict(E=0), dict(E=5), dict(min_count=0), dict(K=3, min_count=4),
           dict(separation=0.0), dict(separation=-1.0), dict(separation=float("inf")), dict(separation=float("nan"))]
    for kw in bad:                                                  # the beams lrc_echo_reduce refuses
        b = _beam(**{"K": 3, "E": 2, "min_count": 1, "separation": 0.05, **kw})
        assert fn(ctx._h, *args, C.byref(b), *outs) == _capi.LRC_ERR_INVALID_ARG, kw
        assert b"lrc_internal_echo_lanes_dev" in lib.lrc_last_error(), kw
        with pytest.raises(ValueError, match="lrc_internal_echo_lanes_dev"):
            echo.reduce_lanes_dev(ctx, np.zeros((1, max(1, min(b.subrays, 16))), np.float32), b)
    b = _beam(3, 2, 1, 0.05)
    assert fn(ctx._h, *args, None, *outs) == _capi.LRC_ERR_INVALID_ARG
    assert fn(None, *args, C.byref(b), *outs) == _capi.LRC_ERR_INVALID_ARG
    assert fn(ctx._h, None, 1, C.byref(b), *outs) == _capi.LRC_ERR_INVALID_ARG
    for missing in range(3):                                         # rep, range, label; the weight column is optional
        o = list(outs)
        o[missing] = None
        assert fn(ctx._h, *args, C.byref(b), *o) == _capi.LRC_ERR_INVALID_ARG, missing
    assert fn(ctx._h, t.data_ptr(), 2 ** 32 // 3 + 1, C.byref(b), *outs) == _capi.LRC_ERR_INVALID_ARG
    assert b"2^32" in lib.lrc_last_error()
    assert fn(ctx._h, None, 0, C.byref(b), None, None, None, None, None) == 0
    got = echo.reduce_lanes_dev(ctx, np.zeros((0, 3), np.float32), b)
    assert got["rep"].shape == (0, 2) and got["weight"].shape == (0, 2)
    # without a weight column the other three are written all the same
    rep.fill_(-2)
    lab.fill_(-2)
    assert fn(ctx._h, *args, C.byref(b), rep.data_ptr(), rng.data_ptr(), lab.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert rep.tolist() == [0, -1, -2, -2] and rng[:2].tolist() == [0.0, float("inf")] and int(lab[0]) == 0 and int(lab[2]) == -2
