"""A pass of tests/test_voxgrid_edges_gpu.py and tests/test_coverage_edges_gpu.py only means something if their inputs hold
the edges they promise and if a wrong kernel would change the expected output on those very inputs.  On the CPU:
  - every kind of ray, record and set pattern the builders of tests/voxgrid_restate.py and tests/coverage_restate.py
    promise is counted: tie equalities, the four kinds of rejected ray, waves of misses only and of rejected rays only,
    run positions, tie indices;
  - mutated restatements (small variants written here, not switches of the shipped ones) change the expected output:
    tie order y before x, < for <= in the axis choice, the length limit at > instead of >=, a return recorded for a
    rejected ray, sem ties to the largest, ins voted over all sems, no tail mask on the last word, greedy ties to the
    largest index, a run not cut at a non-returned ray, the target tested with > instead of >=;
  - the library's host walk (lrc_voxseq_walk) walks the segment form of the hostile set like the restatement;
  - greedy's target rule is the header's: two float64 conversions, then one divide."""
import os
import re
from collections import Counter

import numpy as np
import pytest

import coverage_restate as CR
import voxgrid_restate as VR
from conftest import REPO

G, VS = VR.HOSTILE_ORIGIN, VR.HOSTILE_S
MAIN = (5, 7, 33)
BLOCK_NAMES = ("random0", "random1", "far", "axis", "tie_a", "tie_b", "label")


@pytest.fixture(scope="module")
def sets():
    return {dims: VR.hostile_rays(G, VS, dims) for dims in VR.HOSTILE_DIMS}


# ---- a scalar walk with mutations ---------------------------------------------------------------------------------------
def _steps(o, e, dims):
    """(finite, in range, a, b, n) with nothing zeroed."""
    ov, ev = o.astype(np.float64), e.astype(np.float64)
    fin = np.isfinite(ov).all(1) & np.isfinite(ev).all(1)
    with np.errstate(all="ignore"):
        fa, fb = VR.voxel_of(ov, G, VS), VR.voxel_of(ev, G, VS)
    inr = fin & np.all((fa >= -2.0 ** 31) & (fa < 2.0 ** 31) & (fb >= -2.0 ** 31) & (fb < 2.0 ** 31), axis=1)
    a = np.where(inr[:, None], fa, 0).astype(np.int64)
    b = np.where(inr[:, None], fb, 0).astype(np.int64)
    return fin, inr, a, b, np.abs(b - a)


def _tmax(o, e, a, b):
    ov, ev = o.astype(np.float64), e.astype(np.float64)
    with np.errstate(all="ignore"):
        D = ev - ov
        plane = np.asarray(G) + (a.astype(np.float64) + (b > a)) * VS
        return np.where(b != a, (plane - ov) / D, np.inf), np.where(b != a, VS / np.abs(D), np.inf), D


def _trace(o, e, dims, order=(0, 1, 2), strict=False, limit_gt=False):
    """Per ray: (ok, in-grid voxels that get a free bit, end voxel's linear index or -1).  The axis choice is written in
    the kernel's form: the first axis of ``order`` if its tMax is <= (``strict``: <) both others', else the second
    if <= the third's, else the third."""
    fin, inr, a, b, n = _steps(o, e, dims)
    total = n.sum(1)
    ok = inr & ((total <= VR.MAX_STEPS) if limit_gt else (total < VR.MAX_STEPS))
    tmax, tdel, _ = _tmax(o, e, a, b)
    le = (lambda x, y: x < y) if strict else (lambda x, y: x <= y)
    p, q, r = order
    out = []
    for i in range(len(o)):
        if not ok[i]:
            out.append((False, [], -1))
            continue
        end = int(VR.linear(b[i], dims)) if VR.inside(b[i], dims) else -1
        cur, nn, tm, st = a[i].copy(), n[i].copy(), tmax[i].copy(), np.sign(b[i] - a[i])
        free = []
        if total[i] >= 1 << 16:                              # axis-parallel: the row from a to b, whatever the rule
            ax = int(np.flatnonzero(nn)[0])
            assert (nn > 0).sum() == 1
            while 0 <= cur[ax] < dims[ax] and cur[ax] != b[i, ax]:
                if VR.inside(cur, dims):
                    free.append(int(VR.linear(cur, dims)))
                cur[ax] += st[ax]
            out.append((True, free, end))
            continue
        while nn.sum() > 0:
            if VR.inside(cur, dims):
                free.append(int(VR.linear(cur, dims)))
            if nn[p] > 0 and (nn[q] == 0 or le(tm[p], tm[q])) and (nn[r] == 0 or le(tm[p], tm[r])):
                ax = p
            elif nn[q] > 0 and (nn[r] == 0 or le(tm[q], tm[r])):
                ax = q
            else:
                ax = r
            assert nn[ax] > 0
            cur[ax] += st[ax]
            tm[ax] = tm[ax] + tdel[i, ax]
            nn[ax] -= 1
        assert np.array_equal(cur, b[i])
        out.append((True, free, end))
    return out


def _vote(keys, sem_largest=False, ins_all=False):
    """{idx: (sem, ins, returns)} from (idx, sem, ins) triples."""
    out = {}
    for v in sorted({k[0] for k in keys}):
        mine = [k for k in keys if k[0] == v]
        sems = Counter(k[1] for k in mine)
        top = max(sems.values())
        tied = [x for x in sems if sems[x] == top]
        sem = max(tied) if sem_largest else min(tied)
        inss = Counter(k[2] for k in mine if ins_all or k[1] == sem)
        top = max(inss.values())
        out[v] = (sem, min(x for x in inss if inss[x] == top), len(mine))
    return out


def _variant(blocks, dims, reject_returns=False, sem_largest=False, ins_all=False, **walk):
    """The expected output of accumulating ``blocks``: (free bits, {idx: (sem, ins, returns)}, rejected rays)."""
    o, e, lab = VR.returned_segments(blocks)
    V = int(np.prod(dims))
    free = np.zeros(V, bool)
    keys, rejected = [], 0
    _, inr, a, _, _ = _steps(o, e, dims)
    for i, (ok, cells, end) in enumerate(_trace(o, e, dims, **walk)):
        rejected += not ok
        free[cells] = True
        if not ok and reject_returns and inr[i] and VR.inside(a[i], dims):
            end = int(VR.linear(a[i], dims))                 # the mutation: the rejected ray's start voxel gets a return
        if end >= 0:
            keys.append((end, int(lab[i] & 0xFFFF), int(lab[i] >> 16)))
    return free, _vote(keys, sem_largest, ins_all), rejected


def _shipped(blocks, dims):
    o, e, lab = VR.returned_segments(blocks)
    sp, st, c = VR.grid_from_rays_long(o, e, lab, G, VS, dims)
    free, _, _, _ = VR.walk_long(o, e, G, VS, dims)
    votes = {int(i): (int(s), int(n), int(r)) for i, s, n, r in zip(sp["idx"], sp["sem"], sp["ins"], sp["returns"])}
    return free, votes, c["rejected_rays"]


def _same(x, y):
    return np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2]


# ---- the hostile ray set holds what it promises -------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", VR.HOSTILE_DIMS)
def test_hostile_set_holds_every_kind(sets, dims):
    blocks = sets[dims]
    named = dict(zip(BLOCK_NAMES, blocks))
    assert len(blocks) == len(BLOCK_NAMES)
    g, d = np.asarray(G), np.asarray(dims)
    ext = d * VS
    for b in blocks:
        assert b["dirs"].shape == (7, 3) and len(b["t"]) == 7 * len(b["poses"]) and b["t_label"].dtype == np.uint32
    kinds = Counter(np.concatenate([b["kind"] for b in blocks]).tolist())
    print(dims, dict(kinds))
    total = sum(kinds.values())
    assert kinds["miss"] >= 0.05 * total and kinds["random"] >= 80
    # far outside starts: 2 to 3 extents outside on every axis, within 2^12 voxels; they enter, cross and miss
    far = named["far"]
    c = far["poses"][:, :3, 3]
    outside = np.abs(c - (g + 0.5 * ext)) / ext - 0.5
    assert (outside >= 2.0).all() and (outside <= 3.0).all()
    _, inr, a, b_, n = _steps(far["o"], far["e"], dims)
    assert inr.all() and n.sum(1).max() < 1 << 12 and not VR.inside(a, dims).any()
    tr = _trace(far["o"], far["e"], dims)
    enters = sum(1 for ok, cells, end in tr if end >= 0)
    crosses = sum(1 for ok, cells, end in tr if cells and end < 0)
    misses = sum(1 for ok, cells, end in tr if not cells and end < 0)
    print("far: enter", enters, "cross", crosses, "miss the grid", misses)
    assert enters >= 1 and crosses >= 1 and misses >= 10
    # the axis block: no walk at all, axis-parallel rays, the rejected rays, the boundary pair, the waves
    ax = named["axis"]
    k = ax["kind"]
    fin, inr, a, b_, n = _steps(ax["o"], ax["e"], dims)
    ok, _, _, _ = VR.limits(ax["o"], ax["e"], G, VS, dims)
    tr = _trace(ax["o"], ax["e"], dims)
    zero = k == "nowalk_zero"
    assert zero.sum() == 7 and (ax["t_label"][zero, 0] == 0).all()                  # +0.0, bit for bit
    assert np.array_equal(ax["o"][zero].view(np.uint32), ax["e"][zero].view(np.uint32))
    assert (ax["t"][k == "nowalk_tiny"] == np.float32(2.0 ** -20)).all() and (k == "nowalk_tiny").sum() == 7
    for name in ("nowalk_zero", "nowalk_tiny", "nowalk_voxel"):
        for i in np.flatnonzero(k == name):
            assert ok[i] and n[i].sum() == 0 and tr[i][1] == [] and tr[i][2] >= 0, (name, i)   # a return, no free bit
    par = np.isin(k, ("axis", "len_ok"))
    D = ax["e"][par].astype(np.float64) - ax["o"][par].astype(np.float64)
    assert ((D != 0).sum(1) <= 1).all()
    moved = D[(n[par].sum(1) > 0)]
    for axis in range(3):
        assert (moved[:, axis] > 0).any() and (moved[:, axis] < 0).any(), axis        # +-x, +-y, +-z all step
    for name in VR.REJECTED_KINDS:
        assert (k == name).sum() >= 2, name
        assert not ok[k == name].any(), name
    assert ok[np.isfinite(ax["t"]) & ~np.isin(k, VR.REJECTED_KINDS)].all()
    ofin, efin = np.isfinite(ax["o"]).all(1), np.isfinite(ax["e"]).all(1)
    assert (ofin & ~efin)[k == "rej_e"].all() and (ax["o"][k == "rej_e"][:, 0] == np.float32(3e38)).all()
    assert (~ofin)[k == "rej_o"].all() and np.isinf(ax["o"][k == "rej_o"][:, 1]).all()
    assert (fin & ~inr)[k == "rej_coord"].all()
    assert inr[k == "rej_len"].all() and (n[k == "rej_len"].sum(1) == 1 << 24).all()
    assert VR.inside(a[k == "rej_len"], dims).all()                                   # from inside the grid, along +x
    assert (k == "len_ok").sum() == 2 and (n[k == "len_ok"].sum(1) == (1 << 24) - 1).all() and ok[k == "len_ok"].all()
    for i in np.flatnonzero(k == "len_ok"):                                           # the row to the +x face, no return
        want = [int(VR.linear((x, a[i, 1], a[i, 2]), dims)) for x in range(a[i, 0], dims[0])]
        assert tr[i] == (True, want, -1) and len(want) >= 1
    assert (k[:64] == "miss").all() and np.isinf(ax["t"][:64]).all()                 # a wave of misses only
    assert np.isin(k[64:128], VR.REJECTED_KINDS).all() and not ok[64:128].any()     # a wave of rejected rays only
    assert len({x for x in VR.REJECTED_KINDS if (k[64:128] == x).any()}) == 4
    w2 = slice(128, 192)
    assert np.isin(k[w2], VR.REJECTED_KINDS).any() and (k[w2] == "miss").any() and ok[w2].any()   # a mixed wave
    # exact ties on three and on two axes
    seen3, seen2 = set(), set()
    for name in ("tie_a", "tie_b"):
        tb = named[name]
        _, inr, a, b_, n = _steps(tb["o"], tb["e"], dims)
        tmax, tdel, D = _tmax(tb["o"], tb["e"], a, b_)
        centre = (tb["poses"][:, :3, 3] - g) / VS - 0.5
        assert (centre == centre[:, :1]).all() and (centre == np.rint(centre)).all()   # voxel centres of the main diagonal
        t3 = tb["kind"] == "tie3"
        assert (n[t3] > 0).all() and (np.abs(D[t3]) == np.abs(D[t3][:, :1])).all()
        assert (tmax[t3] == tmax[t3][:, :1]).all() and np.isfinite(tmax[t3]).all()
        assert (tdel[t3] == tdel[t3][:, :1]).all()
        t2 = tb["kind"] == "tie2"
        assert (n[t2][:, :2] > 0).all() and (tmax[t2][:, 0] == tmax[t2][:, 1]).all() and np.isfinite(tmax[t2][:, 0]).all()
        assert (D[t2][:, 2] == 0).all() and (n[t2][:, 2] == 0).all()                   # z takes no part
        seen3 |= {tuple(x) for x in np.sign(D[t3]).astype(int)}
        seen2 |= {tuple(x) for x in np.sign(D[t2]).astype(int)}
    assert len(seen3) == 8 and len(seen2) == 4
    # hostile labels, counted on the label block alone
    lb = named["label"]
    lab = lb["t_label"][np.isfinite(lb["t"]), 1]
    assert {0, 0xFFFF} <= set((lab & 0xFFFF).tolist()) and {0, 0xFFFF} <= set((lab >> 16).tolist())
    _, votes, rej = _shipped([lb], dims)
    assert rej == 0
    vox = {name: int(VR.linear(v, dims)) for name, v in VR.label_voxels(dims).items()}
    V = int(np.prod(dims))
    assert vox["first"] == 0 and vox["last"] == V - 1 and {0, V - 1} <= set(votes)   # returns in voxel 0 and V - 1
    if len(set(vox.values())) == 3:
        assert votes[vox["first"]] == (3, 0, 6)          # three-way sem tie -> the smallest; ins tie -> the smallest
        assert votes[vox["mid"]] == (0, 0xFFFF, 6)       # two-way sem tie
        assert votes[vox["last"]] == (2, 1, 6)           # the most frequent ins (9) belongs to the losing sem 7
        pairs = dict(VR.LABEL_SCENES)
        assert sorted(Counter(s for s, _ in pairs["first"]).values()) == [2, 2, 2]
        assert sorted(Counter(s for s, _ in pairs["mid"]).values()) == [3, 3]
        assert Counter(i for _, i in pairs["last"]).most_common(1)[0] == (9, 2)


def test_grids_sit_on_the_key_end_bit_boundaries():
    V = [int(np.prod(d)) for d in VR.HOSTILE_DIMS]
    assert V == [1155, 1, 31, 1024, 1023]
    assert V[0] % 32 != 0 and VR.HOSTILE_DIMS[0][2] > 32


def test_launch_edge_rays(sets):
    pose, dirs, tl = VR.launch_edge_rays(G, VS, MAIN)
    assert dirs.shape == (257, 3) and tl.shape == (257, 2) and pose.shape == (1, 4, 4)
    t = tl[:, 0].view(np.float32)
    o, e = VR.segments_of(pose, dirs, t)
    ok, a, b, n = VR.limits(o, e, G, VS, MAIN)
    ret = np.isfinite(t)
    for total in (1, 63, 64, 65, 255, 256, 257):
        assert ret[:total].any() and ok[:total][ret[:total]].any()
    assert ok[0] and n[0].sum() > 0 and VR.inside(b[0], MAIN)
    assert (~ret[:63]).any() and (ret & ~ok)[:63].any() and (t[:255] == 0).any()
    assert (~ret[64:]).any() and (ret & ~ok)[64:].any()


# ---- the inputs discriminate ----------------------------------------------------------------------------------------
# mutation -> (the variant's switches, a block whose expected output it must change)
WALK_MUTATIONS = {"tie order y before x": (dict(order=(1, 0, 2)), "tie_a"),
                  "< for <= in the axis choice": (dict(strict=True), "tie_a"),
                  "the length limit at > instead of >=": (dict(limit_gt=True), "axis"),
                  "a return recorded for a rejected ray": (dict(reject_returns=True), "axis"),
                  "sem ties to the largest": (dict(sem_largest=True), "label"),
                  "ins voted over all sems": (dict(ins_all=True), "label")}


@pytest.fixture(scope="module")
def shipped_main(sets):
    blocks = sets[MAIN]
    return [_shipped([b], MAIN) for b in blocks], _shipped(blocks, MAIN)


def test_the_unmutated_variant_is_the_shipped_restatement(sets, shipped_main):
    per_block, whole = shipped_main
    for name, b, want in zip(BLOCK_NAMES, sets[MAIN], per_block):
        assert _same(_variant([b], MAIN), want), name
    assert _same(_variant(sets[MAIN], MAIN), whole)
    for dims in VR.HOSTILE_DIMS[1:]:
        assert _same(_variant(sets[dims], dims), _shipped(sets[dims], dims)), dims


@pytest.mark.parametrize("name", list(WALK_MUTATIONS))
def test_walk_and_vote_mutations_change_the_expected_output(sets, shipped_main, name):
    per_block, whole = shipped_main
    blocks = sets[MAIN]
    switches, block = WALK_MUTATIONS[name]
    changed = [bn for bn, b, want in zip(BLOCK_NAMES, blocks, per_block) if not _same(_variant([b], MAIN, **switches), want)]
    whole_changed = not _same(_variant(blocks, MAIN, **switches), whole)
    print(f"{name}: changes blocks {changed}; the whole set: {whole_changed}")
    assert block in changed and whole_changed
    if "axis choice" in name or "tie order" in name:
        assert "tie_b" in changed                                # the two-axis ties too


# ---- the library's host walk on the segment form of the set -------------------------------------------------------------
@pytest.mark.parametrize("dims", VR.HOSTILE_DIMS)
def test_host_walk_matches_on_the_hostile_segments(sets, dims):
    from lidarcast import voxseq
    import voxseq_restate as SR
    V = int(np.prod(dims))
    o, e, _ = VR.returned_segments(sets[dims])
    free, end, ok, _ = VR.walk_long(o, e, G, VS, dims)
    bits, b, rejected = voxseq.walk(o, e, G, VS, dims)
    assert np.array_equal(bits, SR.pack_bits(free, V)) and np.array_equal(rejected, ~ok) and np.array_equal(b, end)
    for blk in sets[dims]:                                    # block by block: the union hides less
        o, e, _ = VR.returned_segments([blk])
        free, end, ok, _ = VR.walk_long(o, e, G, VS, dims)
        bits, b, rejected = voxseq.walk(o, e, G, VS, dims)
        assert np.array_equal(bits, SR.pack_bits(free, V)) and np.array_equal(rejected, ~ok) and np.array_equal(b, end)


# ---- coverage: the builders ----------------------------------------------------------------------------------------
def test_equal_q_mesh_has_one_q():
    v, f = CR.equal_q_mesh(200)
    q = CR.area_q(v, f)
    assert len(q) == 200 and q[0] > 0 and (q == q[0]).all()
    assert len(np.unique(f)) == 600                                   # every triangle on vertex rows of its own


def _waves_of(i):
    """(workgroup, pass, wave, lane) of ray i of a pose in accumulate_kernel: 1024 rays a workgroup, four passes of 256."""
    r = i % 1024
    return i // 1024, r // 256, (r % 256) // 64, r % 64


def test_edge_records_hold_the_promised_runs():
    T, N = 33, 2049
    t, prim = CR.edge_records(N, T)
    assert len(t) == 3 * N and t.dtype == np.float32 and prim.dtype == np.uint32
    ok = CR.returned(t, prim, T)
    lo, hi = CR.RUN_LANES
    assert len(set(prim[lo:hi])) == 1 and ok[lo:hi].all() and _waves_of(63)[2] != _waves_of(64)[2] and lo <= 63 < 64 < hi
    lo, hi = CR.RUN_STRIDE
    assert len(set(prim[lo:hi])) == 1 and ok[lo:hi].all() and lo <= 255 < 256 < hi
    assert _waves_of(255)[1:] == (0, 3, 63) and _waves_of(256)[1:] == (1, 0, 0)     # another pass of another lane
    lo, hi = CR.RUN_SPLIT
    assert len(set(prim[lo:hi])) == 1 and not ok[CR.SPLIT_AT] and ok[lo:CR.SPLIT_AT].all() and ok[CR.SPLIT_AT + 1:hi].all()
    assert _waves_of(lo)[:3] == _waves_of(hi - 1)[:3]                               # one wave: only the mask cuts the run
    s = CR.SINGLES
    assert prim[s["last_prim"]] == T - 1 and ok[s["last_prim"]]
    assert prim[s["prim_T"]] == T and np.isfinite(t[s["prim_T"]]) and not ok[s["prim_T"]]
    assert prim[s["invalid_prim"]] == CR.INVALID and np.isfinite(t[s["invalid_prim"]]) and not ok[s["invalid_prim"]]
    assert np.isnan(t[s["nan_t"]]) and not ok[s["nan_t"]]
    assert t[s["neg_zero_t"]] == 0 and np.signbit(t[s["neg_zero_t"]]) and ok[s["neg_zero_t"]]
    assert t[s["neg_t"]] < 0 and ok[s["neg_t"]]
    assert (prim[2 * N:] == T // 2).all() and ok[2 * N:].all()
    seen, hits, ret = CR.accumulate(t, prim, 3, N, 2, T, set_of_pose=CR.EDGE_SET_OF_POSE)
    only, h2, r2 = CR.accumulate(np.concatenate([t[:N], t[2 * N:]]), np.concatenate([prim[:N], prim[2 * N:]]), 2, N, 2, T,
                                 set_of_pose=(1, 0))
    assert np.array_equal(seen, only) and np.array_equal(hits, h2) and np.array_equal(ret, r2)   # pose 1 is dropped
    assert ret[0] == N and hits[T // 2] == N + int((ok[:N] & (prim[:N] == T // 2)).sum())
    for n in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):           # shorter poses keep what fits
        t, prim = CR.edge_records(n, T)
        assert len(t) == 3 * n


def _hits_run_not_cut(t, prim, N, T, set_of_pose, S):
    """hits with the mutation: runs are bounded by run heads only, so the non-returned rays behind a run (in its wave) are
    counted into it."""
    hits = np.zeros(T, np.int64)
    ok = CR.returned(t, prim, T)
    for p, s in enumerate(set_of_pose):
        if s >= S:
            continue
        for w0 in range(0, N, 64):
            idx = np.arange(p * N + w0, p * N + min(N, w0 + 64))
            head = [i for j, i in enumerate(idx) if ok[i] and not (j > 0 and ok[i - 1] and prim[i - 1] == prim[i])]
            for h, nxt in zip(head, head[1:] + [idx[0] + 64]):  # lanes past N are not ok and count too
                hits[prim[h]] += nxt - h
    return hits.astype(np.uint32)


def test_a_run_not_cut_at_a_non_returned_ray_changes_hits():
    T, N = 33, 257
    t, prim = CR.edge_records(N, T)
    _, hits, _ = CR.accumulate(t, prim, 3, N, 2, T, set_of_pose=CR.EDGE_SET_OF_POSE)
    wrong = _hits_run_not_cut(t, prim, N, T, CR.EDGE_SET_OF_POSE, 2)
    p = prim[CR.RUN_SPLIT[0]]
    assert wrong[p] > hits[p] and not np.array_equal(wrong, hits)


def test_tie_sets_hold_the_promised_ties():
    v, f = CR.equal_q_mesh(200)
    q = CR.area_q(v, f)
    seen = CR.tie_sets(2500)
    assert CR.tie_groups_below(2500)[:3] == [(300, 1324, 2348), (1030, 900), (2050, 1000)]
    a, b, c = CR.tie_groups_below(2500)[:3]
    assert len({k % 1024 for k in a}) == 1                                # one thread's stride-1024 loop
    assert 1030 % 1024 < 900 % 1024 and 2050 % 1024 < 1000 % 1024         # the smaller index sits in the higher thread
    picks, gains = CR.greedy(seen, q, 12)
    assert picks[:7] == [300, 1324, 2348, 900, 1030, 1000, 2050]          # the smaller index, round after round
    assert gains[0] == gains[1] == gains[2] > gains[3] == gains[4] > gains[5] == gains[6]
    g0 = [int(q[seen[k]].sum()) for k in range(2500)]
    assert sorted(np.flatnonzero(np.array(g0) == max(g0))) == [300, 1324, 2348]
    assert CR.tie_groups_below(1025) == [(0, 1024), (1022, 17)] and CR.tie_groups_below(1024) == [(1022, 17)]
    assert CR.greedy(CR.tie_sets(1025), q, 2)[0] == [0, 1024]
    sparse = CR.tie_sets(1023, sparse=True)
    assert 10 <= sparse.any(1).sum() <= 40
    t, prim, N = CR.seen_records(seen)
    got, _, _ = CR.accumulate(t, prim, 2500, N, 2500, 200)
    assert np.array_equal(got, seen)                                      # one ray per seen triangle writes the pattern


# ---- coverage: the mutations --------------------------------------------------------------------------------------------
def _greedy_variant(seen, q, budget, initial_q=0, target=None, tie_largest=False, target_gt=False):
    seen = np.asarray(seen, bool)
    S, T = seen.shape
    qi = np.array([int(x) for x in q], dtype=object)
    total = int(qi.sum())
    covered = np.zeros(T, bool)
    cq = int(initial_q)
    picks = []
    for _ in range(min(budget, S)):
        if target is not None and target > 0:
            r = float(cq) / float(total)
            if (r > target) if target_gt else (r >= target):
                break
        g = [int(qi[seen[k] & ~covered].sum()) if (seen[k] & ~covered).any() else 0 for k in range(S)]
        best = max(g)
        if best == 0:
            break
        k = max(i for i in range(S) if g[i] == best) if tie_largest else g.index(best)
        picks.append(k)
        covered |= seen[k]
        cq += best
    return picks


def test_greedy_mutations_change_the_picks():
    v, f = CR.equal_q_mesh(200)
    q = CR.area_q(v, f)
    seen = CR.tie_sets(1025)
    picks, gains = CR.greedy(seen, q, 6)
    assert _greedy_variant(seen, q, 6) == picks
    assert _greedy_variant(seen, q, 6, tie_largest=True) != picks
    cum = CR.cumulative_q(gains)
    total = sum(int(x) for x in q)
    target = float(cum[2]) / float(total)
    assert CR.greedy(seen, q, 6, target_ratio=target)[0] == picks[:3]               # reached exactly: stops after pick 3
    assert _greedy_variant(seen, q, 6, target=target) == picks[:3]
    assert _greedy_variant(seen, q, 6, target=target, target_gt=True) == picks[:4]   # > takes one more
    assert CR.greedy(seen, q, 6, target_ratio=float(np.nextafter(target, 2.0)))[0] == picks[:4]


def _cover_q(words, q, T, mask_tail=True):
    """covered q of a (W,) uint32 cover; without the tail mask the stray bits past T count too (here as the last q)."""
    bits = np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little").astype(bool)
    pad = np.concatenate([q, np.full(len(bits) - T, q[-1], q.dtype)])
    if mask_tail:
        bits[T:] = False
    return sum(int(x) for x in pad[bits])


def test_no_tail_mask_changes_the_initial_cover():
    T = 200
    v, f = CR.equal_q_mesh(T)
    q = CR.area_q(v, f)
    init = np.zeros(T, bool)
    init[[3, 199]] = True
    words = CR.pack(init).copy()
    words[-1] |= np.uint32(0xFFFFFF00)                                   # bits 200..223 of the last word: strays
    assert CR.words(T) * 32 - T == 24
    assert _cover_q(words, q, T) == CR.covered_q(init, q) == 2 * int(q[0])
    assert _cover_q(words, q, T, mask_tail=False) == 26 * int(q[0])
    seen = CR.tie_sets(1025)
    seen[:, [3, 199]] = False
    _, gains = CR.greedy(seen, q, 4, initial=init)
    total = T * int(q[0])
    target = float(2 * int(q[0]) + gains[0] + gains[1]) / float(total)
    right = _greedy_variant(seen, q, 4, initial_q=_cover_q(words, q, T), target=target)
    wrong = _greedy_variant(seen, q, 4, initial_q=_cover_q(words, q, T, mask_tail=False), target=target)
    assert len(right) == 2 and len(wrong) < 2


# ---- greedy's target rule is the header's ----------------------------------------------------------------------------------
def test_target_rule_is_two_float64_conversions_then_a_divide():
    with open(os.path.join(REPO, "include", "lidarcast.h")) as fh:
        text = re.sub(r"\s*\n \*\s*", " ", fh.read())
    assert "float64(covered_q) / float64(total_q) >= target_ratio" in text
    cq, total = 9007199255810829, 4611685877708047420
    assert cq > 2 ** 53
    old, new = cq / total, float(cq) / float(total)
    assert old != new and new < old
    # one triangle of q = total - cq and one of q = cq: after the first pick (the larger) ... the ratio is tested on cq
    q = np.array([cq, total - cq], np.uint64)
    seen = np.eye(2, dtype=bool)
    first = np.array([True, False])
    assert CR.greedy(seen, q, 2, initial=first, target_ratio=new)[0] == []         # reached by the header's rule
    assert CR.greedy(seen, q, 2, initial=first, target_ratio=old)[0] == [1]        # int / int would have stopped here
