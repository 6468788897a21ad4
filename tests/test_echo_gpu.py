"""-m gpu: beam footprint and multi-echo returns reduced in the trace kernel (lrc_scan_echoes_dev / lrc_scan_echoes_compact,
GEN = 6).

The comparator, as tests/test_noise_gpu.py does it: the sub-ray rows are restated on the host (tests/echo_restate.py over
noise_restate.jitter_rows), cast through the explicit-ray path with nothing filtered, reduced in numpy, and the echo record
is assembled from the representative's t / prim / normal3 / sem / ins with point3 the float32 o + unit(d_axis) * t and the
range filter in float64.  Every column must agree bit for bit, except incident_deg of echoes whose representative is not
sub-ray 0: there the device's acos meets libm's on identical inputs, rtol 1e-13 (about 450 ulp).  Each case asserts on the
restatement that it exercises what it is for."""
import numpy as np
import pytest

import echo_restate as er
import helpers
from helpers import pose, random_soup, sensor_small

pytestmark = pytest.mark.gpu

HITS = ("t", "prim", "normal3", "point3", "sem", "ins", "incident_deg")
FRAMES = ("point3", "sem", "ins", "incident_deg", "index", "range_origin", "range_origin_stats", "incident_stats")
RAD2DEG = 57.29577951308232
INVALID = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


@pytest.fixture(scope="module")
def room():
    from lidarcast import synth
    return synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)


@pytest.fixture(scope="module")
def soup():
    from lidarcast.synth import TriangleMesh
    v, t = random_soup(300, seed=3, extent=4.0, size=0.8)
    return TriangleMesh(vertices=v, triangles=t)


def assert_bit_equal(a, b, what=""):
    """helpers.assert_bit_equal, and plain equality for the one-byte columns (weights, echo numbers)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.itemsize != 1:
        return helpers.assert_bit_equal(a, b, what)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ne = a != b
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} entries differ; first at {np.argwhere(ne)[0]}"


def table(lines, width):
    """The small sensor's direction table with one row straight up and one straight down (h == 0: its sub-rays coincide)."""
    from lidar import IndoorLidar
    dirs = IndoorLidar(sensor_small(lines, width), np.eye(4)).sensor_directions().copy()
    dirs[7] = (0.0, 0.0, 1.0)
    dirs[11] = (0.0, 0.0, -1.0)
    return dirs


def room_poses(P):
    ps = [pose(1.0 + 0.45 * j, 1.2 + 0.1 * j, 1.0 + 0.05 * j) for j in range(P)]
    ps[1 % P] = pose(1.0 + 0.45 * (1 % P), 1.3, 1.05, yaw=0.7)
    return np.stack(ps)


def soup_poses(P):
    return np.stack([pose(0.3 * j, 0.2 * j, 0.1 * j, yaw=0.7 * j) for j in range(P)])


def ring(K, radius):
    """(K, 2) offsets: the axis and K - 1 sub-rays on a ring."""
    a = np.arange(K - 1) * (2.0 * np.pi / max(K - 1, 1))
    return np.concatenate([np.zeros((1, 2)), np.stack([radius * np.cos(a), radius * np.sin(a)], axis=1)])


def subray_rays(poses, dirs, offsets):
    """(P, K, N, 6) float32 rays of every sub-ray, (P, N, 3) float32 axis directions, (P, 3) float64 centres."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    rows = er.subray_rows(dirs, offsets)
    P, K, N = len(poses), len(rows), len(dirs)
    rays = np.empty((P, K, N, 6), np.float32)
    axis = np.empty((P, N, 3), np.float32)
    for p, M in enumerate(poses):
        rays[p, :, :, :3] = M[:3, 3].astype(np.float32)
        for k in range(K):
            rays[p, k, :, 3:] = np.dot(rows[k], M[:3, :3].T).astype(np.float32)      # the BLAS product of IndoorLidar.get_rays
        axis[p] = np.dot(np.asarray(dirs, np.float64), M[:3, :3].T).astype(np.float32)
    return rays, axis, poses[:, :3, 3].copy()


def assemble(sub, axis, origin, centres, beam, max_range, min_range=0.0, incident_mode=0):
    """The echo records (P * N * E) of sub-ray records ``sub`` (dict of (P, K, N, ...) arrays, t raw): dict of HITS columns,
    ``weight``, ``rep`` (P * N, E) and ``exact_inc`` (P * N * E) bool -- True where incident_deg is the device's own value of
    sub-ray 0 and must match bit for bit."""
    P, K, N = sub["t"].shape
    E = beam.max_echoes
    t_k = np.ascontiguousarray(sub["t"].transpose(0, 2, 1)).reshape(P * N, K)
    rep, weight = er.reduce_rows(t_k, E, beam.min_count, np.float32(beam.separation))
    B = P * N
    pi, ni = np.divmod(np.arange(B), N)
    out = {"t": np.full((B, E), np.inf, np.float32), "prim": np.full((B, E), INVALID, np.uint32),
           "normal3": np.zeros((B, E, 3), np.float32), "point3": np.zeros((B, E, 3), np.float32),
           "sem": np.zeros((B, E), np.uint16), "ins": np.zeros((B, E), np.uint16), "incident_deg": np.zeros((B, E))}
    exact = np.zeros((B, E), bool)
    d = axis.reshape(B, 3)
    o = origin[pi]                                                   # (B, 3) float32
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    h = d / nrm[:, None]                                             # float32, one rounding per operation
    for e in range(E):
        k = rep[:, e]
        has = k >= 0
        kk = np.where(has, k, 0)
        t = sub["t"][pi, kk, ni]
        with np.errstate(invalid="ignore"):          # a slot without an echo carries an infinite t through the arithmetic
            pt = o + h * t[:, None]
            ex = pt.astype(np.float64) - centres[pi]
            dist = np.sqrt((ex[:, 0] * ex[:, 0] + ex[:, 1] * ex[:, 1]) + ex[:, 2] * ex[:, 2])
            keep = has & (dist < max_range)
            if min_range > 0.0:
                keep &= dist >= min_range
            nm = sub["normal3"][pi, kk, ni]
            if incident_mode == 1:
                cs = np.abs((h[:, 0].astype(np.float64) * nm[:, 0] + h[:, 1].astype(np.float64) * nm[:, 1])
                            + h[:, 2].astype(np.float64) * nm[:, 2])
                inc = np.arccos(np.minimum(cs, 1.0)) * RAD2DEG
            else:
                inc = np.arccos(np.abs(ex[:, 2] / dist)) * RAD2DEG
        # sub-ray 0 with a zero offset IS the axis ray: the explicit cast formed its angle on the device from the same inputs
        own = keep & (k == 0) & (beam.offsets[0] == 0.0).all()
        inc = np.where(own, sub["incident_deg"][pi, 0, ni], inc)
        exact[:, e] = own
        out["t"][keep, e] = t[keep]
        out["prim"][keep, e] = sub["prim"][pi, kk, ni][keep]
        out["normal3"][keep, e] = nm[keep]
        out["point3"][keep, e] = pt[keep]
        out["sem"][keep, e] = sub["sem"][pi, kk, ni][keep]
        out["ins"][keep, e] = sub["ins"][pi, kk, ni][keep]
        out["incident_deg"][keep, e] = inc[keep]
    res = {a: v.reshape((B * E,) + v.shape[2:]) for a, v in out.items()}
    res.update(weight=weight.reshape(-1), rep=rep, exact_inc=exact.reshape(-1), t_k=t_k)
    return res


def _views(out):
    for k, dt in (("prim", np.uint32), ("sem", np.uint16), ("ins", np.uint16)):
        if k in out:
            out[k] = out[k].view(dt)
    return out


def explicit_subrays(scene, poses, dirs, offsets, incident_mode=0):
    """Every sub-ray through lrc_cast_segments, one segment per (pose, sub-ray), nothing filtered (max_range = inf, no
    min_range): dict of (P, K, N, ...) arrays."""
    rays, axis, cen = subray_rays(poses, dirs, offsets)
    P, K, N = rays.shape[:3]
    off = np.arange(P * K + 1, dtype=np.uint64) * np.uint64(N)
    try:
        scene.set_options(min_range=0.0, incident_mode=incident_mode)
        rec = _views(scene.cast_segments(rays.reshape(-1, 6), off, np.repeat(cen, K, axis=0), np.inf, want=HITS))
    finally:
        scene.reset_options()
    sub = {a: v.reshape((P, K, N) + v.shape[1:]) for a, v in rec.items()}
    return sub, axis, rays[:, 0, 0, :3].copy(), cen


def echo_dev(scene, poses, dirs, beam, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    P, N, E = len(poses), len(dirs), beam.max_echoes
    hits = DeviceHits(P * N * E, "cuda", want=want)
    w = torch.full((P * N * E,), 255, dtype=torch.uint8, device="cuda")
    scene.scan_echoes_dev(torch.from_numpy(np.ascontiguousarray(poses).reshape(P, 16).copy()).cuda(),
                          torch.from_numpy(np.ascontiguousarray(dirs)).cuda(), hits, max_range, beam, weight_t=w)
    torch.cuda.synchronize()
    out = _views({k: hits[k].cpu().numpy() for k in want})
    out["weight"] = w.cpu().numpy()
    return out


def clean_dev(scene, poses, dirs, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    scene.scan_poses_dev(torch.from_numpy(np.ascontiguousarray(poses).reshape(P, 16).copy()).cuda(),
                         torch.from_numpy(np.ascontiguousarray(dirs)).cuda(), hits, max_range)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


def assert_records(got, want, what):
    for a in HITS:
        if a == "incident_deg":
            ex = want["exact_inc"]
            assert_bit_equal(got[a][ex], want[a][ex], f"{what}: incident_deg of echoes represented by sub-ray 0")
            g, w = got[a][~ex], want[a][~ex]
            err = np.abs(g - w) / np.maximum(np.abs(w), np.finfo(np.float64).tiny)
            print(f"\n[echo] {what}: incident_deg of {len(g)} other echoes, max relative difference {err.max() if len(g) else 0:.3g}")
            np.testing.assert_allclose(g, w, rtol=1e-13, atol=0, err_msg=f"{what}: incident_deg")
        else:
            assert_bit_equal(got[a], want[a], f"{what}: {a}")
    assert_bit_equal(got["weight"], want["weight"], f"{what}: weight")


def run_case(scene, poses, dirs, beam, max_range, min_range=0.0, incident_mode=0, what=""):
    sub, axis, origin, cen = explicit_subrays(scene, poses, dirs, beam.offsets, incident_mode)
    want = assemble(sub, axis, origin, cen, beam, max_range, min_range, incident_mode)
    try:
        scene.set_options(min_range=min_range, incident_mode=incident_mode)
        got = echo_dev(scene, poses, dirs, beam, max_range)
    finally:
        scene.reset_options()
    assert_records(got, want, what)
    return got, want


def beam_model(K, radius, E=2, min_count=1, separation=0.05):
    from lidarcast.echo import BeamModel
    return BeamModel(2.0 * np.sqrt(2.0) * radius, pattern=ring(K, radius), max_echoes=E, separation=separation,
                     min_fraction=(min_count - 0.5) / K if min_count > 1 else 0.0)


def host_frames(rec, weight, P, NE, E):
    """Host compaction of fixed-stride echo records: what lrc_scan_echoes_compact must return."""
    keep = (rec["t"] != np.inf).reshape(P, NE)
    sel = keep.reshape(-1)
    pts = rec["point3"][sel]
    ro = np.linalg.norm(pts, axis=1) if len(pts) else np.zeros(0, np.float32)
    counts = keep.sum(1)
    ends = np.cumsum(counts)
    idx = np.nonzero(keep)[1].astype(np.uint32)
    out = {"counts": counts, "point3": pts, "sem": rec["sem"][sel], "ins": rec["ins"][sel],
           "incident_deg": rec["incident_deg"][sel], "index": idx, "range_origin": ro,
           "beam_index": idx // np.uint32(E), "echo_index": (idx % np.uint32(E)).astype(np.uint8), "echo_weight": weight[sel]}
    for col, a in (("range_origin", ro), ("incident", out["incident_deg"])):
        out[f"{col}_mean"] = np.array([np.mean(a[e - c:e]) if c else 0 for c, e in zip(counts, ends)], dtype=a.dtype)
        out[f"{col}_std"] = np.array([np.std(a[e - c:e]) if c else 0 for c, e in zip(counts, ends)], dtype=a.dtype)
    return out


def assert_frames_equal(fr, want, what):
    assert fr["counts"].tolist() == want["counts"].tolist(), what
    for k in ("point3", "sem", "ins", "incident_deg", "index", "range_origin", "range_origin_mean", "range_origin_std",
              "incident_mean", "incident_std", "beam_index", "echo_index", "echo_weight"):
        assert_bit_equal(fr[k], want[k], f"{what}: {k}")


# ---- the reduction against the restatement ---------------------------------------------------------------------------------

def test_soup_hex_ring_two_echoes(engine, soup):
    """4 x 100, K = 7 (G = 8: 12.5 waves per pose), E = 2 on the triangle soup: two-echo beams, all-miss beams, beams whose axis
    misses while a ring sub-ray hits, beams with more clusters than echoes; then min_count 2."""
    dirs, poses = table(4, 100), soup_poses(3)
    scene = engine.scene_for(soup)
    beam = beam_model(7, 0.02)
    got, want = run_case(scene, poses, dirs, beam, 20.0, what="soup K=7")
    t_k, rep = want["t_k"], want["rep"]
    hit = np.isfinite(t_k)
    nclu = er.count_clusters(t_k, 1, np.float32(0.05))
    print(f"\n[echo] soup K=7: two echoes {int((rep[:, 1] >= 0).sum())}, all miss {int((~hit.any(1)).sum())}, "
          f"axis miss + off-axis hit {int((~hit[:, 0] & hit[:, 1:].any(1)).sum())}, more clusters than E {int((nclu > 2).sum())}")
    assert (rep[:, 1] >= 0).sum() >= 100
    assert (~hit.any(1)).sum() >= 50
    assert (~hit[:, 0] & hit[:, 1:].any(1)).sum() >= 50
    assert (nclu > 2).sum() >= 50
    assert_bit_equal(t_k[7::400], np.repeat(t_k[7::400, :1], 7, axis=1))          # the +-z rows: seven coincident sub-rays
    assert_bit_equal(t_k[11::400], np.repeat(t_k[11::400, :1], 7, axis=1))
    beam2 = beam_model(7, 0.02, min_count=2)
    assert beam2.min_count == 2
    got2, want2 = run_case(scene, poses, dirs, beam2, 20.0, what="soup K=7 min_count 2")
    changed = (want2["rep"] != rep).any(axis=1) | (want2["weight"].reshape(-1, 2) != want["weight"].reshape(-1, 2)).any(axis=1)
    print(f"[echo] soup K=7: min_count 2 changes {int(changed.sum())} beams")
    assert changed.sum() >= 50


def test_room_hex_ring(engine, room):
    dirs, poses = table(4, 100), room_poses(3)
    got, want = run_case(engine.scene_for(room), poses, dirs, beam_model(7, 0.02), 20.0, what="room K=7")
    two = (want["rep"][:, 1] >= 0).sum()
    print(f"\n[echo] room K=7: two-echo beams {int(two)}")
    assert two >= 40


@pytest.mark.parametrize("width,K,radius", [(96, 5, 0.02), (100, 16, 0.03)])
def test_other_group_sizes(engine, soup, width, K, radius):
    """K = 5 on a pose of whole waves (G = 8) and K = 16 (G = 16, four beams per wave)."""
    dirs, poses = table(4, width), soup_poses(3)
    got, want = run_case(engine.scene_for(soup), poses, dirs, beam_model(K, radius), 20.0, what=f"soup K={K}")
    assert (want["rep"][:, 1] >= 0).sum() >= 50
    assert (want["weight"].reshape(-1, 2)[:, 0] >= 2).sum() >= 50


@pytest.mark.parametrize("E", [1, 2, 3])
@pytest.mark.parametrize("min_count", [1, 2])
def test_three_subrays_every_echo_count(engine, soup, E, min_count):
    """K = 3 in groups of four lanes, with one to three echo slots."""
    dirs, poses = table(4, 100), soup_poses(3)
    beam = beam_model(3, 0.02, E=E, min_count=min_count)
    assert (beam.subrays, beam.max_echoes, beam.min_count) == (3, E, min_count)
    got, want = run_case(engine.scene_for(soup), poses, dirs, beam, 20.0, what=f"soup K=3 E={E} min_count={min_count}")
    rep = want["rep"]
    assert (rep[:, 0] >= 0).sum() >= 100
    if min_count == 1:
        assert (rep[:, E - 1] >= 0).sum() >= 5              # the last slot is used
    assert (rep[:, 0] < 0).sum() >= 50


@pytest.mark.parametrize("K,E", [(1, 1), (2, 1), (1, 4), (2, 4), (3, 4), (7, 2), (16, 2)])
def test_launch_shapes_with_partial_waves(engine, soup, K, E):
    """Every group size G = 1, 2, 4, 8, 16 on two poses of 397 beams: a pose is no whole number of waves, so one wave holds
    groups of both poses and the launch ends in a partial wave.  E > K: the echo-writing lanes e >= K cast nothing; G = 2 and
    G = 1 run through the kernel at all."""
    dirs, poses = table(4, 100)[:397], soup_poses(2)
    N, P = len(dirs), len(poses)
    beam = beam_model(K, 0.02, E=E)
    G = 1 << er_group_log2(K, E)
    assert (beam.subrays, beam.max_echoes) == (K, E) and G == {(1, 1): 1, (2, 1): 2, (7, 2): 8, (16, 2): 16}.get((K, E), 4)
    assert P >= 2 and (N * G) % 64 != 0 and (P * N * G) % 64 != 0
    got, want = run_case(engine.scene_for(soup), poses, dirs, beam, 20.0, what=f"soup K={K} E={E} N={N}")
    rep = want["rep"]
    print(f"\n[echo] K={K} E={E} G={G}: echoes per slot {(rep >= 0).sum(axis=0).tolist()}, all-miss beams {int((rep[:, 0] < 0).sum())}")
    assert (rep[:, 0] >= 0).sum() >= 50 and (rep[:, 0] < 0).sum() >= 20
    if min(K, E) >= 2:
        assert (rep[:, 1] >= 0).sum() >= 1
    if E > K:                                                # more slots than sub-rays: the slots behind K are always empty
        assert (rep[:, K:] == -1).all()
        empty = (rep < 0).reshape(-1)
        assert np.isinf(got["t"][empty]).all() and (got["weight"][empty] == 0).all() and (got["prim"][empty] == INVALID).all()


def er_group_log2(K, E):
    g = 0
    while (1 << g) < max(K, E):
        g += 1
    return g


def test_separation_at_a_measured_gap(engine, soup):
    """Three float32 gaps between consecutive sub-rays (in the order by range) that the soup's own beams show, each as the
    separation and one float below it: at the gap itself the two sub-rays share a cluster (the gap does not EXCEED the
    separation), one float below they do not.  In a scan such an equality happens by luck or not at all."""
    dirs, poses = table(4, 100), soup_poses(3)
    scene = engine.scene_for(soup)
    K, E = 7, 4
    sub, _, _, _ = explicit_subrays(scene, poses, dirs, ring(K, 0.02))
    P, _, N = sub["t"].shape
    t_k = np.ascontiguousarray(sub["t"].transpose(0, 2, 1)).reshape(P * N, K)
    found = []                                               # (beam, gap)
    for b in range(len(t_k)):
        s = np.sort(t_k[b][np.isfinite(t_k[b])])
        gaps = (s[1:] - s[:-1]).astype(np.float32)
        ok = gaps[(gaps > np.float32(0.01)) & (gaps < np.float32(0.2))]
        for g in ok:
            below = np.nextafter(g, np.float32(0.0))
            n_at, n_below = (int(er.count_clusters(t_k[b:b + 1], 1, s_)[0]) for s_ in (g, below))
            if n_below == n_at + 1 and n_below <= E:
                found.append((b, g))
                break
    assert len(found) >= 3, len(found)
    for b, g in (found[0], found[len(found) // 2], found[-1]):
        below = np.nextafter(g, np.float32(0.0))
        assert g.dtype == np.float32 and 0.01 < g < 0.2 and below < g
        res = {}
        for name, sep in (("at", g), ("below", below)):
            beam = beam_model(K, 0.02, E=E, separation=float(sep))
            assert np.float32(beam.struct().separation) == sep
            got, want = run_case(scene, poses, dirs, beam, 20.0, what=f"soup K=7 separation {name} the gap {g!r} of beam {b}")
            res[name] = want
        n_at, n_below = (int((res[k]["rep"][b] >= 0).sum()) for k in ("at", "below"))
        print(f"\n[echo] beam {b}: gap {g!r}: {n_at} clusters at the gap, {n_below} one float below; "
              f"beams that differ between the two scans {int((res['at']['rep'] != res['below']['rep']).any(axis=1).sum())}")
        assert n_below == n_at + 1                          # the restatement shows that beam with one cluster fewer at g


def test_range_filter_min_range_and_normal_incidence(engine, room):
    dirs, poses = table(4, 100), room_poses(3)
    scene = engine.scene_for(room)
    got, want = run_case(scene, poses, dirs, beam_model(7, 0.02), 2.2, min_range=0.9, incident_mode=1, what="room cut")
    hit = want["rep"].reshape(-1) >= 0
    kept = np.isfinite(want["t"])
    assert (hit & ~kept).sum() >= 0.05 * hit.size                           # echoes the filter removed
    assert kept.sum() >= 0.05 * hit.size
    assert (got["weight"][hit & ~kept] > 0).all()                           # the weight is the reduction's, filtered or not


# ---- the properties of the header ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [100, 96])
def test_p1_single_subray_is_the_clean_scan(engine, room, width):
    from lidarcast.echo import BeamModel
    dirs, poses = table(4, width), room_poses(3)
    scene = engine.scene_for(room)
    clean = clean_dev(scene, poses, dirs, 3.0)
    got = echo_dev(scene, poses, dirs, BeamModel(0.0, pattern="single", max_echoes=1), 3.0)
    for a in HITS:
        assert_bit_equal(got[a], clean[a], f"P1: {a}")
    assert_bit_equal(got["weight"], np.isfinite(clean_dev(scene, poses, dirs, 1e9, want=("t",))["t"]).astype(np.uint8), "P1: weight")
    assert 0.05 < np.isfinite(got["t"]).mean() < 1.0


def test_p2_echo_of_the_axis_is_the_clean_record(engine, room):
    from lidarcast.echo import BeamModel
    dirs, poses = table(4, 100), room_poses(3)
    scene = engine.scene_for(room)
    beam = BeamModel(1.5e-3, pattern="hex7", max_echoes=2)
    clean = clean_dev(scene, poses, dirs, 20.0)
    got = echo_dev(scene, poses, dirs, beam, 20.0)
    sub, axis, origin, cen = explicit_subrays(scene, poses, dirs, beam.offsets)
    rep = assemble(sub, axis, origin, cen, beam, 20.0)["rep"]
    b, e = np.nonzero(rep == 0)
    assert len(b) >= 0.9 * np.isfinite(clean["t"]).sum() > 100
    for a in HITS:
        assert_bit_equal(got[a].reshape((-1, 2) + got[a].shape[1:])[b, e], clean[a][b], f"P2: {a}")


def test_p3_independent_of_batching(engine, soup):
    dirs = table(4, 100)
    poses = soup_poses(6)
    scene = engine.scene_for(soup)
    beam = beam_model(7, 0.02)
    whole = echo_dev(scene, poses, dirs, beam, 20.0)
    a, b = echo_dev(scene, poses[:2], dirs, beam, 20.0), echo_dev(scene, poses[2:], dirs, beam, 20.0)
    for k in HITS + ("weight",):
        assert_bit_equal(whole[k], np.concatenate([a[k], b[k]]), f"P3: {k}")
    back = echo_dev(scene, poses[::-1], dirs, beam, 20.0)
    n = len(dirs) * 2
    for k in HITS + ("weight",):
        w = whole[k].reshape((6, n) + whole[k].shape[1:])
        assert_bit_equal(back[k].reshape(w.shape)[::-1], w, f"P3 reversed: {k}")


# ---- frames -------------------------------------------------------------------------------------------------------------------

def test_compact_and_engine_frames(engine, room, soup):
    from lidar import IndoorLidar
    for mesh, poses, width in ((soup, soup_poses(3), 100), (room, room_poses(3), 96)):
        dirs = table(4, width)
        scene = engine.scene_for(mesh)
        beam = beam_model(7, 0.02)
        P, NE = len(poses), len(dirs) * 2
        rec = echo_dev(scene, poses, dirs, beam, 3.0)
        fr = scene.scan_echoes_compact(poses, dirs, 3.0, beam, want=FRAMES)
        want = host_frames(rec, rec["weight"], P, NE, 2)
        assert want["counts"].sum() > 100 and (want["echo_index"] == 1).sum() >= 20
        assert_frames_equal(fr, want, "compact")
        small = scene.scan_echoes_compact(poses, dirs, 3.0, beam, want=("point3",))              # no index column asked for
        assert "index" not in small
        assert_bit_equal(small["echo_weight"], want["echo_weight"], "compact without index: echo_weight")
        assert_bit_equal(small["beam_index"], want["beam_index"], "compact without index: beam_index")
        with pytest.raises(ValueError, match="capacity"):
            scene.scan_echoes_compact(poses, dirs, 3.0, beam, want=FRAMES, capacity=10)
    # the engine surface over the resident table of a real sensor record
    k = sensor_small(4, 96)
    kd = IndoorLidar(k, np.eye(4)).sensor_directions()
    poses = room_poses(3)
    scene = engine.scene_for(room)
    beam = beam_model(7, 0.02)
    fr2 = engine.scan_echo_frames(k, poses, room, beam, want=FRAMES)
    rec = echo_dev(scene, poses, kd, beam, k.max_range)
    assert_frames_equal(fr2, host_frames(rec, rec["weight"], 3, len(kd) * 2, 2), "engine")


def test_refusals_on_a_scene(engine, room):
    import torch
    from lidarcast import DeviceHits
    dirs, poses = table(4, 96), room_poses(2)
    scene = engine.scene_for(room)
    beam = beam_model(7, 0.02)
    P, N = len(poses), len(dirs)
    pt = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dt = torch.from_numpy(dirs).cuda()
    with pytest.raises(ValueError, match="tile_count"):
        scene.scan_echoes_dev(pt, dt, DeviceHits(P * N * 2, "cuda", want=("t", "tile_count")), 20.0, beam)
    noise = torch.zeros(P * N * 2, dtype=torch.float32, device="cuda")
    try:
        scene.set_options(range_noise=(noise.data_ptr(), noise.numel()))
        with pytest.raises(ValueError, match="range_noise"):
            scene.scan_echoes_dev(pt, dt, DeviceHits(P * N * 2, "cuda", want=("t",)), 20.0, beam)
        with pytest.raises(ValueError, match="range_noise"):
            scene.scan_echoes_compact(poses, dirs, 20.0, beam)
    finally:
        scene.reset_options()
    with pytest.raises(ValueError, match="P \\* N \\* max_echoes"):
        scene.scan_echoes_dev(pt, dt, DeviceHits(P * N, "cuda", want=("t",)), 20.0, beam)


# ---- the simulator key ---------------------------------------------------------------------------------------------------------

def _sim(config, mesh, **kw):
    import s3dis_simulator
    sim = s3dis_simulator.S3DISSimulator(config, **kw)
    sim.load_scene(mesh, "room")
    return sim


def test_simulator_beam_key(engine, room, monkeypatch):
    from lidarcast.echo import BeamModel
    from trajectory import line_trajectory, poses_from_waypoints
    wps = line_trajectory((1.0, 1.2, 1.0), (3.0, 1.8, 1.0), 4, yaw=0.6)
    base = {"raycast_engine": {"use_gpu": True}}
    key = {"divergence_mrad": 40.0 * np.sqrt(2.0), "pattern": "hex7", "max_echoes": 2}          # ring radius 0.02 rad
    clean = _sim(dict(base), room).run_simulation(wps)
    sim = _sim(dict(base, beam=dict(key)), room)
    one = sim.run_simulation(wps)
    eager = _sim({"raycast_engine": {"use_gpu": True, "eager_labels": True}, "beam": dict(key)}, room).run_simulation(wps)
    assert one.get_total_frames() == 4
    fr = engine.scan_echo_frames(sim.lidar_config, poses_from_waypoints(wps), room, sim._beam_model(),
                                 want=("point3", "sem", "ins", "incident_deg"))
    ends = np.cumsum(fr["counts"])
    second = 0
    for i, (a, b, c) in enumerate(zip(one.frames, eager.frames, clean.frames)):
        lo, hi = ends[i] - fr["counts"][i], ends[i]
        assert_bit_equal(a.points, fr["point3"][lo:hi], "frame points")
        assert_bit_equal(a.points, b.points)
        assert_bit_equal(a.semantic_labels, fr["sem"][lo:hi], "lazy labels come from an echo rescan")
        assert_bit_equal(a.instance_labels, fr["ins"][lo:hi])
        assert_bit_equal(b.semantic_labels, fr["sem"][lo:hi], "eager labels come with the points")
        assert_bit_equal(a.beam_index, fr["beam_index"][lo:hi])
        assert_bit_equal(a.echo_index, fr["echo_index"][lo:hi])
        assert_bit_equal(a.echo_weight, fr["echo_weight"][lo:hi])
        assert len(a.points) == len(a.semantic_labels) == len(a.echo_weight) > len(c.points)     # second echoes add points
        assert (a.echo_weight >= 1).all() and (a.echo_weight <= 7).all() and a.echo_index.max() <= 1
        second += int((a.echo_index == 1).sum())
        assert not hasattr(c, "echo_weight")                                                      # without the key nothing changes
    assert second >= 20
    assert sim._beam_model().offsets.shape == (7, 2) and isinstance(sim._beam_model(), BeamModel)
    # what the key does not cover raises instead of quietly scanning something else
    with pytest.raises(ValueError, match="motion"):
        _sim(dict(base, beam=dict(key), motion={"speed": 0.5}), room).run_simulation(wps)
    with pytest.raises(ValueError, match="noise"):
        _sim(dict(base, beam=dict(key), noise={"seed": 1}), room).run_simulation(wps)
    with pytest.raises(ValueError, match="dual-axis"):
        _sim(dict(base, beam=dict(key)), room, use_blk2go=True).run_simulation(wps[:2])
    with pytest.raises(ValueError, match="unknown entries under the beam key"):
        _sim(dict(base, beam=dict(key, rings=2)), room).run_simulation(wps)
    for export in (lambda: sim.evaluate_surface_coverage(wps), lambda: sim.export_occupancy_grid(wps, "unused"),
                   lambda: sim.export_frame_annotations(wps, "unused")):
        with pytest.raises(NotImplementedError, match="beam key"):
            export()
    import lidarcast.distributed as ld
    monkeypatch.setattr(ld, "active_group", lambda group=None: (object(), group))
    with pytest.raises(ValueError, match="multi-rank"):
        _sim(dict(base, beam=dict(key)), room).run_simulation(wps)
