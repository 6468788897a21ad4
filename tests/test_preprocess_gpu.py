"""GPU: room preprocessing (lidarcast.preprocess_cloud / preprocess_cloud_dev, csrc/lrc_preprocess.hip) against a
numpy / scipy restatement of the contract in include/lidarcast.h "cloud preprocessing" kept in this file, and end to
end through s3dis_data_loader.main on a synthetic S3DIS folder.  The restatement is not Open3D: parity with Open3D
itself (neighbour tie order, summation order, eigenvector sign) is not pinned."""
import pickle

import numpy as np
import pytest

import neighbour_restate as nr

pytestmark = pytest.mark.gpu


# ---- restatement ----------------------------------------------------------------------------------------------------
def _d2(q, p):
    d = q[:, None, :] - p
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def restate_avg(p, k, rows=None, chunk=1 << 16):
    """avg of the given rows: cKDTree candidates, the defined d2, the min(k, n) smallest ascending, square roots summed
    one after the other (np.cumsum), / min(k, n)."""
    from scipy.spatial import cKDTree
    n = len(p)
    rows = np.arange(n) if rows is None else rows
    kk = min(n, k + 8)
    found = min(k, n)
    tree = cKDTree(p)
    out = np.empty(len(rows))
    for a in range(0, len(rows), chunk):
        q = p[rows[a:a + chunk]]
        _, cand = tree.query(q, kk, workers=16)
        d2 = np.sort(_d2(q, p[cand.reshape(len(q), kk)]), axis=1)[:, :found]
        out[a:a + chunk] = np.cumsum(np.sqrt(d2), axis=1)[:, -1] / found
    return out


def restate_filter(avg, std_ratio):
    n = len(avg)
    pos = avg[avg > 0]
    mean = pos.sum() / n
    thr = mean + std_ratio * np.sqrt(((pos - mean) ** 2).sum() / (n - 1))
    return mean, thr


def restate_neighbours(pk, radius, max_nn, rows, spare=40):
    """(count, ordered neighbour indices padded with -1, cumulant covariance) per row: candidates from cKDTree, the
    defined d2, d2 < radius^2, ordered by (d2, index), the first max_nn."""
    from scipy.spatial import cKDTree
    tree = cKDTree(pk)
    kk = min(len(pk), max_nn + spare)
    q = pk[rows]
    dist, cand = tree.query(q, kk, distance_upper_bound=radius * 1.001, workers=16)
    cand = cand.reshape(len(q), kk)
    valid = cand < len(pk)
    cand = np.where(valid, cand, 0)
    d2 = np.where(valid, _d2(q, pk[cand]), np.inf)
    d2 = np.where(d2 < radius * radius, d2, np.inf)
    order = np.lexsort((cand, d2), axis=1)
    d2s = np.take_along_axis(d2, order, 1)[:, :max_nn]
    idx = np.take_along_axis(cand, order, 1)[:, :max_nn]
    cnt = np.isfinite(d2s).sum(1)
    # every row inside the radius was a candidate, or the last one taken is strictly closer than the farthest
    # candidate (so no row tied with it was left out)
    far = np.sort(d2, axis=1)[:, -1]
    last = np.where(np.isfinite(d2s), d2s, -1.0).max(1)
    assert (~np.isfinite(far) | (last < far * (1.0 - 1e-9)) | (kk == len(pk))).all()
    idx = np.where(np.isfinite(d2s), idx, -1)
    s = np.zeros((len(q), 9))
    for j in range(max_nn):
        m = idx[:, j] >= 0
        x, y, z = (pk[idx[m, j], c] for c in range(3))
        s[m] += np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], 1)
    s /= np.maximum(cnt, 1)[:, None]
    cov = np.empty((len(q), 3, 3))
    cov[:, 0, 0] = s[:, 3] - s[:, 0] * s[:, 0]
    cov[:, 0, 1] = cov[:, 1, 0] = s[:, 4] - s[:, 0] * s[:, 1]
    cov[:, 0, 2] = cov[:, 2, 0] = s[:, 5] - s[:, 0] * s[:, 2]
    cov[:, 1, 1] = s[:, 6] - s[:, 1] * s[:, 1]
    cov[:, 1, 2] = cov[:, 2, 1] = s[:, 7] - s[:, 1] * s[:, 2]
    cov[:, 2, 2] = s[:, 8] - s[:, 2] * s[:, 2]
    return cnt, idx, cov


def check_normals(normals, nn, pk, radius, max_nn, rows):
    cnt, _, cov = restate_neighbours(pk, radius, max_nn, rows)
    assert np.array_equal(nn[rows].astype(np.int64), cnt)
    got = normals[rows]
    assert np.isfinite(got).all()
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-12)
    few = cnt < 3
    assert (got[few] == [0.0, 0.0, 1.0]).all()
    if few.all():                                       # max_nn < 3
        return
    # every row, ill-separated eigenvalues included: the normal's Rayleigh quotient is the smallest eigenvalue
    excess, lam = nr.rayleigh_excess(got[~few], cov[~few])
    assert (excess[lam[:, 2] > 0] <= nr.RAYLEIGH_BOUND).all(), np.nanmax(excess)
    w, v = np.linalg.eigh(cov[~few])
    ok = (w[:, 1] - w[:, 0]) >= 1e-3 * np.abs(w[:, 2])
    ok &= w[:, 2] > 0
    ref = v[:, :, 0]
    dev = 1.0 - np.abs(np.einsum("ij,ij->i", got[~few][ok], ref[ok]))
    assert ok.sum() > 0.5 * len(ok)
    assert dev.max() <= 1e-9, dev.max()


# ---- fixtures -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


@pytest.fixture(scope="module")
def room():
    from lidarcast import synth
    mesh = synth.make_room(size=(5.0, 4.0, 3.0), num_boxes=6, seed=11)
    return synth.sample_s3dis_room(mesh, num_points=200_000, num_outliers=300, seed=5)


# ---- tests ----------------------------------------------------------------------------------------------------------
def test_room_matches_the_restatement(ctx, room):
    from lidarcast import preprocess_cloud
    pts = room[0]
    r = preprocess_cloud(ctx, pts, nb_neighbors=20, std_ratio=2.0, radius=0.1, max_nn=30)
    avg = restate_avg(pts, 20)
    assert np.array_equal(r.avg.view(np.uint64), avg.view(np.uint64))
    mean, thr = restate_filter(avg, 2.0)
    assert abs(r.mean - mean) <= 1e-12 * mean and abs(r.threshold - thr) <= 1e-12 * thr
    kept = np.flatnonzero((avg > 0) & (avg < thr))
    assert np.array_equal(r.kept.astype(np.int64), kept)
    assert len(pts) - len(kept) >= 250                       # the outliers (and coincident rows) go
    pk = pts[kept]
    check_normals(r.normals, r.nn_count, pk, 0.1, 30, np.arange(len(pk)))


def test_bytes_identical_over_runs_and_cell_sizes(ctx, room):
    from lidarcast import preprocess_cloud
    pts = room[0][:60_000]
    runs = [preprocess_cloud(ctx, pts, cell_size=c) for c in (0.0, 0.0, 0.005, 0.5)]
    for r in runs[1:]:
        for name in ("kept", "normals", "avg", "nn_count"):
            assert getattr(r, name).tobytes() == getattr(runs[0], name).tobytes(), name
        assert (r.mean, r.threshold) == (runs[0].mean, runs[0].threshold)


def test_host_entry_equals_device_entry(ctx, room):
    import torch
    from lidarcast import preprocess_cloud, preprocess_cloud_dev
    pts = room[0][:80_000]
    h = preprocess_cloud(ctx, pts, nb_neighbors=16, std_ratio=1.5, radius=0.08, max_nn=24)
    d = preprocess_cloud_dev(ctx, torch.from_numpy(np.ascontiguousarray(pts)).cuda(), nb_neighbors=16, std_ratio=1.5,
                             radius=0.08, max_nn=24)
    assert np.array_equal(d.kept.cpu().numpy().view(np.uint32), h.kept)
    for name in ("normals", "avg", "nn_count"):
        assert getattr(d, name).cpu().numpy().tobytes() == getattr(h, name).tobytes(), name
    assert (d.mean, d.threshold) == (h.mean, h.threshold)


def test_normals_only_and_filter_only(ctx, room):
    from lidarcast import estimate_normals, preprocess_cloud, remove_statistical_outlier
    pts = room[0][:40_000]
    full = preprocess_cloud(ctx, pts)
    ind = remove_statistical_outlier(ctx, pts, 20, 2.0)
    assert np.array_equal(ind, full.kept.astype(np.int64))
    n = estimate_normals(ctx, pts[ind], 0.1, 30)
    assert n.tobytes() == full.normals.tobytes()
    r = preprocess_cloud(ctx, pts, remove_outliers=False)
    assert np.array_equal(r.kept, np.arange(len(pts), dtype=np.uint32)) and (r.avg == -1.0).all()
    assert (r.mean, r.threshold) == (0.0, float("inf"))


def test_sparse_variant_and_list_lengths(ctx, room):
    from lidarcast import preprocess_cloud
    rng = np.random.default_rng(2)
    pts = room[0][rng.choice(len(room[0]), len(room[0]) // 20, replace=False)]     # 5 %: many rows with < 3 neighbours
    for k, max_nn in ((1, 1), (2, 1), (32, 32), (5, 3), (20, 30)):
        r = preprocess_cloud(ctx, pts, nb_neighbors=k, radius=0.1, max_nn=max_nn)
        avg = restate_avg(pts, k)
        assert np.array_equal(r.avg, avg), k
        mean, thr = restate_filter(avg, 2.0)
        assert np.array_equal(r.kept.astype(np.int64), np.flatnonzero((avg > 0) & (avg < thr))), k
        pk = pts[r.kept]
        if k == 1:                                          # every avg is 0 (the row itself): nothing is kept
            assert len(pk) == 0 and r.normals.shape == (0, 3)
            continue
        check_normals(r.normals, r.nn_count, pk, 0.1, max_nn, np.arange(len(pk)))
        if max_nn >= 3:
            assert (r.nn_count < 3).any() and (r.nn_count >= 3).any()


def test_small_and_degenerate_clouds(ctx):
    from lidarcast import preprocess_cloud
    one = preprocess_cloud(ctx, np.array([[1.0, 2.0, 3.0]]))
    assert len(one.kept) == 0 and one.avg.tolist() == [0.0] and one.normals.shape == (0, 3)
    rng = np.random.default_rng(8)
    few = np.round(rng.uniform(0, 0.05, (7, 3)), 3)                       # n < k: min(k, n) distances
    r = preprocess_cloud(ctx, few, nb_neighbors=20)
    assert np.array_equal(r.avg, restate_avg(few, 20))
    blob = np.vstack([np.tile([[0.5, 0.5, 0.5]], (20, 1)), np.round(rng.uniform(0, 1, (400, 3)), 3)])
    r = preprocess_cloud(ctx, blob, nb_neighbors=20)
    assert (r.avg[:20] == 0.0).all() and not np.isin(np.arange(20), r.kept).any()   # k coincident rows all go
    flat = np.column_stack([rng.uniform(0, 1, 300), rng.uniform(0, 1, 300), np.zeros(300)])
    r = preprocess_cloud(ctx, flat, remove_outliers=False, radius=0.2)
    assert np.allclose(np.abs(r.normals[:, 2]), 1.0)
    same = np.tile([[1.0, 1.0, 1.0]], (10, 1))                              # zero covariance -> (0, 0, 1)
    r = preprocess_cloud(ctx, same, remove_outliers=False)
    assert (r.normals == [0.0, 0.0, 1.0]).all() and (r.nn_count == 10).all()
    empty = preprocess_cloud(ctx, np.zeros((0, 3)))
    assert len(empty.kept) == 0


def test_invalid_arguments_are_rejected(ctx):
    from lidarcast import preprocess_cloud
    pts = np.random.default_rng(1).uniform(0, 1, (100, 3))
    for kw in (dict(nb_neighbors=0), dict(nb_neighbors=33), dict(max_nn=0), dict(max_nn=33), dict(radius=0.0),
               dict(radius=-1.0), dict(radius=float("inf")), dict(std_ratio=0.0), dict(std_ratio=float("nan"))):
        with pytest.raises(ValueError):
            preprocess_cloud(ctx, pts, **kw)
    for bad in (np.nan, np.inf, -np.inf):
        p = pts.copy()
        p[37, 1] = bad
        with pytest.raises(ValueError):
            preprocess_cloud(ctx, p)
        with pytest.raises(ValueError):
            preprocess_cloud(ctx, p, remove_outliers=False)
    r = preprocess_cloud(ctx, pts)                                          # the context still works afterwards
    assert len(r.kept) > 0


def test_four_million_rows(ctx):
    from lidarcast import preprocess_cloud, synth
    mesh = synth.make_room(size=(8.0, 6.0, 3.0), num_boxes=10, seed=3)
    pts, _, _ = synth.sample_s3dis_room(mesh, num_points=4_000_000, num_outliers=500, seed=1)
    r = preprocess_cloud(ctx, pts)
    rows = np.sort(np.random.default_rng(0).choice(len(pts), 2000, replace=False))
    assert np.array_equal(r.avg[rows], restate_avg(pts, 20, rows))
    assert np.array_equal(np.flatnonzero((r.avg > 0) & (r.avg < r.threshold)), r.kept.astype(np.int64))
    pk = pts[r.kept]
    krows = np.sort(np.random.default_rng(1).choice(len(pk), 2000, replace=False))
    check_normals(r.normals, r.nn_count, pk, 0.1, 30, krows)


def test_main_end_to_end(ctx, tmp_path):
    import yaml
    from lidarcast import estimate_normals, synth
    from lidarcast.ply import read_point_cloud_attributes
    import s3dis_data_loader as sdl
    mesh = synth.make_room(size=(4.0, 3.0, 2.5), num_boxes=3, seed=2)
    p, c, l = synth.sample_s3dis_room(mesh, num_points=60_000, num_outliers=100, seed=3)
    synth.write_s3dis_room(tmp_path / "data", "Area_6", "office_2", p, c)               # S3DIS rooms: 6 columns
    synth.write_s3dis_room(tmp_path / "data", "Area_6", "office_3", p[:20_000], c[:20_000], l[:20_000])
    cfg = {"data": {"data_root": str(tmp_path / "data"), "output_root": str(tmp_path / "out"), "area_name": "Area_6",
                    "room_name": None},
           "preprocessing": {"estimate_normals": True, "use_shs_net": False, "normal_search_radius": 0.1,
                             "normal_max_nn": 30, "remove_outliers": True, "outlier_nb_neighbors": 20,
                             "outlier_std_ratio": 2.0},
           "sparsity_experiments": [{"name": "dense", "keep_ratio": 1.0, "occlusion": False},
                                    {"name": "sparse_50", "keep_ratio": 0.5, "occlusion": False},
                                    {"name": "occluded", "keep_ratio": 0.8, "occlusion": True}]}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    np.random.seed(42)
    done = sdl.main(["--config", str(tmp_path / "cfg.yaml"), "--save_pointclouds", "--save_normal_visualizations"])
    assert list(done) == ["office_2"]            # office_3 fails as in the reference: its labels are the removed rows'
    np.random.seed(42)
    again = sdl.main(["--config", str(tmp_path / "cfg.yaml"), "--kept_labels"])
    assert list(again) == ["office_2", "office_3"]
    v3 = again["office_3"]["sparsity_variants"]["sparse_50"]
    assert len(v3["labels"]) == len(v3["points"])
    assert again["office_2"]["processed_data"]["normals"].tobytes() == done["office_2"]["processed_data"]["normals"].tobytes()
    out = tmp_path / "out" / "preprocessed_data"
    with open(out / "Area_6_office_2_preprocessed.pkl", "rb") as f:
        d = pickle.load(f)
    assert list(d) == ["room_info", "original_data", "processed_data", "sparsity_variants"]
    assert d["original_data"]["points"].shape == (60_100, 3) and d["original_data"]["point_count"] == 60_100
    pd_ = d["processed_data"]
    m = pd_["point_count"]
    assert pd_["points"].shape == (m, 3) and pd_["colors"].shape == (m, 3) and pd_["normals"].shape == (m, 3)
    assert pd_["labels"] is None
    assert list(d["sparsity_variants"]) == ["dense", "sparse_50", "occluded"]
    assert d["sparsity_variants"]["dense"]["normals"] is pd_["normals"]
    for name in ("sparse_50", "occluded"):
        v = d["sparsity_variants"][name]
        assert v["config"] == cfg["sparsity_experiments"][[s["name"] for s in cfg["sparsity_experiments"]].index(name)]
        assert v["normals"].tobytes() == estimate_normals(ctx, v["points"], 0.1, 30).tobytes()
    for name in ("original", "processed", "dense", "sparse_50", "occluded"):
        got = read_point_cloud_attributes(out / "pointclouds" / f"Area_6_office_2_{name}.ply")
        src = d["original_data"] if name == "original" else (pd_ if name == "processed" else d["sparsity_variants"][name])
        assert np.array_equal(got["points"], src["points"])
        if name != "original":
            assert np.array_equal(got["normals"], src["normals"])
    assert (out / "pointclouds" / "Area_6_office_2_summary.txt").exists()
