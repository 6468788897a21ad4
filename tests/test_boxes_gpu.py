"""GPU: detection boxes (lidarcast.instance_boxes / instance_boxes_dev, csrc/lrc_boxes.hip) against a numpy / scipy
restatement of Open3D's statistical outlier filter kept in this file, and end to end on the C3 scan of
synth_A6_office2 against the host path (labelled PLY -> LiDARNetBBoxVisualizer.process_room_instances)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- restatement ----------------------------------------------------------------------------------------------------
def restate_avg(p32, k, chunk=1 << 17):
    """avg of every row: cKDTree for candidates, then the fixed float64 expression (dx*dx + dy*dy) + dz*dz, the k
    smallest ascending, square roots summed one after the other (np.cumsum; np.sum would be pairwise), / k."""
    from scipy.spatial import cKDTree
    p = p32.astype(np.float64)
    n = len(p)
    kk = min(n, k + 4)                       # a few spare candidates: cKDTree's own metric may order near-ties otherwise
    tree = cKDTree(p)
    out = np.empty(n)
    for a in range(0, n, chunk):
        q = p[a:a + chunk]
        _, cand = tree.query(q, kk, workers=-1)
        cand = cand.reshape(len(q), kk)
        d = q[:, None, :] - p[cand]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d2 = np.sort(d2, axis=1)[:, :k]
        out[a:a + chunk] = np.cumsum(np.sqrt(d2), axis=1)[:, -1] / k
    return out


def restate(points, sem, ins, class_ids, min_points=10, k=20, std_ratio=2.0):
    """(boxes as dicts, avg per row, keep per row), the contract of include/lidarcast.h 'detection boxes'."""
    K = len(points)
    avg_all, keep_all = np.full(K, -1.0), np.zeros(K, np.uint8)
    boxes = []
    for sid in class_ids:
        in_class = (sem == sid) & (ins != 0)
        for iid in np.unique(ins[in_class]):
            rows = np.flatnonzero(in_class & (ins == iid))
            n = len(rows)
            if n < min_points:
                continue
            b = {"sem": int(sid), "ins": int(iid), "num_points": n, "filtered": int(n >= k)}
            if n < k:
                keep = np.ones(n, bool)
                b["mean"], b["threshold"] = 0.0, np.inf
            else:
                avg = restate_avg(points[rows], k)
                pos = avg[avg > 0]
                mean = pos.sum() / n
                std = np.sqrt(((pos - mean) ** 2).sum() / (n - 1))
                thr = mean + std_ratio * std
                keep = (avg > 0) & (avg < thr)
                avg_all[rows] = avg
                b["mean"], b["threshold"] = mean, thr
            keep_all[rows] = keep
            b["num_kept"] = int(keep.sum())
            kp = points[rows][keep]
            b["min3"] = kp.min(0) if len(kp) else np.full(3, np.inf, np.float32)
            b["max3"] = kp.max(0) if len(kp) else np.full(3, -np.inf, np.float32)
            boxes.append(b)
    return boxes, avg_all, keep_all


def assert_matches(got, avg, keep, want, want_avg, want_keep):
    assert np.array_equal(avg.view(np.uint64), want_avg.view(np.uint64)), "avg differs from the restatement"
    assert np.array_equal(keep, want_keep), "keep masks differ"
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for key in ("sem", "ins", "num_points", "num_kept", "filtered"):
            assert int(g[key]) == w[key], (key, g, w)
        assert np.array_equal(g["min3"].view(np.uint32), np.asarray(w["min3"], np.float32).view(np.uint32))
        assert np.array_equal(g["max3"].view(np.uint32), np.asarray(w["max3"], np.float32).view(np.uint32))
        for key in ("mean", "threshold"):
            if np.isinf(w[key]):
                assert np.isinf(g[key])
            else:
                assert abs(g[key] - w[key]) <= 1e-12 * abs(w[key]), (key, g[key], w[key])


# ---- inputs ---------------------------------------------------------------------------------------------------------
def surface(rng, n, lo, size, jitter=0.002, outliers=0):
    """n points on the faces of a box (scan points lie on surfaces), plus a few far-off outliers."""
    p = rng.uniform(0, 1, (n, 3)) * size
    face = rng.integers(0, 6, n)
    for a in range(3):
        p[face == 2 * a, a] = 0.0
        p[face == 2 * a + 1, a] = size[a]
    p = p + lo + rng.normal(0, jitter, p.shape)
    if outliers:
        idx = rng.choice(n, outliers, replace=False)
        p[idx] += rng.normal(0, 0.5, (outliers, 3))
    return p.astype(np.float32)


def make_cloud(seed=0):
    rng = np.random.default_rng(seed)
    parts = []
    # (sem, ins, rows, size, outliers)
    spec = [(7, 3, 4000, (1.2, 0.7, 0.75), 12), (7, 9, 2500, (0.9, 0.6, 0.7), 5), (8, 1, 1500, (0.45, 0.45, 0.9), 8),
            (8, 2, 15, (0.4, 0.4, 0.5), 0),              # 10 <= n < k: kept whole
            (8, 4, 9, (0.4, 0.4, 0.5), 0),               # n < min_points: dropped
            (10, 65535, 3000, (1.0, 0.35, 1.8), 10),     # the largest instance id
            (10, 0, 500, (1.0, 1.0, 1.0), 0),            # ins 0: ignored
            (2, 5, 2000, (3.0, 0.1, 2.5), 0),            # a class outside the list: ignored
            (11, 7, 1200, (1.5, 1.0, 0.0), 4)]           # a board: zero extent in z, then outliers in z
    for sid, iid, n, size, out in spec:
        lo = rng.uniform(0, 4, 3)
        p = surface(rng, n, lo, np.array(size), outliers=out)
        if size[2] == 0.0:
            p[:, 2] = np.float32(lo[2])
            p[:out, 2] += np.float32(0.3)
        parts.append((p, np.full(n, sid, np.uint16), np.full(n, iid, np.uint16)))
    # k or more coincident points inside an instance: avg 0, removed
    pc = surface(rng, 300, np.array([1.0, 1.0, 0.0]), np.array([0.5, 0.5, 0.5]))
    pc[:25] = pc[0]
    parts.append((pc, np.full(300, 9, np.uint16), np.full(300, 12, np.uint16)))
    pts = np.concatenate([a for a, _, _ in parts])
    sem = np.concatenate([b for _, b, _ in parts])
    ins = np.concatenate([c for _, _, c in parts])
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), sem[perm], ins[perm]


CLASSES = [5, 7, 8, 9, 10, 11]


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


# ---- tests ----------------------------------------------------------------------------------------------------------
def test_boxes_match_the_restatement(ctx):
    import lidarcast
    pts, sem, ins = make_cloud(1)
    boxes, avg, keep = lidarcast.instance_boxes(ctx, pts, sem, ins, CLASSES, return_rows=True)
    want, wavg, wkeep = restate(pts, sem, ins, CLASSES)
    assert_matches(boxes, avg, keep, want, wavg, wkeep)
    got = {(int(b["sem"]), int(b["ins"])): b for b in boxes}
    assert (10, 65535) in got and (8, 2) in got and (8, 4) not in got and (2, 5) not in got
    assert all(b["ins"] != 0 for b in boxes)
    assert got[(8, 2)]["filtered"] == 0 and got[(8, 2)]["num_kept"] == 15 == got[(8, 2)]["num_points"]
    assert got[(11, 7)]["max3"][2] == got[(11, 7)]["min3"][2]          # the board's outliers in z are gone
    # coincident rows: all 25 removed
    rows = np.flatnonzero((sem == 9) & (ins == 12))
    vals, cnt = np.unique(pts[rows], axis=0, return_counts=True)
    dup = rows[(pts[rows] == vals[np.argmax(cnt)]).all(1)]
    assert len(dup) == 25 and not keep[dup].any() and (avg[dup] == 0).all()
    # ordering: (class list position, ins)
    order = [(CLASSES.index(int(b["sem"])), int(b["ins"])) for b in boxes]
    assert order == sorted(order)


def test_device_rows_equal_host_arrays(ctx):
    import torch
    import lidarcast
    pts, sem, ins = make_cloud(2)
    rows = np.empty((len(pts), 4), np.float32)
    rows[:, :3] = pts
    rows[:, 3] = (sem.astype(np.uint32) | (ins.astype(np.uint32) << 16)).view(np.float32)
    rows_t = torch.from_numpy(rows).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    b_dev, avg_t, keep_t = lidarcast.instance_boxes_dev(ctx, rows_t, CLASSES, return_rows=True, stream=stream)
    b_host, avg, keep = lidarcast.instance_boxes(ctx, pts, sem, ins, CLASSES, return_rows=True)
    assert b_dev.tobytes() == b_host.tobytes()
    assert avg_t.cpu().numpy().tobytes() == avg.tobytes() and keep_t.cpu().numpy().tobytes() == keep.tobytes()


def test_cell_size_and_repeat_do_not_change_bytes(ctx):
    import lidarcast
    pts, sem, ins = make_cloud(3)
    ref = None
    for cs in (0.0, 0.005, 0.5, 50.0, 0.0):
        out = lidarcast.instance_boxes(ctx, pts, sem, ins, CLASSES, cell_size=cs, return_rows=True)
        blob = b"".join(a.tobytes() for a in out)
        ref = ref or blob
        assert blob == ref, cs


@pytest.mark.parametrize("k", [1, 32])
def test_k_limits(ctx, k):
    import lidarcast
    pts, sem, ins = make_cloud(4)
    boxes, avg, keep = lidarcast.instance_boxes(ctx, pts, sem, ins, CLASSES, k=k, return_rows=True)
    want, wavg, wkeep = restate(pts, sem, ins, CLASSES, k=k)
    assert_matches(boxes, avg, keep, want, wavg, wkeep)
    if k == 1:                                   # the only neighbour is the row itself: avg 0, everything removed
        assert (boxes["num_kept"][boxes["filtered"] == 1] == 0).all()


def test_invalid_and_empty(ctx):
    import lidarcast
    pts, sem, ins = make_cloud(5)
    with pytest.raises(ValueError):
        lidarcast.instance_boxes(ctx, pts, sem, ins, CLASSES, k=33)
    with pytest.raises(ValueError):
        lidarcast.instance_boxes(ctx, pts, sem, ins, [7, 7])
    boxes, avg, keep = lidarcast.instance_boxes(ctx, np.zeros((0, 3), np.float32), np.zeros(0, np.uint16),
                                                np.zeros(0, np.uint16), CLASSES, return_rows=True)
    assert len(boxes) == 0 and len(avg) == 0 and len(keep) == 0
    boxes, avg, keep = lidarcast.instance_boxes(ctx, pts, sem, ins, [3], return_rows=True)       # no row in a class
    assert len(boxes) == 0 and (avg == -1).all() and not keep.any()


def test_remove_outliers_single_instance(ctx):
    from lidar_net_bbox_visualizer import LiDARNetBBoxVisualizer
    rng = np.random.default_rng(6)
    p = surface(rng, 800, np.zeros(3), np.array([0.6, 0.5, 0.8]), outliers=6).astype(np.float64)
    c = rng.uniform(0, 1, (800, 3))
    vis = LiDARNetBBoxVisualizer(ctx=ctx)
    fp, fc = vis.remove_outliers(p, c)
    _, _, wkeep = restate(p.astype(np.float32), np.zeros(800, np.uint16), np.ones(800, np.uint16), [0], min_points=1)
    assert np.array_equal(fp, p[wkeep.astype(bool)]) and np.array_equal(fc, c[wkeep.astype(bool)])
    small, col = vis.remove_outliers(p[:19], c[:19])
    assert small is not None and len(small) == 19


def test_one_instance_of_two_million_rows(ctx):
    import lidarcast
    rng = np.random.default_rng(7)
    n = 2_100_000
    pts = surface(rng, n, np.array([0.5, 0.5, 0.0]), np.array([6.0, 5.0, 3.0]), jitter=0.001, outliers=50)
    sem, ins = np.full(n, 7, np.uint16), np.full(n, 1, np.uint16)
    boxes, avg, keep = lidarcast.instance_boxes(ctx, pts, sem, ins, CLASSES, return_rows=True)
    want, wavg, wkeep = restate(pts, sem, ins, CLASSES)
    assert_matches(boxes, avg, keep, want, wavg, wkeep)


# ---- end to end -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3_rows(ctx):
    """The scan pipeline's rows of synth_A6_office2 under the C3 sensor (32 lines x 2048) over 64 poses."""
    import dataclasses
    import torch
    import lidarcast
    from lidar import IndoorLidar, Indoor8LineLidarIntrinsics
    from lidarcast import synth
    from trajectory import line_trajectory, poses_from_waypoints
    mesh = synth.make_scene("synth_A6_office2")
    sensor = dataclasses.replace(Indoor8LineLidarIntrinsics.create_dense_32line(), horizontal_res=2048)
    poses = poses_from_waypoints(line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 64))
    dirs = IndoorLidar(intrinsics=sensor, pose=np.eye(4)).sensor_directions()
    P, N = poses.shape[0], dirs.shape[0]
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    pipe = lidarcast.ScanPipe(scene, P, N)
    rows = torch.empty((P * N, 4), dtype=torch.float32, device="cuda")
    counts = torch.zeros(P, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    pipe.submit(torch.from_numpy(poses.reshape(P, 16)).cuda(), torch.from_numpy(dirs).cuda(), sensor.max_range,
                out_rows_t=rows, counts_t=counts, stream=stream)
    pipe.wait(stream)
    torch.cuda.synchronize()
    K = int(counts.sum())
    out = rows[:K].clone()
    pipe.close()
    scene.close()
    return mesh, out


def test_c3_device_boxes_equal_host_path(ctx, c3_rows, tmp_path, monkeypatch):
    import torch
    import lidarcast
    from containers import write_labeled_ply
    from lidar_net_bbox_visualizer import S3DIS_SEMANTIC_MAPPING, LiDARNetBBoxVisualizer
    mesh, rows_t = c3_rows
    vis = LiDARNetBBoxVisualizer(S3DIS_SEMANTIC_MAPPING, ctx=ctx)
    stream = torch.cuda.current_stream().cuda_stream
    boxes = lidarcast.instance_boxes_dev(ctx, rows_t, list(S3DIS_SEMANTIC_MAPPING.values()), stream=stream)
    assert len(boxes) >= 5
    dev_bboxes = vis.bboxes_from_boxes(boxes)
    vis.generate_detection_annotations(dev_bboxes, tmp_path / "dev.json")

    rows = rows_t.cpu().numpy()
    lab = rows[:, 3].copy().view(np.uint32)
    sem, ins = (lab & 0xFFFF).astype(np.uint16), (lab >> 16).astype(np.uint16)
    ply = tmp_path / "combined_pointcloud_with_label.ply"
    write_labeled_ply(ply, rows[:, :3], np.full((len(rows), 3), 127, np.uint8), sem, ins)
    monkeypatch.chdir(tmp_path)
    host_bboxes = vis.process_room_instances(ply)
    out = tmp_path / "simulation_results" / "combined_pointcloud_with_label"
    assert (out / "combined_pointcloud_with_label.ply").read_bytes() == ply.read_bytes()
    host_json = (out / "combined_pointcloud_with_label_detection_annotations.json").read_bytes()
    assert host_json == (tmp_path / "dev.json").read_bytes()
    assert len(host_bboxes) == len(dev_bboxes) > 0

    # every box inside its object's true AABB (the instance's mesh vertices)
    for b in boxes:
        tri = mesh.triangles[(mesh.triangle_sem == b["sem"]) & (mesh.triangle_ins == b["ins"])]
        v = mesh.vertices[np.unique(tri)]
        if b["num_kept"]:
            assert (b["min3"] >= v.min(0) - 1e-5).all() and (b["max3"] <= v.max(0) + 1e-5).all(), b

    # and equal to the restatement's
    classes = list(S3DIS_SEMANTIC_MAPPING.values())
    got, avg, keep = lidarcast.instance_boxes(ctx, rows[:, :3], sem, ins, classes, return_rows=True)
    assert got.tobytes() == boxes.tobytes()
    want, wavg, wkeep = restate(np.ascontiguousarray(rows[:, :3]), sem, ins, classes)
    assert_matches(got, avg, keep, want, wavg, wkeep)


def test_scene_export_detection_annotations(ctx, tmp_path):
    """S3DISSimScene.export_detection_annotations writes what process_room_instances writes for the saved PLY."""
    import s3dis_simulator
    from lidarcast import synth
    from trajectory import line_trajectory
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=5, seed=5, cell=0.05)
    sim = s3dis_simulator.S3DISSimulator({"raycast_engine": {"use_gpu": True}}, use_dense_lidar=True)
    sim.load_scene(mesh, "room")
    scene = sim.run_simulation(line_trajectory((1.0, 1.5, 1.0), (3.0, 1.5, 1.0), 6))
    scene.save_results(tmp_path / "res", formats=["json"])
    bboxes = scene.export_detection_annotations(tmp_path / "res")
    assert bboxes
    import os
    from lidar_net_bbox_visualizer import S3DIS_SEMANTIC_MAPPING, LiDARNetBBoxVisualizer
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        LiDARNetBBoxVisualizer(S3DIS_SEMANTIC_MAPPING, ctx=ctx).process_room_instances(
            tmp_path / "res" / "combined_pointcloud_with_label.ply")
    finally:
        os.chdir(cwd)
    name = "combined_pointcloud_with_label_detection_annotations.json"
    assert (tmp_path / "res" / name).read_bytes() == \
        (tmp_path / "simulation_results" / "combined_pointcloud_with_label" / name).read_bytes()
