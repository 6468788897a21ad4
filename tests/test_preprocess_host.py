"""CPU: the preprocessing mirror's host methods against the reference's (tests/golden/preprocess_golden.json), the
lrc_preprocess_opts layout, the entry points, the PLY point-cloud writer, and the register budget of
csrc/lrc_preprocess.hip's kernels."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(REPO, "tests", "golden", "preprocess_golden.json")) as f:
        return json.load(f)


def _cfg():
    return {"preprocessing": {"remove_outliers": True, "outlier_nb_neighbors": 20, "outlier_std_ratio": 2.0,
                              "estimate_normals": False, "normal_search_radius": 0.1, "normal_max_nn": 30}}


def test_load_room_data_matches_the_reference(gold, tmp_path):
    from s3dis_data_loader import S3DISLoader
    rd = gold["room_data"]
    pts, rgb, lab = np.array(rd["pts"]), np.array(rd["rgb"]), np.array(rd["lab"])[:, None]
    for room, data in (("office_1", np.hstack([pts, rgb, lab])), ("office_2", np.hstack([pts, rgb]))):
        os.makedirs(tmp_path / "Area_1" / room)
        np.savetxt(tmp_path / "Area_1" / room / f"{room}.txt", data,
                   fmt="%.3f %.3f %.3f %d %d %d" + (" %d" if data.shape[1] == 7 else ""))
    os.makedirs(tmp_path / "Area_1" / "hallway_3")
    np.save(tmp_path / "Area_1" / "hallway_3" / "points.npy", np.hstack([pts[:10], rgb[:10], lab[:10]]))
    (tmp_path / "Area_1" / "notes.md").write_text("")
    loader = S3DISLoader(str(tmp_path))
    for room, want in gold["loaded"].items():
        p, c, l = loader.load_room_data("Area_1", room)
        assert p.tolist() == want["points"] and c.tolist() == want["colors"], room
        assert (l is None and want["labels"] is None) or l.tolist() == want["labels"], room
    assert loader.get_available_rooms("Area_1") == gold["rooms"]
    assert loader.get_available_rooms("Area_9") == gold["rooms_missing_area"] == []
    with pytest.raises(FileNotFoundError):
        loader.load_room_data("Area_1", "nowhere")
    os.makedirs(tmp_path / "Area_1" / "empty_room")
    with pytest.raises(FileNotFoundError):
        loader.load_room_data("Area_1", "empty_room")


def test_seeded_sparsity_matches_the_reference(gold):
    from s3dis_data_loader import S3DISPreprocessor
    pre = S3DISPreprocessor(_cfg())
    src = gold["sparsity_input"]
    pts, rgb, lab = np.array(src["points"]), np.array(src["colors"]), np.array(src["labels"])
    for name, want in gold["sparsity"].items():
        np.random.seed(1234)
        p, c, l = pre.simulate_robot_sparsity(pts, rgb, lab, want["config"])
        assert p.tolist() == want["points"] and c.tolist() == want["colors"] and l.tolist() == want["labels"], name
    assert pre.simulate_robot_sparsity(pts, rgb, lab, None)[0] is pts


def test_summary_file_bytes(gold, tmp_path):
    from s3dis_data_loader import save_pointcloud_variants
    src = gold["sparsity_input"]
    pts, rgb, lab = np.array(src["points"]), np.array(src["colors"]), np.array(src["labels"])
    q = gold["quirk"]
    p, c = np.array(q["points"]), rgb[q["inliers"]]
    room_data = {"room_info": {"area_name": "Area_1", "room_name": "office_1", "processing_time": 0.5},
                 "original_data": {"points": pts, "colors": rgb, "labels": lab, "point_count": len(pts)},
                 "processed_data": {"points": p, "colors": c, "labels": None, "normals": None, "point_count": len(p)},
                 "sparsity_variants": {k: {"points": np.array(v["points"]), "colors": np.array(v["colors"]),
                                           "labels": None, "normals": None, "point_count": len(v["points"]),
                                           "config": v["config"]} for k, v in gold["sparsity"].items()}}
    room_data["sparsity_variants"]["dense"] = {"points": p, "colors": c, "labels": None, "normals": None,
                                               "point_count": len(p), "config": {"name": "dense"}}
    save_pointcloud_variants(room_data, tmp_path, {})
    d = tmp_path / "pointclouds"
    assert (d / "Area_1_office_1_summary.txt").read_bytes() == gold["summary_bytes"].encode("utf-8")
    assert sorted(x.name for x in d.glob("*.ply")) == sorted(gold["written"])
    from lidarcast.ply import read_point_cloud, read_point_cloud_attributes
    assert np.array_equal(read_point_cloud(d / "Area_1_office_1_original.ply"), pts)
    got = read_point_cloud_attributes(d / "Area_1_office_1_sparse_50.ply")
    assert np.array_equal(got["points"], np.array(gold["sparsity"]["sparse_50"]["points"]))
    assert np.array_equal(got["colors"], np.clip(np.array(gold["sparsity"]["sparse_50"]["colors"]) * 255.0, 0, 255)
                          .astype(np.uint8))


def test_write_point_cloud_layout(tmp_path):
    from lidarcast.ply import read_point_cloud, read_point_cloud_attributes, write_point_cloud
    rng = np.random.default_rng(3)
    p, n, c = rng.normal(size=(7, 3)), rng.normal(size=(7, 3)), rng.uniform(-0.2, 1.2, (7, 3))
    write_point_cloud(tmp_path / "a.ply", p, colors=c, normals=n)
    raw = (tmp_path / "a.ply").read_bytes()
    head = raw[:raw.index(b"end_header\n") + 11].decode()
    assert head.split("\n")[3:12] == ["property double x", "property double y", "property double z",
                                      "property double nx", "property double ny", "property double nz",
                                      "property uchar red", "property uchar green", "property uchar blue"]
    assert len(raw) - len(head) == 7 * (6 * 8 + 3)
    got = read_point_cloud_attributes(tmp_path / "a.ply")
    assert np.array_equal(got["points"], p) and np.array_equal(got["normals"], n)
    assert np.array_equal(got["colors"], np.clip(c * 255.0, 0, 255).astype(np.uint8))
    assert np.array_equal(read_point_cloud(tmp_path / "a.ply"), p)
    write_point_cloud(tmp_path / "b.ply", p)
    assert set(read_point_cloud_attributes(tmp_path / "b.ply")) == {"points"}


def test_visualizations_are_out_of_scope():
    from s3dis_data_loader import S3DISPreprocessor
    pre = S3DISPreprocessor(_cfg())
    for name in ("visualize_normals", "visualize_normals_high_quality", "visualize_normal_statistics"):
        with pytest.raises(NotImplementedError, match="DESIGN.md section 9"):
            getattr(pre, name)(np.zeros((1, 3)), np.zeros((1, 3)))


def test_synthetic_room_is_rounded_and_seeded(tmp_path):
    from lidarcast import synth
    mesh = synth.make_room(size=(3.0, 2.5, 2.5), num_boxes=2, seed=4)
    p, c, l = synth.sample_s3dis_room(mesh, num_points=5000, num_outliers=50, seed=9)
    p2, _, _ = synth.sample_s3dis_room(mesh, num_points=5000, num_outliers=50, seed=9)
    assert p.shape == (5050, 3) and c.shape == (5050, 3) and l.shape == (5050,)
    assert np.array_equal(p, p2) and np.array_equal(p, np.round(p, 3))
    assert c.min() >= 0 and c.max() <= 255 and np.array_equal(c, np.round(c))
    path = synth.write_s3dis_room(tmp_path, "Area_1", "office_9", p, c, l)
    from s3dis_data_loader import S3DISLoader
    lp, lc, ll = S3DISLoader(str(tmp_path)).load_room_data("Area_1", "office_9")
    assert path.endswith("office_9.txt") and np.array_equal(lp, p) and np.array_equal(lc, c / 255.0)
    assert np.array_equal(ll, l)


def test_lrc_preprocess_opts_layout_matches_header():
    import ctypes as C
    from lidarcast._capi import LrcPreprocessOpts
    src = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    body = re.search(r"typedef struct lrc_preprocess_opts \{(.*?)\} lrc_preprocess_opts;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    ctypes_of = {"uint32_t": C.c_uint32, "double": C.c_double}
    assert [(t, n) for t, n in decls] == [(t, n) for n, t in
                                          ((f, {C.c_uint32: "uint32_t", C.c_double: "double"}[ct])
                                           for f, ct in LrcPreprocessOpts._fields_)]
    assert all(ctypes_of[t] is ct for (t, _), (_, ct) in zip(decls, LrcPreprocessOpts._fields_))
    assert C.sizeof(LrcPreprocessOpts) == 40
    assert "40 bytes" in src[src.index("} lrc_preprocess_opts;"):src.index("} lrc_preprocess_opts;") + 50]


def test_preprocess_entry_points_are_declared():
    from lidarcast import _capi
    src = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    for name in ("lrc_cloud_preprocess", "lrc_cloud_preprocess_dev"):
        assert name in _capi.SYMBOLS and re.search(r"\bint %s\(" % name, src), name
    import lidarcast
    for name in ("preprocess_cloud", "preprocess_cloud_dev", "remove_statistical_outlier", "estimate_normals"):
        assert callable(getattr(lidarcast, name)), name


def test_preprocess_kernels_use_no_scratch_and_fit_four_waves(tmp_path):
    import __graft_entry__ as entry
    assert "lrc_preprocess.hip" in entry.SOURCES
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(PKG, "csrc", "lrc_preprocess.hip"), "-o", str(tmp_path / "p.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
    vgprs = [int(x) for x in re.findall(r"remark:\s+VGPRs: (\d+)", r.stderr)]
    agprs = [int(x) for x in re.findall(r"remark:\s+AGPRs: (\d+)", r.stderr)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(vgprs) == len(agprs) == len(scratch)
    ours = [(n, v + a, s) for n, v, a, s in zip(names, vgprs, agprs, scratch) if "pp_" in n]
    # bounds, key, gather, sum, final, keep, compact, fill, eight k-NN, five neighbour-list and five PCA list lengths
    assert len(ours) == 26, [n for n, _, _ in ours]
    assert all(s == 0 for _, _, s in ours), [n for n, _, s in ours if s]
    assert all(v <= 128 for _, v, _ in ours), [(n, v) for n, v, _ in ours if v > 128]
    spilling = [n for n, s in zip(names, scratch) if s]
    assert all("rocprim" in n and "radix_sort_onesweep" in n for n in spilling), spilling


def test_preprocess_labels_quirk_matches_the_reference(gold, monkeypatch):
    # the device call stands in with the golden inlier list; the label handling around it is what is checked
    from lidarcast import preprocess
    from s3dis_data_loader import S3DISPreprocessor
    q = gold["quirk"]
    inliers = np.array(q["inliers"], np.uint32)
    monkeypatch.setattr(preprocess, "preprocess_cloud", lambda ctx, pts, **kw: preprocess.Preprocessed(kept=inliers))
    src = gold["sparsity_input"]
    pts, rgb, lab = np.array(src["points"]), np.array(src["colors"]), np.array(src["labels"])
    p, c, l, n = S3DISPreprocessor(_cfg(), ctx=object()).preprocess_pointcloud(pts, rgb, lab)
    assert p.tolist() == q["points"] and np.array_equal(c, rgb[inliers]) and n is None
    assert l.tolist() == q["labels"] and len(l) == len(pts) - len(inliers)        # the removed rows' labels
    _, _, l2, _ = S3DISPreprocessor(_cfg(), ctx=object(), kept_labels=True).preprocess_pointcloud(pts, rgb, lab)
    assert np.array_equal(l2, lab[inliers])
