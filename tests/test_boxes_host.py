"""CPU: the detection-box mirror's host methods against the reference's (tests/golden/bbox_golden.json), the lrc_box
layout, and scratch-free kernels in csrc/lrc_boxes.hip."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(REPO, "tests", "golden", "bbox_golden.json")) as f:
        return json.load(f)


@pytest.fixture()
def vis():
    from lidar_net_bbox_visualizer import LiDARNetBBoxVisualizer
    return LiDARNetBBoxVisualizer()


def test_calculate_bbox_and_quality_match_the_reference(gold, vis):
    for name, pts in gold["clouds"].items():
        b = vis.calculate_bbox(np.array(pts, dtype=np.float64))
        want = gold["bbox"][name]
        assert set(b) == set(want)
        for key in ("center", "size", "min_coords", "max_coords"):
            assert b[key] == want[key], (name, key)                          # exact float64 values
        assert b["volume"] == want["volume"] and b["point_count"] == want["point_count"]
        assert b["aspect_ratio"] == want["aspect_ratio"], name                # inf for a zero extent
        assert list(vis.evaluate_bbox_quality(b, "chair")) == gold["quality"][name], name
    assert vis.calculate_bbox(np.zeros((0, 3))) is None


def test_zero_extent_gives_infinite_aspect_ratio(gold, vis):
    assert gold["bbox"]["planar_z"]["aspect_ratio"] == float("inf")
    assert vis.calculate_bbox(np.array(gold["clouds"]["planar_z"]))["aspect_ratio"] == float("inf")


def test_extract_instances_order_and_filtering(gold, vis):
    room = {k: np.array(v) for k, v in gold["room"].items()}
    room["semantic_labels"] = room["semantic_labels"].astype(np.uint16)
    room["instance_labels"] = room["instance_labels"].astype(np.uint16)
    for sid, want in gold["instances"].items():
        got = vis.extract_instances_by_semantic(room, int(sid))
        assert [int(d["instance_id"]) for d in got] == [w["instance_id"] for w in want], sid
        for d, w in zip(got, want):
            assert int(d["semantic_id"]) == w["semantic_id"]
            assert d["points"].tolist() == w["points"] and d["colors"].tolist() == w["colors"]


def test_annotation_file_bytes(gold, vis, tmp_path):
    bboxes = []
    for name, cname in zip(gold["annotation_names"], gold["annotation_classes"]):
        b = vis.calculate_bbox(np.array(gold["clouds"][name], dtype=np.float64))
        b.update(object_name=cname, instance_id=np.uint16(3), semantic_id=19)
        bboxes.append(b)
    vis.generate_detection_annotations(bboxes, tmp_path / "a.json")
    assert (tmp_path / "a.json").read_bytes() == gold["annotation_bytes"].encode("utf-8")
    vis.generate_detection_annotations([], tmp_path / "e.json")
    assert (tmp_path / "e.json").read_bytes() == gold["annotation_bytes_empty"].encode("utf-8")


def test_semantic_mappings():
    from lidar_net_bbox_visualizer import S3DIS_SEMANTIC_MAPPING, LiDARNetBBoxVisualizer
    assert S3DIS_SEMANTIC_MAPPING == {"window": 5, "table": 7, "chair": 8, "sofa": 9, "bookcase": 10, "board": 11}
    assert list(LiDARNetBBoxVisualizer().semantic_mapping.items()) == [
        ("window", 15), ("table", 18), ("chair", 19), ("sofa", 20), ("bookcase", 23), ("board", 21), ("stairs", 10)]
    assert LiDARNetBBoxVisualizer(S3DIS_SEMANTIC_MAPPING).semantic_mapping == S3DIS_SEMANTIC_MAPPING


def test_lrc_box_layout_matches_header():
    import ctypes as C
    from lidarcast import BOX_DTYPE
    from lidarcast._capi import LrcBox
    src = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    body = re.search(r"typedef struct lrc_box \{(.*?)\} lrc_box;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", d).group(1) for d in decls]
    assert [n for n, _ in LrcBox._fields_] == names
    assert list(BOX_DTYPE.names) == names
    assert C.sizeof(LrcBox) == BOX_DTYPE.itemsize == 56
    for n in names:
        assert getattr(LrcBox, n).offset == BOX_DTYPE.fields[n][1], n
    assert "56 bytes" in src[src.index("} lrc_box;"):src.index("} lrc_box;") + 40]


def test_box_entry_points_are_declared():
    from lidarcast import _capi
    assert {"lrc_instance_boxes", "lrc_instance_boxes_dev"} <= set(_capi.SYMBOLS)


def test_boxes_kernels_use_no_scratch(tmp_path):
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(PKG, "csrc", "lrc_boxes.hip"), "-o", str(tmp_path / "b.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) and len(names) >= 13
    ours = [(n, s) for n, s in zip(names, scratch) if "box_" in n]
    assert len(ours) == 12                 # key, grid, count, stats, eight k-NN list lengths
    assert all(s == 0 for _, s in ours), [n for n, s in ours if s]
    # every rocprim kernel too, except its onesweep radix-sort pass, which spills in this toolchain whoever calls it
    # (lrc_bvh_device.hip's sort compiles to the same 80 bytes per lane)
    spilling = [n for n, s in zip(names, scratch) if s]
    assert all("rocprim" in n and "radix_sort_onesweep" in n for n in spilling), spilling
