"""CPU: the S3DIS annotation-box mirror (s3dis_bbox_visualizer.py) against the reference's values
(tests/golden/s3dis_bbox_golden.json), with its one device method, filter_objects, replaced by the float64 restatement of
tests/objbox_restate.py; the lrc_objbox layout and entry points; the synthetic annotation writer; and the register
budget of csrc/lrc_objboxes.hip's kernels."""
import io
import json
import os
import re
import subprocess
import warnings
from contextlib import redirect_stdout
from pathlib import Path

import numpy as np
import pytest

import objbox_restate
from conftest import PKG, REPO


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(REPO, "tests", "golden", "s3dis_bbox_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def area(gold, tmp_path_factory):
    from lidarcast import synth
    root = tmp_path_factory.mktemp("s3dis")
    synth.make_s3dis_area(root / "data", gold["area"], **gold["area_args"])
    return root / "data"


class _Calls:
    def __init__(self):
        self.sizes = []

    def __call__(self, point_sets, k=20, std_ratio=2.0):
        self.sizes.append([len(p) for p in point_sets])
        return objbox_restate.restate_filter_objects(point_sets, k, std_ratio)


def _visualizer(monkeypatch):
    from s3dis_bbox_visualizer import S3DISBBoxVisualizer
    calls = _Calls()
    monkeypatch.setattr(S3DISBBoxVisualizer, "filter_objects", lambda self, ps, k=20, std_ratio=2.0: calls(ps, k, std_ratio))
    return S3DISBBoxVisualizer(ctx=object()), calls


def _accepted_in_glob_order(room, entries):
    """The golden entries of a room in the order this filesystem lists its annotation files."""
    return [(f.name, entries[f.name]) for f in list((room / "Annotations").glob("*.txt")) if f.name in entries]


def _check_room_json(path, gold_room, room):
    j = json.loads(Path(path).read_text())
    want = _accepted_in_glob_order(room, gold_room["entries"])
    assert j["metadata"] == gold_room["metadata"]
    assert [a["instance_id"] for a in j["annotations"]] == list(range(1, len(want) + 1))
    assert [{k: v for k, v in a.items() if k != "instance_id"} for a in j["annotations"]] == [e for _, e in want]


def test_tables_and_names_match_the_reference():
    from s3dis_bbox_visualizer import S3DISBBoxVisualizer
    v = S3DISBBoxVisualizer(ctx=object())
    assert v.detection_classes == {'window', 'table', 'chair', 'sofa', 'bookcase', 'board', 'stairs'}
    assert v.bbox_params == {'min_points': 10, 'min_volume': 0.001, 'max_aspect_ratio': 10.0, 'max_vis_points': 1000}
    assert v.class_colors['board'] == [1.0, 0.5, 0.0] and len(v.class_colors) == 7


def test_load_annotation_file_matches_the_reference(gold, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    try:
        from make_s3dis_bbox_golden import crafted_files
    finally:
        sys.path.pop(0)
    from s3dis_bbox_visualizer import S3DISBBoxVisualizer
    v = S3DISBBoxVisualizer(ctx=object())
    for name, text in crafted_files(tmp_path).items():
        (tmp_path / name).write_text(text)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = v.load_annotation_file(tmp_path / name)
        want = gold["loaded"][name]
        if want is None:
            assert r is None, name
            continue
        assert r["points"].tolist() == want["points"] and r["object_name"] == want["object_name"], name
        assert r["file_name"] == want["file_name"]
        assert (r["colors"] is None) == (want["colors"] is None) and (r["colors"] is None or r["colors"].tolist() == want["colors"])
        assert (r["labels"] is None) == (want["labels"] is None) and (r["labels"] is None or r["labels"].tolist() == want["labels"])


def test_calculate_bbox_and_quality_match_the_reference(gold):
    from s3dis_bbox_visualizer import S3DISBBoxVisualizer
    v = S3DISBBoxVisualizer(ctx=object())
    for name, case in gold["boxes"].items():
        b = v.calculate_bbox(np.array(case["points"]).reshape(-1, 3))
        if case["bbox"] is None:
            assert b is None
            continue
        got = {k: (x.tolist() if isinstance(x, np.ndarray) else x) for k, x in b.items()}
        assert got == case["bbox"], name
        assert type(b["point_count"]) is int
        for cls, q in case["quality"].items():
            assert list(v.evaluate_bbox_quality(b, cls)) == q, (name, cls)


def test_generate_detection_annotations_bytes(gold, tmp_path):
    from s3dis_bbox_visualizer import S3DISBBoxVisualizer
    v = S3DISBBoxVisualizer(ctx=object())
    boxes = []
    for b in gold["annotations_input"]:
        b = dict(b)
        for key in ("center", "size", "min_coords", "max_coords"):
            b[key] = np.array(b[key])
        boxes.append(b)
    with redirect_stdout(io.StringIO()) as so:
        v.generate_detection_annotations(boxes, tmp_path / "ann.json")
    assert (tmp_path / "ann.json").read_text(encoding="utf-8") == gold["annotations_bytes"]
    assert so.getvalue().replace(str(tmp_path / "ann.json"), "<path>") == gold["annotations_stdout"]


def test_room_json_matches_the_reference(gold, area, tmp_path, monkeypatch):
    v, calls = _visualizer(monkeypatch)
    monkeypatch.chdir(tmp_path)
    for room in sorted((area / gold["area"]).iterdir()):
        with redirect_stdout(io.StringIO()):
            bb = v.visualize_room_bboxes(room, Path("ignored"))
        scene = f"{gold['area']}_{room.name}"
        _check_room_json(Path("simulation_results") / scene / f"{scene}_detection_annotations.json",
                         gold["rooms"][room.name], room)
        want = _accepted_in_glob_order(room, gold["rooms"][room.name]["entries"])
        assert [b["file_name"] for b in bb] == [n for n, _ in want]
        assert all(b["room_name"] == room.name for b in bb)
    assert len(calls.sizes) == len(gold["rooms"])                # one device call per room
    assert not Path("ignored").exists()


def test_process_area_matches_the_reference(gold, area, tmp_path, monkeypatch):
    v, calls = _visualizer(monkeypatch)
    monkeypatch.chdir(tmp_path)
    np.random.seed(gold["rng_seed"])
    with redirect_stdout(io.StringIO()):
        assert v.process_area(area / gold["area"], Path("unused_out")) == gold["process_area_return"] == []
    assert np.random.random(4).tolist() == gold["rng_after"]
    assert len(calls.sizes) == 1                                   # every room of the area in one device call
    written = sorted(Path("simulation_results").glob("*/*.json"))
    assert {f.name: len(json.loads(f.read_text())["annotations"]) for f in written} == gold["process_area_written"]
    for room in (area / gold["area"]).iterdir():
        scene = f"{gold['area']}_{room.name}"
        _check_room_json(Path("simulation_results") / scene / f"{scene}_detection_annotations.json",
                         gold["rooms"][room.name], room)
    assert v.process_area(area / "Area_9") is None


def test_main_modes(gold, area, tmp_path, monkeypatch):
    import s3dis_bbox_visualizer as mod
    _visualizer(monkeypatch)
    monkeypatch.chdir(tmp_path)
    room = next(d for d in (area / gold["area"]).iterdir() if d.is_dir())
    out = io.StringIO()
    with redirect_stdout(out):
        mod.main(["--data_root", str(area), "--area_name", gold["area"], "--room_name", room.name])
    assert out.getvalue().splitlines()[-1] == f"[Main] Room processed: {len(gold['rooms'][room.name]['entries'])} bounding boxes"
    assert (area / "bbox_visualization_results").is_dir()
    with redirect_stdout(io.StringIO()) as out:
        mod.main(["--data_root", str(area), "--area_name", gold["area"]])
    assert out.getvalue().splitlines()[-1] == "[Main] No valid bounding boxes in area"
    with redirect_stdout(io.StringIO()) as out:
        mod.main(["--data_root", str(area), "--process_all_areas", "--output_dir", str(tmp_path / "o")])
    lines = out.getvalue().splitlines()
    assert "[Main] Area Area_1 does not exist" in lines and lines[-1] == "[Main] All areas processed. Total bounding boxes: 0"
    with redirect_stdout(io.StringIO()) as out:
        mod.main(["--data_root", str(tmp_path / "nowhere")])
    assert out.getvalue().startswith("[Error] Data root directory does not exist")
    # first-room mode: the first room of the first existing area, written twice
    os.makedirs(area.parent / "first" / "Area_2", exist_ok=True)
    first_area = area.parent / "first"
    os.symlink(room, first_area / "Area_2" / room.name)
    with redirect_stdout(io.StringIO()) as out:
        mod.main(["--data_root", str(first_area), "--output_dir", str(tmp_path / "fr")])
    scene = f"Area_2_{room.name}"
    a = (Path("simulation_results") / scene / f"{scene}_detection_annotations.json").read_bytes()
    assert (tmp_path / "fr" / f"{scene}_detection_annotations.json").read_bytes() == a
    assert out.getvalue().count("[Annotation] Saved") == 2


def test_non_finite_object_is_skipped_with_a_warning(tmp_path, monkeypatch):
    v, calls = _visualizer(monkeypatch)
    monkeypatch.chdir(tmp_path)
    room = tmp_path / "Area_1" / "office_1"
    (room / "Annotations").mkdir(parents=True)
    rng = np.random.default_rng(0)
    good = np.round(rng.random((40, 3)), 3)
    np.savetxt(room / "Annotations" / "chair_1.txt", np.hstack([good, np.full((40, 3), 9.0)]), fmt="%.3f")
    bad = good.copy()
    bad[3, 1] = np.nan
    np.savetxt(room / "Annotations" / "table_1.txt", np.hstack([bad, np.full((40, 3), 9.0)]), fmt="%.3f")
    np.savetxt(room / "Annotations" / "wall_1.txt", np.hstack([bad, np.full((40, 3), 9.0)]), fmt="%.3f")
    with pytest.warns(UserWarning, match="non-finite"), redirect_stdout(io.StringIO()):
        bb = v.visualize_room_bboxes(room)
    assert [b["file_name"] for b in bb] == ["chair_1.txt"] and calls.sizes == [[40]]


def test_plots_and_meshes_are_out_of_scope():
    from s3dis_bbox_visualizer import S3DISBBoxVisualizer
    v = S3DISBBoxVisualizer(ctx=object())
    for name in ("create_bbox_mesh", "create_area_summary_visualization", "plot_area_bboxes_3d", "draw_bbox_3d",
                 "draw_bbox_2d", "plot_area_bboxes_2d", "plot_area_statistics"):
        with pytest.raises(NotImplementedError, match="DESIGN.md section 9"):
            getattr(v, name)({})


def test_annotation_writer_and_instances(tmp_path):
    from lidarcast import synth
    mesh = synth.make_room(size=(3.0, 2.5, 2.5), num_boxes=2, seed=4)
    p, c, l = synth.sample_s3dis_room(mesh, num_points=3000, num_outliers=20, seed=9)
    p2, c2, l2, ins = synth.sample_s3dis_room(mesh, num_points=3000, num_outliers=20, seed=9, return_instances=True)
    assert np.array_equal(p, p2) and np.array_equal(c, c2) and np.array_equal(l, l2)
    assert ins.shape == l.shape and (ins[l == 12] == 0).all()
    paths = synth.write_s3dis_annotations(tmp_path, "Area_1", "office_1", p, c, l, ins)
    names = [os.path.basename(x) for x in paths]
    assert "chair_1.txt" in names and "wall_4.txt" in names and "clutter_1.txt" in names
    rows = sum(len(np.loadtxt(x).reshape(-1, 6)) for x in paths)
    assert rows == len(p)
    for x in paths:
        d = np.loadtxt(x).reshape(-1, 6)
        name = os.path.basename(x).split("_")[0]
        sem = synth.S3DIS_CLASSES.index(name)
        sel = l == sem
        assert len(np.unique(ins[sel])) >= 1 and np.isin(d[:, :3].view([("", d.dtype)] * 3),
                                                          p[sel].view([("", p.dtype)] * 3)).all()


def test_restated_sum_order_on_known_values():
    # the restated reduction adds in the library's order: a sum whose value depends on the order shows it.  257 rows:
    # chunks of 2 rows, chunk 0 = (1e16, 1.0) -> 1e16, chunk 1 = (-1e16, 1.0) -> -1e16, chunk 128 = 1.0; the tree over
    # the chunks adds chunk 128 to chunk 0 first (1e16 again), then chunk 1: 0.0.  Left to right it is 2.0.
    v = np.array([1e16, 1.0, -1e16, 1.0] + [0.0] * 252 + [1.0])
    assert objbox_restate.fixed_sum(v) == 0.0 and sum(v.tolist()) == 2.0
    assert objbox_restate.fixed_sum(np.arange(1.0, 1001.0)) == 500500.0


def test_lrc_objbox_layout_matches_header():
    import ctypes as C
    from lidarcast import OBJBOX_DTYPE
    from lidarcast._capi import LrcObjBox
    src = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    body = re.search(r"typedef struct lrc_objbox \{(.*?)\} lrc_objbox;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    ctype = {C.c_uint64: "uint64_t", C.c_uint32: "uint32_t", C.c_double: "double"}
    got = []
    for f, ct in LrcObjBox._fields_:
        if hasattr(ct, "_length_"):
            got.append((ctype[ct._type_], f"{f}[{ct._length_}]"))
        else:
            got.append((ctype[ct], f))
    assert [(t, n) for t, n in decls] == got
    assert C.sizeof(LrcObjBox) == OBJBOX_DTYPE.itemsize == 88
    assert "88 bytes" in src[src.index("} lrc_objbox;"):src.index("} lrc_objbox;") + 50]
    assert list(OBJBOX_DTYPE.names) == [f for f, _ in LrcObjBox._fields_]
    assert all(OBJBOX_DTYPE.fields[f][1] == getattr(LrcObjBox, f).offset for f, _ in LrcObjBox._fields_)


def test_object_box_entry_points_are_declared():
    from lidarcast import _capi
    src = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    for name in ("lrc_object_boxes", "lrc_object_boxes_dev"):
        assert name in _capi.SYMBOLS and re.search(r"\bint %s\(" % name, src), name
    import lidarcast
    for name in ("object_boxes", "object_boxes_dev"):
        assert callable(getattr(lidarcast, name)), name


def test_objbox_kernels_use_no_scratch_and_fit_128_vgprs(tmp_path):
    import __graft_entry__ as entry
    assert "lrc_objboxes.hip" in entry.SOURCES
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(PKG, "csrc", "lrc_objboxes.hip"), "-o", str(tmp_path / "o.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
    vgprs = [int(x) for x in re.findall(r"remark:\s+VGPRs: (\d+)", r.stderr)]
    agprs = [int(x) for x in re.findall(r"remark:\s+AGPRs: (\d+)", r.stderr)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(vgprs) == len(agprs) == len(scratch)
    ours = [(n, v + a, s) for n, v, a, s in zip(names, vgprs, agprs, scratch) if "ob_" in n]
    # bounds, grid, key, gather, sum, final, keep, compact, box, and eight k-NN list lengths
    assert len(ours) == 17, [n for n, _, _ in ours]
    assert not any("pp_" in n for n in names)
    assert all(s == 0 for _, _, s in ours), [n for n, _, s in ours if s]
    assert all(v <= 128 for _, v, _ in ours), [(n, v) for n, v, _ in ours if v > 128]
    spilling = [n for n, s in zip(names, scratch) if s]
    assert all("rocprim" in n and "radix_sort_onesweep" in n for n in spilling), spilling
