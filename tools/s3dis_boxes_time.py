#!/usr/bin/env python3
"""S3DIS annotation-box timing on a synthetic area (lidarcast.synth.make_s3dis_area: --rooms rooms, each with walls,
floor, ceiling, tables, chairs and bookcases of 10^3 to 10^5 rows and small windows / boards of 10 to 200 rows, 3-decimal
text files), the reference's parameters (k = 20, std_ratio = 2):

  parse   : np.loadtxt of every detection-class Annotations file of the area (what S3DISBBoxVisualizer reads);
  area    : lidarcast.object_boxes over all of those objects at once (one device call: upload, filter, boxes, download);
  loop    : lidarcast.preprocess_cloud (remove_outliers only) once per object of 20 rows or more, the per-object
            alternative;
  scipy   : the float64 cKDTree restatement (tests/objbox_restate.py, workers = 16) per object.  NOT Open3D, which is
            not installed: a CPU yardstick only.
Each figure is the median of --repeats runs after a warm-up; the device calls return once their work has finished.

    python tools/s3dis_boxes_time.py                  # all four
    python tools/s3dis_boxes_time.py --device-only    # the area call alone (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys
import tempfile
import time
from pathlib import Path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

DETECTION = {'window', 'table', 'chair', 'sofa', 'bookcase', 'board', 'stairs'}


def median_time(fn, repeats):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=20)
    ap.add_argument("--density", type=float, default=2000.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()

    import lidarcast
    from lidarcast import synth
    import objbox_restate

    td = tempfile.TemporaryDirectory()
    t0 = time.perf_counter()
    synth.make_s3dis_area(Path(td.name) / "data", "Area_1", num_rooms=a.rooms, seed=1, density=a.density, num_boxes=8,
                          small_objects=8)
    t_make = time.perf_counter() - t0
    files = [f for room in (Path(td.name) / "data" / "Area_1").iterdir() if room.is_dir()
             for f in (room / "Annotations").glob("*.txt") if f.stem.split('_')[0] in DETECTION]

    def parse():
        return [np.loadtxt(f)[:, :3] for f in files]
    objs = parse()
    sizes = np.array([len(o) for o in objs])
    pts = np.concatenate(objs, 0)
    off = np.concatenate([[0], np.cumsum(sizes)])
    ctx = lidarcast.Context(0)

    def area():
        return lidarcast.object_boxes(ctx, pts, off, k=20, std_ratio=2.0)

    def loop():
        return [lidarcast.preprocess_cloud(ctx, o, nb_neighbors=20, std_ratio=2.0, estimate_normals=False).kept
                for o in objs if len(o) >= 20]

    def scipy():
        return objbox_restate.restate_filter_objects(objs, 20, 2.0)

    area()                                             # warm-up (code objects, pools)
    if a.device_only:
        for _ in range(a.repeats):
            area()
        print(f"device-only: {a.repeats} area calls over {len(objs)} objects / {len(pts)} rows")
        return
    loop()
    r = area()
    kept_loop = loop()
    big = [o for o in objs if len(o) >= 20]
    same = all(np.array_equal(r.kept_rows(j).astype(np.int64) - off[j], k.astype(np.int64))
               for j, k in zip([j for j, o in enumerate(objs) if len(o) >= 20], kept_loop))

    print(f"synthetic area: {a.rooms} rooms, density {a.density:g} /m^2 (made in {t_make:.1f} s); {len(files)} "
          f"detection-class objects, {len(pts)} rows; object rows min / median / max = {sizes.min()} / "
          f"{int(np.median(sizes))} / {sizes.max()}; {len(big)} objects of 20 rows or more")
    rows = [("parse   np.loadtxt of the detection files", median_time(parse, 3)),
            ("area    lidarcast.object_boxes, one call", median_time(area, a.repeats)),
            ("loop    lidarcast.preprocess_cloud per object", median_time(loop, 3)),
            ("scipy   cKDTree restatement per object, 16 workers", median_time(scipy, 1))]
    for name, (med, mn) in rows:
        print(f"{name:55s} median {med * 1e3:10.2f} ms   min {mn * 1e3:10.2f} ms")
    print(f"per-object loop / area call = {rows[2][1][0] / rows[1][1][0]:.1f}x; kept rows identical: {same}")
    td.cleanup()


if __name__ == "__main__":
    main()
