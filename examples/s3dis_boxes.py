#!/usr/bin/env python3
"""S3DIS annotation boxes end to end: a synthetic S3DIS area -> s3dis_bbox_visualizer.main -> one
<Area>_<room>_detection_annotations.json per room under simulation_results/ of the working directory.

    python examples/s3dis_boxes.py [out_dir]      # default s3dis_boxes_out/ (the JSON goes to <out_dir>/simulation_results)

The area has six rooms (walls, floor, ceiling, tables, chairs, bookcases, small windows and boards), written as S3DIS
text files with Annotations/<class>_<k>.txt per object; process_area filters every detection-class object of the area
in one device call (k = 20, std_ratio = 2) and writes each room's file."""
import json
import os
import sys
import time
from pathlib import Path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))


def main():
    import s3dis_bbox_visualizer
    from lidarcast import synth
    out = Path(sys.argv[1] if len(sys.argv) > 1 else "s3dis_boxes_out").absolute()
    synth.make_s3dis_area(out / "data", "Area_1", num_rooms=6, seed=0, density=2000.0)
    os.makedirs(out, exist_ok=True)
    os.chdir(out)                                     # the reference writes under ./simulation_results
    t0 = time.perf_counter()
    s3dis_bbox_visualizer.main(["--data_root", str(out / "data"), "--area_name", "Area_1"])
    dt = time.perf_counter() - t0
    for f in sorted(Path("simulation_results").glob("*/*.json")):
        anns = json.loads(f.read_text())["annotations"]
        print(f"  {f.name}: {len(anns)} boxes ({', '.join(a['original_class_name'] for a in anns)})")
    print(f"{dt:.2f} s (text parsing included); written under {out / 'simulation_results'}")


if __name__ == "__main__":
    main()
