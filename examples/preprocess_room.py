#!/usr/bin/env python3
"""Room preprocessing end to end: a synthetic S3DIS-like room -> s3dis_data_loader.main -> the pickle the reconstruction
stage reads, plus the PLY variants and the summary file.

    python examples/preprocess_room.py [out_dir]      # default preprocess_room_out/

The room is sampled from a synthetic mesh at S3DIS density (about 1.8 M rows, 3-decimal coordinates, 300 outliers) and
written as <out>/data/Area_6/office_2/office_2.txt; the config is the reference's preprocessing section (outliers k = 20,
std_ratio = 2, normals radius 0.1, max_nn 30) with three sparsity variants."""
import os
import pickle
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402


def main():
    import yaml
    import s3dis_data_loader
    from lidarcast import synth
    out = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else "preprocess_room_out")
    pts, cols, labels = synth.sample_s3dis_room(synth.make_room(seed=6), seed=0)
    synth.write_s3dis_room(os.path.join(out, "data"), "Area_6", "office_2", pts, cols, labels)
    cfg = {"data": {"data_root": os.path.join(out, "data"), "output_root": out, "area_name": "Area_6",
                    "room_name": "office_2"},
           "preprocessing": {"estimate_normals": True, "use_shs_net": False, "normal_search_radius": 0.1,
                             "normal_max_nn": 30, "remove_outliers": True, "outlier_nb_neighbors": 20,
                             "outlier_std_ratio": 2.0},
           "sparsity_experiments": [{"name": "dense", "keep_ratio": 1.0, "occlusion": False},
                                    {"name": "sparse_30", "keep_ratio": 0.3, "occlusion": False},
                                    {"name": "robot_scan", "keep_ratio": 0.6, "occlusion": True}]}
    cfg_path = os.path.join(out, "s3dis_config.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    np.random.seed(0)                                   # the sparsity variants draw from the global stream
    t0 = time.perf_counter()
    s3dis_data_loader.main(["--config", cfg_path, "--save_pointclouds"])
    dt = time.perf_counter() - t0
    with open(os.path.join(out, "preprocessed_data", "Area_6_office_2_preprocessed.pkl"), "rb") as f:
        room = pickle.load(f)
    print(f"{room['original_data']['point_count']} rows -> {room['processed_data']['point_count']} kept, "
          f"normals {room['processed_data']['normals'].shape}, {dt:.1f} s (text loading included)")
    for name, v in room["sparsity_variants"].items():
        print(f"  {name}: {v['point_count']} rows")
    print("written under", os.path.join(out, "preprocessed_data"))


if __name__ == "__main__":
    main()
