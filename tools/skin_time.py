#!/usr/bin/env python3
"""Skinned-mover timings, one box, one session.  One lrc_deform_set_dev of a skinned deformable (k_skin
and the refit) against one of the keyframe deformable made from the same clip's host-skinned keyframes (k_blend or the keyframe
copy, and the same refit), on two rigs:

  walker       synth.make_walker_rig(smooth=0.08): 204 vertices, 384 triangles, 6 bones, K = 8
  pedestrian   synth.make_pedestrian(segments=224, rings=222): 49 954 vertices, 99 904 triangles, a chain of three bones with
               linear weights between neighbouring joints, K = 64 key poses of a sway

The keyframe route is the yardstick: this change does not touch its launches.  HIP events around --calls calls on one stream, the
two routes in alternating blocks so that both see the same clocks, --blocks blocks each; per shape kind: "blend" (two different
key poses, 0 < w < 1, the shape changes with every call) and "one" (w = 0: k_skin<false> against the device-to-device copy).
Both deformables' device_bytes and launch counts are reported.  The vertices of the last shape are compared bit for bit before
anything is timed.

    python tools/skin_time.py [--calls 200] [--blocks 7] [--out report.txt]
profiles/skin_c3.txt holds this report.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402


def _stats(v):
    v = np.array(v)
    return {"median_us": round(float(np.median(v)) * 1e3, 2), "min_us": round(float(v.min()) * 1e3, 2),
            "max_us": round(float(v.max()) * 1e3, 2), "n": len(v)}


def walker_rig():
    from lidarcast import synth
    m = synth.make_walker_rig(smooth=0.08)
    return dict(rest=m.vertices.astype(np.float32), tris=np.asarray(m.triangles, np.int32), idx=m.bone_index, wgt=m.bone_weight,
                poses=m.poses12)


def pedestrian_rig(segments=224, rings=222, K=64, height=1.7):
    """make_pedestrian as a chain of three bones (joints on the axis at 0, H / 3 and 2 H / 3); a vertex between two joints
    shares its weight linearly between their bones; key pose k bends the chain about y by 12 deg * sin(2 pi k / K) per joint."""
    from lidarcast import skin, synth
    m = synth.make_pedestrian(height=height, segments=segments, rings=rings)
    rest = np.asarray(m.vertices, np.float64)
    joints = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, height / 3], [0.0, 0.0, 2 * height / 3]])
    x = np.clip(rest[:, 2] / (height / 3), 0.0, 3.0)           # 0 .. 3 along the chain
    lower = np.minimum(np.floor(x), 2).astype(np.int64)         # the bone below the vertex
    share = np.where(lower < 2, x - lower, 0.0)                  # ... and what its upper neighbour takes (the top bone: none)
    idx = np.zeros((len(rest), 4), np.uint8)
    wgt = np.zeros((len(rest), 4), np.float32)
    idx[:, 0], idx[:, 1] = lower, np.minimum(lower + 1, 2)
    wgt[:, 1] = share.astype(np.float32)
    wgt[:, 0] = np.float32(1.0) - wgt[:, 1]
    rot = np.zeros((K, 3, 3, 3))
    for k in range(K):
        a = np.deg2rad(12.0) * np.sin(2.0 * np.pi * k / K)
        c, s = np.cos(a), np.sin(a)
        rot[k, :] = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
        rot[k, 0] = np.eye(3)
    poses = skin.Skeleton([-1, 0, 1], joints).matrices(rot)
    return dict(rest=rest.astype(np.float32), tris=np.asarray(m.triangles, np.int32), idx=idx, wgt=wgt, poses=poses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    import lidarcast
    from lidarcast import deform, skin
    ctx = lidarcast.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"calls_per_block": a.calls, "blocks": a.blocks,
           "what": "one lrc_deform_set_dev (vertices + refit), microseconds, HIP events around a block of calls / calls"}
    for name, g in (("walker", walker_rig()), ("pedestrian_50k", pedestrian_rig())):
        K, B = g["poses"].shape[:2]
        sem = np.full(len(g["tris"]), 13, np.uint16)
        keys = skin.keyframes(g["rest"], g["idx"], g["wgt"], g["poses"])
        routes = {"skinned": deform.SkinnedDeformable(ctx, g["rest"], g["tris"], g["idx"], g["wgt"], g["poses"], sem, sem),
                  "keyframes": deform.Deformable(ctx, keys, g["tris"], sem, sem)}
        out = {"vertices": int(len(g["rest"])), "triangles": int(len(g["tris"])), "bones": int(B), "key_poses": int(K),
               "nodes": int(routes["skinned"].scene.info["num_nodes"]),
               "device_bytes": {n: int(d.scene.info["device_bytes"]) for n, d in routes.items()},
               "launches_blend_one": {n: list(d.launches()) for n, d in routes.items()}}
        out["device_bytes"]["keyframes_over_skinned"] = round(out["device_bytes"]["keyframes"] / out["device_bytes"]["skinned"], 2)
        for d in routes.values():
            d.set(K - 2, K - 1, 0.3, stream=stream)
        same = np.array_equal(routes["skinned"].vertices().view(np.uint32), routes["keyframes"].vertices().view(np.uint32))
        out["vertices_bit_equal"] = bool(same)
        if not same:
            raise SystemExit(f"{name}: the two routes' vertices differ")
        shapes = {"blend": lambda i: (i % K, (i + 1) % K, 0.25 + 0.5 * (i % 2)), "one": lambda i: (i % K, (i + 1) % K, 0.0)}
        for kind, shape in shapes.items():
            for d in routes.values():                        # warm-up: every kernel of the timed window
                for i in range(20):
                    d.set(*shape(i), stream=stream)
            torch.cuda.synchronize()
            per_call = {n: [] for n in routes}
            for _ in range(a.blocks):                        # alternating blocks: both routes see the same clocks
                for n, d in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(a.calls):
                        d.set(*shape(i), stream=stream)
                    e1.record()
                    e1.synchronize()
                    per_call[n].append(e0.elapsed_time(e1) / a.calls)
            r = {n: _stats(v) for n, v in per_call.items()}
            r["skinned_over_keyframes"] = round(r["skinned"]["median_us"] / r["keyframes"]["median_us"], 3)
            out[kind] = r
        for d in routes.values():
            d.close()
        res[name] = out
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
