"""numpy restatement of the seeded sensor noise under movers in sweeps of lrc_scan_noisy_mover_sweeps_* (include/lidarcast.h
"seeded sensor noise under movers in sweeps").  A composition of what exists, nothing of its own:
tests/noisy_sweep_restate.py gives the jittered swept rays, the filter centres c(s), the range term and the keep mask;
tests/mover_sweep_restate.py takes the kept rays into every mover's frame at the ray's own s and merges the casts on the CLEAN
ranges; then t' = t + term is one float32 add, t' <= 0 is a miss, and mover_restate.record about c(s) assembles the record at t'.
It takes any "cast these rays" function; a mover's cast function may take the firing fractions of the rays it is given as a second
argument (``per_ray=True``: span_restate.fraction_cast behind a spanned deformable)."""
import numpy as np

import mover_restate as mv
import mover_sweep_restate as ms
import noisy_sweep_restate as nsr
from mover_noise_restate import cast_kept, table

F32 = np.float32


def scan(cast_static, cast_movers, motion, dirs, fire, records, model, max_range, min_range=0.0, incident_mode=0, tab=None,
         per_ray=()):
    """P sweeps ``motion`` (P, 24) of the table ``dirs`` (N, 3) with the firing fractions ``fire`` (N,) under ``model`` (a
    lidarcast.noise.NoiseModel; sweep p is frame model.first_frame + p), M movers given by their cast functions and ``records``
    (P, M, 24).  ``per_ray``: the indices m whose cast function is called as cast(rays, fire_of_those_rays).  Returns (record
    dict over all P * N rays, winners dict on the clean ranges before any filter, info dict: rays, centres, term, keep)."""
    base, slope = table() if tab is None else tab
    motion = np.asarray(motion, np.float64).reshape(-1, 24)
    fire = np.asarray(fire, np.float64).reshape(-1)
    P, N, M = len(motion), len(dirs), len(cast_movers)
    rays, cen, term, keep, _ = nsr.noisy_sweep_rays(motion, dirs, fire, model, base, slope)
    rec24 = np.asarray(records, F32).reshape(P, M, 24) if M else np.zeros((P, 0, 24), F32)
    wins = []
    for p in range(P):
        sl = slice(p * N, (p + 1) * N)
        r, k = rays[sl], keep[sl]
        static = cast_kept(cast_static, r, k)                           # 1: a dropped ray is cast against nothing
        safe = np.where(k[:, None], r, F32(0))
        movers = []
        for m, c in enumerate(cast_movers):                              # 2: the kept rays in the mover's frame at their own s
            obj = ms.to_object_at(safe, fire, rec24[p, m])
            if m in per_ray:
                fk = fire[k]
                movers.append(cast_kept(lambda q, c=c, fk=fk: c(q, fk), obj, k))
            else:
                movers.append(cast_kept(c, obj, k))
        wins.append(ms.merge(static, movers, fire, rec24[p]))           # 3: the winner on the clean ranges
    win = {a: np.concatenate([w[a] for w in wins]) for a in wins[0]}
    noisy = dict(win)
    with np.errstate(invalid="ignore"):
        t = (win["t"] + term).astype(F32) if model.range_std != 0 else win["t"].copy()       # 4: one float32 add (inf stays inf)
    t[~(t > 0)] = np.inf                                                 # t' <= 0 is no return
    noisy["t"] = t
    safe = np.where(keep[:, None], rays, F32(1))                         # a dropped ray's NaN direction never reaches a record
    rec = mv.record(noisy, safe, cen, max_range, min_range, incident_mode)
    return rec, win, {"rays": rays, "centres": cen, "term": term, "keep": keep}


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------

SEED = 1                # with it the oracle alone satisfies what the GPU cases rely on (tests/test_mover_sweep_noise_host.py asserts it)
JITTER = float(np.deg2rad(0.5))


def model_of(seed=SEED, first_frame=5, **kw):
    """The sensor record's model (the dense 32-line record: 0.01 m, 0.005 degrees, 5 % dropout)."""
    import dataclasses
    from lidar import Indoor8LineLidarIntrinsics
    from lidarcast.noise import NoiseModel
    m = NoiseModel.from_intrinsics(Indoor8LineLidarIntrinsics.create_dense_32line(), seed, first_frame)
    assert (m.range_std, m.dropout) == (0.01, 0.05) and np.isclose(np.rad2deg(m.angle_std), 0.005)
    return dataclasses.replace(m, **kw)


def zero_model(first_frame=5):
    from lidarcast.noise import NoiseModel
    return NoiseModel(seed=SEED, first_frame=first_frame)


def mover_meshes():
    """The three movers of tests/test_mover_sweeps_gpu.py: the 12-triangle box, the pedestrian, a small cube."""
    from lidarcast import synth
    cube = synth.unit_cube(-0.3, 0.3)
    n = len(cube.triangles)
    cube = synth.TriangleMesh(vertices=np.asarray(cube.vertices, np.float64), triangles=np.asarray(cube.triangles, np.int32),
                              triangle_sem=np.full(n, 12, np.uint16), triangle_ins=np.full(n, 1002, np.uint16))
    return [ms.box_mover(13, 77), synth.make_pedestrian(semantic=13, instance=1001), cube]


def conditions(want, win, info, clean_win, N):
    """What a parity case exercises, counted on the restatement: (rays a mover wins in the sweep where movers win fewest, rays
    the clean sweep gives to a mover that the model drops, kept rays whose winner differs from the clean sweep's)."""
    P = len(want["mover"]) // N
    per_sweep = min(int((want["mover"][p * N:(p + 1) * N] != 0).sum()) for p in range(P))
    dropped = int(((clean_win["mover"] != 0) & ~info["keep"]).sum())
    moved = int((info["keep"] & (win["mover"] != clean_win["mover"])).sum())
    return per_sweep, dropped, moved
