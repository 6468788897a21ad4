"""numpy restatement of the movers under moving-sensor sweeps of lrc_scan_mover_sweeps_* (include/lidarcast.h "movers under
moving-sensor sweeps").  Written from the header's text, not from csrc/lrc_movers.h: the tests compare the two.  Every float32
operation stands alone in the order the header gives; numpy never fuses.  The merge and the record are tests/mover_restate.py's,
with the mover's normal turned per ray; the world rays are tests/sweep_restate.py's.

Also here: the inputs of the physical check (a box that crosses the line of sight at 10 m/s during one sweep) and its float64
measure, the distance of a point from the box's surface in the box's own frame by the pose at the point's own time."""
import numpy as np

import mover_restate as mv

F32 = np.float32
ONE_BITS = np.uint32(0x3F800000)


def still(rec):
    """word 12 has the bits of 1.0f, words 13..18 are all +0.0f"""
    w = np.ascontiguousarray(rec, F32).reshape(24).view(np.uint32)
    return bool(w[12] == ONE_BITS and not w[13:19].any())


def _pose_at(rec, s):
    """(c (n, 3), qw, ux, uy, uz, k) of the record at the float32 fractions s (n,)"""
    r = np.asarray(rec, F32).reshape(24)
    s = np.asarray(s, F32)
    c = np.stack([r[3] + s * r[16], r[7] + s * r[17], r[11] + s * r[18]], axis=1)
    qw = (F32(1.0) - s) + s * r[12]
    ux, uy, uz = s * r[13], s * r[14], s * r[15]
    n = ((qw * qw + ux * ux) + uy * uy) + uz * uz
    return c, qw, ux, uy, uz, F32(2.0) / n


def _rot(v, qw, ux, uy, uz, k, inverse):
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    tx, ty, tz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
    wx, wy, wz = uy * tz - uz * ty, uz * tx - ux * tz, ux * ty - uy * tx
    if inverse:
        return np.stack([vx + k * (wx - qw * tx), vy + k * (wy - qw * ty), vz + k * (wz - qw * tz)], axis=1).astype(F32)
    return np.stack([vx + k * (qw * tx + wx), vy + k * (qw * ty + wy), vz + k * (qw * tz + wz)], axis=1).astype(F32)


def _rt(R, v):
    """R^T v as step 2 of the moving objects forms it"""
    out = np.empty_like(v)
    for j in range(3):
        out[:, j] = (R[0, j] * v[:, 0] + R[1, j] * v[:, 1]) + R[2, j] * v[:, 2]
    return out


def to_object_at(rays, fire, rec):
    """step 2 of the header: ray i in the frame the mover of ``rec`` has at s = float32(fire[i])"""
    rays = np.ascontiguousarray(rays, F32)
    rec = np.ascontiguousarray(rec, F32).reshape(24)
    if still(rec):
        return mv.to_object(rays, rec[:12])
    s = np.asarray(fire, np.float64).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        c, qw, ux, uy, uz, k = _pose_at(rec, s)
        e = rays[:, :3] - c
        R = rec[:12].reshape(3, 4)[:, :3]
        out = np.empty_like(rays)
        out[:, :3] = _rt(R, _rot(e, qw, ux, uy, uz, k, True))
        out[:, 3:] = _rt(R, _rot(rays[:, 3:], qw, ux, uy, uz, k, True))
    return out


def to_world_at(n3, fire, rec):
    """step 4's normal: forward(R_start n), not renormalised"""
    n3 = np.ascontiguousarray(n3, F32)
    rec = np.ascontiguousarray(rec, F32).reshape(24)
    w = mv.to_world(n3, rec[:12])
    if still(rec):
        return w
    s = np.asarray(fire, np.float64).astype(F32)
    _, qw, ux, uy, uz, k = _pose_at(rec, s)
    return _rot(w, qw, ux, uy, uz, k, False)


def merge(static, movers, fire, records):
    """mover_restate.merge with the normal of mover m turned by to_world_at(records[m]) at the ray's own fire"""
    t = np.asarray(static["t"], F32).copy()
    out = {"t": t, "prim": np.asarray(static["prim"]).astype(np.uint32).copy(),
           "sem": np.asarray(static["sem"]).astype(np.uint16).copy(), "ins": np.asarray(static["ins"]).astype(np.uint16).copy(),
           "normal3": np.asarray(static["normal3"], F32).copy(), "mover": np.zeros(len(t), np.uint8)}
    fire = np.asarray(fire, np.float64)
    for m, c in enumerate(movers):
        tm = np.asarray(c["t"], F32)
        take = tm < out["t"]
        out["t"][take] = tm[take]
        for a in ("prim", "sem", "ins"):
            out[a][take] = np.asarray(c[a])[take].astype(out[a].dtype)
        out["normal3"][take] = to_world_at(np.asarray(c["normal3"], F32)[take], fire[take], records[m])
        out["mover"][take] = m + 1
    return out


def scan(cast_static, cast_movers, rays, centres, fire, records, rays_per_pose, max_range, min_range=0.0, incident_mode=0,
         to_object=to_object_at):
    """P sweeps of ``rays_per_pose`` world rays each ((P * N, 6) float32 and their (P * N, 3) float64 filter centres, as
    sweep_restate.sweep_rays gives them), ``fire`` (N,), M movers given by their cast functions and ``records`` (P, M, 24).
    ``to_object``: the step that takes rays into a mover's frame (the restatement's, or the library's host step).  Returns
    (record dict over all P * N rays, winners dict before any filter)."""
    rays = np.ascontiguousarray(rays, F32)
    N = int(rays_per_pose)
    P = len(rays) // N
    rec = np.asarray(records, F32).reshape(P, len(cast_movers), 24)
    wins = []
    for p in range(P):
        r = rays[p * N:(p + 1) * N]
        casts = [cast(to_object(r, fire, rec[p, m])) for m, cast in enumerate(cast_movers)]
        wins.append(merge(cast_static(r), casts, fire, rec[p]))
    win = {k: np.concatenate([w[k] for w in wins]) for k in wins[0]}
    return mv.record(win, rays, centres, max_range, min_range, incident_mode), win


def compose_host(cast_static, cast_movers, rays, centres, fire, records, rays_per_pose, max_range, min_range=0.0, incident_mode=0):
    """The composition the issue names, by the library's HOST steps: lidarcast.movers.sweep_rays -> a cast per mover ->
    lidarcast.movers.sweep_normals -> lidarcast.movers.merge -> the write-back restatement (mover_restate.record with the sweep's
    per-ray centres).  merge is given the identity pose: it picks the winner, and the winner's normal is then the turned row
    itself (through the identity a -0.0 component would come out +0.0).  Same return value as ``scan``."""
    from lidarcast import movers
    rays = np.ascontiguousarray(rays, F32)
    N = int(rays_per_pose)
    P, M = len(rays) // N, len(cast_movers)
    rec = np.asarray(records, F32).reshape(P, M, 24)
    ident = np.tile(mv.pose12(0.0, 0.0, 0.0, 0.0), (M, 1))
    wins = []
    for p in range(P):
        r = rays[p * N:(p + 1) * N]
        st = cast_static(r)
        casts = [cast(movers.sweep_rays(r, fire, rec[p, m])) for m, cast in enumerate(cast_movers)]
        turned = [movers.sweep_normals(c["normal3"], fire, rec[p, m]) for m, c in enumerate(casts)]
        t, _, who = movers.merge(st["t"], st["normal3"], np.stack([c["t"] for c in casts]), np.stack(turned), ident)
        win = {"t": t, "mover": who, "normal3": np.asarray(st["normal3"], F32).copy(),
               "prim": np.asarray(st["prim"]).astype(np.uint32).copy(), "sem": np.asarray(st["sem"]).astype(np.uint16).copy(),
               "ins": np.asarray(st["ins"]).astype(np.uint16).copy()}
        for m, c in enumerate(casts):
            take = who == m + 1
            win["normal3"][take] = turned[m][take]
            for a in ("prim", "sem", "ins"):
                win[a][take] = np.asarray(c[a])[take].astype(win[a].dtype)
        wins.append(win)
    win = {k: np.concatenate([w[k] for w in wins]) for k in wins[0]}
    return mv.record(win, rays, centres, max_range, min_range, incident_mode), win


def record24(x, y, z, yaw, dx=0.0, dy=0.0, dz=0.0, dyaw=0.0):
    """(24,) float32: the mover at (x, y, z, yaw) at the start of the sweep, moved by (dx, dy, dz) and turned by dyaw about z at
    its end; float64 arithmetic narrowed last."""
    out = np.zeros(24, np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    out[:12] = [c, -s, 0.0, x, s, c, 0.0, y, 0.0, 0.0, 1.0, z]
    out[12], out[15] = np.cos(0.5 * dyaw), np.sin(0.5 * dyaw)
    out[16:19] = dx, dy, dz
    return out.astype(F32)


def still_record(p12):
    out = np.zeros(24, F32)
    out[:12] = p12
    out[12] = 1.0
    return out


# ---- the physical check ---------------------------------------------------------------------------------------------------------

BOX_LO, BOX_HI = np.array([-0.3, -0.3, 0.0]), np.array([0.3, 0.3, 1.6])
SWEEP_T = 0.1           # seconds: one sweep of a 10 Hz sensor
BOX_STEP = 1.0          # metres: 10 m/s for 0.1 s
BOX_TURN = 0.1          # rad about z during the sweep


def box_mover(semantic=13, instance=77):
    """The 12-triangle box [-0.3, 0.3]^2 x [0, 1.6] around its own origin."""
    from lidarcast import synth
    cube = synth.unit_cube(0.0, 1.0)
    v = BOX_LO + np.asarray(cube.vertices, np.float64) * (BOX_HI - BOX_LO)
    n = len(cube.triangles)
    return synth.TriangleMesh(vertices=v, triangles=np.asarray(cube.triangles, np.int32),
                              triangle_sem=np.full(n, semantic, np.uint16), triangle_ins=np.full(n, instance, np.uint16))


def crossing_inputs():
    """The sensor (6 lines x 256 columns: 1536 rays, 24 whole waves) at rest in the small room, its table and firing fractions,
    the box's path [[t, x, y, z, yaw_deg]] -- across the line of sight from (2.2, 2.6) to (3.2, 2.6) in 0.1 s, 1.5 m in front of
    the sensor -- and the sensor's motion record."""
    from helpers import pose, sensor_small
    from lidar import IndoorLidar
    from lidarcast import motion_records
    k = sensor_small(lines=6, width=256)
    lid = IndoorLidar(k, np.eye(4))
    dirs = np.ascontiguousarray(lid.sensor_directions(), dtype=np.float64)
    fire = np.ascontiguousarray(lid.firing_fractions(), dtype=np.float64)
    start = pose(2.7, 1.1, 1.0, 0.3)[None]
    path = [[0.0, 2.2, 2.6, 0.0, 10.0], [SWEEP_T, 2.2 + BOX_STEP, 2.6, 0.0, 10.0 + np.degrees(BOX_TURN)]]
    return k, dirs, fire, motion_records(start, start), path


def box_distance(points, s, rec):
    """float64: the distance of each world point from the surface of the box, in the box's frame by the pose the record gives at
    the point's own s (the centre c0 + s dc, the rotation R(q(s) / |q(s)|) R_start)."""
    r = np.asarray(rec, np.float64).reshape(24)
    p = np.asarray(points, np.float64)
    s = np.asarray(s, np.float64)
    c = r[[3, 7, 11]][None, :] + s[:, None] * r[16:19][None, :]
    q = np.stack([(1.0 - s) + s * r[12], s * r[13], s * r[14], s * r[15]], axis=1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    R0 = r[:12].reshape(3, 4)[:, :3]
    out = np.empty(len(p))
    for i in range(len(p)):
        w, x, y, z = q[i]
        Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        b = (Rq @ R0).T @ (p[i] - c[i])
        outside = np.maximum(np.maximum(BOX_LO - b, b - BOX_HI), 0.0)
        if outside.any():
            out[i] = np.linalg.norm(outside)
        else:
            out[i] = np.minimum(b - BOX_LO, BOX_HI - b).min()
    return out
