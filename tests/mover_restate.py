"""numpy restatement of the moving objects of lrc_scan_movers_* (include/lidarcast.h "moving objects").  Written from the
header's text, not from csrc/lrc_movers.h: the tests compare the two.  It takes any "cast these rays" function -- the CPU oracle
on the host, the explicit-ray cast on the GPU -- that maps (n, 6) float32 rays to a dict of per-ray t (+inf: a miss), prim, sem,
ins and normal3, nothing filtered and nothing culled."""
import numpy as np

RAD2DEG = 57.29577951308232
INVALID = np.uint32(0xFFFFFFFF)
F32 = np.float32


def unit(d):
    """d / |d|, float32, one rounding per operation."""
    d = np.asarray(d, F32)
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return d / nrm[:, None]


def fmaf(a, b, c):
    """float32 fused multiply-add: the product is exact in float64, the sum is rounded to odd there (two-sum gives the exact
    remainder), so the narrowing is the single rounding of the exact a * b + c."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = (err != 0.0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(F32)


def pose12(x, y, z, yaw):
    """(12,) float32 row-major [Rz(yaw) | c], float64 arithmetic narrowed last."""
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([c, -s, 0.0, x, s, c, 0.0, y, 0.0, 0.0, 1.0, z], np.float64).astype(F32)


def pose12_of(mat):
    """(12,) float32 of a float64 (4, 4) or (3, 4) object-to-world matrix."""
    return np.asarray(mat, np.float64)[:3, :4].reshape(12).astype(F32)


def to_object(rays, p12):
    """step 2: e = o - c, o'_j = (R[0][j] e_x + R[1][j] e_y) + R[2][j] e_z, d' the same expression on d; float32."""
    rays = np.ascontiguousarray(rays, F32)
    m = np.asarray(p12, F32).reshape(3, 4)
    R, c = m[:, :3], m[:, 3]
    e = rays[:, :3] - c[None, :]
    out = np.empty_like(rays)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(3):
            out[:, j] = (R[0, j] * e[:, 0] + R[1, j] * e[:, 1]) + R[2, j] * e[:, 2]
            out[:, 3 + j] = (R[0, j] * rays[:, 3] + R[1, j] * rays[:, 4]) + R[2, j] * rays[:, 5]
    return out


def to_world(n3, p12):
    """step 4: normal3_j = (R[j][0] n_x + R[j][1] n_y) + R[j][2] n_z, float32, not renormalised."""
    n3 = np.asarray(n3, F32)
    R = np.asarray(p12, F32).reshape(3, 4)[:, :3]
    out = np.empty_like(n3)
    for j in range(3):
        out[:, j] = (R[j, 0] * n3[:, 0] + R[j, 1] * n3[:, 1]) + R[j, 2] * n3[:, 2]
    return out


def merge(static, movers, poses12):
    """step 3 and the winner's columns for ONE frame: ``static`` the static cast's dict, ``movers`` the M mover casts' dicts,
    ``poses12`` (M, 12).  The smallest float32 range wins; on a tie the static scene, then the smaller m.  Returns t, prim, sem,
    ins, normal3 (a mover's turned into the world) and mover (0 static, m + 1)."""
    t = np.asarray(static["t"], F32).copy()
    out = {"t": t, "prim": np.asarray(static["prim"]).astype(np.uint32).copy(),
           "sem": np.asarray(static["sem"]).astype(np.uint16).copy(), "ins": np.asarray(static["ins"]).astype(np.uint16).copy(),
           "normal3": np.asarray(static["normal3"], F32).copy(), "mover": np.zeros(len(t), np.uint8)}
    for m, c in enumerate(movers):
        tm = np.asarray(c["t"], F32)
        take = tm < out["t"]
        out["t"][take] = tm[take]
        for a in ("prim", "sem", "ins"):
            out[a][take] = np.asarray(c[a])[take].astype(out[a].dtype)
        out["normal3"][take] = to_world(np.asarray(c["normal3"], F32)[take], poses12[m])
        out["mover"][take] = m + 1
    return out


def record(win, rays, centres, max_range, min_range=0.0, incident_mode=0):
    """step 4: the record of (n, 6) world ``rays`` with winners ``win`` (merge) and per-ray float64 filter centres (n, 3)."""
    rays = np.ascontiguousarray(rays, F32)
    n = len(rays)
    o, h = rays[:, :3], unit(rays[:, 3:])
    hit = win["t"] < np.inf
    nm = win["normal3"]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pt = o + h * win["t"][:, None]
        ex = pt.astype(np.float64) - np.asarray(centres, np.float64)
        dist = np.sqrt((ex[:, 0] * ex[:, 0] + ex[:, 1] * ex[:, 1]) + ex[:, 2] * ex[:, 2])
        keep = hit & (dist < max_range)
        if min_range > 0.0:
            keep &= dist >= min_range
        if incident_mode == 1:
            h64, n64 = h.astype(np.float64), nm.astype(np.float64)
            cs = np.abs((h64[:, 0] * n64[:, 0] + h64[:, 1] * n64[:, 1]) + h64[:, 2] * n64[:, 2])
            inc = np.arccos(np.minimum(cs, 1.0)) * RAD2DEG
        else:
            inc = np.arccos(np.abs(ex[:, 2] / dist)) * RAD2DEG
        inten = np.abs(fmaf(h[:, 2], nm[:, 2], fmaf(h[:, 1], nm[:, 1], h[:, 0] * nm[:, 0])))
    z3 = np.zeros((n, 3), F32)
    k3 = keep[:, None]
    return {"t": np.where(keep, win["t"], F32(np.inf)).astype(F32), "prim": np.where(keep, win["prim"], INVALID).astype(np.uint32),
            "normal3": np.where(k3, nm, z3).astype(F32), "point3": np.where(k3, pt, z3).astype(F32),
            "sem": np.where(keep, win["sem"], 0).astype(np.uint16), "ins": np.where(keep, win["ins"], 0).astype(np.uint16),
            "incident_deg": np.where(keep, inc, 0.0), "intensity": np.where(keep, inten, F32(0)).astype(F32),
            "mover": np.where(keep, win["mover"], 0).astype(np.uint8), "keep": keep}


def scan(cast_static, cast_movers, rays, centres, mover_poses12, rays_per_pose, max_range, min_range=0.0, incident_mode=0):
    """P poses of ``rays_per_pose`` world rays each ((P * N, 6) float32, (P * N, 3) centres), M movers given by their cast
    functions and ``mover_poses12`` (P, M, 12).  Returns (record dict over all P * N rays, winners dict before any filter)."""
    rays = np.ascontiguousarray(rays, F32)
    N = int(rays_per_pose)
    P = len(rays) // N
    mp = np.asarray(mover_poses12, F32).reshape(P, len(cast_movers), 12)
    wins = []
    for p in range(P):
        r = rays[p * N:(p + 1) * N]
        wins.append(merge(cast_static(r), [cast(to_object(r, mp[p, m])) for m, cast in enumerate(cast_movers)], mp[p]))
    win = {k: np.concatenate([w[k] for w in wins]) for k in wins[0]}
    return record(win, rays, centres, max_range, min_range, incident_mode), win


# ---- the inputs the issue names -----------------------------------------------------------------------------------------------

def room_mesh():
    from lidarcast import synth
    return synth.make_room(size=(5, 4, 3), num_boxes=4, seed=6, cell=0.25)


def scan_inputs(width=100):
    """The sensor (6 lines x ``width``), its direction table and the three poses: 600 rays per pose at width 100 (tiles of 64
    straddle poses, the last is partial), 768 = 12 whole waves at width 128."""
    from helpers import pose, sensor_small
    from lidar import IndoorLidar
    k = sensor_small(lines=6, width=width)
    dirs = np.ascontiguousarray(IndoorLidar(k, np.eye(4)).sensor_directions(), dtype=np.float64)
    poses = np.stack([pose(1.2, 1.0, 1.0, 0.3), pose(2.5, 2.0, 1.1, -1.0), pose(3.9, 3.1, 0.9, 2.2)])
    return k, dirs, poses


def walker_state(k):
    """(x, y, z, yaw) of the pedestrian in frame k."""
    return 1.8 + 0.5 * k, 2.6 - 0.4 * k, 0.0, 0.4 + 0.7 * k


def baked(room, mover, state):
    """The room with the mover's vertices moved in float64 by (x, y, z, yaw) and its triangles appended: the scene rebuilt
    for one frame.  Returns (vertices, triangles, first row of the mover's triangles)."""
    x, y, z, yaw = state
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    v = np.asarray(mover.vertices, np.float64) @ R.T + np.array([x, y, z])
    verts = np.concatenate([np.asarray(room.vertices, np.float64), v])
    tris = np.concatenate([np.asarray(room.triangles), np.asarray(mover.triangles) + len(room.vertices)]).astype(np.int32)
    return verts, tris, len(room.triangles)
