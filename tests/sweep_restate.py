"""numpy restatement of the moving-sensor sweep rays (include/lidarcast.h "moving-sensor sweeps", csrc/lrc_device.h
gen_ray_sweep): every float64 operation separately, in the order the header states.  numpy never fuses, and the device
file is built with -ffp-contract=off, so the two agree bit for bit."""
import numpy as np


def sweep_rays(motion, dirs, fire):
    """(P*N, 6) float32 rays (origin | direction) and (P*N, 3) float64 range-filter centres of the sweeps ``motion``
    (P, 24) over the direction table ``dirs`` (N, 3) float64 with firing fractions ``fire`` (N,)."""
    motion = np.asarray(motion, dtype=np.float64).reshape(-1, 24)
    dirs = np.asarray(dirs, dtype=np.float64)
    s = np.asarray(fire, dtype=np.float64).reshape(1, -1)
    P, N = len(motion), len(dirs)
    rays = np.empty((P, N, 6), np.float32)
    centres = np.empty((P, N, 3))
    for k, M in enumerate(motion):
        R = np.stack([M[0:3], M[4:7], M[8:11]])
        v = np.dot(dirs, R.T)                  # the BLAS product of IndoorLidar.get_rays (= dgemm_row)
        vx, vy, vz = v[:, 0][None], v[:, 1][None], v[:, 2][None]
        qw = (1.0 - s) + s * M[12]
        ux, uy, uz = s * M[13], s * M[14], s * M[15]
        n = ((qw * qw + ux * ux) + uy * uy) + uz * uz
        kk = 2.0 / n
        tx, ty, tz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        wx, wy, wz = uy * tz - uz * ty, uz * tx - ux * tz, ux * ty - uy * tx
        d = np.stack([vx + kk * (qw * tx + wx), vy + kk * (qw * ty + wy), vz + kk * (qw * tz + wz)], -1)[0]
        c = np.empty((N, 3))
        for j, (c0, dc) in enumerate(((M[3], M[16]), (M[7], M[17]), (M[11], M[18]))):
            cs = s[0] * dc
            c[:, j] = np.where(cs == 0.0, c0, c0 + cs)
        rays[k, :, :3] = c.astype(np.float32)
        rays[k, :, 3:] = d.astype(np.float32)
        centres[k] = c
    return rays.reshape(P * N, 6), centres.reshape(P * N, 3)


def quat_matrix(q):
    """3x3 rotation of the unit quaternion (w, x, y, z)."""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def slerp_rotation(dq, s):
    """R(dq)^s: the constant-rate rotation by the fraction s of dq's angle about dq's axis."""
    w, v = dq[0], np.asarray(dq[1:], dtype=np.float64)
    sn = np.linalg.norm(v)
    if sn == 0.0:
        return np.eye(3)
    ang = 2.0 * np.arctan2(sn, w)
    a = s * ang / 2.0
    return quat_matrix((np.cos(a), *(np.sin(a) * v / sn)))


def exact_sweep_rays(motion, dirs, fire):
    """(P*N, 6) float64 rays of the sweeps with the slerp-exact pose of each ray: what the nlerp rays approximate."""
    motion = np.asarray(motion, dtype=np.float64).reshape(-1, 24)
    dirs = np.asarray(dirs, dtype=np.float64)
    fire = np.asarray(fire, dtype=np.float64)
    out = np.empty((len(motion), len(dirs), 6))
    cols = np.unique(fire)
    for k, M in enumerate(motion):
        R0 = np.stack([M[0:3], M[4:7], M[8:11]])
        c0, dc = M[[3, 7, 11]], M[16:19]
        for s in cols:
            m = fire == s
            out[k, m, :3] = c0 + s * dc
            out[k, m, 3:] = dirs[m] @ (slerp_rotation(M[12:16], s) @ R0).T
    return out.reshape(-1, 6)
