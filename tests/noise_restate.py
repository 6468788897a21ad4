"""numpy restatement of the seeded sensor noise (include/lidarcast.h "seeded sensor noise", csrc/lrc_noise.h): Philox4x32-10
in uint64 arithmetic, the table lookup of the normal variate, the keep flags, the jittered table rows and the range term --
every operation separately, in the order the header states.  The quantile table is an input (``lidarcast.noise.table()``:
the table in use; tests/test_noise_host.py checks it against the exact quantile on its own)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr (..., 4) and key (..., 2) of 32-bit words -> (..., 4) uint32: ten rounds, the key bumped between rounds."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., j] for j in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        p0 = np.uint64(M0) * c0            # 32 x 32 bits: exact in 64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LOW, (p0 >> S32) ^ c3 ^ k1, p0 & LOW
        k0 = (k0 + np.uint64(W0)) & LOW
        k1 = (k1 + np.uint64(W1)) & LOW
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox4x32_10_inverse(words, key):
    """The counter (..., 4) whose block under key (..., 2) is ``words`` (..., 4): the ten rounds backwards.  A round is a
    bijection of the counter -- its low product words are multiples by odd numbers, undone by the inverses mod 2^32, and the
    high product words then follow from the recovered inputs -- so any four words can be put behind an entry point that takes
    a counter and a key."""
    w = np.asarray(words, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    n0, n1, n2, n3 = (w[..., j] for j in range(4))
    i0, i1 = np.uint64(pow(M0, -1, 1 << 32)), np.uint64(pow(M1, -1, 1 << 32))
    for r in range(9, -1, -1):
        k0 = (key[..., 0] + np.uint64((W0 * r) & 0xFFFFFFFF)) & LOW
        k1 = (key[..., 1] + np.uint64((W1 * r) & 0xFFFFFFFF)) & LOW
        c0 = (n3 * i0) & LOW                 # n3 = low(M0 * c0); 32 x 32 bits: exact in 64
        c2 = (n1 * i1) & LOW
        c1 = n0 ^ ((np.uint64(M1) * c2) >> S32) ^ k0
        c3 = n2 ^ ((np.uint64(M0) * c0) >> S32) ^ k1
        n0, n1, n2, n3 = c0, c1, c2, c3
    return np.stack([n0, n1, n2, n3], axis=-1).astype(np.uint32)


def ray_words(seed, first_frame, P, N):
    """(P, N, 4) uint32: the block of ray i of pose p -- key (seed lo, seed hi), counter (i, frame lo, frame hi, 0) with
    frame = first_frame + p in 64 bits."""
    ctr = np.zeros((P, N, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(N, dtype=np.uint64)[None, :]
    for p in range(P):
        frame = (int(first_frame) + p) & 0xFFFFFFFFFFFFFFFF
        ctr[p, :, 1] = frame & 0xFFFFFFFF
        ctr[p, :, 2] = frame >> 32
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return philox4x32_10(ctr, np.broadcast_to(key, (P, N, 2)))


def fmaf(a, b, c):
    """float32 fused multiply-add of float32 arrays: the product is exact in float64 (24 x 24 bits); the sum is rounded
    to odd in float64 (two-sum gives the exact remainder), which makes the final rounding to float32 the single rounding
    of the exact a*b + c."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0.0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def abs_normal_of(words, base, slope):
    """|z| (float32) of 32-bit words by the segmented quantile table base / slope (24, 64) float32."""
    w = np.asarray(words, dtype=np.uint32)
    r = (w & np.uint32(0x7FFFFFFF)).astype(np.int64)
    small = r < 128
    rr = np.where(small, 128, r)
    L = np.frexp(rr.astype(np.float64))[1].astype(np.int64) - 1          # leading one: exact, rr < 2^53
    sh = L - 6
    below = rr - (np.int64(1) << L)
    c = below >> sh
    e = 30 - L
    f = (below & ((np.int64(1) << sh) - 1)).astype(np.float32) * np.ldexp(np.float32(1.0), -sh).astype(np.float32)
    a = fmaf(f, slope[e, c], base[e, c])
    return np.where(small, base[23, 0], a).astype(np.float32)


def normal_of(words, base, slope):
    """z (float32): the word's top bit set makes it negative."""
    w = np.asarray(words, dtype=np.uint32)
    a = abs_normal_of(w, base, slope)
    return np.where((w >> np.uint32(31)) != 0, -a, a).astype(np.float32)


def drop_threshold(p):
    return min(int(float(p) * 4294967296.0), 0xFFFFFFFF)


def draws(seed, first_frame, P, N, dropout, base, slope):
    """dict z_range, z_az, z_el (P, N) float32 and keep (P, N) bool, as lrc_noise_draws."""
    w = ray_words(seed, first_frame, P, N)
    return {"z_range": normal_of(w[..., 0], base, slope), "z_az": normal_of(w[..., 1], base, slope),
            "z_el": normal_of(w[..., 2], base, slope), "keep": w[..., 3] >= np.uint32(drop_threshold(dropout))}


def jitter_rows(dirs, dp, dt):
    """Table rows (N, 3) float64 moved by azimuth offsets dp and elevation offsets dt (N,) float64 radians."""
    a, b, c = (np.asarray(dirs, dtype=np.float64)[:, j] for j in range(3))
    h = np.sqrt(a * a + b * b)
    flat = h == 0.0
    hs = np.where(flat, 1.0, h)
    ca = (c * a) / hs
    cb = (c * b) / hs
    a1 = (a - dp * b) - dt * ca
    b1 = (b + dp * a) - dt * cb
    c1 = c + dt * h
    n = np.sqrt((a1 * a1 + b1 * b1) + c1 * c1)
    out = np.stack([a1 / n, b1 / n, c1 / n], axis=1)
    out[flat] = np.asarray(dirs, dtype=np.float64)[flat]
    return out


def noisy_rays(poses, dirs, seed, first_frame, range_std, angle_std, dropout, base, slope):
    """What lrc_scan_noisy_dev casts: (rays (P*N, 6) float32 with a NaN direction for a dropped ray, centres (P, 3) float64,
    range term (P*N,) float32 = float32(range_std) * z_range, keep (P*N,) bool, rows (P, N, 3) float64 as rotated)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    dirs = np.asarray(dirs, dtype=np.float64)
    P, N = len(poses), len(dirs)
    d = draws(seed, first_frame, P, N, dropout, base, slope)
    rays = np.empty((P, N, 6), np.float32)
    rows = np.empty((P, N, 3))
    sa = np.float64(angle_std)
    for p, M in enumerate(poses):
        rows[p] = dirs if angle_std == 0 else jitter_rows(dirs, sa * d["z_az"][p].astype(np.float64),
                                                          sa * d["z_el"][p].astype(np.float64))
        rays[p, :, :3] = M[:3, 3].astype(np.float32)
        rays[p, :, 3:] = np.dot(rows[p], M[:3, :3].T).astype(np.float32)      # the BLAS product of IndoorLidar.get_rays
    keep = d["keep"] if dropout != 0 else np.ones((P, N), bool)
    rays[~keep, 3:] = np.nan
    term = np.float32(range_std) * d["z_range"] if range_std != 0 else np.zeros((P, N), np.float32)
    return rays.reshape(P * N, 6), poses[:, :3, 3].copy(), term.reshape(-1).astype(np.float32), keep.reshape(-1), rows
