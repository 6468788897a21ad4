"""numpy restatement of the material chain of lrc_scan_materials_* (include/lidarcast.h "surface materials").  Written from
the header's text, not from csrc/lrc_material.h: the tests compare the two.  It takes any "cast these rays" function -- the
CPU oracle on the host, the explicit-ray cast on the GPU -- that maps (n, 6) float32 rays to a dict of per-ray t (+inf: a miss),
prim, sem, ins, normal3, point3 and intensity, nothing filtered."""
import numpy as np

RAD2DEG = 57.29577951308232
INVALID = np.uint32(0xFFFFFFFF)
SKIN = np.float32(2.0 ** -10)
DIFFUSE, GLASS, MIRROR = 0, 1, 2
RECORD = np.dtype([("kind", np.uint32), ("albedo", np.float32), ("pass", np.float32), ("retro_cos", np.float32)])


def records(num_classes, **classes):
    """(num_classes,) RECORD, every class diffuse with albedo 1 except ``s<id>=(kind, albedo, pass, retro_cos)``."""
    rec = np.zeros(num_classes, RECORD)
    rec["albedo"] = 1.0
    for name, spec in classes.items():
        rec[int(name[1:])] = spec
    return rec


def unit(d):
    """d / |d|, float32, one rounding per operation."""
    d = np.asarray(d, np.float32)
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return d / nrm[:, None]


def record_of(rec, sem):
    """per ray (kind, albedo, pass, retro_cos): an id at or above len(rec) is diffuse with albedo 1."""
    sem = np.asarray(sem).astype(np.int64)
    inside = sem < len(rec)
    r = rec[np.where(inside, sem, 0)]
    kind = np.where(inside, r["kind"], DIFFUSE).astype(np.uint32)
    albedo = np.where(inside, r["albedo"], np.float32(1.0)).astype(np.float32)
    return kind, albedo, r["pass"].astype(np.float32), r["retro_cos"].astype(np.float32)


def chain(cast, rays, rec, max_bounces, min_intensity=0.0):
    """The chains of (n, 6) float32 rays.  Returns a dict: ``ret`` (bool: the ray has a return, before any range filter), ``T``,
    ``I``, ``b`` (uint8, the bounces so far whatever the end), ``surface`` (the last pp), ``prim`` / ``sem`` / ``ins`` /
    ``normal3`` of the final surface, ``capped`` (bool: cut at max_bounces), ``first_continues`` (bool: the first surface sent
    the ray on, or would have but for the cap) and ``segments``: per segment the indices of the rays that were pending, their
    state before it and the cast's columns -- what a per-segment step needs."""
    rays = np.ascontiguousarray(rays, np.float32)
    n = len(rays)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    T, g = np.zeros(n, np.float32), np.ones(n, np.float32)
    b = np.zeros(n, np.uint8)
    pend = np.ones(n, bool)
    out = {"ret": np.zeros(n, bool), "I": np.zeros(n, np.float32), "surface": np.zeros((n, 3), np.float32),
           "prim": np.full(n, INVALID, np.uint32), "sem": np.zeros(n, np.uint16), "ins": np.zeros(n, np.uint16),
           "normal3": np.zeros((n, 3), np.float32), "capped": np.zeros(n, bool), "first_continues": np.zeros(n, bool),
           "segments": []}
    min_intensity = np.float32(min_intensity)
    k = 0
    while pend.any():
        idx = np.flatnonzero(pend)
        c = cast(np.concatenate([o[idx], d[idx]], axis=1))
        t = np.asarray(c["t"], np.float32)
        out["segments"].append({"idx": idx, "o": o[idx].copy(), "d": d[idx].copy(), "T": T[idx].copy(), "g": g[idx].copy(),
                                "b": b[idx].copy(), "t": t.copy(), "sem": np.asarray(c["sem"]).astype(np.uint16),
                                "normal3": np.asarray(c["normal3"], np.float32).copy()})
        hit = t < np.inf
        pend[idx[~hit]] = False                                    # 1: a miss, no return
        idx, t = idx[hit], t[hit]
        nm = np.asarray(c["normal3"], np.float32)[hit]
        pp = np.asarray(c["point3"], np.float32)[hit]              # 2: pp = o + h * t, as the cast forms point3
        cs = np.asarray(c["intensity"], np.float32)[hit]           #    c = |fma(hz, nz, fma(hy, ny, hx * nx))|, the cast's intensity
        h = unit(d[idx])
        T[idx] = T[idx] + t
        kind, albedo, pas, retro = record_of(rec, np.asarray(c["sem"])[hit])
        own = (kind == DIFFUSE) | (cs >= retro)                    # 3: the surface returns
        r = idx[own]
        out["ret"][r] = True
        out["I"][r] = (g[r] * albedo[own]) * cs[own]
        out["surface"][r] = pp[own]
        for a in ("prim", "sem", "ins"):
            out[a][r] = np.asarray(c[a])[hit][own].astype(out[a].dtype)
        out["normal3"][r] = nm[own]
        pend[r] = False
        if k == 0:
            out["first_continues"][idx[~own]] = True
        go = ~own
        cap = go & (b[idx] == max_bounces)                         # 4: the cap
        out["capped"][idx[cap]] = True
        pend[idx[cap]] = False
        go &= ~cap
        j = idx[go]
        b[j] += 1
        g[j] = g[j] * pas[go]
        hg, ng = h[go], nm[go]
        dn = (hg[:, 0] * ng[:, 0] + hg[:, 1] * ng[:, 1]) + hg[:, 2] * ng[:, 2]
        s = dn + dn
        mirror = (kind[go] == MIRROR)[:, None]
        d[j] = np.where(mirror, hg - s[:, None] * ng, d[j])
        o[j] = pp[go] + unit(d[j]) * SKIN
        T[j] = T[j] + SKIN
        k += 1
    weak = out["ret"] & (out["I"] < min_intensity)                  # 5: too weak a return is no return
    out["ret"] &= ~weak
    out["T"], out["b"] = T, b
    return out


def assemble(ch, rays, centres, max_range, min_range=0.0):
    """The records of chains ``ch`` of ``rays`` (n, 6) with per-ray float64 range-filter centres (n, 3): what the scan writes.
    A return lies on the original beam at the total path length; the range filter uses that point."""
    rays = np.ascontiguousarray(rays, np.float32)
    n = len(rays)
    o, h = rays[:, :3], unit(rays[:, 3:])
    with np.errstate(invalid="ignore", over="ignore"):
        pt = o + h * ch["T"][:, None]
        ex = pt.astype(np.float64) - np.asarray(centres, np.float64)
        dist = np.sqrt((ex[:, 0] * ex[:, 0] + ex[:, 1] * ex[:, 1]) + ex[:, 2] * ex[:, 2])
        keep = ch["ret"] & (dist < max_range)
        if min_range > 0.0:
            keep &= dist >= min_range
        inc = np.arccos(np.abs(ex[:, 2] / dist)) * RAD2DEG
    z3 = np.zeros((n, 3), np.float32)
    k3 = keep[:, None]
    return {"t": np.where(keep, ch["T"], np.float32(np.inf)).astype(np.float32),
            "prim": np.where(keep, ch["prim"], INVALID).astype(np.uint32),
            "normal3": np.where(k3, ch["normal3"], z3), "point3": np.where(k3, pt, z3).astype(np.float32),
            "sem": np.where(keep, ch["sem"], 0).astype(np.uint16), "ins": np.where(keep, ch["ins"], 0).astype(np.uint16),
            "incident_deg": np.where(keep, inc, 0.0), "intensity": np.where(keep, ch["I"], np.float32(0)).astype(np.float32),
            "bounces": np.where(keep, ch["b"], 0).astype(np.uint8), "surface_point3": np.where(k3, ch["surface"], z3),
            "keep": keep}


# ---- the inputs the issue names -----------------------------------------------------------------------------------------------

def _quad(p0, eu, ev):
    p0, eu, ev = (np.asarray(a, np.float64) for a in (p0, eu, ev))
    return np.stack([p0, p0 + eu, p0 + eu + ev, p0 + ev]), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def _box(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    e = hi - lo
    ex, ey, ez = (np.array(v) * e for v in ((1, 0, 0), (0, 1, 0), (0, 0, 1)))
    return [_quad(lo, ex, ey), _quad(lo + ez, ex, ey), _quad(lo, ex, ez), _quad(lo + ey, ex, ez), _quad(lo, ey, ez),
            _quad(lo + ex, ey, ez)]


def pane_scene():
    """30 triangles: a closed box (0,0,0)-(4,3,2.5), sem 2; a glass quad at x = 2.0 over y 0.5-2.5 and z 0.3-2.2, sem 5; two
    facing mirror quads at y = 2.99 and y = 0.01 over x 0.3-1.7 and z 0.5-2.0, sem 11; a box (2.8,1.0,0)-(3.4,1.8,0.9) behind
    the glass, sem 7.  Returns (TriangleMesh with labels, the same mesh without the glass pane)."""
    from lidarcast.synth import TriangleMesh
    parts = [(q, 2) for q in _box((0, 0, 0), (4, 3, 2.5))]
    parts.append((_quad((2.0, 0.5, 0.3), (0, 2.0, 0), (0, 0, 1.9)), 5))
    parts.append((_quad((0.3, 2.99, 0.5), (1.4, 0, 0), (0, 0, 1.5)), 11))
    parts.append((_quad((0.3, 0.01, 0.5), (1.4, 0, 0), (0, 0, 1.5)), 11))
    parts += [(q, 7) for q in _box((2.8, 1.0, 0), (3.4, 1.8, 0.9))]

    def mesh(ps):
        v, t, s = [], [], []
        for (qv, qt), sem in ps:
            t.append(qt + 4 * len(v))
            v.append(qv)
            s += [sem, sem]
        sem = np.array(s, np.uint16)
        return TriangleMesh(vertices=np.concatenate(v), triangles=np.concatenate(t).astype(np.int32), triangle_sem=sem,
                            triangle_ins=np.arange(1, len(sem) + 1, dtype=np.uint16) // 2)
    return mesh(parts), mesh([p for p in parts if p[1] != 5])


def bounce_histogram(asm, max_bounces):
    """returns per bounce count 0..max_bounces among the kept rays."""
    return np.bincount(asm["bounces"][asm["keep"]], minlength=max_bounces + 1)


def tile_variety(asm, ch, tile=64):
    """the largest number of different bounce counts among the returns of one aligned run of ``tile`` rays."""
    b = np.where(asm["keep"], ch["b"].astype(np.int64), -1)
    best = 0
    for a in range(0, len(b), tile):
        best = max(best, len(set(b[a:a + tile].tolist()) - {-1}))
    return best


def scan_inputs(width=100):
    """The sensor (8 lines x ``width``), its direction table and the three poses of the tests: 800 rays per pose at width 100,
    12.5 tiles of 64, so tiles straddle poses and the last one is partial."""
    from helpers import pose, sensor_small
    from lidar import IndoorLidar
    k = sensor_small(8, width)
    dirs = np.ascontiguousarray(IndoorLidar(k, np.eye(4)).sensor_directions(), dtype=np.float64)
    poses = np.stack([pose(1.0, 1.2, 1.0), pose(1.3, 1.6, 1.1, yaw=0.7), pose(0.6, 1.5, 1.2, yaw=2.0)])
    return k, dirs, poses


def pane_records(retro_cos=0.999):
    """window (5) glass, board (11) mirror"""
    return records(12, s5=(GLASS, 0.1, 0.9, retro_cos), s11=(MIRROR, 0.05, 0.95, retro_cos))


def room_records(retro_cos=0.995):
    """bookcase (10) glass, table (7) mirror: the classes the synthetic room has"""
    return records(12, s10=(GLASS, 0.1, 0.9, retro_cos), s7=(MIRROR, 0.05, 0.95, retro_cos))


def room_mesh():
    from lidarcast import synth
    return synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)
