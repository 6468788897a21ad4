"""Seeded procedural room meshes standing in for NKSR reconstructions of S3DIS rooms.

No S3DIS data or reconstructed mesh exists in the build container or on the GPU box, so the
benchmark scenes are generated: an inward-facing room box plus furniture
boxes, every face tessellated on a 2 cm grid (the reference reconstructs with voxel_size=0.02,
s3dis_nksr_reconstructor.py:75) into two triangles per cell, vertices jittered by N(0, 2 mm),
triangle rows shuffled (NKSR output is not spatially sorted).  Per-triangle semantic ids follow the
S3DIS class list used by the reference (s3dis_annotation_loader.py:51-65): 0 ceiling, 1 floor,
2 wall, 7 table, 8 chair, 10 bookcase.
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class TriangleMesh:
    """Minimal stand-in for open3d.geometry.TriangleMesh (legacy): float64 vertices, int32 triangles."""
    vertices: np.ndarray
    triangles: np.ndarray
    triangle_sem: np.ndarray = None
    triangle_ins: np.ndarray = None

    def __len__(self):
        return len(self.triangles)


def _grid_face(origin, eu, ev, lu, lv, cell, flip, rng=None):
    """Tessellate the rectangle origin + s*eu + t*ev (0<=s<=lu, 0<=t<=lv) into 2 triangles per cell.  With ``rng`` the
    diagonal of every cell is chosen at random (irregular connectivity)."""
    nu, nv = max(1, int(round(lu / cell))), max(1, int(round(lv / cell)))
    s = np.linspace(0.0, lu, nu + 1)
    t = np.linspace(0.0, lv, nv + 1)
    S, T = np.meshgrid(s, t, indexing="ij")
    verts = origin[None, :] + S.reshape(-1, 1) * eu[None, :] + T.reshape(-1, 1) * ev[None, :]
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a = (i * (nv + 1) + j).reshape(-1)
    b = a + (nv + 1)
    c = b + 1
    d = a + 1
    if rng is None:
        tri = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 0)
    else:
        other = rng.random(len(a)) < 0.5                  # the other diagonal: (a,b,d), (b,c,d)
        t1 = np.where(other[:, None], np.stack([a, b, d], 1), np.stack([a, b, c], 1))
        t2 = np.where(other[:, None], np.stack([b, c, d], 1), np.stack([a, c, d], 1))
        tri = np.concatenate([t1, t2], 0)
    if flip:
        tri = tri[:, ::-1]
    return verts, tri


def _box_faces(lo, hi, cell, inward, rng=None):
    """Six tessellated faces of an axis-aligned box; yields (verts, tris, face_id 0..5 = -x,+x,-y,+y,-z,+z)."""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    ext = hi - lo
    E = np.eye(3)
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            origin = lo.copy()
            if side:
                origin[axis] = hi[axis]
            # outward normal of the (eu, ev) grid is +axis when (u, v, axis) is a right-handed cycle
            flip = (side == 0) != inward
            yield _grid_face(origin, E[u], E[v], ext[u], ext[v], cell, flip, rng) + (2 * axis + side,)


def make_room(size=(5.0, 4.0, 3.0), num_boxes=8, seed=6, cell=0.02, jitter=0.002, corridor=0.6, rough=False):
    """Room of ``size`` with ``num_boxes`` furniture boxes kept clear of the line y = size_y/2 (the
    benchmark trajectory) by ``corridor`` metres on each side.  Deterministic in ``seed``.

    ``rough=True`` makes the unfriendly variant of the same room (what an NKSR reconstruction looks like rather than
    a CAD model): every object tessellated at its own cell size (shell 2.5 cm, furniture 1.5-4 cm: mixed triangle
    sizes), the diagonal of every cell chosen at random, coincident vertices of adjacent faces WELDED (one vertex
    row, so the room shell is a closed manifold: no seams), every vertex moved by up to 0.3 cell in a random 3-D
    direction (irregular shapes and sizes) and the whole surface displaced by a smooth cm-scale noise field (non-planar
    walls); ``jitter`` is ignored."""
    rng = np.random.default_rng(seed)
    frng = rng if rough else None
    vcell = []                                     # rough: cell size of the object each vertex came from
    Lx, Ly, Lz = size
    verts, tris, sem, ins = [], [], [], []
    base = 0

    def add(v, t, s, inst, c=cell):
        nonlocal base
        verts.append(v)
        vcell.append(np.full(len(v), c))
        tris.append(t + base)
        sem.append(np.full(len(t), s, np.uint16))
        ins.append(np.full(len(t), inst, np.uint16))
        base += len(v)

    face_sem = {0: 2, 1: 2, 2: 2, 3: 2, 4: 1, 5: 0}   # walls, floor (-z), ceiling (+z)
    shell_cell = 0.025 if rough else cell
    for v, t, fid in _box_faces((0, 0, 0), (Lx, Ly, Lz), shell_cell, inward=True, rng=frng):
        add(v, t, face_sem[fid], {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6}[fid], shell_cell)

    kinds = [(7, (0.8, 1.6), (0.6, 0.9), (0.70, 0.80)),    # table
             (8, (0.4, 0.5), (0.4, 0.5), (0.45, 0.90)),    # chair
             (10, (0.8, 1.2), (0.3, 0.4), (1.6, 2.0))]     # bookcase
    placed = []
    inst = 7
    tries = 0
    while len(placed) < num_boxes and tries < 10000:
        tries += 1
        s, rx, ry, rz = kinds[int(rng.integers(len(kinds)))]
        wx, wy, wz = rng.uniform(*rx), rng.uniform(*ry), rng.uniform(*rz)
        if rng.random() < 0.5:
            wx, wy = wy, wx
        # snap sizes to the grid so that every face tessellates into whole cells
        wx, wy, wz = (max(cell, round(w / cell) * cell) for w in (wx, wy, wz))
        x0 = round(rng.uniform(0.1, Lx - wx - 0.1) / cell) * cell
        side = rng.random() < 0.5
        y_lo, y_hi = (0.1, Ly / 2 - corridor - wy) if side else (Ly / 2 + corridor, Ly - wy - 0.1)
        if y_hi <= y_lo:
            continue
        y0 = round(rng.uniform(y_lo, y_hi) / cell) * cell
        lo, hi = np.array([x0, y0, 0.0]), np.array([x0 + wx, y0 + wy, wz])
        if any(np.all(lo < phi + 0.05) and np.all(plo < hi + 0.05) for plo, phi in placed):
            continue
        placed.append((lo, hi))
        bcell = cell
        if rough:                                  # a cell size of this object's own that divides its extents
            bcell = float(rng.choice([0.015, 0.02, 0.03, 0.04]))
            hi = lo + np.maximum(np.round((hi - lo) / bcell), 1) * bcell
        for v, t, fid in _box_faces(lo, hi, bcell, inward=False, rng=frng):
            if fid == 4:
                continue   # bottom face rests on the floor
            add(v, t, s, inst, bcell)
        inst += 1

    V = np.concatenate(verts, 0)
    F = np.concatenate(tris, 0)
    S = np.concatenate(sem, 0)
    I = np.concatenate(ins, 0)
    if rough:
        # weld: vertices of adjacent faces that coincide become one row (the shell is then a closed manifold)
        key = np.round(V / 1e-6).astype(np.int64)
        _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
        V, C = V[first], np.concatenate(vcell)[first]
        F = inv.reshape(-1)[F]
        # irregular triangles: every vertex moves by up to 0.3 of its object's cell in a random 3-D direction
        V = V + rng.uniform(-0.3, 0.3, V.shape) * C[:, None]
        # non-planar surfaces: a smooth displacement field, six plane waves of 20-70 cm wavelength, ~1 cm amplitude
        for _ in range(6):
            kvec = rng.normal(size=3)
            kvec *= 2 * np.pi / rng.uniform(0.2, 0.7) / np.linalg.norm(kvec)
            amp = rng.normal(size=3)
            amp *= rng.uniform(0.002, 0.006) / np.linalg.norm(amp)
            V = V + np.sin(V @ kvec + rng.uniform(0, 2 * np.pi))[:, None] * amp[None, :]
    elif jitter > 0:
        V = V + rng.normal(0.0, jitter, V.shape)
    perm = rng.permutation(len(F))
    return TriangleMesh(vertices=np.ascontiguousarray(V, dtype=np.float64),
                        triangles=np.ascontiguousarray(F[perm], dtype=np.int32),
                        triangle_sem=S[perm], triangle_ins=I[perm])


# named stand-ins used by bench.py / tests (sizes and seeds from SURVEY.md section 8(d))
SCENES = {
    "synth_A1_office":  dict(size=(8.0, 6.0, 3.0), num_boxes=12, seed=1),
    "synth_A2_office":  dict(size=(6.0, 5.0, 3.0), num_boxes=10, seed=2),
    "synth_A3_office":  dict(size=(4.0, 4.0, 3.0), num_boxes=6, seed=3),
    "synth_A4_office":  dict(size=(7.0, 4.0, 3.0), num_boxes=9, seed=4),
    "synth_A5_office":  dict(size=(6.0, 6.0, 3.0), num_boxes=11, seed=5),
    "synth_A6_office2": dict(size=(5.0, 4.0, 3.0), num_boxes=8, seed=6),
}
# the same rooms, unfriendly: welded, non-planar, irregular and mixed triangle sizes (see make_room(rough=True))
ROUGH_SCENES = {
    "synth_rough_A1": dict(size=(8.0, 6.0, 3.0), num_boxes=12, seed=1, rough=True),
    "synth_rough_A6": dict(size=(5.0, 4.0, 3.0), num_boxes=8, seed=6, rough=True),
}


# a large hall (~3 M triangles, ~0.3 GB of scene data: past the 256 MiB Infinity Cache) for the regime where the scene no
# longer sits in cache; not one of the BASELINE scenes
EXTRA_SCENES = {
    "synth_hall": dict(size=(16.0, 12.0, 3.0), num_boxes=40, seed=11),
}


def _spec(name):
    return ROUGH_SCENES.get(name) or EXTRA_SCENES.get(name) or SCENES[name]


def make_scene(name, cell=0.02):
    return make_room(cell=cell, **_spec(name))


def scene_size(name):
    return _spec(name)["size"]


def unit_cube(lo=-1.0, hi=1.0):
    """12-triangle cube with inward-facing winding (known-answer scene)."""
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], dtype=np.float64)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = []
    for a, b, c, d in q:
        f += [(a, b, c), (a, c, d)]
    return TriangleMesh(vertices=v, triangles=np.array(f, dtype=np.int32))


def make_pedestrian(height=1.7, radius=0.25, segments=16, rings=8, semantic=13, instance=1):
    """A standing person as a closed prism: ``segments`` sides, ``rings`` bands over the height, a fan at each end --
    2 * segments * rings + 2 * segments triangles (288 by default), wound outward.  Feet at z = 0, standing on its own origin:
    a mover mesh (lidarcast.movers).  Every triangle carries ``semantic`` (default 13: one past the S3DIS class list) and ``instance``."""
    segments, rings = int(segments), int(rings)
    if segments < 3 or rings < 1:
        raise ValueError("a pedestrian needs at least 3 segments and 1 ring")
    ang = 2.0 * np.pi * np.arange(segments) / segments
    z = np.linspace(0.0, float(height), rings + 1)
    ring = np.stack([radius * np.cos(ang), radius * np.sin(ang)], 1)
    v = np.concatenate([np.concatenate([ring, np.full((segments, 1), zk)], 1) for zk in z] +
                       [np.array([[0.0, 0.0, 0.0], [0.0, 0.0, float(height)]])], 0)
    bottom, top = segments * (rings + 1), segments * (rings + 1) + 1
    t = []
    for k in range(rings):
        for j in range(segments):
            a, b = k * segments + j, k * segments + (j + 1) % segments
            c, d = a + segments, b + segments
            t += [(a, b, d), (a, d, c)]
    for j in range(segments):
        a, b = j, (j + 1) % segments
        t.append((bottom, b, a))
        t.append((top, rings * segments + a, rings * segments + b))
    t = np.array(t, dtype=np.int32)
    return TriangleMesh(vertices=v.astype(np.float64), triangles=t, triangle_sem=np.full(len(t), semantic, np.uint16),
                        triangle_ins=np.full(len(t), instance, np.uint16))


def _prism(cx, cy, z0, z1, rx, ry, segments, rings):
    """A closed elliptic prism about the vertical through (cx, cy) from z0 to z1, wound outward: the topology of
    ``make_pedestrian`` (2 * segments * rings + 2 * segments triangles).  Returns (float64 vertices, int32 triangles)."""
    ang = 2.0 * np.pi * np.arange(segments) / segments
    ring = np.stack([cx + rx * np.cos(ang), cy + ry * np.sin(ang)], 1)
    v = np.concatenate([np.concatenate([ring, np.full((segments, 1), zk)], 1) for zk in np.linspace(z0, z1, rings + 1)] +
                       [np.array([[cx, cy, z0], [cx, cy, z1]])], 0)
    bottom, top = segments * (rings + 1), segments * (rings + 1) + 1
    t = []
    for k in range(rings):
        for j in range(segments):
            a, b = k * segments + j, k * segments + (j + 1) % segments
            t += [(a, b, b + segments), (a, b + segments, a + segments)]
    for j in range(segments):
        a, b = j, (j + 1) % segments
        t += [(bottom, b, a), (top, rings * segments + a, rings * segments + b)]
    return v, np.array(t, dtype=np.int32)


def _walker_rest(H):
    """The walker at rest: (float64 vertices, int32 triangles, per vertex the pivot height, the swing sign and the part: 0 torso,
    1 head, 2 left leg, 3 right leg, 4 left arm, 5 right arm), and nothing else; ``make_walker`` and ``make_walker_rig`` share it."""
    seg = 8
    # (centre x, y, z0, z1, radius x, y, rings, pivot height or None, swing sign)
    parts = [(0.0, 0.0, 0.50 * H, 0.85 * H, 0.07 * H, 0.12 * H, 4, None, 0.0),            # torso
             (0.0, 0.0, 0.87 * H, 1.00 * H, 0.06 * H, 0.06 * H, 2, None, 0.0),            # head
             (0.0, 0.06 * H, 0.0, 0.50 * H, 0.045 * H, 0.045 * H, 3, 0.50 * H, 1.0),      # left leg
             (0.0, -0.06 * H, 0.0, 0.50 * H, 0.045 * H, 0.045 * H, 3, 0.50 * H, -1.0),    # right leg
             (0.0, 0.155 * H, 0.47 * H, 0.83 * H, 0.03 * H, 0.03 * H, 3, 0.83 * H, -1.0),  # left arm
             (0.0, -0.155 * H, 0.47 * H, 0.83 * H, 0.03 * H, 0.03 * H, 3, 0.83 * H, 1.0)]  # right arm
    verts, tris, pivot, sign, part, base = [], [], [], [], [], 0
    for n, (cx, cy, z0, z1, rx, ry, rings, pz, sg) in enumerate(parts):
        v, t = _prism(cx, cy, z0, z1, rx, ry, seg, rings)
        verts.append(v)
        tris.append(t + base)
        pivot.append(np.full(len(v), z0 if pz is None else pz))
        sign.append(np.full(len(v), sg))
        part.append(np.full(len(v), n))
        base += len(v)
    return np.concatenate(verts, 0), np.concatenate(tris, 0), np.concatenate(pivot), np.concatenate(sign), np.concatenate(part)


def make_walker(height=1.7, keyframes=8, swing_deg=25, semantic=13, instance=1):
    """A walking person for ``lidarcast.deform``: torso, head, two legs and two arms as closed eight-sided prisms (384
    triangles), facing +x, feet at z = 0, standing on its own origin.  Keyframe k of ``keyframes`` turns the legs about the hip
    axis and the arms about the shoulder axis (both along y) by swing_deg * sin(2 pi k / keyframes), the left leg and the right
    arm one way, the right leg and the left arm the other; every keyframe is then lowered so that its lowest vertex stays at
    z = 0.  Computed in float64 and narrowed to float32.  Returns the ``TriangleMesh`` of keyframe 0 (its vertices are keyframe
    0's float32 values) with ``keyframes``, the (K, V, 3) float32 array, as an attribute; the topology is the same in every
    keyframe."""
    K, H = int(keyframes), float(height)
    if K < 1 or not H > 0.0:
        raise ValueError("a walker needs at least one keyframe and a positive height")
    v0, t, pivot, sign, _ = _walker_rest(H)
    keys = np.empty((K, len(v0), 3), np.float64)
    for k in range(K):
        a = sign * np.deg2rad(float(swing_deg)) * np.sin(2.0 * np.pi * k / K)
        c, s = np.cos(a), np.sin(a)
        dz = v0[:, 2] - pivot
        keys[k, :, 0] = v0[:, 0] * c + dz * s
        keys[k, :, 1] = v0[:, 1]
        keys[k, :, 2] = pivot - v0[:, 0] * s + dz * c
        keys[k, :, 2] -= keys[k, :, 2].min()
    keys = keys.astype(np.float32)
    mesh = TriangleMesh(vertices=keys[0].astype(np.float64), triangles=t, triangle_sem=np.full(len(t), semantic, np.uint16),
                        triangle_ins=np.full(len(t), instance, np.uint16))
    mesh.keyframes = keys
    return mesh


def make_walker_rig(height=1.7, keyframes=8, swing_deg=25, smooth=0.0, semantic=13, instance=1):
    """``make_walker`` as a skinned rig for ``lidarcast.deform.SkinnedDeformable``: the ``TriangleMesh`` of the walker at rest
    (``make_walker``'s keyframe 0: no swing) carrying ``skeleton`` (a ``lidarcast.skin.Skeleton`` of six bones: torso, head, left
    leg, right leg, left arm, right arm; the torso is the root, the limbs turn about the hip and shoulder pivots),
    ``bone_index`` (V, 4) uint8, ``bone_weight`` (V, 4) float32 and ``poses12`` (K, 6, 12) float32.  Key pose k turns the limbs as
    ``make_walker``'s keyframe k does and lowers the whole body by a root translation, as ``make_walker`` lowers its keyframe, so
    that the lowest vertex stays on the floor.  With ``smooth`` = 0 every vertex has one influence of weight 1 and the skinned
    key poses are ``make_walker``'s keyframes up to float32 rounding; with ``smooth`` > 0 a limb vertex closer than ``smooth``
    metres to its limb's pivot shares its weight linearly with the torso (distance / smooth to the limb, the rest to the torso)."""
    from .skin import Skeleton
    K, H, smooth = int(keyframes), float(height), float(smooth)
    if K < 1 or not H > 0.0:
        raise ValueError("a walker needs at least one keyframe and a positive height")
    if not smooth >= 0.0:
        raise ValueError("smooth is a distance in metres, >= 0")
    v0, t, pivot, sign, part = _walker_rest(H)
    rest = v0.astype(np.float32)
    joints = np.array([[0.0, 0.0, 0.50 * H], [0.0, 0.0, 0.87 * H], [0.0, 0.06 * H, 0.50 * H], [0.0, -0.06 * H, 0.50 * H],
                       [0.0, 0.155 * H, 0.83 * H], [0.0, -0.155 * H, 0.83 * H]])
    swing = np.array([0.0, 0.0, 1.0, -1.0, -1.0, 1.0])
    skeleton = Skeleton([-1, 0, 0, 0, 0, 0], joints)
    rot = np.zeros((K, 6, 3, 3))
    drop = np.zeros((K, 3))
    for k in range(K):
        a = swing * np.deg2rad(float(swing_deg)) * np.sin(2.0 * np.pi * k / K)
        c, s = np.cos(a), np.sin(a)
        rot[k, :, 0, 0], rot[k, :, 0, 2], rot[k, :, 1, 1], rot[k, :, 2, 0], rot[k, :, 2, 2] = c, s, 1.0, -s, c
        av = sign * np.deg2rad(float(swing_deg)) * np.sin(2.0 * np.pi * k / K)          # make_walker's own lowest vertex
        drop[k, 2] = -(pivot - v0[:, 0] * np.sin(av) + (v0[:, 2] - pivot) * np.cos(av)).min()
    index = np.zeros((len(rest), 4), np.uint8)
    weight = np.zeros((len(rest), 4), np.float32)
    index[:, 0] = part
    weight[:, 0] = 1.0
    if smooth > 0.0:
        dist = np.linalg.norm(v0 - joints[part], axis=1)
        near = (part >= 2) & (dist < smooth)
        share = (dist[near] / smooth).astype(np.float32)
        weight[near, 0] = share
        weight[near, 1] = np.float32(1.0) - share          # index 0 in column 1: the torso
    mesh = TriangleMesh(vertices=rest.astype(np.float64), triangles=t, triangle_sem=np.full(len(t), semantic, np.uint16),
                        triangle_ins=np.full(len(t), instance, np.uint16))
    mesh.skeleton, mesh.bone_index, mesh.bone_weight = skeleton, index, weight
    mesh.poses12 = skeleton.matrices(rot, root_translation=drop)
    return mesh


def quad(z=2.0, half=1.0):
    """Two triangles forming the square |x|,|y| <= half in the plane z."""
    v = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], dtype=np.float64)
    return TriangleMesh(vertices=v, triangles=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))


# colour per S3DIS class id of make_room's triangles (0 ceiling, 1 floor, 2 wall, 7 table, 8 chair, 10 bookcase)
_ROOM_RGB = {0: (231, 229, 222), 1: (142, 128, 110), 2: (205, 201, 190), 7: (120, 84, 52), 8: (60, 62, 70),
             10: (170, 132, 90)}


def sample_s3dis_room(mesh=None, density=15000.0, num_points=None, num_outliers=300, seed=0, return_instances=False):
    """An S3DIS-like room scan sampled from a synthetic mesh (make_room() when None): area-uniform points on the
    triangles at `density` points per square metre (or exactly `num_points`), coordinates rounded to 3 decimals as in
    the S3DIS text files (which gives coincident rows and distance ties), uint8-valued colours from the triangle's
    class with a little per-point noise, the triangle's semantic id as label, plus `num_outliers` rows scattered
    uniformly through the room's box (off the surfaces).  Returns (points float64 (N,3), colors float64 (N,3) in
    0..255, labels int64 (N,)), and with return_instances also the triangle's instance id per row (int64 (N,); 0 for the
    scattered rows).  Deterministic in `seed`."""
    if mesh is None:
        mesh = make_room()
    rng = np.random.default_rng(seed)
    v = np.asarray(mesh.vertices, np.float64)
    t = np.asarray(mesh.triangles, np.int64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    n = int(num_points) if num_points is not None else int(round(area.sum() * density))
    tri = np.searchsorted(np.cumsum(area) / area.sum(), rng.random(n), side="right").clip(0, len(t) - 1)
    u, w = rng.random(n), rng.random(n)
    flip = u + w > 1.0
    u[flip], w[flip] = 1.0 - u[flip], 1.0 - w[flip]
    pts = a[tri] + u[:, None] * (b[tri] - a[tri]) + w[:, None] * (c[tri] - a[tri])
    sem = (np.asarray(mesh.triangle_sem, np.int64)[tri] if mesh.triangle_sem is not None
           else np.zeros(n, np.int64))
    lo, hi = v.min(0), v.max(0)
    out = lo + rng.random((int(num_outliers), 3)) * (hi - lo)
    pts = np.round(np.vstack([pts, out]), 3)
    labels = np.concatenate([sem, np.full(int(num_outliers), 12, np.int64)])      # 12: clutter
    base = np.array([_ROOM_RGB.get(int(s), (128, 128, 128)) for s in range(max(_ROOM_RGB) + 1)], np.float64)
    rgb = np.where(labels[:, None] <= max(_ROOM_RGB), base[np.minimum(labels, max(_ROOM_RGB))], 128.0)
    rgb = np.clip(np.round(rgb + rng.normal(0.0, 6.0, rgb.shape)), 0, 255)
    perm = rng.permutation(len(pts))                 # S3DIS rows are not sorted by surface
    if return_instances:
        inst = np.concatenate([(np.asarray(mesh.triangle_ins, np.int64)[tri] if mesh.triangle_ins is not None
                                else np.zeros(n, np.int64)), np.zeros(int(num_outliers), np.int64)])
        return pts[perm], rgb[perm], labels[perm], inst[perm]
    return pts[perm], rgb[perm], labels[perm]


def write_s3dis_room(root, area_name, room_name, points, colors, labels=None):
    """<root>/<area_name>/<room_name>/<room_name>.txt in the S3DIS text layout: x y z r g b [label] per row, coordinates
    with 3 decimals, colours and labels as integers.  Returns the file's path."""
    import os
    d = os.path.join(str(root), area_name, room_name)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"{room_name}.txt")
    cols = [np.asarray(points, np.float64), np.asarray(colors, np.float64)]
    fmt = "%.3f %.3f %.3f %d %d %d"
    if labels is not None:
        cols.append(np.asarray(labels, np.float64).reshape(-1, 1))
        fmt += " %d"
    np.savetxt(path, np.hstack(cols), fmt=fmt)
    return path


# S3DIS class names by semantic id (the file stems of Annotations/<class>_<k>.txt)
S3DIS_CLASSES = ("ceiling", "floor", "wall", "beam", "column", "window", "door", "table", "chair", "sofa", "bookcase",
                 "board", "clutter")


def write_s3dis_annotations(root, area_name, room_name, points, colors, labels, instances):
    """<root>/<area_name>/<room_name>/Annotations/<class>_<k>.txt, one file per (label, instance) pair in the S3DIS text
    layout (x y z r g b, coordinates with 3 decimals): k counts the pairs of a class from 1 in ascending instance order,
    rows keep their order.  Returns the written paths in that order."""
    import os
    d = os.path.join(str(root), area_name, room_name, "Annotations")
    os.makedirs(d, exist_ok=True)
    labels, instances = np.asarray(labels, np.int64), np.asarray(instances, np.int64)
    data = np.hstack([np.asarray(points, np.float64), np.asarray(colors, np.float64)])
    paths = []
    for sem in np.unique(labels):
        name = S3DIS_CLASSES[sem] if 0 <= sem < len(S3DIS_CLASSES) else f"class{sem}"
        for k, ins in enumerate(np.unique(instances[labels == sem]), 1):
            path = os.path.join(d, f"{name}_{k}.txt")
            np.savetxt(path, data[(labels == sem) & (instances == ins)], fmt="%.3f %.3f %.3f %d %d %d")
            paths.append(path)
    return paths


def make_s3dis_area(root, area_name="Area_1", num_rooms=4, seed=0, density=4000.0, num_boxes=6, small_objects=4,
                    room_types=("office", "conferenceRoom", "hallway", "storage")):
    """A synthetic S3DIS area: num_rooms rooms <root>/<area_name>/<type>_<i>/ of make_room meshes of varied size (seeded),
    each sampled by sample_s3dis_room and written as the room file plus its Annotations folder.  small_objects adds
    that many small windows and boards per room (flat wall patches of 10 to 200 rows), so object sizes span 10 rows
    to the walls' tens of thousands.  Returns the room directories in creation order."""
    import os
    rng = np.random.default_rng(seed)
    rooms = []
    for i in range(int(num_rooms)):
        size = (float(rng.uniform(3.0, 8.0)), float(rng.uniform(3.0, 6.0)), float(rng.uniform(2.6, 3.4)))
        mesh = make_room(size=size, num_boxes=int(num_boxes), seed=int(seed) * 1000 + i)
        p, c, l, ins = sample_s3dis_room(mesh, density=density, num_outliers=50, seed=int(seed) * 1000 + i,
                                         return_instances=True)
        extra_p, extra_l, extra_i = [p], [l], [ins]
        for j in range(int(small_objects)):
            m = int(rng.integers(10, 201))
            w = rng.uniform(0.2, 1.0, 2)
            x0 = rng.uniform(0.2, size[0] - 1.2)
            z0 = rng.uniform(0.5, size[2] - 1.2)
            patch = np.stack([x0 + rng.random(m) * w[0], np.full(m, 0.01), z0 + rng.random(m) * w[1]], 1)
            extra_p.append(np.round(patch, 3))
            extra_l.append(np.full(m, 5 if j % 2 == 0 else 11, np.int64))
            extra_i.append(np.full(m, 1000 + j, np.int64))
        p, l, ins = np.vstack(extra_p), np.concatenate(extra_l), np.concatenate(extra_i)
        c = np.vstack([c, np.full((len(p) - len(c), 3), 128.0)])
        name = f"{room_types[i % len(room_types)]}_{i // len(room_types) + 1}"
        write_s3dis_room(root, area_name, name, p, c, l)
        write_s3dis_annotations(root, area_name, name, p, c, l, ins)
        rooms.append(os.path.join(str(root), area_name, name))
    return rooms
