"""CPU: the host side of the surface materials (lrc_material_step, the checks of lrc_material_table_create,
lidarcast.material.MaterialTable, the simulator key).  The segment step is compared bit for bit with the numpy restatement of
the header's text (tests/material_restate.py) on the per-segment columns the CPU oracle gives for the pane scene and the
synthetic room; looking through clear glass is compared with the oracle on the mesh without the pane."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import material_restate as mr
from conftest import REPO
from helpers import assert_bit_equal, table_rays
from noise_restate import fmaf


def oracle_cast(mesh):
    """A "cast these rays" function over the CPU oracle: t, prim, sem, ins, normal3 as the oracle gives them, point3 and
    intensity restated in float32 numpy (o + unit(d) * t; |fma(hz, nz, fma(hy, ny, hx * nx))|)."""
    from oracle.c_oracle import OracleMesh
    om = OracleMesh(mesh.vertices, mesh.triangles).build()
    sem_t = np.zeros(len(mesh.triangles), np.uint16) if mesh.triangle_sem is None else np.asarray(mesh.triangle_sem, np.uint16)
    ins_t = np.zeros(len(mesh.triangles), np.uint16) if mesh.triangle_ins is None else np.asarray(mesh.triangle_ins, np.uint16)

    def cast(rays):
        rays = np.ascontiguousarray(rays, np.float32)
        t, prim = om.cast(rays)
        hit = t < np.inf
        safe = np.where(hit, prim, 0)
        nm = om.normals(np.where(hit, prim, mr.INVALID).astype(np.uint32))
        h = mr.unit(rays[:, 3:])
        with np.errstate(invalid="ignore", over="ignore"):
            pp = np.where(hit[:, None], rays[:, :3] + h * t[:, None], np.float32(0)).astype(np.float32)
        c = np.abs(fmaf(h[:, 2], nm[:, 2], fmaf(h[:, 1], nm[:, 1], h[:, 0] * nm[:, 0])))
        return {"t": t, "prim": np.where(hit, prim, mr.INVALID).astype(np.uint32), "sem": np.where(hit, sem_t[safe], 0),
                "ins": np.where(hit, ins_t[safe], 0), "normal3": nm, "point3": pp, "intensity": np.where(hit, c, np.float32(0))}
    cast.oracle = om
    return cast


@pytest.fixture(scope="module")
def inputs():
    k, dirs, poses = mr.scan_inputs()
    rays, cen = table_rays(dirs, poses)
    return rays, np.repeat(cen, len(dirs), axis=0), k


@pytest.fixture(scope="module")
def pane(inputs):
    mesh, bare = mr.pane_scene()
    cast = oracle_cast(mesh)
    return mesh, bare, cast, mr.chain(cast, inputs[0], mr.pane_records(), 4)


@pytest.fixture(scope="module")
def room(inputs):
    mesh = mr.room_mesh()
    cast = oracle_cast(mesh)
    return mesh, cast, mr.chain(cast, inputs[0], mr.room_records(), 3)


def table_of(rec, max_bounces, min_intensity=0.0):
    from lidarcast.material import MaterialTable
    return MaterialTable(rec, max_bounces=max_bounces, min_intensity=min_intensity)


# ---- the restatement exercises what the tests are for ---------------------------------------------------------------------------

def test_pane_scene_exercises_every_bounce_count(inputs, pane):
    mesh, _, _, ch = pane
    assert len(mesh.triangles) == 30
    asm = mr.assemble(ch, inputs[0], inputs[1], inputs[2].max_range)
    hist = mr.bounce_histogram(asm, 4)
    print(f"\n[material] pane scene: returns after 0..4 bounces {hist.tolist()}, capped {int(ch['capped'].sum())}, "
          f"own returns from glass {int((ch['ret'] & (ch['sem'] == 5)).sum())}, tile variety {mr.tile_variety(asm, ch)}")
    assert (hist > 0).all(), hist
    assert ch["capped"].sum() > 0
    assert (ch["ret"] & (ch["sem"] == 5)).sum() > 0          # glass answers near normal incidence
    assert mr.tile_variety(asm, ch) >= 3
    assert len(ch["segments"]) == 5


def test_room_exercises_every_bounce_count(inputs, room):
    mesh, _, ch = room
    assert len(mesh.triangles) == 61760
    asm = mr.assemble(ch, inputs[0], inputs[1], inputs[2].max_range)
    hist = mr.bounce_histogram(asm, 3)
    print(f"\n[material] room: returns after 0..3 bounces {hist.tolist()}, without a return {int((~asm['keep']).sum())}, "
          f"capped {int(ch['capped'].sum())}, tile variety {mr.tile_variety(asm, ch)}")
    assert (hist > 0).all(), hist
    assert ch["capped"].sum() > 0
    assert (ch["ret"] & (ch["sem"] == 10)).sum() > 0
    assert mr.tile_variety(asm, ch) >= 3


# ---- lrc_material_step against the restatement ---------------------------------------------------------------------------------

def step_chain(cast, rays, table):
    """The chain driven by lrc_material_step: the state per segment and the end of every ray."""
    from lidarcast import material
    rays = np.ascontiguousarray(rays, np.float32)
    n = len(rays)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    T, g, b, st = np.zeros(n, np.float32), np.ones(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    inten, surf = np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    sem_f, nm_f = np.zeros(n, np.uint16), np.zeros((n, 3), np.float32)
    states = []
    while (st == material.PENDING).any():
        idx = np.flatnonzero(st == material.PENDING)
        states.append({"idx": idx, "o": o[idx].copy(), "d": d[idx].copy(), "T": T[idx].copy(), "g": g[idx].copy(), "b": b[idx].copy()})
        c = cast(np.concatenate([o[idx], d[idx]], axis=1))
        o2, d2, T2, g2, b2, st2, i2, s2 = table.step(c["t"], c["sem"], c["normal3"], o[idx], d[idx], T[idx], g[idx], b[idx], st[idx])
        o[idx], d[idx], T[idx], g[idx], b[idx], st[idx] = o2, d2, T2, g2, b2, st2
        done = st2 == material.RETURNED
        inten[idx[done]], surf[idx[done]] = i2[done], s2[done]
        sem_f[idx[done]], nm_f[idx[done]] = np.asarray(c["sem"])[done], c["normal3"][done]
    return {"states": states, "ret": st == material.RETURNED, "T": T, "I": inten, "b": b, "surface": surf, "sem": sem_f,
            "normal3": nm_f}


@pytest.mark.parametrize("which", ["pane", "room"])
def test_step_equals_the_restatement_bit_for_bit(which, inputs, pane, room):
    if which == "pane":
        cast, ch, rec, mb = pane[2], pane[3], mr.pane_records(), 4
    else:
        cast, ch, rec, mb = room[1], room[2], mr.room_records(), 3
    got = step_chain(cast, inputs[0], table_of(rec, mb))
    assert len(got["states"]) == len(ch["segments"])
    for k, (a, w) in enumerate(zip(got["states"], ch["segments"])):
        assert a["idx"].tolist() == w["idx"].tolist(), f"segment {k}: the pending rays differ"
        for col in ("o", "d", "T", "g"):
            assert_bit_equal(a[col], w[col], f"segment {k}: {col}")
        assert a["b"].tolist() == w["b"].tolist(), f"segment {k}: b"
    assert got["ret"].tolist() == ch["ret"].tolist()
    r = ch["ret"]
    for col in ("T", "I", "surface", "normal3"):
        assert_bit_equal(got[col][r], ch[col][r], col)
    assert got["b"][r].tolist() == ch["b"][r].tolist()
    assert got["sem"][r].tolist() == ch["sem"][r].tolist()


def test_step_applies_min_intensity(inputs, pane):
    _, _, cast, ch = pane
    thr = float(np.median(ch["I"][ch["ret"]]))
    want = mr.chain(cast, inputs[0], mr.pane_records(), 4, min_intensity=thr)
    got = step_chain(cast, inputs[0], table_of(mr.pane_records(), 4, thr))
    dropped = ch["ret"] & ~want["ret"]
    assert 0 < dropped.sum() < ch["ret"].sum()
    assert got["ret"].tolist() == want["ret"].tolist()


def test_step_leaves_finished_rays_alone_and_takes_a_miss():
    from lidarcast import material
    tab = table_of(mr.pane_records(2.0), 4)        # retro_cos 2: glass and mirrors never answer themselves
    n = 4
    t = np.array([1.0, np.inf, 1.0, 1.0], np.float32)
    sem = np.array([5, 5, 11, 200], np.uint16)
    nm = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (n, 1))
    o = np.zeros((n, 3), np.float32)
    d = np.tile(np.array([[2.0, 0.0, 0.0]], np.float32), (n, 1))
    st = np.array([0, 0, 1, 0], np.uint8)
    o2, d2, T2, g2, b2, st2, i2, s2 = tab.step(t, sem, nm, o, d, np.zeros(n, np.float32), np.ones(n, np.float32), np.zeros(n, np.uint8), st)
    assert st2.tolist() == [material.PENDING, material.NO_RETURN, material.RETURNED, material.RETURNED]
    # glass: the direction is kept as it is (not normalised), the origin is the hit point plus the skin, T = t + skin
    assert d2[0].tolist() == [2.0, 0.0, 0.0] and o2[0].tolist() == [1.0 + 2.0 ** -10, 0.0, 0.0]
    assert T2[0] == np.float32(1.0) + np.float32(2.0 ** -10) and g2[0] == np.float32(0.9) and b2[0] == 1
    # a ray that had returned is untouched; a semantic id beyond the table is diffuse with albedo 1
    assert T2[2] == 0.0 and b2[2] == 0 and o2[2].tolist() == [0.0, 0.0, 0.0]
    assert i2[3] == 1.0 and s2[3].tolist() == [1.0, 0.0, 0.0] and T2[3] == 1.0


# ---- looking through clear glass changes nothing -----------------------------------------------------------------------------

def test_clear_glass_changes_nothing(inputs, pane):
    """sem 5 glass with pass 1 that never answers itself, mirrors diffuse: every ray that crosses the pane ends on the triangle
    the oracle finds on the mesh WITHOUT the pane, at the oracle's range to within 2^-17 m (a crossing adds two roundings of a
    coordinate below 4 m, ulp 4.8e-7; measured 7.2e-7)."""
    mesh, bare, cast, _ = pane
    rays = inputs[0]
    rec = mr.records(12, s5=(mr.GLASS, 0.0, 1.0, 2.0))
    ch = mr.chain(cast, rays, rec, 4)
    crossed = ch["b"] > 0
    assert crossed.sum() > 500 and ch["ret"][crossed].all() and (ch["b"][crossed] == 1).all()
    from oracle.c_oracle import OracleMesh
    t_ref, prim_ref = OracleMesh(bare.vertices, bare.triangles).build().cast(rays)
    # the bare mesh lists the same triangles without the pane's two (rows 12, 13)
    prim = ch["prim"].astype(np.int64)
    prim = np.where(prim > 13, prim - 2, prim)
    same = prim[crossed] == prim_ref[crossed]
    err = np.abs(ch["T"][crossed].astype(np.float64) - t_ref[crossed])
    print(f"\n[material] clear glass: {int(same.sum())} of {int(crossed.sum())} crossing rays end on the oracle's triangle, "
          f"max |T - t_oracle| = {err.max():.3g} m")
    assert same.all()
    assert err.max() <= 2.0 ** -17
    # the library's step over the same table: the restatement's chain, bit for bit, so the property is lrc_material_step's too
    got = step_chain(cast, rays, table_of(rec, 4))
    assert got["ret"].tolist() == ch["ret"].tolist() and got["b"].tolist() == ch["b"].tolist()
    assert_bit_equal(got["T"][ch["ret"]], ch["T"][ch["ret"]], "T through clear glass")
    assert_bit_equal(got["surface"][crossed], ch["surface"][crossed], "the final hit point")
    assert_bit_equal(got["normal3"][crossed], ch["normal3"][crossed], "the final triangle's normal")
    assert got["sem"][crossed].tolist() == ch["sem"][crossed].tolist()
    err_lib = np.abs(got["T"][crossed].astype(np.float64) - t_ref[crossed])
    assert err_lib.max() <= 2.0 ** -17
    # ... and the rays that do not cross are the clean cast, bit for bit
    assert_bit_equal(ch["T"][~crossed & ch["ret"]], t_ref[~crossed & ch["ret"]])


# ---- the table, the symbols, the refusals -------------------------------------------------------------------------------------

def test_new_symbols_load():
    from lidarcast import _capi
    lib = _capi.load()
    for name in ("lrc_material_table_create", "lrc_material_table_destroy", "lrc_scan_materials_dev", "lrc_scan_materials_compact",
                 "lrc_material_step"):
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
    header = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    for name in ("lrc_scan_materials_dev", "lrc_scan_materials_compact", "lrc_material_step", "lrc_material_table_create"):
        assert re.search(rf"\bint {name}\(", header), name


def test_struct_layouts_match_the_header():
    from lidarcast._capi import LrcMaterial, LrcMaterialModel
    from lidarcast.material import RECORD
    src = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    for cname, cls, names in (("lrc_material", LrcMaterial, ["kind", "albedo", "pass", "retro_cos"]),
                              ("lrc_material_model", LrcMaterialModel, ["num_classes", "max_bounces", "min_intensity", "reserved_"])):
        body = re.search(rf"typedef struct {cname} \{{(.*?)\}} {cname};", src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        decls = [d.strip() for d in body.split(";") if d.strip()]
        assert [re.search(r"(\w+)\s*$", d).group(1) for d in decls] == names
        assert [n.rstrip("_") if n == "pass_" else n for n, _ in cls._fields_] == names
        ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
        assert [t for _, t in cls._fields_] == [ctype[d.split()[0]] for d in decls]
        assert C.sizeof(cls) == 16
    assert RECORD.itemsize == 16 and list(RECORD.names) == ["kind", "albedo", "pass", "retro_cos"]
    assert RECORD == mr.RECORD


def test_material_table_validation():
    from lidarcast.material import MaterialTable
    from lidarcast.synth import S3DIS_CLASSES
    t = MaterialTable.from_classes({"window": {"kind": "glass", "pass": 0.9, "albedo": 0.1, "retro_deg": 3},
                                    "board": {"kind": "mirror", "pass": 0.95, "albedo": 0.05, "retro_cos": 0.999}}, max_bounces=4)
    assert S3DIS_CLASSES.index("window") == 5 and S3DIS_CLASSES.index("board") == 11
    assert t.num_classes == 12 and t.max_bounces == 4 and t.min_intensity == 0.0
    assert t.records[5].tolist() == (1, np.float32(0.1), np.float32(0.9), np.float32(math.cos(math.radians(3))))
    assert t.records[11]["kind"] == 2 and t.records[11]["retro_cos"] == np.float32(0.999)
    assert (t.records["kind"][[0, 1, 2, 3, 4, 6, 7, 8, 9, 10]] == 0).all() and (t.records["albedo"][:5] == 1).all()
    s = t.struct()
    assert (s.num_classes, s.max_bounces, s.min_intensity) == (12, 4, 0.0)
    t2 = MaterialTable.from_classes({7: {"kind": "mirror"}}, mapping={"x": 3})
    assert t2.num_classes == 8 and t2.records[7]["kind"] == 2 and t2.records[7]["retro_cos"] == 2.0
    assert MaterialTable.diffuse(3).records.tolist() == [(0, 1.0, 0.0, 0.0)] * 3
    for classes in ({"glasswall": {"kind": "glass"}}, {"window": {"kind": "water"}}, {"window": {"kind": "glass", "gain": 1}},
                    {"window": {"retro_deg": 3, "retro_cos": 0.9}}, {300: {"kind": "glass"}}, {"window": {"albedo": 1.5}},
                    {"window": {"pass": -0.1}}, {"window": {"albedo": float("nan")}}, {"window": {"retro_cos": -0.5}},
                    {"window": {"retro_cos": float("inf")}}):
        with pytest.raises(ValueError):
            MaterialTable.from_classes(classes)
    for kw in (dict(max_bounces=9), dict(max_bounces=-1), dict(max_bounces=1.5), dict(min_intensity=1.5), dict(min_intensity=-0.1),
               dict(min_intensity=float("nan"))):
        with pytest.raises(ValueError):
            MaterialTable.diffuse(2, **kw)
    with pytest.raises(ValueError):
        MaterialTable(np.zeros(0, mr.RECORD))
    with pytest.raises(ValueError):
        MaterialTable(np.zeros(257, mr.RECORD))
    bad = np.zeros(2, mr.RECORD)
    bad["kind"][1] = 3
    with pytest.raises(ValueError):
        MaterialTable(bad)


def test_library_refusals():
    """The library checks the model and the records again, before it looks at anything else."""
    from lidarcast import _capi
    from lidarcast._capi import LrcMaterialModel
    lib = _capi.load()

    def model(num_classes=2, max_bounces=4, min_intensity=0.0):
        m = LrcMaterialModel()
        m.num_classes, m.max_bounces, m.min_intensity = num_classes, max_bounces, min_intensity
        return m
    good = mr.records(2)
    n = 1
    arrs = [np.zeros(n, np.float32), np.zeros(n, np.uint16), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32),
            np.ones((n, 3), np.float32), np.zeros(n, np.float32), np.ones(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8),
            np.zeros(n, np.float32), np.zeros((n, 3), np.float32)]
    ptrs = [a.ctypes.data for a in arrs]

    def step(m, rec):
        return lib.lrc_material_step(C.byref(m), None if rec is None else rec.ctypes.data, n, *ptrs)

    def create(m, rec):
        h = C.c_void_p()
        return lib.lrc_material_table_create(None, C.byref(m), None if rec is None else rec.ctypes.data, C.byref(h))
    assert step(model(), good) == 0
    for kw in (dict(num_classes=0), dict(num_classes=257), dict(max_bounces=9), dict(min_intensity=-0.5), dict(min_intensity=1.5),
               dict(min_intensity=float("nan")), dict(min_intensity=float("inf"))):
        for fn, who in ((step, b"lrc_material_step"), (create, b"lrc_material_table_create")):
            assert fn(model(**kw), good) == _capi.LRC_ERR_INVALID_ARG, kw
            assert who in lib.lrc_last_error() and b"context" not in lib.lrc_last_error(), kw
    for field, value in (("kind", 3), ("albedo", 1.5), ("albedo", -0.1), ("albedo", np.nan), ("pass", 2.0), ("pass", np.inf),
                         ("retro_cos", -0.1), ("retro_cos", np.nan), ("retro_cos", np.inf)):
        rec = mr.records(2)
        rec[field][1] = value
        for fn in (step, create):
            assert fn(model(), rec) == _capi.LRC_ERR_INVALID_ARG, (field, value)
            assert b"class 1" in lib.lrc_last_error(), (field, value)
    assert step(model(), None) == _capi.LRC_ERR_INVALID_ARG
    assert lib.lrc_material_step(None, good.ctypes.data, n, *ptrs) == _capi.LRC_ERR_INVALID_ARG
    assert lib.lrc_material_step(C.byref(model()), good.ctypes.data, n, None, *ptrs[1:]) == _capi.LRC_ERR_INVALID_ARG
    assert lib.lrc_material_step(C.byref(model()), good.ctypes.data, 0, *([None] * 11)) == 0
    assert create(model(), good) == _capi.LRC_ERR_INVALID_ARG and b"NULL context" in lib.lrc_last_error()
    # the scans want a table before they look at the scene
    hits, fr = _capi.LrcHits(), _capi.LrcFrames()
    assert lib.lrc_scan_materials_dev(None, None, 0, None, 0, None, 1.0, C.byref(hits), None, None, None) == _capi.LRC_ERR_INVALID_ARG
    assert b"materials is NULL" in lib.lrc_last_error()
    assert lib.lrc_scan_materials_compact(None, None, 0, None, None, 1.0, C.byref(fr), None, None, None, 0, None) == _capi.LRC_ERR_INVALID_ARG
    assert b"materials is NULL" in lib.lrc_last_error()
    assert lib.lrc_material_table_destroy(None) == 0


def test_simulator_materials_key():
    """What needs no engine: the key's own entries, the keys it refuses beside it, and the exporters that would scan without
    it."""
    import s3dis_simulator
    from lidarcast.material import MaterialTable

    def sim_with(config):
        sim = s3dis_simulator.S3DISSimulator.__new__(s3dis_simulator.S3DISSimulator)      # no engine is built
        sim.config = config
        sim.scene = object()
        return sim
    key = {"max_bounces": 4, "min_intensity": 0.0,
           "classes": {"window": {"kind": "glass", "pass": 0.9, "albedo": 0.1, "retro_deg": 3},
                       "board": {"kind": "mirror", "pass": 0.95, "albedo": 0.05, "retro_deg": 2}}}
    assert sim_with({})._material_table() is None
    t = sim_with({"materials": key})._material_table()
    assert isinstance(t, MaterialTable) and t.num_classes == 12 and t.max_bounces == 4
    assert t.records[5]["kind"] == 1 and t.records[5]["retro_cos"] == np.float32(math.cos(math.radians(3)))
    assert t.records[11]["kind"] == 2 and t.records[11]["retro_cos"] == np.float32(math.cos(math.radians(2)))
    for other, cfg in (("motion", {"speed": 1.0}), ("noise", {"seed": 1}), ("beam", {"divergence_mrad": 3.0})):
        with pytest.raises(ValueError, match=f"materials key cannot be combined with the {other} key"):
            sim_with({"materials": key, other: cfg})._material_table()
    with pytest.raises(ValueError, match="unknown entries under the materials key"):
        sim_with({"materials": {"classes": {}, "bounces": 3}})._material_table()
    with pytest.raises(ValueError):
        sim_with({"materials": {"classes": {"window": {"kind": "water"}}}})._material_table()
    with pytest.raises(ValueError):
        sim_with({"materials": {"classes": {}, "max_bounces": 9}})._material_table()
    sim = sim_with({"materials": key})
    for export in (lambda: sim.evaluate_surface_coverage([]), lambda: sim.export_occupancy_grid([], "unused"),
                   lambda: sim.export_frame_annotations([], "unused")):
        with pytest.raises(NotImplementedError, match="materials key"):
            export()
