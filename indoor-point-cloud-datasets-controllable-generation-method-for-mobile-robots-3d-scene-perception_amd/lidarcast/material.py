"""Surface materials: glass, mirrors and return intensity (include/lidarcast.h "surface materials").

``MaterialTable`` gives every semantic class a material -- diffuse, glass or mirror -- and the model's limits:
``Scene.scan_materials_dev`` / ``Scene.scan_materials_compact`` continue a ray that meets glass or a mirror inside the trace
kernel; ``MaterialTable.step`` applies one segment's step on the host, without a GPU (lrc_material_step).
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import LrcMaterial, LrcMaterialModel, check

KINDS = {"diffuse": 0, "glass": 1, "mirror": 2}
RECORD = np.dtype([("kind", np.uint32), ("albedo", np.float32), ("pass", np.float32), ("retro_cos", np.float32)])
PENDING, RETURNED, NO_RETURN = 0, 1, 2


def _default_mapping():
    from .synth import S3DIS_CLASSES
    return {name: i for i, name in enumerate(S3DIS_CLASSES)}


class MaterialTable:
    """records: (num_classes,) array of ``RECORD`` -- kind (0 diffuse, 1 glass, 2 mirror), albedo and pass in [0, 1], retro_cos
    >= 0 (above 1: the surface never answers itself) -- for semantic ids 0..num_classes-1, 1 <= num_classes <= 256; an id at or
    above num_classes is diffuse with albedo 1.  max_bounces in [0, 8]; min_intensity in [0, 1]: weaker returns are dropped."""

    def __init__(self, records, max_bounces=4, min_intensity=0.0):
        rec = np.array(records, dtype=RECORD, copy=True).reshape(-1)
        if not 1 <= len(rec) <= 256:
            raise ValueError("a material table has 1 to 256 classes")
        if (rec["kind"] > 2).any():
            raise ValueError("kind must be 0 (diffuse), 1 (glass) or 2 (mirror)")
        for name in ("albedo", "pass"):
            v = rec[name]
            if not np.isfinite(v).all() or (v < 0).any() or (v > 1).any():
                raise ValueError(f"{name} must be finite and lie in [0, 1]")
        if not np.isfinite(rec["retro_cos"]).all() or (rec["retro_cos"] < 0).any():
            raise ValueError("retro_cos must be finite and not negative")
        if int(max_bounces) != max_bounces or not 0 <= int(max_bounces) <= 8:
            raise ValueError("max_bounces must lie in [0, 8]")
        if not (np.isfinite(min_intensity) and 0.0 <= float(min_intensity) <= 1.0):
            raise ValueError("min_intensity must be finite and lie in [0, 1]")
        rec.setflags(write=False)
        self.records = rec
        self.max_bounces = int(max_bounces)
        self.min_intensity = float(min_intensity)
        self._resident = {}          # id(context) -> (context, handle)

    @classmethod
    def diffuse(cls, num_classes=1, **kw):
        """Every class diffuse with albedo 1: the clean scan."""
        rec = np.zeros(num_classes, dtype=RECORD)
        rec["albedo"] = 1.0
        return cls(rec, **kw)

    @classmethod
    def from_classes(cls, classes, mapping=None, max_bounces=4, min_intensity=0.0):
        """classes: {class name or semantic id: {kind: diffuse | glass | mirror, albedo, pass, retro_cos or retro_deg}};
        mapping: class name -> semantic id (default: the S3DIS class list).  Classes that are not named are diffuse with albedo
        1.  ``retro_deg`` is the half angle about the normal inside which the surface answers itself: retro_cos =
        cos(retro_deg)."""
        mapping = _default_mapping() if mapping is None else dict(mapping)
        ids = {}
        for name, spec in classes.items():
            if isinstance(name, (int, np.integer)):
                sid = int(name)
            elif name in mapping:
                sid = int(mapping[name])
            else:
                raise ValueError(f"unknown class {name!r}")
            if not 0 <= sid < 256:
                raise ValueError(f"semantic id {sid} of class {name!r} is outside [0, 256)")
            ids[sid] = (name, dict(spec))
        rec = np.zeros(max(ids) + 1 if ids else 1, dtype=RECORD)
        rec["albedo"] = 1.0
        rec["retro_cos"] = 2.0
        for sid, (name, spec) in ids.items():
            unknown = set(spec) - {"kind", "albedo", "pass", "retro_cos", "retro_deg"}
            if unknown:
                raise ValueError(f"unknown entries of class {name!r}: {sorted(unknown)}")
            kind = spec.get("kind", "diffuse")
            if kind not in KINDS:
                raise ValueError(f"class {name!r}: kind must be one of {sorted(KINDS)}")
            if "retro_cos" in spec and "retro_deg" in spec:
                raise ValueError(f"class {name!r}: give retro_cos or retro_deg, not both")
            retro = float(spec["retro_cos"]) if "retro_cos" in spec else \
                math.cos(math.radians(float(spec["retro_deg"]))) if "retro_deg" in spec else 2.0
            rec[sid] = (KINDS[kind], float(spec.get("albedo", 1.0)), float(spec.get("pass", 0.0)), retro)
        return cls(rec, max_bounces=max_bounces, min_intensity=min_intensity)

    @property
    def num_classes(self):
        return len(self.records)

    def struct(self):
        m = LrcMaterialModel()
        m.num_classes, m.max_bounces, m.min_intensity, m.reserved_ = self.num_classes, self.max_bounces, self.min_intensity, 0
        return m

    def resident(self, ctx):
        """The table's handle on ``ctx`` (lrc_material_table_create), uploaded on first use and kept."""
        hit = self._resident.get(id(ctx))
        if hit is not None and hit[0] is ctx and getattr(ctx, "_h", None):
            return hit[1]
        lib = _capi.load()
        h = C.c_void_p()
        m = self.struct()
        check(lib.lrc_material_table_create(ctx._h, C.byref(m), self.records.ctypes.data, C.byref(h)),
              "lrc_material_table_create")
        self._resident[id(ctx)] = (ctx, h)
        return h

    def close(self):
        lib = _capi.load()
        for ctx, h in self._resident.values():
            if getattr(ctx, "_h", None):
                lib.lrc_material_table_destroy(h)
        self._resident = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, t, sem, normal3, origin3, dir3, path, gain, bounces, status):
        """One segment's step for n rays on the host (lrc_material_step).  t, sem, normal3: the segment's closest hit (t = +inf:
        a miss); origin3, dir3, path, gain, bounces, status (0 pending, 1 returned, 2 no return): the state, taken by value.
        Returns the new (origin3, dir3, path, gain, bounces, status, intensity, surface_point3)."""
        return step(self.struct(), self.records, t, sem, normal3, origin3, dir3, path, gain, bounces, status)

    def __repr__(self):
        kinds = np.bincount(self.records["kind"], minlength=3)
        return (f"MaterialTable(num_classes={self.num_classes}, glass={kinds[1]}, mirror={kinds[2]}, "
                f"max_bounces={self.max_bounces}, min_intensity={self.min_intensity!r})")


def step(model, records, t, sem, normal3, origin3, dir3, path, gain, bounces, status):
    """lrc_material_step with an ``LrcMaterialModel`` and its records: see ``MaterialTable.step``."""
    lib = _capi.load()
    rec = np.ascontiguousarray(records, dtype=RECORD).reshape(-1)
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
    n = len(t)
    sem = np.ascontiguousarray(sem, dtype=np.uint16).reshape(-1)
    normal3 = np.ascontiguousarray(normal3, dtype=np.float32).reshape(-1, 3)
    o = np.array(origin3, dtype=np.float32, copy=True).reshape(-1, 3)
    d = np.array(dir3, dtype=np.float32, copy=True).reshape(-1, 3)
    T = np.array(path, dtype=np.float32, copy=True).reshape(-1)
    g = np.array(gain, dtype=np.float32, copy=True).reshape(-1)
    b = np.array(bounces, dtype=np.uint8, copy=True).reshape(-1)
    st = np.array(status, dtype=np.uint8, copy=True).reshape(-1)
    if not (len(sem) == len(normal3) == len(o) == len(d) == len(T) == len(g) == len(b) == len(st) == n):
        raise ValueError("every argument must have one entry per ray")
    if 1 <= int(model.num_classes) <= 256 and len(rec) != int(model.num_classes):
        raise ValueError("records must hold num_classes entries")
    inten = np.zeros(n, np.float32)
    surf = np.zeros((n, 3), np.float32)
    check(lib.lrc_material_step(C.byref(model), rec.ctypes.data, n, t.ctypes.data, sem.ctypes.data, normal3.ctypes.data,
                                o.ctypes.data, d.ctypes.data, T.ctypes.data, g.ctypes.data, b.ctypes.data, st.ctypes.data,
                                inten.ctypes.data, surf.ctypes.data), "lrc_material_step")
    return o, d, T, g, b, st, inten, surf
