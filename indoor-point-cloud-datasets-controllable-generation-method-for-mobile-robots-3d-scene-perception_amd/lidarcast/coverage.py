"""Surface coverage of scans over the C ABI (lrc_coverage_*, csrc/lrc_coverage.hip).

A ray RETURNS a point iff its t is finite after the range filter; triangle j is SEEN by a set of poses iff one returned
ray of those poses hit it.  Areas are quantised to q = rint(area * 2^32) in uint64, so covered and total areas are exact
integer sums: ``covered_q`` / ``total_q`` are those integers, the ``*_m2`` figures are q * 2^-32.

"Seen" is sampled: a triangle smaller than the gap between two scan lines can be missed by every pose, so the covered
area converges on the visible area as poses are added; nothing is dilated to correct for it.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np

from . import _capi
from ._capi import LrcCoverageInfo, LrcCoverageStats, check

Q_SCALE = 2.0 ** -32          # m^2 per unit of quantised area


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def pack_bits(seen, num_triangles):
    """(T,) bool -> (ceil(T/32),) uint32 bitset, bit j of word j // 32, least significant bit first."""
    seen = np.asarray(seen, dtype=bool).reshape(-1)
    if seen.size != num_triangles:
        raise ValueError("need one flag per triangle")
    W = (num_triangles + 31) // 32
    pad = np.zeros(W * 32, dtype=bool)
    pad[:num_triangles] = seen
    return np.packbits(pad, bitorder="little").view("<u4").astype(np.uint32)


def unpack_bits(words, num_triangles):
    """(W,) uint32 bitset -> (T,) bool."""
    w = np.ascontiguousarray(words, dtype="<u4")
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:num_triangles].astype(bool)


@dataclass
class CoverageSummary:
    seen: np.ndarray               # (T,) bool
    hits: np.ndarray               # (T,) uint32: returned rays per triangle, over all sets of the object
    covered_q: int
    total_q: int
    covered_area: float            # m^2
    total_area: float
    ratio: float
    per_class: Dict[int, Tuple[float, float, float]] = field(default_factory=dict)   # sem -> (covered, total, ratio)
    per_class_q: Dict[int, Tuple[int, int]] = field(default_factory=dict)            # sem -> (covered_q, total_q)
    returns: int = 0               # returned rays of the set(s)
    redundancy: float = 0.0        # returns per covered m^2
    seen_triangles: int = 0

    def to_dict(self, class_names=None):
        """JSON-ready figures (no per-triangle arrays).  ``class_names``: sem -> name, where known."""
        def name(s):
            return class_names[s] if class_names is not None and s in class_names else str(s)
        return {"covered_area_m2": self.covered_area, "total_area_m2": self.total_area, "ratio": self.ratio,
                "seen_triangles": self.seen_triangles, "num_triangles": int(self.seen.size), "returns": self.returns,
                "redundancy_returns_per_m2": self.redundancy,
                "per_class": {name(s): {"covered_m2": c, "total_m2": t, "ratio": r}
                              for s, (c, t, r) in self.per_class.items()}}


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


class SurfaceCoverage:
    """Per-set bitsets of seen triangles, per-triangle hit counts and the quantised area table of one mesh, in HBM."""

    def __init__(self, ctx, vertices, triangles, tri_sem=None, num_sets=1):
        self._lib = _capi.load()
        self.ctx = ctx
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        f = np.ascontiguousarray(triangles, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("vertices and triangles must be (V, 3) and (T, 3)")
        sem = None if tri_sem is None else np.ascontiguousarray(tri_sem, dtype=np.uint16)
        if sem is not None and sem.shape != (f.shape[0],):
            raise ValueError("tri_sem must have shape (T,)")
        h = C.c_void_p()
        check(self._lib.lrc_coverage_create(ctx._h, _ptr(v), v.shape[0], _ptr(f), f.shape[0], _ptr(sem), int(num_sets),
                                            C.byref(h)), "lrc_coverage_create")
        self._h = h
        info = LrcCoverageInfo()
        check(self._lib.lrc_coverage_get_info(self._h, C.byref(info)), "lrc_coverage_get_info")
        self.num_triangles, self.num_sets = int(info.num_triangles), int(info.num_sets)
        self.words_per_set, self.total_q = int(info.words_per_set), int(info.total_q)
        nc = int(info.num_classes)
        self.class_ids = np.zeros(nc, dtype=np.uint16)
        self.class_total_q = np.zeros(nc, dtype=np.uint64)
        if nc:
            check(self._lib.lrc_coverage_classes(self._h, _ptr(self.class_ids), _ptr(self.class_total_q)),
                  "lrc_coverage_classes")

    @property
    def total_area(self):
        return float(self.total_q) * Q_SCALE

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                self._lib.lrc_coverage_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=0):
        check(self._lib.lrc_coverage_reset(self._h, C.c_void_p(int(stream))), "lrc_coverage_reset")

    def accumulate_dev(self, t_t, prim_t, num_poses, rays_per_pose, set_of_pose_t=None, stream=0):
        """t_t float32 / prim_t int32 (or uint32 bits) device tensors of num_poses x rays_per_pose rays, pose-major;
        set_of_pose_t: optional int32 device tensor, one set index per pose (default: pose p -> set p)."""
        n = int(num_poses) * int(rays_per_pose)
        if t_t.numel() < n or prim_t.numel() < n:
            raise ValueError("t_t and prim_t need num_poses * rays_per_pose entries")
        if t_t.element_size() != 4 or prim_t.element_size() != 4:
            raise ValueError("t_t and prim_t must hold 4-byte entries")
        if set_of_pose_t is not None and (set_of_pose_t.numel() < int(num_poses) or set_of_pose_t.element_size() != 4):
            raise ValueError("set_of_pose_t needs one 4-byte set index per pose")
        sop = None if set_of_pose_t is None else C.c_void_p(set_of_pose_t.data_ptr())
        check(self._lib.lrc_coverage_accumulate_dev(self._h, C.c_void_p(t_t.data_ptr()), C.c_void_p(prim_t.data_ptr()),
                                                    int(num_poses), int(rays_per_pose), sop, C.c_void_p(int(stream))),
              "lrc_coverage_accumulate_dev")

    def export(self):
        """(bits (S, W) uint32, hits (T,) uint32, returns (S,) uint64), after all enqueued work."""
        bits = np.zeros((self.num_sets, self.words_per_set), dtype=np.uint32)
        hits = np.zeros(self.num_triangles, dtype=np.uint32)
        ret = np.zeros(self.num_sets, dtype=np.uint64)
        check(self._lib.lrc_coverage_export(self._h, _ptr(bits), _ptr(hits), _ptr(ret), None), "lrc_coverage_export")
        return bits, hits, ret

    def summary(self, set_index=None):
        """CoverageSummary of one set, or of the union of all sets (set_index=None)."""
        st = LrcCoverageStats()
        cls_q = np.zeros(max(1, len(self.class_ids)), dtype=np.uint64)
        words = np.zeros(self.words_per_set, dtype=np.uint32)
        k = -1 if set_index is None else int(set_index)
        if set_index is not None and not (0 <= k < self.num_sets):
            raise ValueError("set_index out of range")
        check(self._lib.lrc_coverage_summary(self._h, k, C.byref(st), _ptr(cls_q), _ptr(words)), "lrc_coverage_summary")
        hits = np.zeros(self.num_triangles, dtype=np.uint32)
        check(self._lib.lrc_coverage_export(self._h, None, _ptr(hits), None, None), "lrc_coverage_export")
        cov_q, tot_q = int(st.covered_q), int(st.total_q)
        per_class, per_class_q = {}, {}
        for i, s in enumerate(self.class_ids):
            c, t = int(cls_q[i]), int(self.class_total_q[i])
            per_class_q[int(s)] = (c, t)
            per_class[int(s)] = (float(c) * Q_SCALE, float(t) * Q_SCALE, _ratio(c, t))
        covered_area = float(cov_q) * Q_SCALE
        returns = int(st.returns)
        return CoverageSummary(seen=unpack_bits(words, self.num_triangles), hits=hits, covered_q=cov_q, total_q=tot_q,
                               covered_area=covered_area, total_area=float(tot_q) * Q_SCALE, ratio=_ratio(cov_q, tot_q),
                               per_class=per_class, per_class_q=per_class_q, returns=returns,
                               redundancy=float(returns) / covered_area if covered_area > 0 else float("inf") if returns else 0.0,
                               seen_triangles=int(st.seen_triangles))

    def select(self, budget, initial=None, target_ratio=None):
        """Greedy view selection over the sets: (picks (M,) int64, gains_m2 (M,), cumulative_ratio (M,)).
        ``initial``: already covered triangles, (T,) bool or a (W,) uint32 bitset.  ``target_ratio``: stop at the first
        pick whose covered / total area (initial cover included) reaches it."""
        budget = int(budget)
        if budget < 0:
            raise ValueError("budget must be >= 0")
        budget = min(budget, self.num_sets)
        init = None
        init_q = 0
        if initial is not None:
            a = np.asarray(initial)
            init = pack_bits(a, self.num_triangles) if a.dtype == bool else np.ascontiguousarray(a, dtype=np.uint32)
            if init.shape != (self.words_per_set,):
                raise ValueError("initial must be (T,) bool or (W,) uint32")
        tr = 0.0 if target_ratio is None else float(target_ratio)
        if not np.isfinite(tr):
            raise ValueError("target_ratio must be finite")
        picks = np.zeros(max(1, budget), dtype=np.uint32)
        gains = np.zeros(max(1, budget), dtype=np.uint64)
        n = C.c_uint32(0)
        check(self._lib.lrc_coverage_select(self._h, budget, tr, _ptr(init), _ptr(picks), _ptr(gains), C.byref(n)),
              "lrc_coverage_select")
        m = int(n.value)
        if init is not None:
            seen0 = unpack_bits(init, self.num_triangles)
            init_q = int(self._q_of(seen0))
        cum = init_q + np.cumsum(gains[:m].astype(object)) if m else np.zeros(0, dtype=object)
        ratio = np.array([_ratio(int(c), self.total_q) for c in cum], dtype=np.float64)
        return picks[:m].astype(np.int64), gains[:m].astype(np.float64) * Q_SCALE, ratio

    def _q_of(self, seen):
        """Exact covered q of a (T,) bool mask."""
        return int(self.area_q()[seen].sum(dtype=np.uint64)) if seen.any() else 0

    def area_q(self):
        """(T,) uint64 quantised triangle areas, the device's table."""
        q = np.zeros(self.num_triangles, dtype=np.uint64)
        check(self._lib.lrc_coverage_export(self._h, None, None, None, _ptr(q)), "lrc_coverage_export")
        return q


def scan_coverage(scene, coverage, poses, dirs, max_range, set_of_pose=None, chunk_poses=None, stream=0):
    """Scan ``poses`` (P, 4, 4) with the sensor-frame direction table ``dirs`` (N, 3) float64 (numpy or a device tensor)
    on ``scene`` (lidarcast.Scene) and accumulate every returned ray into ``coverage``.  ``set_of_pose``: (P,) set
    index per pose (default: pose p -> set p).  The scan runs in chunks of ``chunk_poses`` poses through
    Scene.scan_poses_dev into one reused t / prim buffer (default: about 256 MB of hit records), so the buffers stay
    bounded however many poses there are.  Returns ``coverage``."""
    import torch
    from .core import DeviceHits
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)
    P = poses.shape[0]
    dev = torch.device("cuda", scene.ctx.device)
    dirs_t = dirs if isinstance(dirs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float64))
    dirs_t = dirs_t.to(dev, dtype=torch.float64).contiguous()
    if dirs_t.ndim != 2 or dirs_t.shape[1] != 3 or dirs_t.shape[0] == 0:
        raise ValueError("dirs must be a non-empty (N, 3) table")
    N = int(dirs_t.shape[0])
    if set_of_pose is None:
        if P > coverage.num_sets:
            raise ValueError("without set_of_pose every pose is its own set: need num_sets >= number of poses")
        sop = np.arange(P, dtype=np.int64)
    else:
        sop = np.asarray(set_of_pose, dtype=np.int64).reshape(-1)
        if sop.shape != (P,):
            raise ValueError("set_of_pose needs one entry per pose")
        if P and (sop.min() < 0 or sop.max() >= coverage.num_sets):
            raise ValueError("set_of_pose entries must lie in [0, num_sets)")
    if P == 0:
        return coverage
    chunk = int(chunk_poses) if chunk_poses else max(1, (32 << 20) // N)
    chunk = max(1, min(chunk, P))
    hits = DeviceHits(chunk * N, dev, want=("t", "prim"))
    poses_t = torch.from_numpy(poses).to(dev)
    sop_t = torch.from_numpy(sop.astype(np.int32)).to(dev)
    for p0 in range(0, P, chunk):
        p1 = min(P, p0 + chunk)
        scene.scan_poses_dev(poses_t[p0:p1], dirs_t, hits, max_range, stream=stream)
        coverage.accumulate_dev(hits["t"], hits["prim"], p1 - p0, N, sop_t[p0:p1], stream=stream)
    torch.cuda.synchronize(dev)
    return coverage
