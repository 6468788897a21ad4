"""Dynamic occupancy over the C ABI: per-frame grids under movers (lrc_voxseq_*, csrc/lrc_voxseq.hip).

``lidarcast.voxgrid`` ORs the free space of every pose into one grid, which is wrong as soon as something moves.  An
``OccupancySequence`` is F frame slots of one grid geometry: every returned ray of a scan walks, in float64, from its float32
origin to its float32 end point (the scan's own ``point3`` row) and carves the slot of its frame only.  Each voxel gets, per
frame, its state (occupied / free / unknown), sem and ins by the vote of ``lidarcast.voxgrid``, and -- by a second, independent
vote -- the mover id most of its returns carry (0 is the room, m + 1 mover m) and the number of returns off movers.  With
``static_only`` and every pose mapped to one slot the same object accumulates the static map: the movers' rays still carve free
space, but their returns are left out.  The full statement is in include/lidarcast.h and tests/voxseq_restate.py.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import LrcVoxseqInfo, LrcVoxseqOut, check
from .voxgrid import FREE, OCCUPIED, UNKNOWN, OccupancyResult, check_grid  # noqa: F401  (the states are re-exported)

STATIC_ONLY = 1
MAX_BITS = (1 << 31) - 1


def check_frames(frames, dims):
    """Validated F, or ValueError: F >= 1 and F * 32 * ceil(V / 32) <= 2^31 - 1."""
    try:
        F = int(frames)
    except (TypeError, ValueError):
        raise ValueError("frames must be an integer") from None
    if F < 1 or F != frames:
        raise ValueError("frames must be an integer >= 1")
    V = int(dims[0]) * int(dims[1]) * int(dims[2])
    if F * 32 * ((V + 31) // 32) > MAX_BITS:
        raise ValueError("frames * 32 * ceil(nx*ny*nz / 32) must not exceed 2^31 - 1")
    return F


def walk(o, e, origin, s, dims):
    """lrc_voxseq_walk, the host step (no GPU): walk the segments o[r] -> e[r] ((n, 3) float32) on a grid.  Returns (free
    (ceil(V/32),) uint32 bitset, end (n, 3) int64 = the voxel of e (zeros where a point or a coordinate was refused),
    rejected (n,) bool)."""
    lib = _capi.load()
    g, sz, d = check_grid(origin, s, dims)
    o32 = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    e32 = np.ascontiguousarray(e, dtype=np.float32).reshape(-1, 3)
    if len(o32) != len(e32):
        raise ValueError("o and e must hold the same number of points")
    n = len(o32)
    bits = np.zeros((d[0] * d[1] * d[2] + 31) // 32, np.uint32)
    end = np.zeros((n, 3), np.int64)
    rej = np.zeros(n, np.uint8)
    dd = (C.c_int64 * 3)(*d)
    check(lib.lrc_voxseq_walk(g.ctypes.data, sz, dd, o32.ctypes.data, e32.ctypes.data, n, bits.ctypes.data, end.ctypes.data,
                              rej.ctypes.data), "lrc_voxseq_walk")
    return bits, end, rej.astype(bool)


@dataclass
class DynamicOccupancyResult:
    origin: np.ndarray             # (3,) float64
    voxel_size: float
    dims: tuple
    frames: int
    min_returns: int
    frame_offsets: np.ndarray      # (F + 1,) uint64 into the sparse list
    idx: np.ndarray                # (K,) uint32, ascending by (slot, idx): linear index within the slot
    sem: np.ndarray                # (K,) uint16
    ins: np.ndarray                # (K,) uint16
    returns: np.ndarray            # (K,) uint32
    mover: np.ndarray              # (K,) uint8: the mover vote, 0 is the room
    mover_returns: np.ndarray      # (K,) uint32: returns with mover id != 0
    counts: np.ndarray             # (F, 6) uint64: sparse entries, free, occupied, unknown, rejected rays, returns
    skipped: int                   # returned rays of poses without a slot
    state: np.ndarray = None       # (F, nx, ny, nz) uint8; None without dense

    def _range(self, f):
        f = int(f)
        if not 0 <= f < self.frames:
            raise IndexError(f"frame {f} is outside 0 .. {self.frames - 1}")
        return f, int(self.frame_offsets[f]), int(self.frame_offsets[f + 1])

    def frame(self, f):
        """Slot f as a ``lidarcast.OccupancyResult`` (views of this result's arrays), so its consumers work as they are."""
        f, a, b = self._range(f)
        c = self.counts[f]
        r = OccupancyResult(origin=self.origin.copy(), voxel_size=self.voxel_size, dims=self.dims, min_returns=self.min_returns,
                            idx=self.idx[a:b], sem=self.sem[a:b], ins=self.ins[a:b], returns=self.returns[a:b],
                            num_free=int(c[1]), num_occupied=int(c[2]), num_unknown=int(c[3]), rejected_rays=int(c[4]),
                            state=None if self.state is None else self.state[f])
        occ = r.occupied
        if occ.any():
            u, n = np.unique(r.sem[occ], return_counts=True)
            r.per_class = {int(x): int(y) for x, y in zip(u, n)}
        return r

    def mover_of(self, f):
        """(idx, mover, mover_returns) of slot f's sparse entries."""
        f, a, b = self._range(f)
        return self.idx[a:b], self.mover[a:b], self.mover_returns[a:b]

    def dynamic_voxels(self, f):
        """(idx, mover) of slot f's voxels that are occupied with mover != 0."""
        f, a, b = self._range(f)
        m = (self.returns[a:b] >= self.min_returns) & (self.mover[a:b] != 0)
        return self.idx[a:b][m], self.mover[a:b][m]

    def dynamic_per_mover(self, f):
        """{mover id: dynamic voxels} of slot f."""
        _, m = self.dynamic_voxels(f)
        u, n = np.unique(m, return_counts=True)
        return {int(x): int(y) for x, y in zip(u, n)}

    def to_dict(self, class_names=None):
        """JSON-ready summary: the grid and, per frame, the counts, occupied voxels per class and dynamic voxels per mover."""
        frames = []
        for f in range(self.frames):
            d = self.frame(f).to_dict(class_names)
            frames.append({"frame": f, "counts": d["counts"], "per_class_occupied_voxels": d["per_class_occupied_voxels"],
                           "dynamic_voxels_per_mover": {str(k): v for k, v in self.dynamic_per_mover(f).items()}})
        return {"origin": [float(x) for x in self.origin], "voxel_size": self.voxel_size, "dims": [int(x) for x in self.dims],
                "num_frames": self.frames, "min_returns": self.min_returns, "skipped_rays": int(self.skipped), "frames": frames}

    def to_npz(self, path):
        """state (F, nx, ny, nz), the sparse list (frame_offsets, idx, sem, ins, returns, mover, mover_returns), counts,
        skipped, origin, voxel_size, dims, min_returns."""
        if self.state is None:
            raise ValueError("finalize(dense=True) is needed for the npz (it holds the dense state)")
        np.savez_compressed(path, state=self.state, frame_offsets=self.frame_offsets, idx=self.idx, sem=self.sem, ins=self.ins,
                            returns=self.returns, mover=self.mover, mover_returns=self.mover_returns, counts=self.counts,
                            skipped=np.uint64(self.skipped), origin=self.origin, voxel_size=np.float64(self.voxel_size),
                            dims=np.array(self.dims, dtype=np.int64), min_returns=np.uint32(self.min_returns))


class OccupancySequence:
    """Free bits and returns of F frame slots of one voxel grid, in HBM, accumulated over scans until ``reset``."""

    def __init__(self, ctx, origin, voxel_size, dims, frames):
        o, s, d = check_grid(origin, voxel_size, dims)
        F = check_frames(frames, d)
        self._lib = _capi.load()
        self.ctx = ctx
        h = C.c_void_p()
        dd = (C.c_int64 * 3)(*d)
        check(self._lib.lrc_voxseq_create(ctx._h, o.ctypes.data_as(C.c_void_p), s, dd, F, C.byref(h)), "lrc_voxseq_create")
        self._h = h
        self.origin, self.voxel_size, self.dims, self.frames = o, s, d, F
        self.num_voxels = d[0] * d[1] * d[2]

    def info(self):
        i = LrcVoxseqInfo()
        check(self._lib.lrc_voxseq_get_info(self._h, C.byref(i)), "lrc_voxseq_get_info")
        return i

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                self._lib.lrc_voxseq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=0):
        check(self._lib.lrc_voxseq_reset(self._h, C.c_void_p(int(stream))), "lrc_voxseq_reset")

    def accumulate_dev(self, origins_t, hits, num_poses, rays_per_pose, mover_t=None, frame_of_pose_t=None, first_frame=0,
                       origin_per_ray=False, static_only=False, stream=0):
        """Carve the returned rays of ``hits`` (``lidarcast.DeviceHits`` or a slice of one with t, point3, sem and ins:
        num_poses * rays_per_pose records, pose-major).  ``origins_t``: (num_poses, 3) float32 device tensor, or (num_poses *
        rays_per_pose, 3) with ``origin_per_ray``; ``mover_t``: optional (num_poses * rays_per_pose) uint8; ``frame_of_pose_t``:
        optional (num_poses,) int32 device tensor of slots (read as uint32; a slot >= frames skips the pose), default slot
        ``first_frame + p``."""
        import torch
        P, N = int(num_poses), int(rays_per_pose)
        if hits.n != P * N:
            raise ValueError("hits must hold num_poses * rays_per_pose records")
        for a in ("t", "point3", "sem", "ins"):
            if not getattr(hits.struct, a):
                raise ValueError(f"the records need t, point3, sem and ins ({a} is missing)")
        need = (P * N if origin_per_ray else P) * 3
        if origins_t.dtype != torch.float32 or not origins_t.is_cuda or not origins_t.is_contiguous() or origins_t.numel() != need:
            raise ValueError("origins_t must be a contiguous float32 device tensor of (num_poses, 3), or (num_poses * "
                             "rays_per_pose, 3) with origin_per_ray")
        if mover_t is not None and (mover_t.dtype != torch.uint8 or not mover_t.is_cuda or not mover_t.is_contiguous() or
                                    mover_t.numel() != P * N):
            raise ValueError("mover_t must be a contiguous uint8 device tensor of num_poses * rays_per_pose entries")
        if frame_of_pose_t is not None and (frame_of_pose_t.dtype != torch.int32 or not frame_of_pose_t.is_cuda or
                                            not frame_of_pose_t.is_contiguous() or frame_of_pose_t.numel() != P):
            raise ValueError("frame_of_pose_t must be a contiguous int32 device tensor of num_poses entries")
        check(self._lib.lrc_voxseq_accumulate_dev(
            self._h, C.c_void_p(origins_t.data_ptr()), int(bool(origin_per_ray)), P, N,
            None if frame_of_pose_t is None else C.c_void_p(frame_of_pose_t.data_ptr()), int(first_frame), C.byref(hits.struct),
            None if mover_t is None else C.c_void_p(mover_t.data_ptr()), STATIC_ONLY if static_only else 0,
            C.c_void_p(int(stream))), "lrc_voxseq_accumulate_dev")

    def free_bits(self):
        """(F, ceil(V/32)) uint32 free bitsets after all enqueued work."""
        i = self.info()
        w = np.zeros(int(i.num_frames) * int(i.words_per_frame), dtype=np.uint32)
        check(self._lib.lrc_voxseq_export_bits(self._h, w.ctypes.data_as(C.c_void_p)), "lrc_voxseq_export_bits")
        return w.reshape(int(i.num_frames), int(i.words_per_frame))

    def finalize(self, min_returns=1, dense=True, stream=0):
        """DynamicOccupancyResult of everything accumulated so far (the accumulation itself is kept).  Runs on the device
        (lrc_voxseq_finalize_dev) and synchronises once, on the frame offsets."""
        import torch
        mr = int(min_returns)
        if mr < 1 or mr > 0xFFFFFFFF:
            raise ValueError("min_returns must be >= 1")
        dev = torch.device("cuda", self.ctx.device)
        F, V = self.frames, self.num_voxels
        bound = max(1, int(self.info().sparse_bound))
        t = {"idx": torch.empty(bound, dtype=torch.int32, device=dev), "sem": torch.empty(bound, dtype=torch.int16, device=dev),
             "ins": torch.empty(bound, dtype=torch.int16, device=dev), "returns": torch.empty(bound, dtype=torch.int32, device=dev),
             "mover": torch.empty(bound, dtype=torch.uint8, device=dev),
             "mover_returns": torch.empty(bound, dtype=torch.int32, device=dev),
             "frame_offsets": torch.zeros(F + 1, dtype=torch.int64, device=dev),
             "counts": torch.zeros((F, 6), dtype=torch.int64, device=dev), "skipped": torch.zeros(1, dtype=torch.int64, device=dev)}
        if dense:
            t["state"] = torch.empty(F * V, dtype=torch.uint8, device=dev)
        out = LrcVoxseqOut()
        for k, v in t.items():
            setattr(out, k, v.data_ptr())
        check(self._lib.lrc_voxseq_finalize_dev(self._h, mr, C.byref(out), bound, C.c_void_p(int(stream))),
              "lrc_voxseq_finalize_dev")
        off = t["frame_offsets"].cpu().numpy().astype(np.uint64)          # the one synchronisation
        k = int(off[F])
        return DynamicOccupancyResult(
            origin=self.origin.copy(), voxel_size=self.voxel_size, dims=self.dims, frames=F, min_returns=mr, frame_offsets=off,
            idx=t["idx"][:k].cpu().numpy().view(np.uint32), sem=t["sem"][:k].cpu().numpy().view(np.uint16),
            ins=t["ins"][:k].cpu().numpy().view(np.uint16), returns=t["returns"][:k].cpu().numpy().view(np.uint32),
            mover=t["mover"][:k].cpu().numpy(), mover_returns=t["mover_returns"][:k].cpu().numpy().view(np.uint32),
            counts=t["counts"].cpu().numpy().astype(np.uint64), skipped=int(t["skipped"].cpu().numpy()[0]),
            state=t["state"].cpu().numpy().reshape((F,) + tuple(self.dims)) if dense else None)


def pose_origins(poses):
    """(P, 3) float32 ray origins of pose-batched scans: the float32 of each pose's translation, as the scan forms it."""
    return np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)[:, :3, 3].astype(np.float32))


def scan_dynamic_occupancy(scene, seq, poses, dirs, max_range, movers=None, mover_poses=None, shapes=None, noise=None,
                           static_only=False, frame_of_pose=None, chunk_poses=None, stream=0, static_seq=None):
    """Scan ``poses`` (P, 4, 4) with the direction table ``dirs`` (N, 3) float64 on ``scene`` and carve every returned ray into
    ``seq`` (OccupancySequence): pose p goes to slot ``frame_of_pose[p]`` (default p).  ``movers``: a ``lidarcast.movers.MoverSet``
    with ``mover_poses`` (P, M, 12) float32, or None (the clean scan's records and a zero mover column); ``shapes`` (P, D, 3):
    the set's deformables change shape from frame to frame (``lidarcast.deform.scan_deforming_dev``); ``noise``: a
    ``lidarcast.noise.NoiseModel``, pose p is frame ``noise.first_frame + p``.  The scan runs in chunks of ``chunk_poses`` poses
    into one reused record buffer and each chunk is accumulated on the same stream with no host wait in between.
    ``static_seq``: a second OccupancySequence that receives every chunk as well, with STATIC_ONLY and every pose in its slot 0
    (the static map from the same scan).  Returns ``seq``."""
    import torch
    from . import deform
    from .core import DeviceHits
    from .movers import scan_noisy_movers_dev
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)
    P = poses.shape[0]
    dev = torch.device("cuda", scene.ctx.device)
    dirs_t = dirs if isinstance(dirs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float64))
    dirs_t = dirs_t.to(dev, dtype=torch.float64).contiguous()
    if dirs_t.ndim != 2 or dirs_t.shape[1] != 3 or dirs_t.shape[0] == 0:
        raise ValueError("dirs must be a non-empty (N, 3) table")
    if shapes is not None and movers is None:
        raise ValueError("shapes need a mover set")
    mp_t = None
    if movers is not None:
        mp = np.ascontiguousarray(mover_poses, dtype=np.float32)
        if mp.shape != (P, len(movers), 12):
            raise ValueError(f"mover_poses must be (P, M, 12) = ({P}, {len(movers)}, 12), got {mp.shape}")
        mp_t = torch.from_numpy(mp).to(dev)
    if shapes is not None:
        shapes = np.asarray(shapes, dtype=np.float64)
    fop_t = None
    if frame_of_pose is not None:
        fop = np.asarray(frame_of_pose).reshape(-1)
        if len(fop) != P or fop.dtype.kind not in "iu" or (fop < 0).any() or (fop > 0x7FFFFFFF).any():
            raise ValueError("frame_of_pose must hold one slot (0 .. 2^31 - 1) per pose")
        fop_t = torch.from_numpy(fop.astype(np.int32)).to(dev)
    elif P > seq.frames:
        raise ValueError(f"{P} poses do not fit {seq.frames} frame slots (give frame_of_pose)")
    if P == 0:
        return seq
    N = int(dirs_t.shape[0])
    chunk = int(chunk_poses) if chunk_poses else max(1, (8 << 20) // N)
    chunk = max(1, min(chunk, P))
    hits = DeviceHits(chunk * N, dev, want=("t", "point3", "sem", "ins"))
    mover_t = torch.zeros(chunk * N, dtype=torch.uint8, device=dev)
    poses_t = torch.from_numpy(poses).to(dev)
    origins_t = torch.from_numpy(pose_origins(poses)).to(dev)
    zero_t = torch.zeros(chunk, dtype=torch.int32, device=dev) if static_seq is not None else None
    for p0 in range(0, P, chunk):
        p1 = min(P, p0 + chunk)
        n = p1 - p0
        part = hits if n == chunk else deform._HitsSlice(hits, 0, n * N)
        rows = mover_t[:n * N]
        nz = None if noise is None else noise.at_frame(noise.first_frame + p0)
        mpc = None if mp_t is None else mp_t[p0:p1]
        if shapes is not None:
            deform.scan_deforming_dev(scene, poses_t[p0:p1], dirs_t, part, max_range, movers, mpc, shapes[p0:p1], rows,
                                      stream=stream, noise=nz)
        elif nz is not None:
            scan_noisy_movers_dev(scene, poses_t[p0:p1], dirs_t, part, max_range, movers, mpc, nz, rows, stream=stream)
        else:
            scene.scan_movers_dev(poses_t[p0:p1], dirs_t, part, max_range, movers, mpc, rows, stream=stream)
        seq.accumulate_dev(origins_t[p0:p1], part, n, N, mover_t=rows, frame_of_pose_t=None if fop_t is None else fop_t[p0:p1],
                           first_frame=p0, static_only=static_only, stream=stream)
        if static_seq is not None:
            static_seq.accumulate_dev(origins_t[p0:p1], part, n, N, mover_t=rows, frame_of_pose_t=zero_t[:n], static_only=True,
                                      stream=stream)
    torch.cuda.synchronize(dev)
    return seq


def dynamic_occupancy(engine, intrinsics, poses, mesh, movers=None, mover_poses=None, shapes=None, noise=None, voxel_size=0.05,
                      origin=None, dims=None, min_returns=1, static_map=True, max_range=None, chunk_poses=None):
    """``RaycastEngineHIP.dynamic_occupancy`` (bound by ``raycast_engine``; the engine is the first argument, as for the other
    scans that live beside their feature).  Scan ``poses`` (P, 4, 4) with a multi-line grid sensor over ``mesh`` and the movers
    (``movers`` a ``lidarcast.movers.MoverSet`` with ``mover_poses`` (P, M, 12), optionally ``shapes`` (P, D, 3) for its
    deformables and a ``lidarcast.noise.NoiseModel``; None: the room alone) and carve one occupancy grid PER FRAME: a
    ``DynamicOccupancyResult`` with P slots.  With ``static_map`` a one-slot result comes from the same scan: every pose mapped
    to slot 0 and the movers' returns left out (their rays still carve free space) -- the room's static map.  Returns (per-frame
    result, static map or None).  Default extent as ``occupancy_grid``: the mesh's bounds with a one-voxel margin."""
    from raycast_engine.raycast_engine_hip import mesh_arrays
    from .voxgrid import default_extent
    if hasattr(intrinsics, "swing_amplitude") or not hasattr(intrinsics, "horizontal_res"):
        raise NotImplementedError("dynamic occupancy covers multi-line grid sensors only; the dual-axis sensor and "
                                  "moving-sensor sweeps are outside its scope")
    if (origin is None) != (dims is None):
        raise ValueError("give both origin and dims, or neither (default extent)")
    if origin is None:
        origin, dims = default_extent(mesh_arrays(mesh)[0], voxel_size)
    check_grid(origin, voxel_size, dims)
    if int(min_returns) < 1:
        raise ValueError("min_returns must be >= 1")
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    reach = intrinsics.max_range if max_range is None else float(max_range)
    seq = OccupancySequence(engine.ctx, origin, voxel_size, dims, max(1, len(poses)))
    static = None
    try:
        if static_map:
            static = OccupancySequence(engine.ctx, origin, voxel_size, dims, 1)
        scan_dynamic_occupancy(engine.scene_for(mesh), seq, poses, engine._direction_table(intrinsics), reach, movers=movers,
                               mover_poses=mover_poses, shapes=shapes, noise=noise, chunk_poses=chunk_poses, static_seq=static)
        return (seq.finalize(min_returns=min_returns, dense=True),
                None if static is None else static.finalize(min_returns=min_returns, dense=True))
    finally:
        seq.close()
        if static is not None:
            static.close()
