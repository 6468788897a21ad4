"""Skinned deforming movers: the host side (include/lidarcast.h "skinned deforming movers").

A skinned deformable has a rest mesh, up to four bone influences per vertex (``bone_index`` (V, 4) uint8, ``bone_weight`` (V, 4)
float32; an unused influence carries weight 0) and a clip of K key poses ``poses12`` (K, B, 12) float32, each bone pose the
row-major 3 x 4 [A | c] of a mover pose.  ``apply`` skins the rest shape under one pose by the inline function the kernel calls
(lrc_skin_apply, no GPU); ``keyframes`` does so for every key pose: the (K, V, 3) array a keyframe ``Deformable`` would be
made from.  ``Skeleton`` turns per-bone rotations into skinning matrices by forward kinematics, and bone matrices into joint
positions -- the ground truth of LiDAR human-pose estimation.  ``lidarcast.deform.SkinnedDeformable`` is the device side.
"""
import numpy as np

from . import _capi
from ._capi import check


def influences(rest, bone_index, bone_weight):
    """The three per-vertex arrays as the library takes them: (V, 3) float32, (V, 4) uint8, (V, 4) float32, contiguous."""
    r = np.ascontiguousarray(np.asarray(rest), dtype=np.float32)
    if r.ndim != 2 or r.shape[1] != 3:
        raise ValueError("rest must be (V, 3)")
    i = np.asarray(bone_index)
    if i.shape != (len(r), 4):
        raise ValueError(f"bone_index must be (V, 4) = ({len(r)}, 4), got {i.shape}")
    if i.size and (i.dtype.kind not in "ui" or i.min() < 0 or i.max() > 255):
        raise ValueError("bone_index must hold integers 0 .. 255")
    w = np.asarray(bone_weight)
    if w.shape != (len(r), 4):
        raise ValueError(f"bone_weight must be (V, 4) = ({len(r)}, 4), got {w.shape}")
    return r, np.ascontiguousarray(i, dtype=np.uint8), np.ascontiguousarray(w, dtype=np.float32)


def clip_poses(poses12):
    """(K, B, 12) float32, contiguous."""
    p = np.ascontiguousarray(np.asarray(poses12), dtype=np.float32)
    if p.ndim != 3 or p.shape[2] != 12:
        raise ValueError("poses12 must be (K, B, 12)")
    return p


def apply(rest, bone_index, bone_weight, bones12):
    """lrc_skin_apply: the (V, 3) float32 vertices of the rest shape under ONE pose ``bones12`` (B, 12); no GPU.  All four
    influences are evaluated, in index order: p_j = A_j x + c_j, v = ((w0 p_0 + w1 p_1) + w2 p_2) + w3 p_3, float32 with one
    rounding per operation."""
    lib = _capi.load()
    r, i, w = influences(rest, bone_index, bone_weight)
    b = np.ascontiguousarray(np.asarray(bones12), dtype=np.float32)
    if b.ndim != 2 or b.shape[1] != 12:
        raise ValueError("bones12 must be (B, 12)")
    out = np.empty_like(r)
    check(lib.lrc_skin_apply(r.ctypes.data, len(r), i.ctypes.data, w.ctypes.data, b.ctypes.data, len(b), out.ctypes.data),
          "lrc_skin_apply")
    return out


def keyframes(rest, bone_index, bone_weight, poses12):
    """The (K, V, 3) float32 host-skinned keyframes of a clip: ``apply`` under each of the K key poses."""
    p = clip_poses(poses12)
    r, i, w = influences(rest, bone_index, bone_weight)
    return np.stack([apply(r, i, w, p[k]) for k in range(len(p))]) if len(p) else np.zeros((0, len(r), 3), np.float32)


class Skeleton:
    """B bones in a tree: ``parents`` (B,) the parent of each bone, -1 for a root, every parent before its children;
    ``joints_rest`` (B, 3) each bone's joint (the point it turns about) in the rest shape."""

    def __init__(self, parents, joints_rest):
        self.parents = np.asarray(parents, dtype=np.int64).reshape(-1)
        self.joints_rest = np.asarray(joints_rest, dtype=np.float64).reshape(-1, 3)
        B = len(self.parents)
        if not 1 <= B <= 255 or len(self.joints_rest) != B:
            raise ValueError("a skeleton has 1 to 255 bones and one rest joint per bone")
        if any(not -1 <= p < b for b, p in enumerate(self.parents)):
            raise ValueError("every parent must precede its children (-1: a root)")
        if not np.isfinite(self.joints_rest).all():
            raise ValueError("rest joints must be finite")

    def __len__(self):
        return len(self.parents)

    def matrices(self, rotations, root_translation=None):
        """Forward kinematics about the rest joints, in float64: ``rotations`` (..., B, 3, 3) turns each bone about its own
        joint relative to its parent, ``root_translation`` (..., 3) moves every root.  Bone b maps a rest point x to
        M_parent(j_b + R_b (x - j_b)), a root to j_b + R_b (x - j_b) + translation: A_b = A_parent R_b and
        c_b = A_parent (j_b - R_b j_b) + c_parent.  Identity rotations give identity matrices exactly.  Returns (..., B, 12),
        narrowed to float32 once."""
        R = np.asarray(rotations, dtype=np.float64)
        B = len(self)
        if R.ndim < 3 or R.shape[-3:] != (B, 3, 3):
            raise ValueError(f"rotations must be (..., {B}, 3, 3)")
        lead = R.shape[:-3]
        t = np.zeros(lead + (3,)) if root_translation is None else np.broadcast_to(np.asarray(root_translation, np.float64), lead + (3,))
        A = np.empty(lead + (B, 3, 3))
        c = np.empty(lead + (B, 3))
        j = self.joints_rest
        for b, p in enumerate(self.parents):
            own = j[b] - np.einsum("...ij,j->...i", R[..., b, :, :], j[b])      # x -> j_b + R_b (x - j_b); exactly 0 for R_b = I
            if p < 0:
                A[..., b, :, :] = R[..., b, :, :]
                c[..., b, :] = own + t
            else:
                A[..., b, :, :] = A[..., p, :, :] @ R[..., b, :, :]
                c[..., b, :] = np.einsum("...ij,...j->...i", A[..., p, :, :], own) + c[..., p, :]
        return np.concatenate([A, c[..., None]], -1).reshape(lead + (B, 12)).astype(np.float32)

    def joints(self, bones12):
        """The (..., B, 3) float64 joint positions under the bone matrices ``bones12`` (..., B, 12): A_b j_b + c_b."""
        m = np.asarray(bones12, dtype=np.float64)
        if m.shape[-2:] != (len(self), 12):
            raise ValueError(f"bones12 must be (..., {len(self)}, 12)")
        m = m.reshape(m.shape[:-1] + (3, 4))
        return np.einsum("...bij,bj->...bi", m[..., :3], self.joints_rest) + m[..., 3]
