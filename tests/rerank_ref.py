"""TEST INFRASTRUCTURE ONLY. CPU restatement (numpy) of verified retrieval, the quantities
``mvae_rerank`` and ``mvae_overlap_place`` compute (``include/mvae.h``), built on
``tests/overlap_ref.max_overlap_ref`` (area and pose of one pair) and
``oracle.input_oracle.rotate_nearest`` (the batch producer's rotation):

  rerank   pair (i, c) = lock lock_idx[i] (None: i) with key cand[i][c]; a negative key is an empty
           entry (area -1, pose 0). Each row is ordered by area, larger first; ties keep the column
           order of ``cand``, empties come last in their column order (a stable sort by -area).
  place    P[y, x] = Kr_r[y - dy, x - dx] inside the image, 0 outside; overlay = Lb | 2 P;
           stats = (|Lb|, |Kr_r|, |P|, |Lb & P|). A pose out of range (r outside [0, n_rot),
           |dy| >= H or |dx| >= W): the lock alone and (|Lb|, -1, -1, -1).
"""
from __future__ import annotations

import numpy as np

from oracle.input_oracle import rotate_nearest
from tests.overlap_ref import max_overlap_ref


def pair_table(locks: np.ndarray, keys: np.ndarray, coef: np.ndarray):
    """(area int32 [n, m], pose int32 [n, m, 3]) of every lock with every key: the reference a test
    computes once and shares."""
    n, m = len(locks), len(keys)
    area = np.zeros((n, m), np.int32)
    pose = np.zeros((n, m, 3), np.int32)
    for i in range(n):
        for j in range(m):
            area[i, j], pose[i, j] = max_overlap_ref(locks[i], keys[j], coef)
    return area, pose


def stable_order(areas: np.ndarray) -> np.ndarray:
    """[N, R] areas (empties -1) -> order [N, R]: order[i, t] is the column that takes rank t."""
    return np.argsort(-np.asarray(areas, np.int64), axis=1, kind="stable")


def rerank_ref(cand: np.ndarray, area_tab: np.ndarray, pose_tab: np.ndarray, lock_idx=None):
    """(key, area, pose, src), int32 [N, R] ([N, R, 3] for pose), from ``pair_table``'s tables."""
    cand = np.asarray(cand, np.int64)
    n, r = cand.shape
    li = np.arange(n) if lock_idx is None else np.asarray(lock_idx, np.int64)
    empty = cand < 0
    kj = np.where(empty, 0, cand)
    area = np.where(empty, -1, area_tab[li[:, None], kj])
    pose = np.where(empty[..., None], 0, pose_tab[li[:, None], kj])
    src = stable_order(area)
    take = lambda a: np.take_along_axis(a, src, axis=1)  # noqa: E731
    key = np.where(empty, -1, cand)
    pose_o = np.take_along_axis(pose, src[..., None], axis=1)
    return take(key).astype(np.int32), take(area).astype(np.int32), pose_o.astype(np.int32), src.astype(np.int32)


def place_ref(lock_u8: np.ndarray, key_u8: np.ndarray, coef: np.ndarray, pose):
    """(overlay uint8 [H, W], stats int32 [4]) of one pair at pose (r, dy, dx)."""
    lb = np.asarray(lock_u8) >= 128
    h, w = lb.shape
    coef = np.asarray(coef, np.float32).reshape(-1, 4)
    r, dy, dx = (int(v) for v in pose)
    if not (0 <= r < len(coef) and abs(dy) < h and abs(dx) < w):
        return lb.astype(np.uint8), np.array([lb.sum(), -1, -1, -1], np.int32)
    kr = rotate_nearest((np.asarray(key_u8) >= 128).astype(np.uint8), coef[r]).astype(bool)
    p = np.zeros_like(kr)
    # P[y, x] = Kr[y - dy, x - dx]: rows max(dy, 0) .. min(h, h + dy) - 1 take rows y - dy of Kr
    y0, y1, x0, x1 = max(dy, 0), min(h, h + dy), max(dx, 0), min(w, w + dx)
    p[y0:y1, x0:x1] = kr[y0 - dy:y1 - dy, x0 - dx:x1 - dx]
    overlay = lb.astype(np.uint8) | (p.astype(np.uint8) << 1)
    return overlay, np.array([lb.sum(), kr.sum(), p.sum(), (lb & p).sum()], np.int32)
