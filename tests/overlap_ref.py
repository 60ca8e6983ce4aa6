"""TEST INFRASTRUCTURE ONLY. CPU restatement (numpy) of the maximum overlap of a lock and a key,
the quantity ``mvae_overlap_pairs`` computes (``include/mvae.h``):

  Lb, Kb     foreground = table byte >= 128
  Kr_r       the key rotated by coef[r] = (cos, sin, x_off, y_off), bit for bit
             ``oracle.input_oracle.rotate_nearest`` (the batch producer's rotation)
  ov(r, dy, dx) = sum_{y,x} Lb[y, x] * Kr_r[y - dy, x - dx],  |dy| <= H - 1, |dx| <= W - 1
  area       max ov;  pose = the lexicographically smallest (r, dy, dx) reaching it,
             (0, 0, 0) when the area is 0.

The correlation map of one angle is computed by zero-padded FFT and rounded: its values are
integers <= H * W <= 65536 and the transforms' error is many orders below 0.5 in float64.
"""
from __future__ import annotations

import numpy as np

from oracle.input_oracle import rotate_nearest


def overlap_maps(lock_u8: np.ndarray, key_u8: np.ndarray, coef: np.ndarray) -> np.ndarray:
    """int64 [n_rot, 2H - 1, 2W - 1]: ov(r, dy, dx) at index [r, dy + H - 1, dx + W - 1]."""
    lb = (np.asarray(lock_u8) >= 128).astype(np.float64)
    kb = (np.asarray(key_u8) >= 128).astype(np.uint8)
    h, w = lb.shape
    coef = np.asarray(coef, np.float32).reshape(-1, 4)
    fh, fw = 2 * h - 1, 2 * w - 1
    fl = np.fft.rfft2(lb, s=(fh, fw))
    maps = np.empty((len(coef), fh, fw), np.int64)
    for r, cf in enumerate(coef):
        kr = rotate_nearest(kb, cf).astype(np.float64)
        # correlation = convolution with the key flipped: c[i, j] = sum L[y, x] Kf[i - y, j - x],
        # Kf[a, b] = Kr[H - 1 - a, W - 1 - b]  =>  c[dy + H - 1, dx + W - 1] = ov(r, dy, dx)
        c = np.fft.irfft2(fl * np.fft.rfft2(kr[::-1, ::-1], s=(fh, fw)), s=(fh, fw))
        maps[r] = np.rint(c).astype(np.int64)
    return maps


def max_overlap_ref(lock_u8: np.ndarray, key_u8: np.ndarray, coef: np.ndarray):
    """(area, (r, dy, dx)) of one pair: the largest overlap and its first pose in (r, dy, dx) order."""
    maps = overlap_maps(lock_u8, key_u8, coef)
    h, w = np.asarray(lock_u8).shape
    area = int(maps.max())
    if area == 0:
        return 0, (0, 0, 0)
    r, i, j = np.unravel_index(int(np.argmax(maps)), maps.shape)  # first maximum in C order
    return area, (int(r), int(i) - (h - 1), int(j) - (w - 1))


def angle_coefficients(n_rot: int, height: int, width: int) -> np.ndarray:
    """coef [n_rot, 4] of the angles 2 pi r / n_rot (float64, cast to fp32), as ``max_overlap(angles=R)``."""
    from oracle.input_oracle import rotation_coefficients
    ang = (2.0 * np.pi * np.arange(n_rot, dtype=np.float64) / n_rot).astype(np.float32)
    return rotation_coefficients(ang, height, width)
