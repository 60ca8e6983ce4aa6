"""Batch producer with the reference's layout (``11a/overlap_input.py:76-261``), assembled on
the GPU by the HIP kernel ``mvae_make_batch``.

``inputs(normalize=True, reshape=True, rotation=True)`` returns a ``BatchStream``; each
``next(stream)`` (the reference's ``sess.run([images_batch, labels_batch])``) yields

  images: float32 [B, H*W*3] — per pixel (h*W+w) three channels (lock, rotated lock, key),
          ``tf.concat([lock, rotated_lock, key], axis=2)`` (``:201``) reshaped (``:117-119``),
          divided by 255 (``:113-115``);
  labels: float32 [B] overlap areas.

Sources: a directory or .zip of ``{N}_L.png`` / ``{N}_K.png`` pairs with an areas array
(``.npy``), or the synthetic shape generator (``synthetic=True``; BASELINE.json asks for
100x100 synthetic pairs). The rotated lock is the lock rotated by U[0, 2pi) about the image
centre with nearest-neighbour sampling and zero fill, the ``tf.contrib.image.rotate``
semantics (``11a/utils.py:453-464``); decoded images live in HBM as uint8 tables and each
batch is gathered, rotated, interleaved and normalised by one HIP kernel.
"""
from __future__ import annotations

import io
import math
import os
import zipfile
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from .constants import FLAGS


def rotation_coefficients(angles, height: int, width: int) -> np.ndarray:
    """Per-example ``tf.contrib.image.rotate`` coefficients (cos, sin, x_off, y_off), float32
    as TF's ``angles_to_projective_transforms`` computes them; [B] radians -> [B, 4]."""
    a = np.asarray(angles, np.float32)
    c = np.cos(a).astype(np.float32)
    s = np.sin(a).astype(np.float32)
    w1, h1 = np.float32(width - 1), np.float32(height - 1)
    xo = ((w1 - (c * w1 - s * h1)) / np.float32(2.0)).astype(np.float32)
    yo = ((h1 - (s * w1 + c * h1)) / np.float32(2.0)).astype(np.float32)
    return np.ascontiguousarray(np.stack([c, s, xo, yo], axis=1), dtype=np.float32)


def make_batch(locks: torch.Tensor, keys: torch.Tensor, idx: torch.Tensor, coef: torch.Tensor,
               out: Optional[torch.Tensor] = None, normalize: bool = True,
               key_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """HIP batch producer (``mvae_make_batch``): uint8 device tables [n, H, W], idx int32 [B],
    coef float32 [B, 4] -> X float32 [B, H*W*3] = per pixel (lock, rotated lock, key) / 255
    (``normalize=False``: the raw 0..255 values, ``11a/overlap_input.py:113-115``). ``key_idx`` int32
    [B] (``mvae_make_batch_x``): row b takes key ``key_idx[b]`` of a key table [m, H, W] instead of
    key ``idx[b]``."""
    from . import _lib
    lib = _lib.load()
    n, h, w = locks.shape
    B = idx.shape[0]
    for t, dt in ((locks, torch.uint8), (keys, torch.uint8), (idx, torch.int32), (coef, torch.float32)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise ValueError("make_batch: device tensors (uint8 tables, int32 idx, float32 coef) expected")
    out = out if out is not None else torch.empty(B, 3 * h * w, device=locks.device)
    st = torch.cuda.current_stream(locks.device).cuda_stream
    if key_idx is not None:
        if not key_idx.is_cuda or key_idx.dtype != torch.int32 or not key_idx.is_contiguous() \
                or key_idx.shape != idx.shape:
            raise ValueError("make_batch: key_idx must be an int32 device tensor of idx's shape")
        if keys.dim() != 3 or tuple(keys.shape[1:]) != (h, w):
            raise ValueError("make_batch: the key table must share H and W with the lock table")
        rc = lib.mvae_make_batch_x(locks.data_ptr(), keys.data_ptr(), h, w, idx.data_ptr(), key_idx.data_ptr(),
                                   coef.data_ptr(), B, 255.0 if normalize else 1.0, out.data_ptr(), st)
        _lib.check(lib, None, rc)
        return out
    rc = lib.mvae_make_batch(locks.data_ptr(), keys.data_ptr(), h, w, idx.data_ptr(), coef.data_ptr(),
                             B, 255.0 if normalize else 1.0, out.data_ptr(), st)
    _lib.check(lib, None, rc)
    return out


def angle_coefficients(angles, height: int, width: int) -> np.ndarray:
    """The rotations ``max_overlap`` searches: an int R means the angles ``2 pi r / R`` (float64, cast
    to fp32), anything else an array of radians; through ``rotation_coefficients`` -> [n_rot, 4]."""
    if isinstance(angles, (int, np.integer)):
        if angles < 1:
            raise ValueError("max_overlap: at least one angle expected")
        angles = (2.0 * np.pi * np.arange(int(angles), dtype=np.float64) / int(angles)).astype(np.float32)
    a = np.asarray(angles, np.float32).reshape(-1)
    if a.size < 1:
        raise ValueError("max_overlap: at least one angle expected")
    return rotation_coefficients(a, height, width)


def max_overlap(locks: torch.Tensor, keys: torch.Tensor, lock_idx: Optional[torch.Tensor] = None,
                key_idx: Optional[torch.Tensor] = None, angles=360) -> Tuple[torch.Tensor, torch.Tensor]:
    """The label the distance is trained on, computed (``mvae_overlap_pairs``): for pair ``i`` of
    lock ``lock_idx[i]`` and key ``key_idx[i]`` (``None``: ``i``), the largest number of foreground
    pixels (byte >= 128) the lock shares with the key rotated by one of ``angles`` (the batch
    producer's nearest-neighbour rotation) and shifted by whole pixels. uint8 device tables
    [n, H, W] and [m, H, W], int32 device index lists [count] -> (areas int32 [count], pose int32
    [count, 3] = the smallest (angle index, dy, dx) reaching the area; (0, 0, 0) for area 0)."""
    from . import _lib
    lib = _lib.load()
    for t in (locks, keys):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous() \
                or t.dim() != 3:
            raise ValueError("max_overlap: contiguous uint8 device tables [n, H, W] expected")
    if keys.shape[1:] != locks.shape[1:] or keys.device != locks.device:
        raise ValueError("max_overlap: the tables must share H, W and the device")
    for t in (lock_idx, key_idx):
        if t is not None and (not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 1):
            raise ValueError("max_overlap: int32 device index lists [count] expected")
    if lock_idx is not None and key_idx is not None and lock_idx.shape != key_idx.shape:
        raise ValueError("max_overlap: lock_idx and key_idx must have one length")
    given = lock_idx if lock_idx is not None else key_idx
    count = given.shape[0] if given is not None else min(locks.shape[0], keys.shape[0])
    if (lock_idx is None and count > locks.shape[0]) or (key_idx is None and count > keys.shape[0]):
        raise ValueError("max_overlap: more pairs than images in the table without an index list")
    h, w = int(locks.shape[1]), int(locks.shape[2])
    dev = locks.device
    coef = torch.from_numpy(angle_coefficients(angles, h, w)).to(dev)
    n_rot = coef.shape[0]
    areas = torch.empty(count, dtype=torch.int32, device=dev)
    pose = torch.empty(count, 3, dtype=torch.int32, device=dev)
    nbytes = lib.mvae_overlap_work_bytes(count, n_rot, h, w)
    work = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        rc = lib.mvae_overlap_pairs(locks.data_ptr(), keys.data_ptr(), h, w, ptr(lock_idx), ptr(key_idx), count,
                                    coef.data_ptr(), n_rot, areas.data_ptr(), pose.data_ptr(), work.data_ptr(),
                                    torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib, None, rc)
    return areas, pose


def _check_tables(what: str, locks, keys):
    for t in (locks, keys):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous() \
                or t.dim() != 3:
            raise ValueError(f"{what}: contiguous uint8 device tables [n, H, W] expected")
    if keys.shape[1:] != locks.shape[1:] or keys.device != locks.device:
        raise ValueError(f"{what}: the tables must share H, W and the device")


def _is_list(t, dim: int) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() \
        and t.dim() == dim


def rerank(locks: torch.Tensor, keys: torch.Tensor, cand: torch.Tensor, lock_idx: Optional[torch.Tensor] = None,
           angles=360) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """A shortlist verified (``mvae_rerank``): ``cand`` int32 device ``[N, R]``, R <= 64, holds for lock
    ``lock_idx[i]`` (``None``: ``i``) the keys a model proposes, best first; a negative entry is empty.
    Every listed pair gets its exact ``max_overlap`` over ``angles`` and each row is ordered by that area
    (larger first, ties in ``cand``'s order, empties last). uint8 device tables as for ``max_overlap``.
    Returns int32 device tensors ``(keys [N, R], areas [N, R], poses [N, R, 3], src [N, R])``: -1, -1 and
    (0, 0, 0) for empties; ``src`` is the column of ``cand`` an entry came from."""
    from . import _lib
    lib = _lib.load()
    _check_tables("rerank", locks, keys)
    if not _is_list(cand, 2) or cand.shape[0] < 1 or not 1 <= cand.shape[1] <= 64:
        raise ValueError("rerank: cand must be an int32 device tensor [N, R] with N >= 1 and 1 <= R <= 64")
    if lock_idx is not None and (not _is_list(lock_idx, 1) or lock_idx.shape[0] != cand.shape[0]):
        raise ValueError("rerank: lock_idx must be an int32 device list [N]")
    N, R = int(cand.shape[0]), int(cand.shape[1])
    if lock_idx is None and N > locks.shape[0]:
        raise ValueError("rerank: more rows than locks in the table without an index list")
    h, w = int(locks.shape[1]), int(locks.shape[2])
    dev = locks.device
    coef = torch.from_numpy(angle_coefficients(angles, h, w)).to(dev)
    n_rot = coef.shape[0]
    new = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)  # noqa: E731
    key_o, area_o, pose_o, src_o = new(N, R), new(N, R), new(N, R, 3), new(N, R)
    nbytes = lib.mvae_rerank_work_bytes(N, R, n_rot, h, w)
    work = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.mvae_rerank(locks.data_ptr(), keys.data_ptr(), h, w,
                             lock_idx.data_ptr() if lock_idx is not None else None, cand.data_ptr(), N, R,
                             coef.data_ptr(), n_rot, key_o.data_ptr(), area_o.data_ptr(), pose_o.data_ptr(),
                             src_o.data_ptr(), work.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib, None, rc)
    return key_o, area_o, pose_o, src_o


def place(locks: torch.Tensor, keys: torch.Tensor, lock_idx: Optional[torch.Tensor],
          key_idx: Optional[torch.Tensor], pose: torch.Tensor, angles=360) -> Tuple[torch.Tensor, torch.Tensor]:
    """A key shown at a pose (``mvae_overlap_place``): for pair ``i`` of lock ``lock_idx[i]`` and key
    ``key_idx[i]`` (``None``: ``i``) and ``pose[i] = (angle index, dy, dx)`` (int32 device ``[count, 3]``, as
    ``max_overlap`` / ``rerank`` return them, over the same ``angles``) -> ``(overlay uint8 [count, H, W],
    stats int32 [count, 4])``: overlay bit 0 is the lock's foreground, bit 1 the key's after the rotation
    and the shift; stats = (lock pixels, rotated key pixels, of those inside the image after the shift,
    shared pixels = the area). A pose out of range shows the lock alone with stats (lock pixels, -1, -1,
    -1)."""
    from . import _lib
    lib = _lib.load()
    _check_tables("place", locks, keys)
    if not _is_list(pose, 2) or pose.shape[0] < 1 or pose.shape[1] != 3:
        raise ValueError("place: pose must be an int32 device tensor [count, 3] with count >= 1")
    count = int(pose.shape[0])
    for t, table in ((lock_idx, locks), (key_idx, keys)):
        if t is not None and (not _is_list(t, 1) or t.shape[0] != count):
            raise ValueError("place: int32 device index lists [count] expected")
        if t is None and count > table.shape[0]:
            raise ValueError("place: more pairs than images in the table without an index list")
    h, w = int(locks.shape[1]), int(locks.shape[2])
    dev = locks.device
    coef = torch.from_numpy(angle_coefficients(angles, h, w)).to(dev)
    overlay = torch.empty(count, h, w, dtype=torch.uint8, device=dev)
    stats = torch.empty(count, 4, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        rc = lib.mvae_overlap_place(locks.data_ptr(), keys.data_ptr(), h, w, ptr(lock_idx), ptr(key_idx), count,
                                    coef.data_ptr(), coef.shape[0], pose.data_ptr(), overlay.data_ptr(),
                                    stats.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib, None, rc)
    return overlay, stats


class PairBatch:
    """One batch described by its sources instead of materialised: the uint8 device tables
    ``locks`` / ``keys`` [n, H, W], the example ``idx`` int32 [B] of each row and its rotation
    ``coef`` float32 [B, 4] (``rotation_coefficients``). ``Engine`` and ``TangoEncoder`` take it
    wherever they take X (``mvae_*_pairs``): where the step writes its layer-0 bit operands, one
    HIP kernel reads them straight from the tables, and no [B, H*W*3] float32 array exists.
    ``materialize()`` is that array, ``make_batch(...)``: the results are bitwise the same.

    ``key_idx`` int32 [B]: a cross-pair batch (``mvae_*_xpairs``) -- row b is lock ``idx[b]``, its
    rotation, and key ``key_idx[b]`` of a key table [m, H, W] that only has to share H and W with
    ``locks``. Without it the batch takes the own-pair entry points, untouched."""

    def __init__(self, locks: torch.Tensor, keys: torch.Tensor, idx: torch.Tensor, coef: torch.Tensor,
                 normalize: bool = True, key_idx: Optional[torch.Tensor] = None):
        for t, dt in ((locks, torch.uint8), (keys, torch.uint8), (idx, torch.int32), (coef, torch.float32)):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise ValueError("PairBatch: device tensors (uint8 tables, int32 idx, float32 coef) expected")
        if key_idx is None:
            tables = locks.dim() == 3 and keys.shape == locks.shape
        else:
            tables = locks.dim() == 3 and keys.dim() == 3 and keys.shape[1:] == locks.shape[1:]
            if not key_idx.is_cuda or key_idx.dtype != torch.int32 or not key_idx.is_contiguous() \
                    or key_idx.shape != idx.shape:
                raise ValueError("PairBatch: key_idx must be an int32 device tensor of idx's shape")
        if not tables or idx.dim() != 1 or coef.shape != (idx.shape[0], 4):
            raise ValueError("PairBatch: tables [n, H, W] of one shape (with key_idx: of one H, W), idx [B], "
                             "coef [B, 4] expected")
        self.locks, self.keys, self.idx, self.coef = locks, keys, idx, coef
        self.key_idx = key_idx
        self.normalize = bool(normalize)

    @property
    def shape(self):
        return (self.idx.shape[0], 3 * self.locks.shape[1] * self.locks.shape[2])

    @property
    def device(self):
        return self.locks.device

    def materialize(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return make_batch(self.locks, self.keys, self.idx, self.coef, out=out, normalize=self.normalize,
                          key_idx=self.key_idx)


class PairLabels:
    """The labels of the pairs a sampler draws: a lazily filled ``[n, m]`` int32 device matrix of
    ``max_overlap`` areas over ``angles``, -1 where not yet computed. Which entries exist is kept in
    a host bitmap, so a lookup decides what is missing without waiting for the device.
    ``max_pairs`` bounds n*m (the default to a 256 MB matrix): a stated limit, not a measurement."""

    def __init__(self, locks: torch.Tensor, keys: torch.Tensor, angles=360, max_pairs: int = 1 << 26):
        for t in (locks, keys):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 3 \
                    or not t.is_contiguous():
                raise ValueError("PairLabels: contiguous uint8 device tables [n, H, W] expected")
        if keys.shape[1:] != locks.shape[1:] or keys.device != locks.device:
            raise ValueError("PairLabels: the tables must share H, W and the device")
        self.n, self.m = int(locks.shape[0]), int(keys.shape[0])
        if self.n * self.m > max_pairs:
            raise ValueError(f"PairLabels: {self.n} x {self.m} pairs exceed max_pairs = {max_pairs}")
        self.locks, self.keys, self.angles = locks, keys, angles
        self.matrix = torch.full((self.n, self.m), -1, dtype=torch.int32, device=locks.device)
        self.known = np.zeros(self.n * self.m, dtype=bool)
        self.computed = 0  # distinct pairs labelled so far

    def _compute(self, flat: np.ndarray):
        """Label the distinct, missing pairs ``flat`` (= i*m + j, int64) with one ``max_overlap`` call."""
        dev = self.locks.device
        li = torch.from_numpy((flat // self.m).astype(np.int32)).to(dev)
        ki = torch.from_numpy((flat % self.m).astype(np.int32)).to(dev)
        areas = max_overlap(self.locks, self.keys, li, ki, angles=self.angles)[0]
        self.matrix.view(-1)[torch.from_numpy(flat).to(dev)] = areas
        self.known[flat] = True
        self.computed += int(flat.size)

    def lookup(self, lock_idx, key_idx) -> torch.Tensor:
        """float32 device areas [B] of the pairs (``lock_idx[b]``, ``key_idx[b]``), host integer
        arrays; the pairs not yet in the matrix are deduplicated and computed first."""
        li = np.asarray(lock_idx, dtype=np.int64).reshape(-1)
        kj = np.asarray(key_idx, dtype=np.int64).reshape(-1)
        if li.shape != kj.shape:
            raise ValueError("PairLabels.lookup: lock_idx and key_idx must have one length")
        if li.size and (li.min() < 0 or li.max() >= self.n or kj.min() < 0 or kj.max() >= self.m):
            raise ValueError("PairLabels.lookup: an index is outside its table")
        flat = li * self.m + kj
        miss = np.unique(flat[~self.known[flat]])
        if miss.size:
            self._compute(miss)
        return self.matrix.view(-1)[torch.from_numpy(flat).to(self.matrix.device)].float()

    def fill(self, chunk: int = 1 << 16) -> torch.Tensor:
        """Compute every missing entry, at most ``chunk`` pairs per call; returns the matrix (what
        ``retrieval.retrieve(truth=)`` takes)."""
        if chunk < 1:
            raise ValueError("PairLabels.fill: chunk must be at least 1")
        miss = np.flatnonzero(~self.known)
        for p0 in range(0, miss.size, chunk):
            self._compute(miss[p0:p0 + chunk])
        return self.matrix


def random_shapes(n: int, size: int, gen: torch.Generator, device) -> torch.Tensor:
    """Binary images {0,1} of 1-3 random filled ellipses/rectangles (foreground ~3-15%, like
    the reference's overlap_micro PNGs), [n, size, size] float32."""
    dev = torch.device(device)
    ys, xs = torch.meshgrid(torch.arange(size, dtype=torch.float32),
                            torch.arange(size, dtype=torch.float32), indexing="ij")
    ys, xs = ys.to(dev), xs.to(dev)
    img = torch.zeros(n, size, size, device=dev)
    for _ in range(3):
        u = torch.rand(n, 7, generator=gen).to(dev)
        cx, cy = (0.25 + 0.5 * u[:, 0]) * size, (0.25 + 0.5 * u[:, 1]) * size
        ra, rb = (0.05 + 0.12 * u[:, 2]) * size, (0.05 + 0.12 * u[:, 3]) * size
        th = u[:, 4] * math.pi
        keep = (u[:, 5] < 0.7).float().reshape(n, 1, 1)
        kind = (u[:, 6] < 0.5).reshape(n, 1, 1)
        dx = xs[None] - cx.reshape(n, 1, 1)
        dy = ys[None] - cy.reshape(n, 1, 1)
        ct, st = torch.cos(th).reshape(n, 1, 1), torch.sin(th).reshape(n, 1, 1)
        px, py = ct * dx + st * dy, -st * dx + ct * dy
        ell = (px / ra.reshape(n, 1, 1)) ** 2 + (py / rb.reshape(n, 1, 1)) ** 2 <= 1.0
        rect = (px.abs() <= ra.reshape(n, 1, 1)) & (py.abs() <= rb.reshape(n, 1, 1))
        m = torch.where(kind, ell, rect).float() * keep
        img = torch.maximum(img, m)
    return img


# areas resampled from the reference's 2a/OVERLAP_AREAS empirical
# distribution (range 296-6426). magic_amd/data/overlap_areas.npy holds the 2000 values (package
# data, extracted as text without unpickling by tests/golden/make_golden.py); a log-normal fit is
# the fallback when the table is absent.
_AREAS_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "overlap_areas.npy")


def area_distribution() -> np.ndarray:
    if os.path.exists(_AREAS_FIXTURE):
        return np.load(_AREAS_FIXTURE).astype(np.float32)
    rng = np.random.default_rng(1)
    return np.clip(np.exp(rng.normal(7.4, 0.62, 2000)), 296, 6426).round().astype(np.float32)


def draw_keys(rng: np.random.Generator, idx: np.ndarray, m: int, cross: float,
              candidates: Optional[np.ndarray] = None) -> np.ndarray:
    """The key of each row of a cross-pair batch, int64 [B]. Exactly two draws, in this order:
    ``u = rng.random(B)``, ``kj = rng.integers(0, m, B)``. A row with ``u < cross`` takes key ``kj``
    -- or, with ``candidates`` int [n, k] (a lock's mined keys), ``candidates[idx, kj % k]`` --
    and every other row keeps its own key ``idx``."""
    idx = np.asarray(idx, dtype=np.int64)
    B = idx.shape[0]
    u = rng.random(B)
    kj = rng.integers(0, m, B)
    pick = kj if candidates is None else np.asarray(candidates)[idx, kj % np.asarray(candidates).shape[1]]
    return np.where(u < cross, pick, idx).astype(np.int64)


def _check_labels(labels: str) -> bool:
    if labels not in ("sampled", "computed"):
        raise ValueError(f"labels must be 'sampled' or 'computed', not {labels!r}")
    return labels == "computed"


def synthetic_batch(batch: int, image_size: int, seed: int = 1, device="cuda",
                    dtype=torch.float32, labels: str = "sampled",
                    label_angles=360) -> Tuple[torch.Tensor, torch.Tensor]:
    """One seeded synthetic batch (X [B, 3D] in {0,1}, areas [B]) through the HIP producer.
    ``labels="computed"``: the areas are ``max_overlap`` of each row's lock and key over
    ``label_angles`` instead of draws from the reference's recorded areas."""
    computed = _check_labels(labels)
    gen = torch.Generator().manual_seed(seed)
    dev = torch.device(device)
    lock = (random_shapes(batch, image_size, gen, device) * 255).to(torch.uint8).contiguous()
    key = (random_shapes(batch, image_size, gen, device) * 255).to(torch.uint8).contiguous()
    ang = torch.rand(batch, generator=gen).numpy() * (2 * math.pi)
    coef = torch.from_numpy(rotation_coefficients(ang, image_size, image_size)).to(dev)
    idx = torch.arange(batch, dtype=torch.int32, device=dev)
    x = make_batch(lock, key, idx, coef).to(dtype)
    dist = area_distribution()
    sel = torch.randint(0, len(dist), (batch,), generator=gen).numpy()
    areas = torch.from_numpy(dist[sel]).to(dev)
    if computed:
        areas = max_overlap(lock, key, angles=label_angles)[0].float()
    return x, areas


class PairSource:
    """Lock/key PNG pairs from a directory or a zip (``{N}_L.png``/``{N}_K.png``)."""

    def __init__(self, path: str, areas: Optional[np.ndarray] = None, limit: Optional[int] = None):
        from PIL import Image
        self.locks, self.keys = [], []
        if path.endswith(".zip"):
            z = zipfile.ZipFile(path)
            names = set(z.namelist())
            prefix = os.path.commonprefix([n for n in names if n.endswith("_L.png")]).rsplit("/", 1)
            prefix = prefix[0] + "/" if len(prefix) == 2 else ""
            read = lambda n: z.read(prefix + n)  # noqa: E731
            exists = lambda n: (prefix + n) in names  # noqa: E731
        else:
            read = lambda n: open(os.path.join(path, n), "rb").read()  # noqa: E731
            exists = lambda n: os.path.exists(os.path.join(path, n))  # noqa: E731
        i = 0
        while exists(f"{i}_L.png") and exists(f"{i}_K.png") and (limit is None or i < limit):
            for lst, nm in ((self.locks, f"{i}_L.png"), (self.keys, f"{i}_K.png")):
                a = np.array(Image.open(io.BytesIO(read(nm))).convert("L"), dtype=np.float32)
                lst.append(a)
            i += 1
        if i == 0:
            raise ValueError(f"no {{N}}_L.png/{{N}}_K.png pairs under {path}")
        self.locks = np.stack(self.locks)
        self.keys = np.stack(self.keys)
        if areas is None:
            areas = area_distribution()
        self.areas = np.asarray(areas, np.float32)[:i]

    @classmethod
    def from_packed(cls, npz_path: str, areas: Optional[np.ndarray] = None, limit: Optional[int] = None):
        """Pairs from a packed-bit archive (``lock_bits``, ``key_bits``, ``shape``) such as
        tests/golden/overlap_micro.npz, the reference's overlap_micro.zip images."""
        z = np.load(npz_path)
        n, h, w = (int(v) for v in z["shape"])
        n = n if limit is None else min(n, limit)
        self = cls.__new__(cls)
        self.locks = np.unpackbits(z["lock_bits"][:n], axis=-1)[..., :w].astype(np.float32) * 255.0
        self.keys = np.unpackbits(z["key_bits"][:n], axis=-1)[..., :w].astype(np.float32) * 255.0
        self.areas = np.asarray(areas if areas is not None else area_distribution(), np.float32)[:n]
        return self

    def __len__(self):
        return len(self.locks)


class BatchStream:
    """Shuffled epochs over a source (``slice_input_producer(shuffle=True)`` +
    ``shuffle_batch``), a uniform [0, 2pi) rotation per example, /255 normalisation — the
    per-batch assembly runs in the HIP batch producer (``mvae_make_batch``). ``fused=True``: the
    same draws yield ``(PairBatch, areas)`` and launch nothing; the step reads the tables.
    ``labels="sampled"`` (default): the areas are the source's, or for the synthetic pool draws from
    the reference's recorded areas, unrelated to the images. ``labels="computed"``: the area of pair
    ``i`` of the pool is ``max_overlap`` of its lock and key over ``label_angles``, computed once here.

    ``pairs="own"`` (default): row b is pair ``idx[b]`` of the pool. ``"cross"``: after the draws
    of ``"own"`` the stream draws a key of its own per row (``draw_keys``): with probability
    ``cross`` a uniform one of the pool, else the lock's own. ``"mined"``: the same with the drawn
    key taken from the lock's ``k`` best keys under the model as of the last
    ``refresh_candidates(vae, k)`` (uniform before the first). Both need ``labels="computed"``: the
    label of a row is ``max_overlap`` of its lock and its key, looked up in ``self.pair_labels``
    (``PairLabels``), which computes the pairs it has not seen."""

    def __init__(self, batch: int, image_size: int, source: Optional[PairSource] = None,
                 normalize: bool = True, seed: int = 1, device="cuda", synthetic_pool: int = 960,
                 reshape: bool = True, fp16: bool = False, fused: bool = False, labels: str = "sampled",
                 label_angles=360, pairs: str = "own", cross: float = 1.0):
        computed = _check_labels(labels)
        if pairs not in ("own", "cross", "mined"):
            raise ValueError(f"pairs must be 'own', 'cross' or 'mined', not {pairs!r}")
        if pairs != "own" and not computed:
            raise ValueError(f"pairs={pairs!r} needs labels='computed': a sampled label says nothing about "
                             "a lock and another lock's key")
        if not 0.0 <= cross <= 1.0:
            raise ValueError("cross must be a probability")
        self.pairs, self.cross = pairs, float(cross)
        self.candidates = None  # "mined": int [n, k], a lock's best keys under the model
        self.pair_labels = None
        if fused and (not reshape or fp16):
            raise ValueError("fused=True yields a PairBatch, not an array: reshape=False and USE_FP16 "
                             "ask for the array")
        self.fused = fused
        self.batch, self.size = batch, image_size
        self.normalize, self.reshape, self.fp16 = normalize, reshape, fp16
        self.device = torch.device(device)
        self.rng = np.random.default_rng(seed)
        if source is None:  # synthetic pool of pairs, re-rotated every draw
            g = torch.Generator().manual_seed(seed + 1000)
            lock = random_shapes(synthetic_pool, image_size, g, "cpu") * 255.0
            key = random_shapes(synthetic_pool, image_size, g, "cpu") * 255.0
            dist = area_distribution()
            idx = torch.randint(0, len(dist), (synthetic_pool,), generator=g).numpy()
            locks, keys, self.areas = lock, key, torch.from_numpy(dist[idx])
        else:
            if source.locks.shape[1] != image_size:
                raise ValueError(f"images are {source.locks.shape[1]}px, expected {image_size}")
            locks, keys = torch.from_numpy(source.locks), torch.from_numpy(source.keys)
            self.areas = torch.from_numpy(source.areas)
        self.locks = locks.round().clamp(0, 255).to(torch.uint8).contiguous().to(self.device)
        self.keys = keys.round().clamp(0, 255).to(torch.uint8).contiguous().to(self.device)
        self.areas = self.areas.float().to(self.device)
        if computed:
            self.areas = max_overlap(self.locks, self.keys, angles=label_angles)[0].float()
        if pairs != "own":
            self.pair_labels = PairLabels(self.locks, self.keys, angles=label_angles)
        self._perm = np.empty(0, dtype=np.int64)
        self._pos = 0

    def _take(self, n):
        out = []
        while n > 0:
            if self._pos >= len(self._perm):
                self._perm = self.rng.permutation(len(self.locks))
                self._pos = 0
            k = min(n, len(self._perm) - self._pos)
            out.append(self._perm[self._pos:self._pos + k])
            self._pos += k
            n -= k
        return np.concatenate(out)

    def refresh_candidates(self, vae, k: int = 16, order: int = 1) -> np.ndarray:
        """``pairs="mined"``: embed both tables with ``vae`` and keep, on the host, the ``k`` keys it
        ranks first for every lock (``order`` +1: the largest predicted overlap first, as
        ``retrieval.retrieve``) -- the pairs where the model claims the most overlap. Draws no
        random number and leaves the model's training state alone."""
        zl = vae.embed(self.locks, normalize=self.normalize)
        zk = vae.embed(self.keys, normalize=self.normalize)
        k = int(min(k, len(zk), 64))
        self.candidates = np.asarray(vae.match(zl, zk, k=k, order=order)[1], dtype=np.int64)
        return self.candidates

    def __iter__(self) -> Iterator:
        return self

    def __next__(self):
        idx = self._take(self.batch)
        ang = self.rng.uniform(0.0, 2 * math.pi, self.batch)
        coef = torch.from_numpy(rotation_coefficients(ang, self.size, self.size)).to(self.device)
        idx_t = torch.from_numpy(idx.astype(np.int32)).to(self.device)
        kidx_t = None
        if self.pairs == "own":
            a = self.areas[idx_t.long()]
        else:
            key = draw_keys(self.rng, idx, len(self.keys), self.cross,
                            self.candidates if self.pairs == "mined" else None)
            kidx_t = torch.from_numpy(key.astype(np.int32)).to(self.device)
            a = self.pair_labels.lookup(idx, key)
        if self.fused:
            return PairBatch(self.locks, self.keys, idx_t, coef, normalize=self.normalize, key_idx=kidx_t), a
        x = make_batch(self.locks, self.keys, idx_t, coef, normalize=self.normalize, key_idx=kidx_t)
        if not self.reshape:  # [B, H, W, 3] (11a/overlap_input.py:117-119 not applied)
            x = x.view(self.batch, self.size, self.size, 3)
        if self.fp16:  # FLAGS.USE_FP16 casts images and labels (11a/overlap_input.py:109-111)
            x, a = x.half(), a.half()
        return x, a


def inputs(normalize: bool = False, reshape: bool = False, rotation: bool = False,
           batch_size: Optional[int] = None, image_size: Optional[int] = None,
           data_dir: Optional[str] = None, device="cuda", seed: int = 1,
           fused: bool = False, labels: str = "sampled", label_angles=360, pairs: str = "own",
           cross: float = 1.0) -> BatchStream:
    """``11a/overlap_input.py:76-122``: images [B, H*W*3] (``reshape=True``) or [B, H, W, 3],
    divided by 255 when ``normalize``, cast to float16 with labels when ``FLAGS.USE_FP16``;
    ``rotation=False`` raises as in the reference (``:95-96``). ``fused=True`` (needs
    ``reshape=True`` and no ``USE_FP16``): images are ``PairBatch`` descriptions of the same
    batches, which ``TangoEncoder`` takes as X. ``labels`` / ``label_angles`` / ``pairs`` / ``cross``: see
    ``BatchStream``."""
    if not rotation:
        raise ValueError("Rotation has to be True.")
    size = image_size or FLAGS.IMAGE_SIZE
    bs = batch_size or FLAGS.BATCH_SIZE
    d = data_dir if data_dir is not None else FLAGS.DATA_DIR
    src = None
    if d:
        lim = FLAGS.NUM_EXAMPLES_TO_LOAD_INTO_QUEUE
        src = PairSource.from_packed(d, limit=lim) if d.endswith(".npz") else PairSource(d, limit=lim)
    return BatchStream(bs, size, src, normalize=normalize, seed=seed, device=device, reshape=reshape,
                       fp16=bool(getattr(FLAGS, "USE_FP16", False)), fused=fused, labels=labels,
                       label_angles=label_angles, pairs=pairs, cross=cross)
