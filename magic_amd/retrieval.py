"""Retrieval with a trained metric model: embed every lock and every key once, score all pairs
with the model's distance, keep each lock's ``k`` best keys.

The latent distance is trained to predict the overlap area of a lock and a key, so the best key
of lock ``i`` is the one the model expects to overlap it most. The dataset pairs lock ``i`` with
key ``i``; ``hit@k`` is the share of locks whose own key is among their ``k`` best.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch


class Retrieval(NamedTuple):
    values: np.ndarray   # [n_locks, k] scores, best first
    indices: np.ndarray  # [n_locks, k] key of each score
    hit_at_1: float
    hit_at_k: float
    k: int
    order: int
    ranks: Optional[np.ndarray] = None   # [min(n, m)] keys ahead of key i for lock i (0: it is the best)
    mrr: Optional[float] = None          # mean of 1 / (ranks + 1)
    median_rank: Optional[float] = None  # median of ranks + 1
    true_hit_at_1: Optional[float] = None  # share of locks whose truly best key (``truth``) comes first
    true_hit_at_k: Optional[float] = None  # ... or is among the k returned
    # filled only by ``retrieve(rerank=R)``: the list above is then the k best of the model's R by exact area
    areas: Optional[np.ndarray] = None      # [n_locks, k] exact overlap area of each returned key
    poses: Optional[np.ndarray] = None      # [n_locks, k, 3] its pose (angle index, dy, dx)
    shortlist: Optional[np.ndarray] = None  # [n_locks, R] the model's list before verification
    moved: Optional[float] = None           # share of locks whose first key changed
    area_regret: Optional[float] = None     # with ``truth``: mean of truth[i].max() - truth[i, indices[i, 0]]


def _sharded(vae, locks, keys, k, order, normalize, return_dist, shard, ranks):
    """``retrieve`` over a gallery in pieces: at most ``shard`` images per ``embed`` call, the
    embeddings kept on the host between the sweeps, one shard of key embeddings on the device at a
    time; the lists carried from shard to shard, the ranks counted in the scoring pass."""
    eng = vae.engine
    n, m = len(locks), len(keys)
    step = int(shard) if shard else max(n, m)
    if step < 1:
        raise ValueError("retrieve: shard must be at least 1")
    zl = torch.from_numpy(np.concatenate([vae.embed(locks[i:i + step], normalize=normalize)
                                          for i in range(0, n, step)])).to(eng.dev)
    zk = [(j, vae.embed(keys[j:j + step], normalize=normalize)) for j in range(0, m, step)]  # host
    up = lambda a: torch.from_numpy(a).to(eng.dev)  # noqa: E731
    rl = rk = None
    if vae.config.metric == "cosine":  # the norms of the whole galleries, summed shard by shard
        cl = ck = None
        for i in range(0, n, step):
            cl = eng.match_colsq(zl[i:i + step], out=cl, accumulate=cl is not None)
        for _, z in zk:
            ck = eng.match_colsq(up(z), out=ck, accumulate=ck is not None)
        rl, rk = eng.match_rnorm(cl), eng.match_rnorm(ck)
    k = int(min(k, m, 64))
    nn = min(n, m)
    val = torch.full((n, k), float("nan"), device=eng.dev)
    ind = torch.full((n, k), -1, device=eng.dev, dtype=torch.int32)
    dist = torch.empty(n, m, device=eng.dev) if return_dist else None
    target = ahead = None
    if ranks:  # lock i's threshold entry: its score against key i, at index i (none for i >= m)
        tv = torch.full((n,), float("nan"), device=eng.dev)
        ti = torch.full((n,), -1, device=eng.dev, dtype=torch.int32)
        ti[:nn] = torch.arange(nn, device=eng.dev, dtype=torch.int32)
        for j, z in zk:
            c = min(j + len(z), nn) - j
            if c > 0:
                tv[j:j + c] = eng.pair_scores(zl[j:j + c], up(z[:c]), rl, rk)
        target, ahead = (tv, ti), torch.zeros(n, device=eng.dev, dtype=torch.int32)
    for j, z in zk:
        eng.match(zl, up(z), k, order=order, rl=rl, rk=rk, key_base=j, carry=(val, ind), target=target, ahead=ahead,
                  dist_out=None if dist is None else dist[:, j:j + len(z)])
    out = (val.cpu().numpy(), ind.cpu().numpy()) + ((dist.cpu().numpy(),) if return_dist else ())
    return out + ((ahead[:nn].cpu().numpy(),) if ranks else ())


def overlap_matrix(locks, keys, angles=360, chunk: int = 1 << 16) -> np.ndarray:
    """The true label of every pair: ``[n, m]`` int32, entry (i, j) = ``max_overlap`` of lock ``i``
    and key ``j`` over ``angles``. uint8 tables ``[n, H, W]`` and ``[m, H, W]`` (arrays or device
    tensors); the index lists of at most ``chunk`` pairs at a time are built on the device."""
    from .overlap_input import max_overlap
    dev = locks.device if isinstance(locks, torch.Tensor) and locks.is_cuda else torch.device("cuda")
    up = lambda t: torch.as_tensor(t).to(dev).contiguous()  # noqa: E731
    locks, keys = up(locks), up(keys)
    n, m = len(locks), len(keys)
    if chunk < 1:
        raise ValueError("overlap_matrix: chunk must be at least 1")
    out = torch.empty(n * m, dtype=torch.int32, device=dev)
    for p0 in range(0, n * m, chunk):
        p = torch.arange(p0, min(p0 + chunk, n * m), device=dev, dtype=torch.int64)
        li = torch.div(p, m, rounding_mode="floor").to(torch.int32)
        ki = (p % m).to(torch.int32)
        out[p0:p0 + len(p)] = max_overlap(locks, keys, li, ki, angles=angles)[0]
    return out.view(n, m).cpu().numpy()


def retrieve(vae, locks, keys, k: int = 10, order: int = 1, normalize: bool = True,
             return_dist: bool = False, shard: Optional[int] = None, ranks: bool = False, truth=None,
             rerank: Optional[int] = None, rerank_angles=360):
    """``locks``, ``keys``: uint8 tables ``[n, S, S]`` and ``[m, S, S]`` (arrays or device tensors).
    Returns a ``Retrieval`` (and the ``[n, m]`` score matrix when ``return_dist``). The distance is
    trained to equal the overlap area, so the default ``order`` +1 ranks the largest predicted
    overlap first. ``hit@1`` / ``hit@k`` judge key ``i`` for lock ``i``
    over the locks that have such a key (``i < m``).

    ``shard``: embed at most that many images per call and match the keys shard by shard (only one
    shard of key embeddings is on the device at a time); the lists are those of the one-shot call
    (for a cosine preset bit for bit when ``shard`` is a multiple of 256, else to the rounding of
    the fp64 column sums). ``ranks``: also, for each lock ``i < m``, how many keys rank before key
    ``i`` (``Retrieval.ranks``, 0 = best), counted in the scoring pass without the score matrix,
    with ``mrr`` and ``median_rank`` (1-based) of them. ``truth``: an ``[n, m]`` matrix of true labels
    (``overlap_matrix``); ``true_hit_at_1`` / ``true_hit_at_k`` are then the share of locks whose
    truly best key (the largest entry of its row, the smallest index on ties) is the first / among the
    ``k`` returned.

    ``rerank=R`` (k <= R <= min(m, 64)): retrieve, then verify. The model's ``R`` best keys of every lock
    (the same one-shot or sharded path with ``k`` replaced by ``R``) are the shortlist; the exact overlap
    and pose of those n R pairs over ``rerank_angles`` are computed on the device
    (``overlap_input.rerank``; both tables go there whole, as for ``overlap_matrix``), each list is
    ordered by exact area (ties keep the model's order) and ``indices`` / ``values`` are its ``k`` best
    with each key's model score. Every hit rate is then judged on that verified list, and ``areas``,
    ``poses``, ``shortlist``, ``moved`` and (with ``truth``) ``area_regret`` are filled."""
    if rerank is not None:
        if not (1 <= k <= rerank <= min(len(keys), 64)):
            raise ValueError(f"retrieve: rerank must satisfy k <= rerank <= min(m, 64) (k = {k}, rerank = {rerank}, "
                             f"m = {len(keys)})")
    k_out, k = k, (k if rerank is None else int(rerank))
    if truth is not None:
        truth = truth.cpu().numpy() if isinstance(truth, torch.Tensor) else np.asarray(truth)
        if truth.shape != (len(locks), len(keys)):
            raise ValueError(f"retrieve: truth must be [{len(locks)}, {len(keys)}], not {list(truth.shape)}")
    if shard is not None or ranks:
        out = _sharded(vae, locks, keys, k, order, normalize, return_dist, shard, ranks)
    else:
        out = _one_shot(vae, locks, keys, k, order, normalize, return_dist)
    val, ind = out[0], out[1]
    verified = (None,) * 5
    if rerank is not None:
        val, ind, verified = _verify(locks, keys, val, ind, k_out, rerank_angles, truth)
    k = val.shape[1]
    n = min(len(val), len(keys))
    own = np.arange(n)[:, None]
    hit1 = float((ind[:n, :1] == own).any(1).mean())
    hitk = float((ind[:n] == own).any(1).mean())
    extra = (None, None, None)
    if ranks:
        r = out[-1].astype(np.int64)
        extra = (r, float((1.0 / (r + 1)).mean()), float(np.median(r + 1)))
    if truth is not None:
        best = np.argmax(truth, axis=1)[:, None]  # the first maximum of a row
        extra += (float((ind[:, :1] == best).any(1).mean()), float((ind == best).any(1).mean()))
    else:
        extra += (None, None)
    res = Retrieval(val, ind, hit1, hitk, k, order, *extra, *verified)
    return (res, out[2]) if return_dist else res


def _verify(locks, keys, val, ind, k, angles, truth):
    """The model's lists ``val`` / ``ind`` [n, R] -> the k best of each by exact area, with the model's
    score of each key, and the ``Retrieval`` fields of the verified list."""
    from .overlap_input import rerank
    dev = locks.device if isinstance(locks, torch.Tensor) and locks.is_cuda else torch.device("cuda")
    up = lambda t: torch.as_tensor(t).to(dev).contiguous()  # noqa: E731
    cand = torch.from_numpy(np.ascontiguousarray(ind, dtype=np.int32)).to(dev)
    key, area, pose, src = (t.cpu().numpy() for t in rerank(up(locks), up(keys), cand, angles=angles))
    score = np.take_along_axis(val, src.astype(np.int64), axis=1)
    moved = float((key[:, 0] != ind[:, 0]).mean())
    regret = None
    if truth is not None:
        regret = float((truth.max(1) - truth[np.arange(len(truth)), key[:, 0]]).mean())
    return score[:, :k], key[:, :k], (area[:, :k], pose[:, :k], np.asarray(ind), moved, regret)


def placed(r: Retrieval, locks, keys, rank: int = 0, angles=360):
    """Each lock with its ``rank``-th verified key at that key's pose: ``(overlay uint8 [n, H, W], stats
    int32 [n, 4])`` device tensors of ``overlap_input.place``; ``stats[:, 3]`` is ``r.areas[:, rank]``.
    ``r`` comes from ``retrieve(..., rerank=R, rerank_angles=angles)`` over the same tables."""
    from .overlap_input import place
    if r.areas is None:
        raise ValueError("placed: the Retrieval holds no poses; call retrieve(..., rerank=R)")
    if not 0 <= rank < r.indices.shape[1]:
        raise ValueError(f"placed: rank must be in [0, {r.indices.shape[1]})")
    dev = locks.device if isinstance(locks, torch.Tensor) and locks.is_cuda else torch.device("cuda")
    up = lambda t: torch.as_tensor(t).to(dev).contiguous()  # noqa: E731
    n = len(r.indices)
    dn = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
    return place(up(locks), up(keys), torch.arange(n, dtype=torch.int32, device=dev), dn(r.indices[:, rank]),
                 dn(r.poses[:, rank]), angles=angles)


def _one_shot(vae, locks, keys, k, order, normalize, return_dist):
    zl = vae.embed(locks, normalize=normalize)
    zk = vae.embed(keys, normalize=normalize)
    k = int(min(k, len(zk), 64))
    return vae.match(zl, zk, k=k, order=order, return_dist=return_dist)


def report(r: Retrieval) -> str:
    s = (f"retrieval over {len(r.indices)} locks: hit@1 = {r.hit_at_1:.4f}, hit@{r.k} = {r.hit_at_k:.4f} "
         f"({'largest' if r.order > 0 else 'smallest'} distance first)")
    if r.ranks is not None:
        s += f", MRR = {r.mrr:.4f}, median rank = {r.median_rank:g} over {len(r.ranks)} locks"
    if r.true_hit_at_1 is not None:
        s += f"; truly best key: hit@1 = {r.true_hit_at_1:.4f}, hit@{r.k} = {r.true_hit_at_k:.4f}"
    if r.areas is not None:
        s += (f"; verified: the hit rates are of the model's {r.shortlist.shape[1]} best ordered by exact overlap, "
              f"first key moved for {r.moved:.4f} of the locks, mean area of the first key = {r.areas[:, 0].mean():.1f}")
        if r.area_regret is not None:
            s += f", area regret = {r.area_regret:.2f}"
    return s
