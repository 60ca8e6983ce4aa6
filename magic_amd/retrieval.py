"""Retrieval with a trained metric model: embed every lock and every key once, score all pairs
with the model's distance, keep each lock's ``k`` best keys.

The latent distance is trained to predict the overlap area of a lock and a key, so the best key
of lock ``i`` is the one the model expects to overlap it most. The dataset pairs lock ``i`` with
key ``i``; ``hit@k`` is the share of locks whose own key is among their ``k`` best.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np


class Retrieval(NamedTuple):
    values: np.ndarray   # [n_locks, k] scores, best first
    indices: np.ndarray  # [n_locks, k] key of each score
    hit_at_1: float
    hit_at_k: float
    k: int
    order: int


def retrieve(vae, locks, keys, k: int = 10, order: int = 1, normalize: bool = True,
             return_dist: bool = False):
    """``locks``, ``keys``: uint8 tables ``[n, S, S]`` and ``[m, S, S]`` (arrays or device tensors).
    Returns a ``Retrieval`` (and the ``[n, m]`` score matrix when ``return_dist``). The distance is
    trained to equal the overlap area, so the default ``order`` +1 ranks the largest predicted
    overlap first. ``hit@1`` / ``hit@k`` judge key ``i`` for lock ``i``
    over the locks that have such a key (``i < m``)."""
    zl = vae.embed(locks, normalize=normalize)
    zk = vae.embed(keys, normalize=normalize)
    k = int(min(k, len(zk), 64))
    out = vae.match(zl, zk, k=k, order=order, return_dist=return_dist)
    val, ind = out[0], out[1]
    n = min(len(zl), len(zk))
    own = np.arange(n)[:, None]
    hit1 = float((ind[:n, :1] == own).any(1).mean())
    hitk = float((ind[:n] == own).any(1).mean())
    res = Retrieval(val, ind, hit1, hitk, k, order)
    return (res, out[2]) if return_dist else res


def report(r: Retrieval) -> str:
    return (f"retrieval over {len(r.indices)} locks: hit@1 = {r.hit_at_1:.4f}, hit@{r.k} = {r.hit_at_k:.4f} "
            f"({'largest' if r.order > 0 else 'smallest'} distance first)")
