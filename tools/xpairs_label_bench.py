#!/usr/bin/env python3
"""What the labels of cross pairs cost while a ``PairLabels`` cache fills.

Two figures, written as JSON under profiles/:

* the labelling cost per new pair: ``PairLabels.lookup`` of batches whose pairs are all new and all
  distinct, over the synthetic pool at ``--image-size``, a host clock around a device synchronise
  (the time includes the host's bitmap, the index upload and the scatter: what a training loop
  pays), at each of ``--angles``;
* how long the cache keeps missing: the sampler's own draws (``BatchStream``'s permutation of the
  locks and ``draw_keys``) replayed on the host for a pool of ``--pool`` pairs and batches of
  ``--batch`` -- the number of new pairs per step, the first step without one, and the step after
  which none is left. No GPU is needed for this part (``--no-gpu`` runs it alone).

  python tools/xpairs_label_bench.py [--image-size 100] [--pool 960] [--batch 4096] [--angles 72 360]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from magic_amd.overlap_input import draw_keys  # noqa: E402


def replay(pool, batch, cross, seed=7, max_steps=20000):
    """New pairs per step of a cross stream over a pool x pool cache that starts with the own pairs."""
    rng = np.random.default_rng(seed)
    known = np.zeros(pool * pool, dtype=bool)
    known[np.arange(pool) * (pool + 1)] = True  # the stream's own labels are looked up first
    perm, pos = np.empty(0, np.int64), 0
    new, first_zero = [], None
    reachable = pool * pool if cross > 0 else pool
    for step in range(max_steps):
        idx = []
        n = batch
        while n > 0:  # BatchStream._take
            if pos >= len(perm):
                perm, pos = rng.permutation(pool), 0
            k = min(n, len(perm) - pos)
            idx.append(perm[pos:pos + k])
            pos += k
            n -= k
        idx = np.concatenate(idx)
        rng.uniform(0.0, 2 * np.pi, batch)  # the angles
        key = draw_keys(rng, idx, pool, cross)
        miss = np.unique((idx * pool + key)[~known[idx * pool + key]])
        known[miss] = True
        new.append(int(miss.size))
        if miss.size == 0 and first_zero is None:
            first_zero = step
        if int(known.sum()) == reachable:
            break
    total = int(known.sum()) - pool
    marks = [s for s in (0, 1, 10, 50, 100, 200, 500, 1000, 1500, 2000, 3000, 5000) if s < len(new)]
    cum = np.cumsum(new)
    return {"cross": cross, "steps_run": len(new), "first_step_without_a_new_pair": first_zero,
            "step_after_which_the_cache_is_full": len(new) - 1 if int(known.sum()) == reachable else None,
            "pairs_labelled": total, "new_pairs_at_step": {str(s): new[s] for s in marks},
            "share_labelled_after_step": {str(s): round(float(cum[s]) / (pool * pool - pool), 4) for s in marks}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=100)
    ap.add_argument("--pool", type=int, default=960)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--angles", type=int, nargs="+", default=[72, 360])
    ap.add_argument("--batches", type=int, default=3, help="fully new batches timed per angle count")
    ap.add_argument("--no-gpu", action="store_true", help="only the host replay of the sampler")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"image_size": a.image_size, "pool": a.pool, "batch": a.batch,
           "cache_fill": [replay(a.pool, a.batch, c) for c in (1.0, 0.5, 0.1)]}
    for r in rec["cache_fill"]:
        print(json.dumps(r), flush=True)
    if not a.no_gpu:
        import torch
        from magic_amd.overlap_input import BatchStream, PairLabels
        if not torch.cuda.is_available():
            sys.exit("xpairs_label_bench: no GPU visible (use --no-gpu for the host replay alone)")
        s = BatchStream(64, a.image_size, seed=7, synthetic_pool=a.pool)
        rng = np.random.default_rng(11)
        rec["device"] = torch.cuda.get_device_name(0)
        rec["labelling"] = []
        for R in a.angles:
            pl = PairLabels(s.locks, s.keys, angles=R)
            pl.lookup([0], [0])  # warm-up: allocations, the first launch
            flat = rng.permutation(a.pool * a.pool - 1)[:a.batches * a.batch] + 1  # distinct, never pair (0, 0)
            ms = []
            for b in range(a.batches):
                f = flat[b * a.batch:(b + 1) * a.batch]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pl.lookup(f // a.pool, f % a.pool)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            assert pl.computed == 1 + a.batches * a.batch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pl.lookup(flat[:a.batch] // a.pool, flat[:a.batch] % a.pool)  # all known: the gather alone
            torch.cuda.synchronize()
            hit = (time.perf_counter() - t0) * 1e3
            r = {"angles": R, "new_batch_ms": [round(v, 3) for v in ms],
                 "ms_per_new_pair": round(float(np.median(ms)) / a.batch, 6), "known_batch_ms": round(hit, 3)}
            rec["labelling"].append(r)
            print(json.dumps(r), flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "xpairs_labels.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": out}))


if __name__ == "__main__":
    main()
