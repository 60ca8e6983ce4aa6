#!/usr/bin/env python3
"""Verified retrieval (``mvae_rerank``, ``mvae_overlap_place``): ms per call on the GPU.

The synthetic pool of ``BatchStream`` at S = 100: N = 960 locks, a shortlist of R = 16 keys each
(seeded random keys of the pool), 360 angles. Three things are timed in the same run, alternating
within each window:

  rerank   ``mvae_rerank`` on the 960 x 16 lists (expansion, exact overlap of the 15 360 pairs, ordering)
  overlap  ``mvae_overlap_pairs`` on the same 15 360 pairs, given as two ready index lists: the
           yardstick -- ``rerank`` should exceed it only by the expansion and ordering launches
  place    ``mvae_overlap_place`` on 960 pairs (each lock with its best verified key at its pose)

Each is the C entry point on preallocated buffers: a host clock around a device synchronise,
``--reps`` calls per window, ``--windows`` windows, median and spread over the windows; the
difference rerank - overlap is taken window by window. The verified areas are compared with those of
the overlap call (the same pairs) before anything is timed.

Writes profiles/rerank_bench.json. Needs the GPU: without one it fails, it never falls back.

  python tools/rerank_bench.py [--reps 3] [--windows 3] [--out ...json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from magic_amd import _lib  # noqa: E402
from magic_amd.overlap_input import BatchStream, angle_coefficients  # noqa: E402

S, N, R, ANGLES = 100, 960, 16, 360


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="calls per window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rerank_bench: no GPU visible; this tool measures on the MI355X only")
    lib = _lib.load()
    sync = torch.cuda.synchronize
    st = torch.cuda.current_stream().cuda_stream
    s = BatchStream(64, S, seed=1, synthetic_pool=N)
    locks, keys = s.locks, s.keys
    cand_h = np.random.default_rng(1).integers(0, N, (N, R)).astype(np.int32)
    cand = torch.from_numpy(cand_h).cuda()
    li = torch.arange(N, dtype=torch.int32, device="cuda").repeat_interleave(R).contiguous()
    ki = cand.reshape(-1).contiguous()
    coef = torch.from_numpy(angle_coefficients(ANGLES, S, S)).cuda()
    new = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")  # noqa: E731
    key_o, area_o, pose_o, src_o = new(N, R), new(N, R), new(N, R, 3), new(N, R)
    area_p, pose_p = new(N * R), new(N * R, 3)
    work_r = torch.empty(lib.mvae_rerank_work_bytes(N, R, ANGLES, S, S) // 8, dtype=torch.int64, device="cuda")
    work_o = torch.empty(lib.mvae_overlap_work_bytes(N * R, ANGLES, S, S) // 8, dtype=torch.int64, device="cuda")
    overlay = torch.empty(N, S, S, dtype=torch.uint8, device="cuda")
    stats = new(N, 4)
    p = lambda t: t.data_ptr()  # noqa: E731

    def rerank():
        _lib.check(lib, None, lib.mvae_rerank(p(locks), p(keys), S, S, None, p(cand), N, R, p(coef), ANGLES, p(key_o),
                                              p(area_o), p(pose_o), p(src_o), p(work_r), st))

    def overlap():
        _lib.check(lib, None, lib.mvae_overlap_pairs(p(locks), p(keys), S, S, p(li), p(ki), N * R, p(coef), ANGLES,
                                                     p(area_p), p(pose_p), p(work_o), st))

    rerank()   # warm-up, and the values
    overlap()
    sync()
    best_key, best_pose = key_o[:, 0].contiguous(), pose_o[:, 0].contiguous()
    lock_i = torch.arange(N, dtype=torch.int32, device="cuda")

    def place():
        _lib.check(lib, None, lib.mvae_overlap_place(p(locks), p(keys), S, S, p(lock_i), p(best_key), N, p(coef),
                                                     ANGLES, p(best_pose), p(overlay), p(stats), st))

    place()
    sync()
    srt = torch.gather(area_p.view(N, R), 1, src_o.long())
    equal = bool(torch.equal(srt, area_o) and torch.equal(stats[:, 3], area_o[:, 0])
                 and bool((area_o[:, :-1] >= area_o[:, 1:]).all()))

    def window(fn):
        sync()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        sync()
        return (time.perf_counter() - t0) / a.reps * 1e3

    win = {"rerank": [], "overlap": [], "place": []}
    for _ in range(a.windows):  # the three alternate within a window
        win["overlap"].append(window(overlap))
        win["rerank"].append(window(rerank))
        win["place"].append(window(place))
    diff = [r - o for r, o in zip(win["rerank"], win["overlap"])]
    summ = lambda v: {"ms_per_call": [round(x, 3) for x in v], "median_ms": round(statistics.median(v), 3),  # noqa: E731
                      "spread_ms": round(max(v) - min(v), 3)}
    rec = {"device": torch.cuda.get_device_name(0), "calls_per_window": a.reps, "windows": a.windows,
           "note": "ms per call: host clock around a device synchronise, per window; the three calls alternate "
                   "within a window; rerank_minus_overlap is taken window by window",
           "size": [S, S], "locks": N, "shortlist": R, "pairs": N * R, "angles": ANGLES,
           "areas_equal_to_overlap_pairs_and_place": equal,
           "mean_first_area": round(float(area_o[:, 0].float().mean()), 1),
           "rerank": dict(summ(win["rerank"]), ms_per_pair=round(statistics.median(win["rerank"]) / (N * R), 5)),
           "overlap_pairs_same_pairs": dict(summ(win["overlap"]),
                                            ms_per_pair=round(statistics.median(win["overlap"]) / (N * R), 5)),
           "rerank_minus_overlap": summ(diff),
           "place_960_pairs": dict(summ(win["place"]), us_per_pair=round(statistics.median(win["place"]) / N * 1e3, 3))}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))
    if not equal:
        sys.exit("rerank_bench: the verified areas differ from mvae_overlap_pairs / mvae_overlap_place")


if __name__ == "__main__":
    main()
