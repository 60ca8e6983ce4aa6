#!/usr/bin/env python3
"""Maximum-overlap labels (``mvae_overlap_pairs``): ms per pair on the GPU, with the CPU restatement's
seconds per pair beside it.

  synthetic  the 960 pairs of ``BatchStream``'s synthetic pool at S = 100
  fixture    the 100 pairs of tests/golden/overlap_micro.npz at S = 200
  noise      64 pairs of ~50 % random pixels at S = 100: the bounding boxes prune nothing, so this
             is the kernel's unpruned rate (pruning is not a switch: it never changes the result)

each at 72 and 360 angles: a host clock around a device synchronise, ``--reps`` calls per window,
``--windows`` windows, median and spread over the windows. The CPU reference (tests/overlap_ref.py,
FFT per angle, one thread) is timed on ``--cpu-pairs`` pairs of each set and its areas and poses
are compared with the GPU's.

Writes profiles/overlap_bench.json. Needs the GPU: without one it fails, it never falls back.

  python tools/overlap_bench.py [--reps 3] [--windows 3] [--cpu-pairs 2] [--out ...json]
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

from magic_amd.overlap_input import BatchStream, angle_coefficients, max_overlap  # noqa: E402
from tests.overlap_ref import max_overlap_ref  # noqa: E402


def tables():
    s = BatchStream(64, 100, seed=1, synthetic_pool=960)
    z = np.load(os.path.join(ROOT, "tests", "golden", "overlap_micro.npz"))
    n, h, w = (int(v) for v in z["shape"])
    up = lambda a: torch.from_numpy((np.unpackbits(a, axis=-1)[..., :w] * 255).astype(np.uint8)).cuda()  # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(1)
    noise = lambda: ((torch.rand(64, 100, 100, device="cuda", generator=g) < 0.5) * 255).to(torch.uint8)  # noqa: E731
    return {"synthetic_960x100": (s.locks, s.keys), "fixture_100x200": (up(z["lock_bits"]), up(z["key_bits"])),
            "noise_64x100": (noise(), noise())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="calls per window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--cpu-pairs", type=int, default=2, help="pairs of each set timed on the CPU reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("overlap_bench: no GPU visible; this tool measures on the MI355X only")
    sync = torch.cuda.synchronize
    rec = {"device": torch.cuda.get_device_name(0), "calls_per_window": a.reps, "windows": a.windows,
           "note": "ms per call: host clock around a device synchronise, per window; cpu: tests/overlap_ref.py, "
                   "one thread, seconds per pair", "sets": {}}
    for name, (locks, keys) in tables().items():
        n, h, w = locks.shape
        fg = float(((locks >= 128).float().mean() + (keys >= 128).float().mean()) / 2)
        for R in (72, 360):
            area, pose = max_overlap(locks, keys, angles=R)  # warm-up, and the values
            sync()
            win = []
            for _ in range(a.windows):
                sync()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    max_overlap(locks, keys, angles=R)
                sync()
                win.append((time.perf_counter() - t0) / a.reps * 1e3)
            med = statistics.median(win)
            coef = angle_coefficients(R, h, w)
            L, K = locks[:a.cpu_pairs].cpu().numpy(), keys[:a.cpu_pairs].cpu().numpy()
            t0 = time.perf_counter()
            want = [max_overlap_ref(l, k, coef) for l, k in zip(L, K)]
            cpu = (time.perf_counter() - t0) / max(len(want), 1)
            equal = all(int(area[i]) == wa and tuple(pose[i].tolist()) == wp for i, (wa, wp) in enumerate(want))
            r = {"pairs": n, "size": [h, w], "angles": R, "foreground": round(fg, 4),
                 "ms_per_call": [round(v, 3) for v in win], "median_ms": round(med, 3),
                 "spread_ms": round(max(win) - min(win), 3), "ms_per_pair": round(med / n, 5),
                 "us_per_pair_angle": round(med / n / R * 1e3, 4), "cpu_s_per_pair": round(cpu, 3),
                 "cpu_pairs": len(want), "equal_to_cpu_reference": bool(equal),
                 "speedup_over_cpu": round(cpu * 1e3 / (med / n), 1)}
            rec["sets"][f"{name}_r{R}"] = r
            print(json.dumps({f"{name}_r{R}": r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
