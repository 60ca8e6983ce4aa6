#!/usr/bin/env python3
"""inputs() -> partial_fit with and without the fp32 X, in one process on one engine.

  route A: next(stream)        -> partial_fit(X)           make_batch writes X, the step reads it
  route B: next(fused stream)  -> partial_fit(PairBatch)   the step reads the uint8 tables

Both streams make the same seeded draws. After a warm-up of both routes the windows alternate
A B A B A B (``--steps`` each, a host clock around a device synchronise), so the A/A and B/B
spread of the run stands beside the A/B difference. Each window is timed twice over: through
``TangoEncoder.partial_fit`` (fetches the losses: one host synchronise per step, what a
``main.py`` loop pays) and through ``Engine.train_step`` (nothing fetched: the steps queue up, as
bench.py's ``pipeline`` leg runs them). Then the kernels alone, by HIP events: ``make_batch`` plus
the step's ``deinterleave`` region against its ``pairs_bits`` region, with the bytes each must
move computed from the shapes and the rate against the HBM peak of MI355X_MICROARCH.md. Writes
JSON under profiles/. Needs the GPU: without one it fails, it never falls back.

``--pairs cross`` adds the two routes over cross pairs (any lock with any key, ``BatchStream(pairs=
"cross")``) to the same run, the windows alternating A B C D:

  route C: next(cross stream)        -> partial_fit(X)          mvae_make_batch_x writes X
  route D: next(fused cross stream)  -> partial_fit(PairBatch)  mvae_train_step_xpairs

Their label cache is filled before the first window (at ``--label-angles``, whose value does not
change what the step computes), so the loops time the sampler's host work, the label gather and
the step, not the labelling of new pairs. The kernel regions are then timed ``--windows`` times in
turn, so that the spread of the own-pair region between windows (A/A) stands beside the difference
between the own-pair and the cross region, which move the same bytes.

  python tools/pipeline_bench.py --config C3 [--steps 200] [--windows 3] [--pairs cross] [--out profiles/...json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from magic_amd.config import baseline_config  # noqa: E402
from magic_amd.overlap_input import BatchStream  # noqa: E402
from magic_amd.vae import TangoEncoder  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E peak, spec
HBM_MEASURED_GBS = 6290.0  # ... and its measured float4 copy


def traffic(B, D):
    """Algorithmic bytes per batch, from shapes. The bit operands: the forward and weight-gradient
    BitMats (3 B x (D + 1) bits each, padded to 64) and the target bits (B x D)."""
    bits = 2 * 3 * B * (D + 64) // 8 + B * D // 8
    t = {"A_make_batch": {"read": 2 * B * D, "write": 12 * B * D},
         "A_deinterleave": {"read": 12 * B * D, "write": bits},
         "B_pairs_bits": {"read": 2 * B * D, "write": bits}}
    t.update({"C_make_batch": t["A_make_batch"], "C_deinterleave": t["A_deinterleave"],
              "D_pairs_bits": t["B_pairs_bits"]})
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C2", "C3", "C5"])
    ap.add_argument("--steps", type=int, default=200, help="steps per window (>= 200 for a record)")
    ap.add_argument("--windows", type=int, default=3, help="windows per route (alternating)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", choices=("own", "cross"), default="own",
                    help="cross: also routes C / D over cross pairs, in the same run")
    ap.add_argument("--label-angles", type=int, default=8, help="with --pairs cross: angles of the labels")
    a = ap.parse_args()
    cross = a.pairs == "cross"
    routes = "ABCD" if cross else "AB"
    if not torch.cuda.is_available():
        sys.exit("pipeline_bench: no GPU visible; this tool measures on the MI355X only")
    cfg = baseline_config(a.config)
    B, D = cfg.batch, cfg.D
    vae = TangoEncoder(None, config=cfg)
    eng = vae.engine
    streams = {r: BatchStream(B, cfg.image_size, normalize=True, seed=7, device=eng.dev, fused=(r == "B"))
               for r in "AB"}
    fill_s = None
    if cross:
        for r in "CD":
            streams[r] = BatchStream(B, cfg.image_size, normalize=True, seed=7, device=eng.dev, fused=(r == "D"),
                                     labels="computed", label_angles=a.label_angles, pairs="cross")
        torch.cuda.synchronize(eng.dev)
        t0 = time.perf_counter()
        streams["C"].pair_labels.fill()
        torch.cuda.synchronize(eng.dev)
        fill_s = time.perf_counter() - t0
        d = streams["D"].pair_labels  # one cache serves both streams: the same tables and angles
        d.matrix, d.known, d.computed = (getattr(streams["C"].pair_labels, k) for k in ("matrix", "known", "computed"))
    sync = lambda: torch.cuda.synchronize(eng.dev)  # noqa: E731
    losses, dist = torch.empty(5, device=eng.dev), torch.empty(B, device=eng.dev)
    loops = {
        "partial_fit": lambda s: vae.partial_fit(*next(s)),
        "train_step": lambda s: eng.train_step(*next(s), None, losses_out=losses, dist_out=dist),
    }
    for r in routes:
        for loop in loops.values():
            for _ in range(a.warmup):
                loop(streams[r])
    sync()
    res = {}
    for name, loop in loops.items():
        win = {r: [] for r in routes}
        for _ in range(a.windows):
            for r in routes:
                sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loop(streams[r])
                sync()
                win[r].append((time.perf_counter() - t0) / a.steps * 1e3)
        res[name] = {}
        for r in routes:
            res[name].update({f"{r}_ms_per_step": [round(v, 4) for v in win[r]],
                              f"{r}_median": round(statistics.median(win[r]), 4),
                              f"{r}_spread": round(max(win[r]) - min(win[r]), 4)})
        print(f"{a.config} {name}: " + " ".join(f"{r} {win[r]}" for r in routes) + " ms/step", flush=True)
    # the kernels alone: HIP events
    nk = 20
    tr = traffic(B, D)
    xa, _ = next(streams["A"])
    pb, areas = next(streams["B"])
    jobs = [("A", pb, xa, "deinterleave"), ("B", pb, pb, "pairs_bits")]
    if cross:
        xc, _ = next(streams["C"])
        pd, _ = next(streams["D"])
        jobs += [("C", pd, xc, "deinterleave"), ("D", pd, pd, "pairs_bits")]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kwin = {}
    for _ in range(a.windows):  # every kernel once per window, in turn
        for r, src, x, region in jobs:
            if x is not src:  # the producer of the materialising routes
                e0.record()
                for _ in range(nk):
                    src.materialize(out=x)
                e1.record()
                e1.synchronize()
                kwin.setdefault(r + "_make_batch", []).append(e0.elapsed_time(e1) / nk)
            eng.timing_reset()
            eng.timing_enable(True)
            if region in eng.timing_names():  # (a region exists once it has run: the warm-up ran both)
                eng.timing_select(region)
            for _ in range(nk):
                eng.train_step(x, areas, None)
            sync()
            t = eng.timing_read()
            eng.timing_enable(False)
            eng.timing_select(None)
            if region not in t:
                sys.exit(f"pipeline_bench: route {r} never ran region {region}: {sorted(t)}")
            kwin.setdefault(f"{r}_{region}", []).append(t[region][0] / t[region][1])
    kern = {k: statistics.median(v) for k, v in kwin.items()}
    kernels = {}
    for k, ms in kern.items():
        by = tr[k]["read"] + tr[k]["write"]
        gbs = by / (ms * 1e-3) / 1e9
        kernels[k] = {"avg_ms": round(ms, 4), "windows_ms": [round(v, 4) for v in kwin[k]],
                      "spread_ms": round(max(kwin[k]) - min(kwin[k]), 4),
                      "read_bytes": tr[k]["read"], "write_bytes": tr[k]["write"],
                      "gbs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                      "frac_of_measured_copy": round(gbs / HBM_MEASURED_GBS, 4)}
        print(f"{a.config} {k}: {ms * 1e3:.1f} us {[round(v * 1e3, 1) for v in kwin[k]]}, {by / 1e6:.1f} MB, "
              f"{gbs:.0f} GB/s", flush=True)
    rec = {"config": a.config, "batch": B, "image_size": cfg.image_size, "precision": cfg.precision,
           "steps_per_window": a.steps, "windows_per_route": a.windows, "order": " ".join(routes) * a.windows,
           "pairs": a.pairs,
           "device": torch.cuda.get_device_name(eng.dev), "loops": res, "kernels": kernels,
           "kernels_A_ms": round(kern["A_make_batch"] + kern["A_deinterleave"], 4),
           "kernels_B_ms": round(kern["B_pairs_bits"], 4),
           "x_bytes_not_materialised": 12 * B * D, "hbm_peak_gbs": HBM_PEAK_GBS,
           **({"kernels_C_ms": round(kern["C_make_batch"] + kern["C_deinterleave"], 4),
               "kernels_D_ms": round(kern["D_pairs_bits"], 4),
               "cross_minus_own_pairs_bits_ms": round(kern["D_pairs_bits"] - kern["B_pairs_bits"], 4),
               "own_pairs_bits_spread_ms": round(max(kwin["B_pairs_bits"]) - min(kwin["B_pairs_bits"]), 4),
               "label_angles": a.label_angles, "label_fill_s": round(fill_s, 3),
               "label_pairs": int(streams["C"].pair_labels.computed)} if cross else {}),
           "note": "ms/step: host clock around a device synchronise, per window; kernels: HIP events; bytes: "
                   "algorithmic, from shapes (the rotated lock's gathers re-read the lock image from cache and "
                   "are not counted)"}
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                f"{'xpairs_pipeline' if cross else 'pipeline_bench'}_{a.config.lower()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"config": a.config, "loops": res, "kernels_A_ms": rec["kernels_A_ms"],
                      "kernels_B_ms": rec["kernels_B_ms"], "out": out}))
    vae.close()


if __name__ == "__main__":
    main()
