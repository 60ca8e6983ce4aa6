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

  python tools/pipeline_bench.py --config C3 [--steps 200] [--windows 3] [--out profiles/...json]
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
    return {"A_make_batch": {"read": 2 * B * D, "write": 12 * B * D},
            "A_deinterleave": {"read": 12 * B * D, "write": bits},
            "B_pairs_bits": {"read": 2 * B * D, "write": bits}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C2", "C3", "C5"])
    ap.add_argument("--steps", type=int, default=200, help="steps per window (>= 200 for a record)")
    ap.add_argument("--windows", type=int, default=3, help="windows per route (alternating)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pipeline_bench: no GPU visible; this tool measures on the MI355X only")
    cfg = baseline_config(a.config)
    B, D = cfg.batch, cfg.D
    vae = TangoEncoder(None, config=cfg)
    eng = vae.engine
    streams = {r: BatchStream(B, cfg.image_size, normalize=True, seed=7, device=eng.dev, fused=(r == "B"))
               for r in "AB"}
    sync = lambda: torch.cuda.synchronize(eng.dev)  # noqa: E731
    losses, dist = torch.empty(5, device=eng.dev), torch.empty(B, device=eng.dev)
    loops = {
        "partial_fit": lambda s: vae.partial_fit(*next(s)),
        "train_step": lambda s: eng.train_step(*next(s), None, losses_out=losses, dist_out=dist),
    }
    for r in "AB":
        for loop in loops.values():
            for _ in range(a.warmup):
                loop(streams[r])
    sync()
    res = {}
    for name, loop in loops.items():
        win = {"A": [], "B": []}
        for _ in range(a.windows):
            for r in "AB":
                sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loop(streams[r])
                sync()
                win[r].append((time.perf_counter() - t0) / a.steps * 1e3)
        res[name] = {
            "A_ms_per_step": [round(v, 4) for v in win["A"]], "B_ms_per_step": [round(v, 4) for v in win["B"]],
            "A_median": round(statistics.median(win["A"]), 4), "B_median": round(statistics.median(win["B"]), 4),
            "A_spread": round(max(win["A"]) - min(win["A"]), 4), "B_spread": round(max(win["B"]) - min(win["B"]), 4),
        }
        print(f"{a.config} {name}: A {win['A']} B {win['B']} ms/step", flush=True)
    # the kernels alone: HIP events
    nk = 20
    tr = traffic(B, D)
    xa, _ = next(streams["A"])
    pb, areas = next(streams["B"])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(nk):
        pb.materialize(out=xa)
    e1.record()
    e1.synchronize()
    kern = {"A_make_batch": e0.elapsed_time(e1) / nk}
    for r, x, region in (("A", xa, "deinterleave"), ("B", pb, "pairs_bits")):
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
        kern[("A_" if r == "A" else "B_") + region] = t[region][0] / t[region][1]
    kernels = {}
    for k, ms in kern.items():
        by = tr[k]["read"] + tr[k]["write"]
        gbs = by / (ms * 1e-3) / 1e9
        kernels[k] = {"avg_ms": round(ms, 4), "read_bytes": tr[k]["read"], "write_bytes": tr[k]["write"],
                      "gbs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                      "frac_of_measured_copy": round(gbs / HBM_MEASURED_GBS, 4)}
        print(f"{a.config} {k}: {ms * 1e3:.1f} us, {by / 1e6:.1f} MB, {gbs:.0f} GB/s", flush=True)
    rec = {"config": a.config, "batch": B, "image_size": cfg.image_size, "precision": cfg.precision,
           "steps_per_window": a.steps, "windows_per_route": a.windows, "order": "A B " * a.windows,
           "device": torch.cuda.get_device_name(eng.dev), "loops": res, "kernels": kernels,
           "kernels_A_ms": round(kern["A_make_batch"] + kern["A_deinterleave"], 4),
           "kernels_B_ms": round(kern["B_pairs_bits"], 4),
           "x_bytes_not_materialised": 12 * B * D, "hbm_peak_gbs": HBM_PEAK_GBS,
           "note": "ms/step: host clock around a device synchronise, per window; kernels: HIP events; bytes: "
                   "algorithmic, from shapes (the rotated lock's gathers re-read the lock image from cache and "
                   "are not counted)"}
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                f"pipeline_bench_{a.config.lower()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"config": a.config, "loops": res, "kernels_A_ms": rec["kernels_A_ms"],
                      "kernels_B_ms": rec["kernels_B_ms"], "out": out}))
    vae.close()


if __name__ == "__main__":
    main()
