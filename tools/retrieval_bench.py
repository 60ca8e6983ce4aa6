#!/usr/bin/env python3
"""Gallery embedding and all-pairs matching, each against the only other route to the same numbers,
in one process with alternating windows (a host clock around a device synchronise).

  embed   12 B images of one uint8 table at the configuration's shapes:
          route A: 12 ``transform`` calls on PairBatches with the images as locks (what the library
                   offered before ``mvae_embed_images``: 12 passes, two thirds of each unwanted)
          route B: one ``Engine.embed`` (4 passes, every row wanted)
          plus the ``images_bits`` kernel alone by HIP events, with its algorithmic bytes.
  match   k = 10, no stored matrix, N = M = 16384, L in {20, 200, 2000}, both metrics:
          route A: torch on the same device -- scores by matrix product, then ``torch.topk``
          route B: ``Engine.match``
          plus the achieved fraction of the 157 TF/s fp32 rate at 3 flops per element (sqdiff) or
          2 (cosine).
  sharded (--sharded; record profiles/retrieval_bench_sharded_<config>.json) the same shape, L in
          {20, 200}, both metrics:
          one_shot: ``Engine.match`` over the 16384 keys
          sharded:  8 shards of 2048 keys with ``key_base`` / ``carry`` (cosine: norms given)
          ranks_off / ranks_on: one call over all keys without / with the fused count of the keys
          before each lock's own key (cosine: norms given in both)

Writes JSON under profiles/. Needs the GPU: without one it fails, it never falls back.

  python tools/retrieval_bench.py --config C3 [--reps 5] [--windows 3] [--no-match] [--sharded] [--out ...json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from magic_amd.config import MVAEConfig, baseline_config  # noqa: E402
from magic_amd.engine import Engine  # noqa: E402
from magic_amd.overlap_input import PairBatch, rotation_coefficients  # noqa: E402

HBM_PEAK_GBS = 8000.0    # MI355X_MICROARCH.md: HBM3E peak, spec
FP32_PEAK_TFS = 157.0    # ... and the fp32 rate


def windows(routes, reps, nwin, sync):
    """routes: name -> callable. Alternating windows A B A B ...; ms per call of each window."""
    win = {r: [] for r in routes}
    for _ in range(nwin):
        for r, fn in routes.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            sync()
            win[r].append((time.perf_counter() - t0) / reps * 1e3)
    return {r: {"ms": [round(v, 4) for v in w], "median": round(statistics.median(w), 4),
                "spread": round(max(w) - min(w), 4)} for r, w in win.items()}


def bench_embed(cfg, reps, nwin):
    B, D, S = cfg.batch, cfg.D, cfg.image_size
    eng = Engine(cfg, 0)
    eng.init_params(0)
    n = 12 * B
    g = torch.Generator(device="cuda").manual_seed(1)
    table = ((torch.rand(n, S, S, device="cuda", generator=g) < 0.3) * 255).to(torch.uint8)
    coef = torch.from_numpy(rotation_coefficients(np.zeros(B, np.float32), S, S)).cuda()
    idx = [torch.arange(i * B, (i + 1) * B, dtype=torch.int32, device="cuda") for i in range(12)]
    out_a = torch.empty(n, cfg.latent, device="cuda")
    out_b = torch.empty(n, cfg.latent, device="cuda")

    def route_a():
        for i in range(12):
            eng.transform(PairBatch(table, table, idx[i], coef), out=out_a[i * B:(i + 1) * B])

    def route_b():
        eng.embed(table, out=out_b)

    sync = lambda: torch.cuda.synchronize()  # noqa: E731
    for _ in range(2):
        route_a()
        route_b()
    sync()
    equal = bool(torch.equal(out_a, out_b))  # (the same images in other rows of the same GEMMs)
    w = windows({"A_transform_x12": route_a, "B_embed": route_b}, reps, nwin, sync)
    a, b = w["A_transform_x12"]["median"], w["B_embed"]["median"]
    # the kernel alone
    eng.timing_reset()
    eng.timing_enable(True)
    kern = None
    if "images_bits" in eng.timing_names():
        eng.timing_select("images_bits")
        for _ in range(5):
            route_b()
        sync()
        t = eng.timing_read()["images_bits"]
        ms = t[0] / t[1]
        rd, wr = 3 * B * D, 3 * B * (D + 64) // 8 + B * D // 8  # table bytes; forward BitMat + target bits
        kern = {"avg_us": round(ms * 1e3, 1), "read_bytes": rd, "write_bytes": wr,
                "gbs": round((rd + wr) / (ms * 1e-3) / 1e9, 1),
                "frac_of_hbm_peak": round((rd + wr) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    eng.timing_enable(False)
    eng.timing_select(None)
    eng.close()
    return {"images": n, "windows": w, "us_per_image_A": round(a * 1e3 / n, 3), "us_per_image_B": round(b * 1e3 / n, 3),
            "speedup_B_over_A": round(a / b, 3), "meets_2x": bool(a / b >= 2.0),
            "bitwise_equal_A_B": equal, "images_bits_kernel": kern}


def torch_route(metric, zl, zk, k):
    """The scores as a matrix (written, then read back by topk), the same distance definitions."""
    if metric == "cosine":
        a = zl * torch.rsqrt(torch.clamp((zl * zl).sum(0), min=1e-12))
        b = zk * torch.rsqrt(torch.clamp((zk * zk).sum(0), min=1e-12))
        return torch.topk(a @ b.T, k, dim=1)
    d = (zl * zl).sum(1)[:, None] + (zk * zk).sum(1)[None, :] - 2.0 * (zl @ zk.T)
    return torch.topk(d, k, dim=1, largest=False)


def bench_match(reps, nwin, n=16384, k=10):
    out = {}
    sync = lambda: torch.cuda.synchronize()  # noqa: E731
    for L in (20, 200, 2000):
        for metric in ("sqdiff", "cosine"):
            eng = Engine(MVAEConfig(image_size=8, batch=64, enc=(40,), dec=(28, 20), latent=L, metric=metric,
                                    reciprocal=False, precision="f32"), 0)
            g = torch.Generator(device="cuda").manual_seed(L)
            zl = torch.randn(n, L, device="cuda", generator=g)
            zk = torch.randn(n, L, device="cuda", generator=g)
            order = 1 if metric == "cosine" else -1
            routes = {"A_torch": lambda: torch_route(metric, zl, zk, k),
                      "B_match": lambda: eng.match(zl, zk, k, order=order)}
            for fn in routes.values():
                fn()
            sync()
            agree = float((routes["A_torch"]()[1] == routes["B_match"]()[1].long()).float().mean())
            w = windows(routes, reps, nwin, sync)
            a, b = w["A_torch"], w["B_match"]
            flops = (3 if metric == "sqdiff" else 2) * n * n * L
            out[f"L{L}_{metric}"] = {
                "windows": w, "index_agreement_with_torch": round(agree, 5),
                "B_tflops": round(flops / (b["median"] * 1e-3) / 1e12, 2),
                "B_frac_of_fp32_peak": round(flops / (b["median"] * 1e-3) / 1e12 / FP32_PEAK_TFS, 4),
                "no_slower_beyond_spread": bool(b["median"] <= a["median"] + max(a["spread"], b["spread"])),
            }
            print(f"match L={L} {metric}: torch {a['median']} ms, match {b['median']} ms", flush=True)
            eng.close()
    return out


def bench_sharded(reps, nwin, n=16384, k=10, shards=8):
    out = {}
    sync = lambda: torch.cuda.synchronize()  # noqa: E731
    step = n // shards
    for L in (20, 200):
        for metric in ("sqdiff", "cosine"):
            eng = Engine(MVAEConfig(image_size=8, batch=64, enc=(40,), dec=(28, 20), latent=L, metric=metric,
                                    reciprocal=False, precision="f32"), 0)
            g = torch.Generator(device="cuda").manual_seed(L)
            zl = torch.randn(n, L, device="cuda", generator=g)
            zk = torch.randn(n, L, device="cuda", generator=g)
            order = 1 if metric == "cosine" else -1
            rl = rk = None
            if metric == "cosine":
                rl, rk = eng.match_rnorm(eng.match_colsq(zl)), eng.match_rnorm(eng.match_colsq(zk))
            tv = eng.pair_scores(zl, zk, rl, rk)
            ti = torch.arange(n, device="cuda", dtype=torch.int32)
            ahead = torch.zeros(n, device="cuda", dtype=torch.int32)

            def sharded():
                carry = None
                for j in range(0, n, step):
                    carry = eng.match(zl, zk[j:j + step], k, order=order, rl=rl, rk=rk, key_base=j, carry=carry)
                return carry

            routes = {"one_shot": lambda: eng.match(zl, zk, k, order=order),
                      "sharded": sharded,
                      "ranks_off": lambda: eng.match(zl, zk, k, order=order, rl=rl, rk=rk),
                      "ranks_on": lambda: eng.match(zl, zk, k, order=order, rl=rl, rk=rk, target=(tv, ti), ahead=ahead)}
            res = {r: fn() for r, fn in routes.items()}
            sync()
            equal = all(bool(torch.equal(res[r][0].view(torch.int32), res["one_shot"][0].view(torch.int32))
                             and torch.equal(res[r][1], res["one_shot"][1])) for r in routes)
            w = windows(routes, reps, nwin, sync)
            out[f"L{L}_{metric}"] = {
                "windows": w, "lists_bitwise_equal_to_one_shot": equal,
                "sharded_over_one_shot": round(w["sharded"]["median"] / w["one_shot"]["median"], 3),
                "ranks_on_over_off": round(w["ranks_on"]["median"] / w["ranks_off"]["median"], 3),
                "mean_rank_of_own_key": round(float(res["ranks_on"][2].float().mean()), 1)}
            print(f"sharded L={L} {metric}: " + ", ".join(f"{r} {w[r]['median']} ms" for r in routes), flush=True)
            eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C2", "C3"])
    ap.add_argument("--reps", type=int, default=5, help="calls per window")
    ap.add_argument("--windows", type=int, default=3, help="windows per route (alternating)")
    ap.add_argument("--no-match", action="store_true", help="the embedding comparison only")
    ap.add_argument("--sharded", action="store_true",
                    help="the sharded-sweep and ranks legs only (record retrieval_bench_sharded_<config>.json)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retrieval_bench: no GPU visible; this tool measures on the MI355X only")
    cfg = baseline_config(a.config)
    rec = {"config": a.config, "batch": cfg.batch, "image_size": cfg.image_size, "precision": cfg.precision,
           "latent": cfg.latent, "calls_per_window": a.reps, "windows_per_route": a.windows,
           "order": "A B " * a.windows, "device": torch.cuda.get_device_name(0),
           "note": "ms per call: host clock around a device synchronise, per window; kernel: HIP events; bytes: "
                   "algorithmic, from shapes"}
    if a.sharded:
        rec["order"] = "one_shot sharded ranks_off ranks_on " * a.windows
        rec["sharded"] = bench_sharded(a.reps, a.windows)
    else:
        rec["embed"] = bench_embed(cfg, a.reps, a.windows)
        print(json.dumps(rec["embed"]), flush=True)
        if not a.no_match:
            rec["match"] = bench_match(a.reps, a.windows)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                f"retrieval_bench{'_sharded' if a.sharded else ''}_{a.config.lower()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"config": a.config, "out": out}))


if __name__ == "__main__":
    main()
