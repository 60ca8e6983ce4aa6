#!/usr/bin/env python3
"""Regenerate the committed fixtures under tests/golden/ (run here, where the read-only
reference is mounted; the GPU box only reads the committed files).

  magic_amd/data/overlap_areas.npy  the 2000 int64 labels of the reference's ``2a/OVERLAP_AREAS``
                         (package data: the synthetic batches resample it)
                         (a Python-2 protocol-0 pickle of numpy int64 scalars). The file is
                         NOT unpickled: its ``S'...'`` string literals (8 raw little-endian
                         bytes each) are parsed as text and decoded with escape rules only.
  overlap_micro.npz      the reference's ``overlap_micro.zip`` (100 lock/key pairs, 200x200
                         binary PNGs) as packed bits: data, not code.
  step_<flavour>.npz     oracle (float64) golden vectors for one training step of a tiny
                         config per preset flavour (and the conv-encoder variant): inputs,
                         5 losses, distance, g1, g2, post-Adam parameters.
  gemm_plans.npz         the GEMM planner's decisions for gemm_plan_cases() below, as the built
                         library reports them (mvae_debug_plan; no GPU, no reference needed):
                         ``--gemm-plans`` writes this file alone. It was recorded from the planner
                         as it stood before gemm_plan.cpp; regenerate it only for
                         a change of plans that is meant.

Usage: python tests/golden/make_golden.py [--reference /root/reference] [--gemm-plans]
"""
from __future__ import annotations

import argparse
import codecs
import io
import os
import re
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import mvae_oracle as O  # noqa: E402

FLAVOURS = {
    "8c_cosine_tanh": dict(act="tanh", metric="cosine", reciprocal=False, deform_weight=10.0),
    "9a_recip_cosine": dict(act="tanh", metric="cosine", reciprocal=True, deform_weight=10.0),
    "11a_recip_sqdiff_elu": dict(act="elu", metric="sqdiff", reciprocal=True, deform_weight=100.0),
    "sqdiff_tanh": dict(act="tanh", metric="sqdiff", reciprocal=False, deform_weight=10.0),
    # conv-encoder variant (tower of 6b/net.py:50-60): image side a multiple of 4
    "conv_recip_sqdiff": dict(act="tanh", metric="sqdiff", reciprocal=True, deform_weight=10.0,
                              conv=True, image_size=12),
}
TINY = dict(image_size=10, enc=(24, 16), dec=(12, 14), latent=4, lr=(1e-3, 1e-4))
TINY_B = 8


def parse_overlap_areas(path: str) -> np.ndarray:
    raw = open(path, "rb").read().decode("latin-1")
    vals = []
    # Python 2's repr quotes with ' unless the bytes contain ' (then with ")
    for lit in re.findall(r"S(?:'((?:[^'\\]|\\.)*)'|\"((?:[^\"\\]|\\.)*)\")\n", raw):
        b = codecs.escape_decode((lit[0] or lit[1]).encode("latin-1"))[0]
        if len(b) == 8:
            vals.append(np.frombuffer(b, "<i8")[0])
    return np.array(vals, np.int64)


def pack_micro(path: str) -> dict:
    from PIL import Image
    z = zipfile.ZipFile(path)
    locks, keys = [], []
    i = 0
    while f"overlap_micro/{i}_L.png" in z.namelist():
        for lst, nm in ((locks, f"{i}_L"), (keys, f"{i}_K")):
            a = np.array(Image.open(io.BytesIO(z.read(f"overlap_micro/{nm}.png"))).convert("L"))
            assert set(np.unique(a)) <= {0, 255}
            lst.append(a > 0)
        i += 1
    L, K = np.stack(locks), np.stack(keys)
    return {"lock_bits": np.packbits(L, axis=-1), "key_bits": np.packbits(K, axis=-1),
            "shape": np.array(L.shape)}


def golden_cfg(flav: dict) -> O.OracleConfig:
    return O.OracleConfig(**dict(TINY, **flav))


def step_golden(name: str, flav: dict) -> dict:
    cfg = golden_cfg(flav)
    P = O.init_params(cfg, seed=0, dtype=np.float64)
    rng = np.random.default_rng(7)
    for k in P:
        if k.endswith("_b"):
            P[k] = rng.normal(0, 0.05, P[k].shape)
    X = (np.random.default_rng(1).random((TINY_B, 3 * cfg.D)) < 0.2).astype(np.float64)
    areas = np.random.default_rng(1).integers(296, 6427, TINY_B).astype(np.float64)
    eps = np.random.default_rng(2).standard_normal((3, TINY_B, cfg.latent))
    st = O.adam_init(cfg, P)
    losses, dist, Pn, st, (g1, g2) = O.train_step(P, st, X, areas, eps, cfg)
    out = {"X": X, "areas": areas, "eps": eps, "losses": losses, "dist": dist}
    for k, v in P.items():
        out["P/" + k] = v
    for k, v in g1.items():
        out["g1/" + k] = v
    for k, v in g2.items():
        out["g2/" + k] = v
    for k, v in Pn.items():
        out["Pn/" + k] = v
    return out


# ---- gemm_plans.npz: the GEMM planner's decisions (mvae_debug_plan), recorded from the library
# before the planner was rewritten and compared column by column ever since.
# A case is one row of PLAN_IN (the fields of mvae_plan_args; a pointer column holds 0 = NULL,
# 1 = a 16-byte aligned address, 2 = that address + 4); PLAN_OUT are the fields of mvae_plan_out.
PLAN_PTRS = ("Ap", "Bp", "C", "cp", "aux", "auxp", "x", "xp", "y", "ws")
PLAN_IN = ("M", "N", "K", "batch", "at", "bt", "lda", "ldb", "ldc", "prec", "nA", "nB", "dynA", "epi", "c32", "xdyn",
           "padw", "ld_aux", "ldx", "ldy", "abits", "x3", "tm", "split", "valu", "variant", "pA", "pB", "sA", "sB",
           "sC", "pc", "max_ws") + PLAN_PTRS
PLAN_OUT = ("kernel", "staging", "tm", "tn", "ntm", "ntn", "group", "split", "kchunk", "lds_epilogue",
            "vec_epilogue", "epi_launched", "valu_fits", "refused", "ws_elems")
PLAN_VARIANTS = tuple(range(16))
UNLIMITED = (1 << 64) - 1
STORE, ACT, DACT, BCE, SIGMOID = range(5)
DIMS = (40, 64, 127, 128, 191, 192, 255, 256, 257, 300, 500, 512, 4096, 12288, 24576)
KS = (21, 40, 64, 65, 127, 128, 501, 2048, 4096, 8192)


def _r8(v: int) -> int:
    return (v + 7) // 8 * 8


def plan_case(M, N, K, *, at=0, bt=0, batch=1, prec=1, epi=STORE, planes=True, auxp=False, target="plane", **kw):
    """One GEMM as the step's wiring would describe it: rows padded to 8 elements, whole planes,
    aligned buffers, the output as planes (and fp32 unless c32=0) in the plane modes; **kw overrides
    any PLAN_IN column afterwards."""
    lda, ldb, ldc = _r8(M if at else K), _r8(K if bt else N), _r8(N)
    np_ = {0: 1, 1: 1, 2: 3}[prec]
    c = dict.fromkeys(PLAN_IN, 0)
    c.update(M=M, N=N, K=K, batch=batch, at=at, bt=bt, lda=lda, ldb=ldb, ldc=ldc, prec=prec, nA=np_, nB=np_,
             epi=epi, c32=1, pA=(K if at else M) * lda * batch, pB=(N if bt else K) * ldb * batch,
             sA=(K if at else M) * lda if batch > 1 else 0, sB=(N if bt else K) * ldb if batch > 1 else 0,
             sC=M * ldc if batch > 1 else 0, pc=M * ldc * batch, max_ws=UNLIMITED, Ap=1, Bp=1, C=1, ws=1)
    if prec and planes and epi != SIGMOID:
        c["cp"] = 1
    if epi == DACT:
        c.update(aux=1, ld_aux=ldc, auxp=1 if auxp else 0)
    if epi == BCE:
        c.update(x=1, ldx=ldc, y=1, ldy=ldc)
        if target == "plane" and prec:
            c.update(xp=1, xdyn=1)
    c.update(kw)
    return c


def step_shapes(cid: str):
    """(M, N, K, at, bt, batch, epilogue) of every GEMM of one training step of a baseline config."""
    from magic_amd.config import baseline_config
    cfg = baseline_config(cid)
    B, L, d0, d1 = cfg.batch, cfg.latent, cfg.dec[0], cfg.dec[1]
    F = (cfg.image_size // 4) ** 2 * 64 if cfg.conv else cfg.D  # layer-0 fan-in
    w = [F] + list(cfg.enc)
    out = []
    for a, b in zip(w[:-1], w[1:]):
        out += [(3 * B, b, a + 1, 0, 0, 1, ACT), (4 * B, a, b, 0, 1, 1, DACT), (a + 1, b, 2 * B, 1, 0, 2, STORE)]
    e = w[-1]
    out += [(3 * B, 2 * L, e + 1, 0, 0, 1, STORE), (4 * B, e, 2 * L, 0, 1, 1, DACT), (e + 1, 2 * L, 2 * B, 1, 0, 2, STORE),
            (B, d0, L + 1, 0, 0, 1, ACT), (L + 1, d0, B, 1, 0, 1, STORE), (B, L, d0, 0, 1, 1, STORE),
            (B, d1, d0 + 1, 0, 0, 1, ACT), (B, d0, d1, 0, 1, 1, DACT), (d0 + 1, d1, B, 1, 0, 1, STORE),
            (B, cfg.D, d1 + 1, 0, 0, 1, BCE), (B, d1, cfg.D, 0, 1, 1, DACT), (d1 + 1, cfg.D, B, 1, 0, 1, STORE)]
    return sorted(set(out))


def gemm_plan_cases() -> list:
    rng = np.random.default_rng(20)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]  # noqa: E731
    cases = []
    # 1. the step's own GEMMs, in every precision, on the planner and on the forces the wiring
    #    sets (3 thin ring, 13 e8=2, 15 e8=0), with the pixel operand's flags on layer 0
    for cid in ("C2", "C3", "C5", "C5CONV"):
        for (M, N, K, at, bt, batch, epi) in step_shapes(cid):
            for prec in (0, 1, 2):
                for variant, x3 in ((0, 0), (0, 2), (3, 1), (13 if prec == 1 else 15, 0)):
                    kw = dict(at=at, bt=bt, batch=batch, prec=prec, epi=epi, variant=variant, x3=x3,
                              auxp=prec == 1, c32=int(prec != 1 or epi in (STORE, BCE)))
                    cases.append(plan_case(M, N, K, **kw))
                    if variant == 0 and x3 == 0 and prec and (K > 8192 or (at and batch == 2)):
                        cases.append(plan_case(M, N, K, **kw, dynA=int(prec == 2), abits=1))
                        cases.append(plan_case(M, N, K, **kw, dynA=int(prec == 2)))
    # 2. every pair of output dimensions with every K once, the rest drawn
    for M in DIMS:
        for N in DIMS:
            for K in rng.choice(KS, 4, replace=False).tolist():
                prec = pick((0, 1, 1, 2, 2))
                epi = pick((STORE, STORE, ACT, DACT, BCE, SIGMOID))
                cases.append(plan_case(M, N, K, at=pick((0, 1)), bt=pick((0, 1)), batch=pick((1, 1, 2)), prec=prec,
                                       epi=epi, variant=pick((0, 0, 0, 0) + PLAN_VARIANTS), x3=pick((0, 0, 1, 2)),
                                       tm=pick((0, 0, 0, 192, 256)), auxp=bool(pick((0, 1))),
                                       target=pick(("plane", "f32")), dynA=pick((0, 0, 1)) if prec == 2 else 0,
                                       abits=pick((0, 0, 0, 1)) if prec else 0,
                                       max_ws=pick((UNLIMITED, UNLIMITED, 0, M * N * pick((1, 2)))),
                                       c32=pick((1, 1, 0)) if prec and epi != SIGMOID else 1))
    # 3. every number, layout, epilogue and tile force on shapes around the kernels' thresholds
    shapes = ((128, 128, 64), (127, 300, 501), (256, 256, 65), (257, 500, 2048), (4096, 256, 4096),
              (4096, 257, 4096), (12288, 500, 501), (4096, 4096, 64), (24576, 512, 128), (500, 12288, 8192),
              (300, 40, 4096))
    epis = (dict(epi=STORE), dict(epi=ACT), dict(epi=DACT), dict(epi=DACT, auxp=True), dict(epi=BCE, target="f32"),
            dict(epi=BCE), dict(epi=SIGMOID), dict(epi=STORE, planes=False))
    for (M, N, K) in shapes:
        for variant in PLAN_VARIANTS:
            for prec in (0, 1, 2):
                for e in epis[(variant + prec) % 2::2]:
                    cases.append(plan_case(M, N, K, prec=prec, variant=variant, at=pick((0, 0, 1)), bt=pick((0, 1)),
                                           tm=pick((0, 192, 256)), x3=pick((0, 1, 2)), **e))
        for at in (0, 1):
            for bt in (0, 1):
                for tm in (0, 192, 256):
                    for x3 in (0, 1, 2):
                        for dynA in (0, 1):
                            cases.append(plan_case(M, N, K, prec=2, at=at, bt=bt, tm=tm, x3=x3, dynA=dynA,
                                                   epi=pick((STORE, ACT, BCE)), variant=pick((0, 11, 12, 15))))
    # 4. what the eligibility tests read: strides, alignment, plane sizes, the epilogue's operands
    big = 1 << 27
    for (M, N, K) in ((4096, 4096, 4096), (300, 500, 501), (40, 500, 128), (500, 40, 128)):
        for variant in (0, 6, 13, 11, 7):
            for prec in (1, 2):
                for kw in (dict(lda=_r8(K) + 4), dict(ldb=_r8(N) + 2), dict(pA=M * _r8(K) + 4), dict(pB=K * _r8(N) + 1),
                           dict(Ap=2), dict(Bp=2), dict(batch=2, sA=M * _r8(K) + 4), dict(batch=2, sB=4),
                           dict(lda=big, pA=M * big), dict(ldb=big, pB=K * big), dict(bt=1, ldb=big, pB=N * big),
                           dict(at=1, lda=big, pA=K * big), dict(pA=1 << 33, pB=1 << 33), dict(abits=1),
                           dict(abits=1, lda=big, pA=M * big), dict(abits=1, tm=192)):
                    cases.append(plan_case(M, N, K, prec=prec, variant=variant, **kw))
                for e in epis[:-1] if (variant, prec) in ((0, 1), (13, 2), (11, 2)) else ():
                    for kw in (dict(C=2), dict(ldc=_r8(N) + 1), dict(ldc=_r8(N) + 4), dict(cp=2), dict(pc=M * _r8(N) + 4),
                               dict(aux=2), dict(auxp=2), dict(ld_aux=_r8(N) + 2), dict(ld_aux=_r8(N) + 4), dict(x=2),
                               dict(xp=2), dict(ldx=_r8(N) + 4), dict(ldx=_r8(N) + 2), dict(y=2), dict(ldy=_r8(N) + 1),
                               dict(y=0), dict(ws=2, split=2), dict(batch=2, sC=M * _r8(N) + 2), dict(padw=1)):
                        if "auxp" in kw and not e.get("auxp") or "xp" in kw and e != dict(epi=BCE):
                            continue
                        cases.append(plan_case(M, N, K, prec=prec, variant=variant, **{**e, **kw}))
    # 5. split-K: forced, against the workspace (none, one slab, exactly enough, unlimited), and VALU
    for (M, N, K) in ((501, 500, 8192), (501, 40, 8192), (256, 256, 4096), (21, 500, 4096), (4096, 4096, 8192),
                      (64, 64, 2048), (40, 300, 64), (501, 4000, 16384)):
        for prec in (0, 1, 2):
            for split in (0, 2, 4, 7):
                for max_ws in (0, M * N, 4 * M * N, UNLIMITED):
                    for valu in (0, 1):
                        cases.append(plan_case(M, N, K, at=1, prec=prec, split=split, max_ws=max_ws, valu=valu,
                                               epi=pick((STORE, STORE, ACT, DACT, SIGMOID)),
                                               variant=0 if valu else pick((0, 0, 3, 9, 15)), ws=pick((1, 1, 0))))
    return cases


def write_gemm_plans(path: str):
    """Ask the built library (mvae_debug_plan: host only) for the plan of every case."""
    import ctypes
    from magic_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    base = (ctypes.addressof(buf) + 15) & ~15
    cases = gemm_plan_cases()
    cin = np.array([[c[k] for k in PLAN_IN] for c in cases], dtype=np.uint64)
    cout = np.zeros((len(cases), len(PLAN_OUT)), np.uint64)
    for i, c in enumerate(cases):
        a, o = _lib.mvae_plan_args(), _lib.mvae_plan_out()
        for k in PLAN_IN:
            setattr(a, k, (None, base, base + 4)[c[k]] if k in PLAN_PTRS else c[k])
        rc = lib.mvae_debug_plan(ctypes.byref(a), ctypes.byref(o))
        assert rc == 0, (c, lib.mvae_last_error(None))
        cout[i] = [getattr(o, k) for k in PLAN_OUT]
    np.savez_compressed(path, cases=cin, plans=cout, in_names=np.array(PLAN_IN), out_names=np.array(PLAN_OUT))
    print("gemm_plans", cin.shape, cout.shape, os.path.getsize(path), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--gemm-plans", action="store_true",
                    help="write gemm_plans.npz from the built library alone (no reference needed)")
    args = ap.parse_args()
    if args.gemm_plans:
        return write_gemm_plans(os.path.join(HERE, "gemm_plans.npz"))
    areas = parse_overlap_areas(os.path.join(args.reference, "2a", "OVERLAP_AREAS"))
    np.save(os.path.join(os.path.dirname(os.path.dirname(HERE)), "magic_amd", "data", "overlap_areas.npy"), areas)
    print("overlap_areas", areas.shape, areas.min(), areas.max(), areas.mean())
    np.savez_compressed(os.path.join(HERE, "overlap_micro.npz"),
                        **pack_micro(os.path.join(args.reference, "overlap_micro.zip")))
    for name, flav in FLAVOURS.items():
        np.savez_compressed(os.path.join(HERE, f"step_{name}.npz"), **step_golden(name, flav))
        print("wrote", name)


if __name__ == "__main__":
    main()
