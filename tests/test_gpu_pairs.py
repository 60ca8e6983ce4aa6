"""A batch described by its sources (uint8 tables, idx, rotation coefficients) against the same
batch materialised by ``mvae_make_batch``: the direct kernel's bit buffers, whole training steps
and inference calls, the materialising path of every other configuration, argument validation,
the Python surface (``PairBatch``, ``inputs(fused=True)``, ``TangoEncoder``, ``main.train``) and
data parallelism. Every comparison is bitwise (``torch.equal`` / ``assert_array_equal``): both
routes run the same arithmetic on the same bits, so there is no tolerance to state."""
import ctypes as C
import functools
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from magic_amd import _lib
from magic_amd.config import preset
from tests.gpu_helpers import make_params

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap_micro.npz")
N_IMG = 5
SPECIAL = [0.0, math.pi / 2, math.pi, 3 * math.pi / 2, 2 * math.pi - 1e-6, 1e-6]


def tables(S, hi, seed):
    """n = 5 lock / key images of values {0, hi}, ~30 % foreground"""
    rng = np.random.default_rng(seed)
    L = ((rng.random((N_IMG, S, S)) < 0.3) * hi).astype(np.uint8)
    K = ((rng.random((N_IMG, S, S)) < 0.3) * hi).astype(np.uint8)
    return L, K


def draws(B, S, seed):
    """idx with repeats that holds 0 and n - 1; the producer test's angles, then uniform draws"""
    from magic_amd.overlap_input import rotation_coefficients
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N_IMG, B).astype(np.int32)
    idx[0], idx[1], idx[2] = 0, N_IMG - 1, 0
    ang = rng.uniform(0, 2 * math.pi, B).astype(np.float32)
    ang[:len(SPECIAL)] = SPECIAL
    return idx, rotation_coefficients(ang, S, S)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ 1. bit buffers
def debug_bits(mode, L, K, idx, coef, div, no_xbw):
    """mvae_debug_pairs_bits on zero-filled buffers -> dict of host tensors"""
    lib = _lib.load()
    B, S = len(idx), L.shape[1]
    D = S * S
    ldx, ldbits = D + 8, (D // 8 + 15) // 16 * 16
    ceil = lambda a, b: (a + b - 1) // b  # noqa: E731
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    out = dict(xbf=z(ceil(3 * B, 256) * ceil(D + 1, 64) * 512, torch.int32),
               xbw=z(ceil(D + 1, 256) * ceil(3 * B, 64) * 512, torch.int32),
               xbits=z(B * ldbits, torch.uint8), dyn=z(4, torch.int32), plane=z(3 * B * ldx, torch.int16))
    x = z(B * 3 * D, torch.float32) if mode == 0 else None
    t = [dev(L), dev(K), dev(idx), dev(coef)]
    rc = lib.mvae_debug_pairs_bits(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), B, S,
                                   float(div), mode, int(no_xbw), x.data_ptr() if mode == 0 else None,
                                   out["xbf"].data_ptr(), out["xbw"].data_ptr(), out["xbits"].data_ptr(), ldbits,
                                   out["dyn"].data_ptr(), out["plane"].data_ptr(), ldx,
                                   torch.cuda.current_stream().cuda_stream)
    _lib.check(lib, None, rc)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def compare_bits(L, K, B, div, no_xbw, expect_grey):
    idx, coef = draws(B, L.shape[1], seed=B + L.shape[1])
    ref = debug_bits(0, L, K, idx, coef, div, no_xbw)
    got = debug_bits(1, L, K, idx, coef, div, no_xbw)
    assert ref["xbf"].any() and ref["xbits"].any()  # the reference route wrote something
    assert bool(ref["dyn"][2]) == expect_grey
    for k in ("xbf", "xbits", "dyn", "plane") + (() if no_xbw else ("xbw",)):
        assert torch.equal(got[k], ref[k]), k
    if not no_xbw:
        assert ref["xbw"].any()
    return ref


BIT_SHAPES = [(64, 8), (64, 12), (64, 16), (128, 20), (192, 20), (320, 12), (64, 100)]


@pytest.mark.parametrize("no_xbw", [0, 1], ids=["xbw", "no_xbw"])
@pytest.mark.parametrize("hi,div", [(255, 255.0), (1, 1.0)], ids=["div255", "div1"])
@pytest.mark.parametrize("B,S", BIT_SHAPES, ids=[f"B{b}_S{s}" for b, s in BIT_SHAPES])
def test_bit_buffers_equal_make_batch_then_deint(B, S, hi, div, no_xbw):
    """The direct kernel (mode 1) writes the BitMats, target bits and flag words that
    mvae_make_batch followed by the step's de-interleave to bits (mode 0) writes."""
    L, K = tables(S, hi, seed=S)
    ref = compare_bits(L, K, B, div, no_xbw, expect_grey=False)
    assert not ref["plane"].any()  # a 0/1 batch: the grey pass returned at once


def test_bit_buffers_grey_byte():
    """One byte 7 in a referenced lock image: both routes raise the not-binary word (and the
    inexact flag: 7/255 is no bf16 value), and plane 0 of the grey pass is equal."""
    L, K = tables(20, 255, seed=20)
    L[0, 9, 11] = 7  # (idx holds example 0)
    ref = compare_bits(L, K, 128, 255.0, 0, expect_grey=True)
    assert ref["dyn"][0] != 0 and ref["plane"].any()


def test_bit_buffers_255_at_divisor_1():
    """Tables in {0, 255} at divisor 1: 255.0 is not binary, but exact in bf16."""
    L, K = tables(20, 255, seed=21)
    ref = compare_bits(L, K, 128, 1.0, 0, expect_grey=True)
    assert ref["dyn"][0] == 0 and ref["plane"].any()


# ------------------------------------------------------------------ 2. / 3. steps
@functools.lru_cache(maxsize=None)
def step_batches(S, B):
    """Four seeded batches over one pair of tables (host arrays; the second batch's lock table
    holds one grey byte) and their areas."""
    L, K = tables(S, 255, seed=100 + S)
    Lg = L.copy()
    Lg[N_IMG - 1, S // 2, S // 3] = 7  # (idx holds example n - 1)
    rng = np.random.default_rng(7)
    out = []
    for k in range(4):
        idx, coef = draws(B, S, seed=1000 + k)
        out.append((Lg if k == 1 else L, K, idx, coef, rng.integers(296, 6427, size=B).astype(np.float32)))
    return out


def pair_batch(L, K, idx, coef, normalize=True):
    from magic_amd.overlap_input import PairBatch
    return PairBatch(dev(L), dev(K), dev(idx), dev(coef), normalize=normalize)


def engine_state(eng):
    st = {f"{kind}/{k}": v.clone() for kind in (_lib.KIND_PARAM, _lib.KIND_M1, _lib.KIND_V1, _lib.KIND_M2,
                                                _lib.KIND_V2) for k, v in eng.tensors(kind).items()}
    return st, eng.get_rng()


def run_both(cfg, nsteps, inference=True):
    """Two fresh engines with the same parameters: one fed PairBatches, one their materialize().
    Returns the timing regions each engine ran (name -> launches)."""
    from magic_amd.engine import Engine
    P = make_params(cfg)
    batches = step_batches(cfg.image_size, cfg.batch)
    res, regions = [], []
    for fused in (True, False):
        eng = Engine(cfg, 0)
        eng.load_params(P)
        eng.timing_enable(True)
        rec = []
        for k in range(nsteps + (1 if inference else 0)):
            L, K, idx, coef, areas = batches[k]
            pb = pair_batch(L, K, idx, coef)
            x = pb if fused else pb.materialize()
            if k < nsteps:
                losses, dist = torch.zeros(5, device="cuda"), torch.zeros(cfg.batch, device="cuda")
                eng.train_step(x, dev(areas), None, losses_out=losses, dist_out=dist)
                rec += [losses, dist]
            else:
                rec += [eng.predict(x), eng.transform(x), eng.reconstruct(x)]
        torch.cuda.synchronize()
        st, rng = engine_state(eng)
        regions.append({k: v[1] for k, v in eng.timing_read().items()})
        res.append((rec, st, rng))
        eng.close()
    show = ("pairs_bits", "pairs_make_batch", "deinterleave", "deint_fwd0")
    print("input regions, pairs engine / materialised:", [{k: r[k] for k in show if k in r} for r in regions])
    (rec_a, st_a, rng_a), (rec_b, st_b, rng_b) = res
    assert rng_a == rng_b
    for i, (a, b) in enumerate(zip(rec_a, rec_b)):
        assert torch.equal(a, b), f"output {i}"
    assert all(torch.isfinite(a).all() for a in rec_a)
    assert st_a.keys() == st_b.keys()
    for k in st_a:
        assert torch.equal(st_a[k], st_b[k]), k
    return regions


@pytest.mark.parametrize("options", ["", "xbw_split=0", "xbw_split=1"], ids=["default", "xbw_split0", "xbw_split1"])
@pytest.mark.parametrize("prec", ["bf16", "f32x"])
@pytest.mark.parametrize("name", ["8c", "11a"])
def test_steps_equal_materialised(name, prec, options):
    """Three training steps (the second batch grey) and the inference calls of a fourth batch:
    losses, distances, parameters, Adam state and RNG counters bitwise equal."""
    cfg = preset(name, image_size=20, batch=128, precision=prec, options=options)
    fused, plain = run_both(cfg, 3)
    # every pass of the pairs engine (3 steps + 3 inference calls) took the direct kernel
    assert "pairs_bits" not in plain and "pairs_make_batch" not in plain and plain["deinterleave"] == 6
    assert fused.get("pairs_bits") == 6 and "pairs_make_batch" not in fused and "deinterleave" not in fused


def test_steps_equal_materialised_c3_image():
    """The workload's image (100 x 100, 79 pixel tasks), bf16, two steps, the direct kernel."""
    cfg = preset("8d", image_size=100, batch=64, precision="bf16")
    fused, _ = run_both(cfg, 2, inference=False)
    assert fused.get("pairs_bits") == 2 and "pairs_make_batch" not in fused


MATERIALISING = {
    "f32": dict(precision="f32"),
    "batch96": dict(batch=96),
    "image10": dict(image_size=10),
    "conv": dict(conv=True, image_size=8, batch=64),
    "bits0": dict(options="bits=0"),
    "e8_0": dict(options="e8=0"),
}


@pytest.mark.parametrize("case", sorted(MATERIALISING))
def test_materialising_path(case):
    """Configurations the direct kernel does not serve: the pairs calls work and change nothing."""
    kw = dict(image_size=20, batch=128, precision="bf16")
    kw.update(MATERIALISING[case])
    fused, _ = run_both(preset("8c", **kw), 2)
    if case in ("f32", "batch96", "image10", "conv", "bits0"):  # no bits branch to take at all
        assert "pairs_bits" not in fused and fused.get("pairs_make_batch") == 5


# ------------------------------------------------------------------ 4. validation
def test_validation():
    from magic_amd.engine import Engine
    from magic_amd.overlap_input import PairBatch
    cfg = preset("8c", image_size=20, batch=128, precision="bf16")
    eng = Engine(cfg, 0)
    eng.load_params(make_params(cfg))
    L, K, idx, coef, areas = step_batches(20, 128)[0]
    a = dev(areas)
    # tables of another height
    L21 = np.zeros((N_IMG, 21, 20), np.uint8)
    with pytest.raises(_lib.MVAEError) as ei:
        p = eng._pairs(PairBatch(dev(L21), dev(L21), dev(idx), dev(coef)))
        eng._check(eng.lib.mvae_train_step_pairs(eng.ctx, C.byref(p), a.data_ptr(), None, None, None, eng.stream))
    assert ei.value.code == -1 and "image_size" in str(ei.value)
    # coef offset by one float
    buf = torch.zeros(128 * 4 + 4, device="cuda")
    off = buf[1:1 + 128 * 4].view(128, 4)
    off.copy_(dev(coef))
    assert off.data_ptr() % 16 == 4
    with pytest.raises(_lib.MVAEError) as ei:
        eng.train_step(PairBatch(dev(L), dev(K), dev(idx), off), a)
    assert ei.value.code == -1 and "16-byte" in str(ei.value)
    # a batch of the wrong size
    with pytest.raises(ValueError):
        eng.train_step(pair_batch(L, K, idx[:64], coef[:64]), a)
    # ... and the engine still steps
    eng.train_step(pair_batch(L, K, idx, coef), a)
    torch.cuda.synchronize()
    eng.close()


# ------------------------------------------------------------------ 5. Python surface
def micro_stream(fused, reshape=True):
    from magic_amd.overlap_input import inputs
    return inputs(normalize=True, reshape=reshape, rotation=True, batch_size=64, image_size=200, data_dir=GOLD,
                  seed=3, fused=fused)


def test_fused_stream_yields_the_same_batches():
    from magic_amd.overlap_input import PairBatch
    a, b = micro_stream(False), micro_stream(True)
    n = len(a.locks)
    draws_ = -(-n // 64) + 1  # past the first epoch's end
    for _ in range(max(3, draws_)):
        (x, ar), (pb, br) = next(a), next(b)
        assert isinstance(pb, PairBatch) and pb.shape == tuple(x.shape) == (64, 3 * 200 * 200)
        assert torch.equal(ar, br)
        assert torch.equal(pb.materialize(), x)
    with pytest.raises(ValueError):
        micro_stream(True, reshape=False)


def test_partial_fit_and_driver_on_a_fused_stream():
    """TangoEncoder.partial_fit returns identical tuples on both streams, and main.train (1 epoch of
    4 steps with an evaluation) an identical history."""
    from magic_amd import main
    from magic_amd.vae import TangoEncoder
    cfg = preset("11a", image_size=200, batch=64, precision="bf16")
    outs, hist = [], []
    for fused in (False, True):
        vae = TangoEncoder(None, config=cfg)
        s = micro_stream(fused)
        outs.append(vae.partial_fit(*next(s)))
        _, h = main.train(vae, s, 4 * 64, 1, driver="11a", eval_at=lambda epoch, i: i == 1, log=lambda m: None)
        hist.append(h)
        vae.close()
    assert len(outs[0]) == 6
    for u, v in zip(*outs):
        np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
    assert any(r[0] == "mse" for r in hist[0]) and any(r[0] == "epoch" for r in hist[0])
    assert hist[0] == hist[1]


# ------------------------------------------------------------------ 6. data parallel
def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    from magic_amd.engine import Engine
    from magic_amd.parallel import DataParallelStep
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = preset("8c", image_size=20, batch=64 * world, precision="bf16")
    L, K, idx, coef, areas = step_batches(20, 64 * world)[0]
    sl = slice(rank * 64, (rank + 1) * 64)
    out = []
    for fused in (False, True):  # both ranks run the two engines in the same order
        eng = Engine(cfg.replace(batch=64, global_batch=64 * world), 0)
        eng.load_params(make_params(cfg))
        eng.set_shard(rank * 64)
        pb = pair_batch(L, K, idx[sl], np.ascontiguousarray(coef[sl]))
        st = DataParallelStep(eng)
        # (host copies only: a view of the engine's memory must not outlive the engine)
        losses = st.step(pb if fused else pb.materialize(), dev(areas[sl])).cpu().numpy().copy()
        torch.cuda.synchronize()
        out.append((losses, {k: v.cpu().numpy() for k, v in eng.params().items()}))
        del st
        eng.close()
    q.put((rank, out))
    dist.destroy_process_group()


def test_dp2_pair_batches():
    """DataParallelStep.step on per-rank PairBatches against per-rank X: two gloo ranks on this GPU,
    losses and parameters bitwise equal on each rank."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(2):
        (l_x, p_x), (l_p, p_p) = res[r]
        assert np.isfinite(l_x[:5]).all()
        np.testing.assert_array_equal(l_p, l_x)
        for k in p_x:
            np.testing.assert_array_equal(p_p[k], p_x[k])
