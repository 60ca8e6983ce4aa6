"""Cross-pair batches -- row b is lock ``idx[b]``, its rotation, and key ``key_idx[b]`` of a key
table that holds another number of images -- against the same batch materialised by
``mvae_make_batch_x``: the producer against the numpy oracle on gathered tables, the direct kernel's
bit buffers, whole training steps and inference calls, the materialising configurations, argument
validation, the label cache ``PairLabels``, the sampler (``BatchStream(pairs=...)``), the driver and
data parallelism. Every comparison is bitwise (``torch.equal`` / ``assert_array_equal``): both
routes run the same arithmetic on the same bits, and the labels are integer work.

The tables hold n = 5 locks and m = 7 keys, and every ``key_idx`` holds 0 and 6: a kernel that
indexes the key table with the lock's index never reads key images 5 and 6, and one that uses the
lock table for the key reads another image or runs off the lock-shaped range."""
import ctypes as C
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from magic_amd import _lib
from magic_amd.config import preset
from tests.gpu_helpers import make_params
from tests.overlap_ref import angle_coefficients, max_overlap_ref
from tests.test_gpu_pairs import dev, draws, engine_state

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap_micro.npz")
N_LOCK, N_KEY = 5, 7


def xtables(S, hi, seed):
    """n = 5 lock and m = 7 key images of values {0, hi}, ~30 % foreground"""
    rng = np.random.default_rng(seed)
    L = ((rng.random((N_LOCK, S, S)) < 0.3) * hi).astype(np.uint8)
    K = ((rng.random((N_KEY, S, S)) < 0.3) * hi).astype(np.uint8)
    return L, K


def xdraws(B, S, seed):
    """``draws`` of tests/test_gpu_pairs.py (lock idx with repeats holding 0 and n - 1, its special
    angles) plus a key_idx with repeats that holds 0 and m - 1"""
    idx, coef = draws(B, S, seed)
    kidx = np.random.default_rng(seed + 50000).integers(0, N_KEY, B).astype(np.int32)
    kidx[0], kidx[1], kidx[2] = N_KEY - 1, 0, N_KEY - 1
    assert idx.max() == N_LOCK - 1 and kidx.max() == N_KEY - 1 and (kidx != idx).any()
    return idx, kidx, coef


def make_batch_x(L, K, idx, kidx, coef, div):
    lib = _lib.load()
    B, S = len(idx), L.shape[1]
    x = torch.full((B, 3 * S * S), -1.0, device="cuda")
    t = [dev(L), dev(K), dev(idx), None if kidx is None else dev(kidx), dev(coef)]
    rc = lib.mvae_make_batch_x(t[0].data_ptr(), t[1].data_ptr(), S, S, t[2].data_ptr(),
                               None if kidx is None else t[3].data_ptr(), t[4].data_ptr(), B, float(div),
                               x.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(lib, None, rc)
    torch.cuda.synchronize()
    return x.cpu().numpy()


# ------------------------------------------------------------------ 1. producer
@pytest.mark.parametrize("hi,div", [(255, 255.0), (1, 1.0)], ids=["div255", "div1"])
@pytest.mark.parametrize("S", [9, 12, 20])  # 81 pixels: the scalar kernel; 144 and 400: four per thread
def test_producer_equals_the_oracle_on_gathered_tables(S, hi, div):
    from oracle import input_oracle
    B = 64
    L, K = xtables(S, hi, seed=S)
    idx, kidx, coef = xdraws(B, S, seed=B + S)
    want = input_oracle.make_batch(L[idx], K[kidx], np.arange(B), coef, scale_div=div)
    got = make_batch_x(L, K, idx, kidx, coef, div)
    assert want.any()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("S", [9, 20])
def test_producer_with_the_own_key_is_make_batch(S):
    """key_idx NULL or equal to lock_idx, n = m: the bits of mvae_make_batch."""
    from magic_amd.overlap_input import make_batch
    B = 64
    L, K = xtables(S, 255, seed=S + 1)
    K = K[:N_LOCK]
    idx, _, coef = xdraws(B, S, seed=B + S)
    want = make_batch(dev(L), dev(K), dev(idx), dev(coef)).cpu().numpy()
    np.testing.assert_array_equal(make_batch_x(L, K, idx, idx, coef, 255.0), want)
    np.testing.assert_array_equal(make_batch_x(L, K, idx, None, coef, 255.0), want)
    # ... and the Python producer takes the key index through
    got = make_batch(dev(L), dev(K), dev(idx), dev(coef), key_idx=dev(idx)).cpu().numpy()
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------ 2. bit buffers
def debug_bits(mode, L, K, idx, kidx, coef, div, no_xbw):
    """mvae_debug_xpairs_bits on zero-filled buffers -> dict of host tensors"""
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
    t = [dev(L), dev(K), dev(idx), dev(kidx), dev(coef)]
    rc = lib.mvae_debug_xpairs_bits(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                    t[4].data_ptr(), B, S, float(div), mode, int(no_xbw),
                                    x.data_ptr() if mode == 0 else None, out["xbf"].data_ptr(),
                                    out["xbw"].data_ptr(), out["xbits"].data_ptr(), ldbits, out["dyn"].data_ptr(),
                                    out["plane"].data_ptr(), ldx, torch.cuda.current_stream().cuda_stream)
    _lib.check(lib, None, rc)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def compare_bits(L, K, B, div, no_xbw, expect_grey):
    idx, kidx, coef = xdraws(B, L.shape[1], seed=B + L.shape[1])
    ref = debug_bits(0, L, K, idx, kidx, coef, div, no_xbw)
    got = debug_bits(1, L, K, idx, kidx, coef, div, no_xbw)
    assert ref["xbf"].any() and ref["xbits"].any()  # the reference route wrote something
    assert bool(ref["dyn"][2]) == expect_grey
    for k in ("xbf", "xbits", "dyn", "plane") + (() if no_xbw else ("xbw",)):
        assert torch.equal(got[k], ref[k]), k
    if not no_xbw:
        assert ref["xbw"].any()
    return ref


BIT_SHAPES = [(64, 8), (64, 12), (128, 20), (192, 20), (64, 100)]


@pytest.mark.parametrize("no_xbw", [0, 1], ids=["xbw", "no_xbw"])
@pytest.mark.parametrize("B,S", BIT_SHAPES, ids=[f"B{b}_S{s}" for b, s in BIT_SHAPES])
def test_bit_buffers_equal_make_batch_x_then_deint(B, S, no_xbw):
    """The direct kernel (mode 1) writes the BitMats, target bits and flag words that
    mvae_make_batch_x followed by the step's de-interleave to bits (mode 0) writes."""
    L, K = xtables(S, 255, seed=S)
    ref = compare_bits(L, K, B, 255.0, no_xbw, expect_grey=False)
    assert not ref["plane"].any()  # a 0/1 batch: the grey pass returned at once


def test_bit_buffers_follow_the_key_index():
    """The own-pair operand of the same rows differs (the key index is read, not ignored); the
    target bits, which hold no key pixel, do not."""
    L, K = xtables(20, 255, seed=20)
    idx, kidx, coef = xdraws(128, 20, seed=148)
    cross = debug_bits(1, L, K, idx, kidx, coef, 255.0, 0)
    own = debug_bits(1, L, K, idx, idx, coef, 255.0, 0)
    assert not torch.equal(cross["xbf"], own["xbf"]) and not torch.equal(cross["xbw"], own["xbw"])
    assert torch.equal(cross["xbits"], own["xbits"])


@pytest.mark.parametrize("no_xbw", [0, 1], ids=["xbw", "no_xbw"])
def test_bit_buffers_grey_byte_in_a_key_only_key_idx_reaches(no_xbw):
    """One byte 7 in key image 6 (no lock index is 6): both routes raise the not-binary word (and
    the inexact flag: 7/255 is no bf16 value), and plane 0 of the grey pass is equal."""
    L, K = xtables(20, 255, seed=20)
    K[N_KEY - 1, 9, 11] = 7
    ref = compare_bits(L, K, 128, 255.0, no_xbw, expect_grey=True)
    assert ref["dyn"][0] != 0 and ref["plane"].any()


def test_debug_entry_point_serves_modes_0_and_1_only():
    lib = _lib.load()
    L, K = xtables(8, 255, seed=1)
    idx, kidx, coef = xdraws(64, 8, seed=2)
    for mode in (2, 3, -1):
        with pytest.raises(_lib.MVAEError, match="mvae_debug_xpairs_bits"):
            debug_bits(mode, L, K, idx, kidx, coef, 255.0, 0)
    assert lib.mvae_last_error(None).decode().startswith("mvae_debug_xpairs_bits")


# ------------------------------------------------------------------ 3. steps
@functools.lru_cache(maxsize=None)
def step_batches(S, B):
    """Four seeded cross-pair batches over one pair of tables (host arrays; the second batch's key
    table holds one grey byte in image 6) and their areas."""
    L, K = xtables(S, 255, seed=100 + S)
    Kg = K.copy()
    Kg[N_KEY - 1, S // 2, S // 3] = 7
    rng = np.random.default_rng(7)
    out = []
    for k in range(4):
        idx, kidx, coef = xdraws(B, S, seed=1000 + k)
        out.append((L, Kg if k == 1 else K, idx, kidx, coef, rng.integers(296, 6427, size=B).astype(np.float32)))
    return out


def pair_batch(L, K, idx, kidx, coef):
    from magic_amd.overlap_input import PairBatch
    return PairBatch(dev(L), dev(K), dev(idx), dev(coef), key_idx=None if kidx is None else dev(kidx))


def run_both(cfg, nsteps, inference=True):
    """Two fresh engines with the same parameters: one fed cross PairBatches, one their
    materialize(). Returns the timing regions each engine ran (name -> launches)."""
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
            L, K, idx, kidx, coef, areas = batches[k]
            pb = pair_batch(L, K, idx, kidx, coef)
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
    (rec_a, st_a, rng_a), (rec_b, st_b, rng_b) = res
    assert rng_a == rng_b
    for i, (a, b) in enumerate(zip(rec_a, rec_b)):
        assert torch.equal(a, b), f"output {i}"
    assert all(torch.isfinite(a).all() for a in rec_a)
    assert st_a.keys() == st_b.keys()
    for k in st_a:
        assert torch.equal(st_a[k], st_b[k]), k
    return regions


@pytest.mark.parametrize("prec", ["bf16", "f32x"])
@pytest.mark.parametrize("name", ["8c", "11a"])
def test_steps_equal_materialised(name, prec):
    """Three training steps (the second batch grey through a key) and the inference calls of a
    fourth batch: losses, distances, parameters, Adam state and RNG counters bitwise equal."""
    cfg = preset(name, image_size=20, batch=128, precision=prec)
    fused, plain = run_both(cfg, 3)
    assert "pairs_bits" not in plain and "pairs_make_batch" not in plain and plain["deinterleave"] == 6
    assert fused.get("pairs_bits") == 6 and "pairs_make_batch" not in fused and "deinterleave" not in fused


MATERIALISING = {
    "f32": dict(precision="f32"),
    "batch96": dict(batch=96),
    "bits0": dict(options="bits=0"),
}


@pytest.mark.parametrize("case", sorted(MATERIALISING))
def test_materialising_path(case):
    """Configurations the direct kernel does not serve: the xpairs calls materialise and agree."""
    kw = dict(image_size=20, batch=128, precision="bf16")
    kw.update(MATERIALISING[case])
    fused, _ = run_both(preset("8c", **kw), 2)
    assert "pairs_bits" not in fused and fused.get("pairs_make_batch") == 5


def test_key_idx_equal_to_idx_is_the_own_pair_batch():
    """A PairBatch with key_idx = idx (the xpairs entry points) against the one without (the pairs
    entry points): two steps and a prediction, everything bitwise equal."""
    from magic_amd.engine import Engine
    cfg = preset("8c", image_size=20, batch=128, precision="bf16")
    P = make_params(cfg)
    res = []
    for own in (False, True):
        eng = Engine(cfg, 0)
        eng.load_params(P)
        rec = []
        for k in range(2):
            L, K, idx, _, coef, areas = step_batches(20, 128)[k]
            pb = pair_batch(L, K[:N_LOCK], idx, None if own else idx, coef)
            assert isinstance(eng._pairs(pb), _lib.mvae_pairs if own else _lib.mvae_xpairs)
            losses = torch.zeros(5, device="cuda")
            eng.train_step(pb, dev(areas), None, losses_out=losses)
            rec += [losses, eng.predict(pb)]
        torch.cuda.synchronize()
        res.append((rec, engine_state(eng)))
        eng.close()
    (rec_a, (st_a, rng_a)), (rec_b, (st_b, rng_b)) = res
    assert rng_a == rng_b
    for a, b in zip(rec_a, rec_b):
        assert torch.equal(a, b)
    for k in st_a:
        assert torch.equal(st_a[k], st_b[k]), k


# ------------------------------------------------------------------ 4. validation
def test_validation():
    from magic_amd.engine import Engine
    from magic_amd.overlap_input import PairBatch
    cfg = preset("8c", image_size=20, batch=128, precision="bf16")
    eng = Engine(cfg, 0)
    eng.load_params(make_params(cfg))
    L, K, idx, kidx, coef, areas = step_batches(20, 128)[0]
    a = dev(areas)
    # tables of another height
    L21, K21 = np.zeros((N_LOCK, 21, 20), np.uint8), np.zeros((N_KEY, 21, 20), np.uint8)
    with pytest.raises(_lib.MVAEError) as ei:
        p = eng._pairs(PairBatch(dev(L21), dev(K21), dev(idx), dev(coef), key_idx=dev(kidx)))
        assert isinstance(p, _lib.mvae_xpairs)
        eng._check(eng.lib.mvae_train_step_xpairs(eng.ctx, C.byref(p), a.data_ptr(), None, None, None, eng.stream))
    assert ei.value.code == -1 and "image_size" in str(ei.value) and "mvae_train_step_xpairs:" in str(ei.value)
    # coef offset by one float
    buf = torch.zeros(128 * 4 + 4, device="cuda")
    off = buf[1:1 + 128 * 4].view(128, 4)
    off.copy_(dev(coef))
    assert off.data_ptr() % 16 == 4
    with pytest.raises(_lib.MVAEError) as ei:
        eng.train_step(PairBatch(dev(L), dev(K), dev(idx), off, key_idx=dev(kidx)), a)
    assert ei.value.code == -1 and "16-byte" in str(ei.value) and "mvae_train_step_xpairs:" in str(ei.value)
    # a null descriptor
    assert eng.lib.mvae_forward_xpairs(eng.ctx, None, None, eng.stream) == -1
    assert eng.lib.mvae_last_error(eng.ctx).decode().startswith("mvae_forward_xpairs:")
    # a batch of the wrong size, a key index of another length, key tables of another size
    with pytest.raises(ValueError):
        eng.train_step(pair_batch(L, K, idx[:64], kidx[:64], coef[:64]), a)
    with pytest.raises(ValueError):
        pair_batch(L, K, idx, kidx[:64], coef)
    with pytest.raises(ValueError):
        pair_batch(L, K[:, :10], idx, kidx, coef)
    with pytest.raises(ValueError):
        pair_batch(L, K, idx, None, coef)  # without key_idx the tables must have one shape
    # ... and the engine still steps
    eng.train_step(pair_batch(L, K, idx, kidx, coef), a)
    torch.cuda.synchronize()
    eng.close()


# ------------------------------------------------------------------ 5. the label cache
def test_pair_labels():
    from magic_amd import retrieval
    from magic_amd.overlap_input import PairLabels
    S, R = 20, 8
    L, K = xtables(S, 255, seed=31)
    coef = angle_coefficients(R, S, S)
    pl = PairLabels(dev(L), dev(K), angles=R)
    assert pl.computed == 0 and tuple(pl.matrix.shape) == (N_LOCK, N_KEY) and pl.matrix.dtype == torch.int32
    assert (pl.matrix == -1).all()
    rng = np.random.default_rng(5)
    li, kj = rng.integers(0, N_LOCK, 64), rng.integers(0, N_KEY, 64)
    li[:2], kj[:2] = (0, N_LOCK - 1), (N_KEY - 1, 0)
    distinct = sorted(set(zip(li.tolist(), kj.tolist())))
    assert len(distinct) < 64  # the draw repeats pairs
    want = {p: max_overlap_ref(L[p[0]], K[p[1]], coef)[0] for p in distinct}
    got = pl.lookup(li, kj)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (64,)
    np.testing.assert_array_equal(got.cpu().numpy(), np.array([want[p] for p in zip(li.tolist(), kj.tolist())],
                                                               np.float32))
    assert pl.computed == len(distinct)
    m = pl.matrix.cpu().numpy()
    assert (m >= 0).sum() == len(distinct) and all(m[p] == want[p] for p in distinct)
    # the same pairs again: nothing is computed
    again = pl.lookup(li, kj)
    assert pl.computed == len(distinct) and torch.equal(again, got)
    # fill(): the rest, equal to the all-pairs matrix
    full = pl.fill(chunk=9)
    assert pl.computed == N_LOCK * N_KEY and full is pl.matrix
    np.testing.assert_array_equal(full.cpu().numpy(), retrieval.overlap_matrix(L, K, angles=R))
    assert pl.fill() is pl.matrix and pl.computed == N_LOCK * N_KEY
    with pytest.raises(ValueError, match="max_pairs"):
        PairLabels(dev(L), dev(K), angles=R, max_pairs=N_LOCK * N_KEY - 1)
    with pytest.raises(ValueError):
        pl.lookup([0], [N_KEY])


# ------------------------------------------------------------------ 6. the stream
def pool_stream(**kw):
    from magic_amd.overlap_input import BatchStream
    return BatchStream(16, 20, seed=3, synthetic_pool=48, labels="computed", label_angles=8, **kw)


@pytest.mark.parametrize("fused", [False, True])
def test_own_stream_is_todays(fused):
    a, b = pool_stream(fused=fused), pool_stream(fused=fused, pairs="own", cross=0.5)
    assert b.pair_labels is None
    for _ in range(5):  # 48 / 16: past the first epoch's end
        (xa, la), (xb, lb) = next(a), next(b)
        assert torch.equal(la, lb)
        if fused:
            assert xb.key_idx is None and torch.equal(xa.idx, xb.idx) and torch.equal(xa.coef, xb.coef)
            xa, xb = xa.materialize(), xb.materialize()
        assert torch.equal(xa, xb)


def test_cross_stream_fused_and_unfused_and_its_labels():
    from magic_amd.overlap_input import PairBatch
    a, b = pool_stream(pairs="cross", cross=0.75), pool_stream(pairs="cross", cross=0.75, fused=True)
    L, K = a.locks.cpu().numpy(), a.keys.cpu().numpy()
    coef = angle_coefficients(8, 20, 20)
    crossed = kept = 0
    for _ in range(4):  # past the first epoch's end
        (x, la), (pb, lb) = next(a), next(b)
        assert isinstance(pb, PairBatch) and pb.key_idx is not None and pb.key_idx.dtype == torch.int32
        assert torch.equal(pb.materialize(), x) and torch.equal(la, lb)
        i, j = pb.idx.cpu().numpy(), pb.key_idx.cpu().numpy()
        want = [max_overlap_ref(L[p], K[q], coef)[0] for p, q in zip(i, j)]
        np.testing.assert_array_equal(la.cpu().numpy(), np.array(want, np.float32))
        own = torch.from_numpy(i).cuda().long()
        assert torch.equal(la[torch.from_numpy(i == j).cuda()], a.areas[own][torch.from_numpy(i == j).cuda()])
        crossed += int((i != j).sum())
        kept += int((i == j).sum())
    assert crossed > 0 and kept > 0
    assert a.pair_labels.computed == b.pair_labels.computed <= 64


def test_cross_pairs_need_computed_labels():
    from magic_amd.overlap_input import BatchStream, inputs
    with pytest.raises(ValueError, match="computed"):
        BatchStream(16, 20, synthetic_pool=48, labels="sampled", pairs="cross")
    with pytest.raises(ValueError, match="computed"):
        inputs(normalize=True, reshape=True, rotation=True, batch_size=16, image_size=20, pairs="mined")


def test_mined_stream_draws_from_the_models_best_keys():
    from magic_amd.config import MVAEConfig
    from magic_amd.vae import TangoEncoder
    cfg = MVAEConfig(image_size=20, batch=64, enc=(40, 24), dec=(28, 20), latent=6, metric="cosine",
                     reciprocal=False, precision="f32")
    vae = TangoEncoder(None, config=cfg, init_seed=3)
    try:
        s = pool_stream(pairs="mined", fused=True)
        pb, _ = next(s)  # before the first refresh: the uniform draw
        assert s.candidates is None and pb.key_idx is not None
        cand = s.refresh_candidates(vae, k=3)
        L, K = s.locks.cpu().numpy(), s.keys.cpu().numpy()
        want = vae.match(vae.embed(L), vae.embed(K), k=3)[1]
        assert cand.shape == (48, 3)
        np.testing.assert_array_equal(cand, want)
        seen = set()
        for _ in range(4):
            pb, a = next(s)
            i, j = pb.idx.cpu().numpy(), pb.key_idx.cpu().numpy()
            assert all(q in cand[p] for p, q in zip(i, j))
            seen |= {int(np.where(cand[p] == q)[0][0]) for p, q in zip(i, j)}
            assert torch.equal(a, s.pair_labels.lookup(i, j))
        assert seen == {0, 1, 2}  # every candidate rank is drawn
    finally:
        vae.close()


# ------------------------------------------------------------------ 7. the driver
def micro_cross_stream(fused):
    from magic_amd.overlap_input import BatchStream, PairSource
    src = PairSource.from_packed(GOLD, limit=8)
    return BatchStream(64, 200, src, seed=3, fused=fused, labels="computed", label_angles=4, pairs="cross")


def test_driver_on_a_cross_stream():
    """main.train (1 epoch of 2 steps with an evaluation) on a cross stream: an identical history
    fused and unfused."""
    from magic_amd import main
    from magic_amd.vae import TangoEncoder
    cfg = preset("11a", image_size=200, batch=64, precision="bf16")
    hist = []
    for fused in (False, True):
        vae = TangoEncoder(None, config=cfg)
        _, h = main.train(vae, micro_cross_stream(fused), 2 * 64, 1, driver="11a", eval_at=lambda epoch, i: i == 1,
                          log=lambda m: None)
        hist.append(h)
        vae.close()
    assert any(r[0] == "mse" for r in hist[0]) and any(r[0] == "epoch" for r in hist[0])
    assert all(np.isfinite(r[-1]) for r in hist[0])
    assert hist[0] == hist[1]


def test_driver_refuses_cross_pairs_without_computed_labels(capsys):
    from magic_amd import main
    for pairs in ("cross", "mined"):
        with pytest.raises(SystemExit) as ei:
            main.main(["--preset", "11a", "--image-size", "32", "--batch", "64", "--pairs", pairs])
        assert ei.value.code == 2
        assert "--labels computed" in capsys.readouterr().err


def test_driver_trains_on_cross_and_mined_pairs(capsys):
    from magic_amd import main
    for pairs in ("cross", "mined"):
        main.main(["--preset", "11a", "--image-size", "32", "--batch", "64", "--epochs", "1", "--samples-per-epoch",
                   "128", "--labels", "computed", "--label-angles", "8", "--pairs", pairs, "--cross", "0.5",
                   "--mine-k", "4", "--fused-input", "--retrieve", "10"])
        lines = [l for l in capsys.readouterr().out.splitlines() if "hit@1 = " in l]
        assert len(lines) == 1 and "hit@10 = " in lines[0]


# ------------------------------------------------------------------ 8. data parallel
def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    from magic_amd.engine import Engine
    from magic_amd.parallel import DataParallelStep
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = preset("8c", image_size=20, batch=64 * world, precision="bf16")
    L, K, idx, kidx, coef, areas = step_batches(20, 64 * world)[0]
    sl = slice(rank * 64, (rank + 1) * 64)
    out = []
    for fused in (False, True):  # both ranks run the two engines in the same order
        eng = Engine(cfg.replace(batch=64, global_batch=64 * world), 0)
        eng.load_params(make_params(cfg))
        eng.set_shard(rank * 64)
        pb = pair_batch(L, K, idx[sl], kidx[sl], np.ascontiguousarray(coef[sl]))
        st = DataParallelStep(eng)
        # (host copies only: a view of the engine's memory must not outlive the engine)
        losses = st.step(pb if fused else pb.materialize(), dev(areas[sl])).cpu().numpy().copy()
        torch.cuda.synchronize()
        out.append((losses, {k: v.cpu().numpy() for k, v in eng.params().items()}))
        del st
        eng.close()
    q.put((rank, out))
    dist.destroy_process_group()


def test_dp2_cross_pair_batches():
    """DataParallelStep.step on per-rank cross PairBatches against per-rank X: two gloo ranks on
    this GPU, losses and parameters bitwise equal on each rank."""
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
