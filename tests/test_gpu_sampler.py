"""The internal N(0,1) sampler (Philox4x32-10 + Box-Muller, mvae_kernels.hip normal4) pinned
value by value to oracle/philox_oracle.py: the counter -> word mapping, the [3, B, L] slot
layout, the L % 4 != 0 path, the high words of seed and call counter, the eval stream's bit 63,
the sharded stream, and that the draw the latent kernels regenerate in registers (forward and
backward) is bit for bit the one MVAE_BUF_EPS hands out.

Not reachable at test size: the second counter word (q >> 32) is nonzero only from 2^34
elements of one draw on.
"""
import numpy as np
import pytest
import torch

from magic_amd import _lib
from magic_amd.config import MVAEConfig
from oracle import philox_oracle as PH
from tests.gpu_helpers import make_inputs, make_params, to_dev

pytestmark = pytest.mark.gpu

# |gpu - reference| per element. A structural bar, not an accuracy claim: with u rounded as the
# kernel rounds it the only difference is the hardware log2 / sin / cos / sqrt (about 1 ulp by the
# kernel's comments, on values <= 6.8), while an element that took another word or index is an
# unrelated normal and lands within 1e-3 with probability < 1e-3.
EPS_BAR = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cfg(B, L, seed=2, metric="sqdiff", precision="f32", global_batch=None):
    return MVAEConfig(image_size=8, batch=B, global_batch=global_batch, enc=(32,), dec=(28, 20), latent=L,
                      act="tanh", metric=metric, reciprocal=False, deform_weight=10.0, lr=(1e-3, 1e-4),
                      precision=precision, seed=seed)


def _engine(cfg, load=True):
    from magic_amd.engine import Engine
    eng = Engine(cfg, 0)
    if load:
        eng.load_params(make_params(cfg))
    return eng


def _eps(eng):
    """The last forward's eps [3, B, L] as float64 (the pointer is re-fetched: mvae.h)."""
    e = eng.buffer(_lib.BUF_EPS).clone()
    torch.cuda.synchronize()
    return e.cpu().numpy().astype(np.float64).reshape(3, eng.cfg.batch, eng.cfg.latent)


def _max_err(got, ref, what):
    err = float(np.abs(got - ref).max())
    print(f"sampler {what}: max |gpu - reference| = {err:.3e} over {got.size} elements")
    return err


@pytest.mark.parametrize("B,L,seed,counter", [
    (24, 8, 2, 0),                      # 4 columns per lane, one Philox block each
    (7, 5, 0x9E3779B97F4A7C15, 3),      # scalar path; slots start off a block boundary; high seed word
    (4, 1024, 2, 2 ** 32 + 5),          # four waves per row; high counter word
    (9, 2, 2, 0),                       # L = 2
])
def test_internal_eps_matches_philox_reference(B, L, seed, counter):
    """forward(x, None) draws call `counter` of the training stream, the next forward call
    counter + 1.

    Measured on MI355X, maximum |gpu - reference| over the four cases and both calls: 4.4e-7
    (2.9e-7, 2.4e-7, 4.4e-7, 2.9e-7 per case; the eval-stream and shard draws of the next test:
    2.8e-7) -- a few fp32 ulp of values up to ~4, far under the bar."""
    cfg = _cfg(B, L, seed)
    eng = _engine(cfg)
    try:
        x = to_dev(make_inputs(cfg, B)[0])
        eng.set_rng(counter, 0)
        for k in range(2):
            eng.forward(x, None)
            got = _eps(eng)
            ref = PH.eps_reference(seed, counter + k, B, L)
            assert _max_err(got, ref, f"B={B} L={L} call {counter + k}") <= EPS_BAR
        assert eng.get_rng() == (counter + 2, 0)
    finally:
        eng.close()


def test_eval_stream_and_shard_match_reference():
    """predict draws from the stream with bit 63 set and moves only the eval counter; a rank of a
    row-sharded batch draws its slice of the global batch's eps."""
    B, L, seed = 7, 5, 2
    cfg = _cfg(B, L, seed)
    eng = _engine(cfg)
    try:
        x = to_dev(make_inputs(cfg, B)[0])
        assert eng.get_rng() == (0, 0)
        for k in range(2):
            eng.predict(x, None)
            ref = PH.eps_reference(seed, PH.EVAL_STREAM | k, B, L)
            assert _max_err(_eps(eng), ref, f"eval call {k}") <= EPS_BAR
            assert eng.get_rng() == (0, k + 1)
    finally:
        eng.close()
    for L in (5, 8):
        cfg = _cfg(8, L, seed, global_batch=24)
        eng = _engine(cfg)
        try:
            eng.set_shard(8)
            eng.forward(to_dev(make_inputs(cfg, 8)[0]), None)
            ref = PH.eps_reference(seed, 0, Bg=24, L=L, off=8, B=8)
            assert _max_err(_eps(eng), ref, f"shard rows 8..15 of 24, L={L}") <= EPS_BAR
        finally:
            eng.close()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("prec", ["f32", "f32x", "bf16"])
@pytest.mark.parametrize("B,L,metric", [(24, 8, "cosine"), (7, 5, "sqdiff"), (4, 1024, "cosine")])
def test_regenerated_eps_equals_materialised(prec, B, L, metric):
    """The draw regenerated in registers by the latent forward and backward is the draw
    MVAE_BUF_EPS writes out: a second engine fed that buffer as the caller's eps gives bitwise the
    losses, distances and the whole gradient bucket; the same for predict on the eval stream."""
    cfg = _cfg(B, L, metric=metric, precision=prec)
    X, areas, _ = make_inputs(cfg, B)
    x, a = to_dev(X), to_dev(areas)
    e1, e2 = _engine(cfg), _engine(cfg)
    try:
        e1.forward(x, None)
        e1.metric(a)
        e1.backward()
        e = e1.buffer(_lib.BUF_EPS).clone().reshape(3, B, L)
        e2.forward(x, e)
        e2.metric(a)
        e2.backward()
        torch.cuda.synchronize()
        assert np.isfinite(e1.losses.cpu().numpy()).all()
        assert torch.equal(_bits(e1.losses), _bits(e2.losses))
        assert torch.equal(_bits(e1.dist), _bits(e2.dist))
        assert torch.equal(_bits(e1.grads), _bits(e2.grads))
        assert e1.grads.abs().max().item() > 0
        d1 = e1.predict(x, None)
        ee = e1.buffer(_lib.BUF_EPS).clone().reshape(3, B, L)
        assert not torch.equal(ee, e)
        d2 = e2.predict(x, ee)
        torch.cuda.synchronize()
        assert torch.equal(_bits(d1), _bits(d2))
    finally:
        e1.close()
        e2.close()


def test_counter_validation():
    """Counters own 63 bits (bit 63 is the eval stream); step counters are not negative."""
    eng = _engine(_cfg(4, 4), load=False)
    try:
        with pytest.raises(_lib.MVAEError):
            eng.set_rng(1 << 63, 0)
        with pytest.raises(_lib.MVAEError):
            eng.set_rng(0, 1 << 63)
        with pytest.raises(_lib.MVAEError):
            eng.set_step(-1, 0)
        assert eng.get_rng() == (0, 0) and eng.get_step() == (0, 0)
        eng.set_rng((1 << 63) - 1, 5)
        assert eng.get_rng() == ((1 << 63) - 1, 5)
    finally:
        eng.close()
