"""Every route that turns a batch into the layer-0 bit operand -- the step's de-interleave of an
fp32 X, the pairs kernel on the uint8 lock / key tables, the embedding kernel on one image table --
against the host reference of ``tests/bits_ref.py``: every word of the forward and weight-gradient
BitMats, the target bits, the four flag ints and bf16 plane 0. One batch per (shape, values) is built
on the host and handed to the three routes in their own form, so they share one reference. All
comparisons are exact: the kernels move bits and round once to bf16."""
import functools

import numpy as np
import pytest
import torch

from magic_amd import _lib
from oracle import input_oracle
from tests import bits_ref
from tests.test_gpu_pairs import dev, draws

pytestmark = pytest.mark.gpu

N_LOCK, N_KEY = 5, 7
SHAPES = [(64, 8),    # D = 64: the ones column alone in k-tile 1, at the pq > D boundary
          (64, 12),   # D = 144: a pixel half-task partly past D
          (64, 16),   # D = 256: the ones row opens a new 256-pixel strip of xbw
          (128, 20),  # D = 400: the partial last octet group
          (320, 12)]  # 3B = 960: block boundaries at rows 320 and 640; rows past 3B in the last strip
VALUES = {"bin255": (255, 255.0), "bin1": (1, 1.0), "grey7": (255, 255.0), "255div1": (255, 1.0)}


@functools.lru_cache(maxsize=None)
def batch(B, S, values):
    """One batch in the three routes' forms and its reference: the pairs tables with (idx, key_idx,
    coef); the stacked rows' images, shuffled, as one table with its idx [3B]; the host's X."""
    hi, div = VALUES[values]
    rng = np.random.default_rng(1000 * B + S)
    L = ((rng.random((N_LOCK, S, S)) < 0.3) * hi).astype(np.uint8)
    K = ((rng.random((N_KEY, S, S)) < 0.3) * hi).astype(np.uint8)
    if values == "grey7":
        L[0, S // 2, S // 3] = 7  # (idx holds lock 0)
    idx, coef = draws(B, S, seed=B + S)
    kidx = rng.integers(0, N_KEY, B).astype(np.int32)
    kidx[0], kidx[1] = N_KEY - 1, 0
    x = input_oracle.make_batch(L[idx], K[kidx], np.arange(B), coef, scale_div=div)
    rows = np.concatenate([np.stack([input_oracle.rotate_nearest(L[i], c) for i, c in zip(idx, coef)]),
                           L[idx], K[kidx]])  # [3B][S][S] uint8: rot | lock | key
    perm = rng.permutation(3 * B)
    table, tidx = rows[perm], np.argsort(perm).astype(np.int32)
    D = S * S
    ref = bits_ref.operand(x, B, D, D + 8, (D // 8 + 15) // 16 * 16)
    for v in ref.values():
        v.setflags(write=False)
    return dict(L=L, K=K, idx=idx, kidx=kidx, coef=coef, x=x, table=table, tidx=tidx, div=div, ref=ref)


def run_route(mode, b, B, S, no_xbw):
    """mvae_debug_pairs_bits / mvae_debug_xpairs_bits on buffers sized as
    tests/test_gpu_pairs.py::debug_bits sizes them, zero-filled but for the other flag slot (dyn[1],
    dyn[3]: the kernel has to zero it) -> dict of host arrays"""
    lib = _lib.load()
    D = S * S
    ldx, ldbits = D + 8, (D // 8 + 15) // 16 * 16
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    out = dict(xbf=z(bits_ref.bitmat_words(3 * B, D + 1), torch.int32),
               xbw=z(bits_ref.bitmat_words(D + 1, 3 * B), torch.int32), xbits=z(B * ldbits, torch.uint8),
               dyn=torch.tensor([0, 5, 0, 9], dtype=torch.int32, device="cuda"), plane=z(3 * B * ldx, torch.int16))
    tail = (out["xbf"].data_ptr(), out["xbw"].data_ptr(), out["xbits"].data_ptr(), ldbits, out["dyn"].data_ptr(),
            out["plane"].data_ptr(), ldx, torch.cuda.current_stream().cuda_stream)
    if mode == 1:
        t = [dev(b[k]) for k in ("L", "K", "idx", "kidx", "coef")]
        rc = lib.mvae_debug_xpairs_bits(*(a.data_ptr() for a in t), B, S, b["div"], 1, int(no_xbw), None, *tail)
    elif mode == 2:
        t = [dev(b["table"]), dev(b["tidx"])]
        rc = lib.mvae_debug_pairs_bits(t[0].data_ptr(), None, t[1].data_ptr(), None, B, S, b["div"], 2, int(no_xbw),
                                       None, *tail)
    else:
        t = [dev(b["x"])]
        rc = lib.mvae_debug_pairs_bits(None, None, None, None, B, S, b["div"], 3, int(no_xbw), t[0].data_ptr(), *tail)
    _lib.check(lib, None, rc)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("no_xbw", [0, 1], ids=["xbw", "no_xbw"])
@pytest.mark.parametrize("mode", [3, 1, 2], ids=["x", "pairs", "images"])
@pytest.mark.parametrize("values", list(VALUES))
@pytest.mark.parametrize("B,S", SHAPES, ids=[f"B{b}_S{s}" for b, s in SHAPES])
def test_bit_operand_is_the_host_reference(B, S, values, mode, no_xbw):
    b = batch(B, S, values)
    ref = b["ref"]
    grey = values in ("grey7", "255div1")
    assert ref["dyn"].tolist() == [int(values == "grey7"), 0, int(grey), 0]  # the case is what it says
    assert ref["plane"].any() == grey and ref["xbf"].any() and ref["xbw"].any() and ref["xbits"].any()
    got = run_route(mode, b, B, S, no_xbw)
    for k in ("xbf", "xbits", "dyn", "plane") + (() if no_xbw else ("xbw",)):
        want = ref[k]
        np.testing.assert_array_equal(got[k].view(want.dtype), want, err_msg=k)
    if no_xbw:
        assert not got["xbw"].any()  # the forward words only
