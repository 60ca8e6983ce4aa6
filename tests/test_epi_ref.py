"""tests/epi_ref.py (the float64 restatement the GEMM epilogues are held to) checked independently of
the kernels: the BCE head against oracle/mvae_oracle.py on a tiny configuration and against float64
torch autograd, its bit packer and plane split against their definitions, and the bar itself: a
plain fp32 form of the formula stays inside 2e-6 mag at the input scales tests/test_gpu_bce.py uses,
while a reference that drops one column does not."""
import numpy as np
import pytest
import torch

from magic_amd.config import MVAEConfig
from tests import epi_ref as E
from tests.gpu_helpers import make_inputs, make_params, oracle_phases

REL = 1e-12
BAR = 2e-6
# K and the scale of B at which the accuracy cases of tests/test_gpu_bce.py run (largest |logit| 5.5-6.7)
SCALES = {21: 0.25, 65: 0.15, 200: 0.1}


def _case(M, N, K, seed, grey):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = (rng.standard_normal((K, N)) * SCALES.get(K, 1.0 / np.sqrt(K))).astype(np.float32)
    x = (rng.random((M, N)) < 0.3).astype(np.float32)
    if grey:
        x *= (rng.integers(1, 256, size=x.shape) / 255.0).astype(np.float32)
        x[0, :8] = (0, 1, 0.5, 1, 0, 0.25, 1, 0)
    return A, B, x


def test_bce_matches_the_oracle():
    cfg = MVAEConfig(image_size=6, enc=[10], dec=[7, 9], latent=4, act="tanh")
    Bt = 5
    P = make_params(cfg)
    for grey in (False, True):
        X, areas, eps = make_inputs(cfg, Bt, seed=3, density=0.3, grey=grey)
        _, _, _, _, c = oracle_phases(cfg, P, X, areas, eps)
        A = np.concatenate([c["d2"], np.ones((Bt, 1))], 1)
        Bm = np.concatenate([np.asarray(P["dec_out_mean_W"], np.float64), np.asarray(P["dec_out_mean_b"], np.float64)[None]], 0)
        r = E.bce(A, Bm, c["xl"], 1.0 / Bt)
        assert r["rowpart"].shape == (Bt, E.nblk(cfg.D))
        assert np.abs(r["rowpart"].sum(1) - c["R"]).max() <= REL * np.abs(c["R"]).max()
        assert np.abs(r["y"] - c["y"]).max() <= REL
        assert np.abs(r["du"] - (c["y"] - c["xl"]) / Bt).max() <= REL


@pytest.mark.parametrize("grey", [False, True])
def test_bce_du_is_the_gradient_of_the_row_partials(grey):
    M, N, K, scale = 9, 140, 21, 1.0 / 9
    A, B, x = _case(M, N, K, 5, grey)
    r = E.bce(A, B, x, scale)
    v = torch.tensor(r["v"], requires_grad=True)
    xt = torch.tensor(x.astype(np.float64))
    ls = torch.nn.functional.logsigmoid
    terms = xt * ls(v) + (1 - xt) * ls(-v)
    loss = -scale * terms.sum()
    g, = torch.autograd.grad(loss, v)
    assert np.abs(r["du"] - g.numpy()).max() <= REL
    assert abs(scale * r["rowpart"].sum() - loss.item()) <= REL * r["rowpart_mag"].sum()
    # the blocks: 128 columns and the 12 left
    t = -terms.detach().numpy()
    assert np.abs(r["rowpart"][:, 0] - t[:, :128].sum(1)).max() <= REL * r["rowpart_mag"].max()
    assert np.abs(r["rowpart"][:, 1] - t[:, 128:].sum(1)).max() <= REL * r["rowpart_mag"].max()


def test_bce_saturation_semantics():
    A = np.array([[30.0], [100.0], [1.0]])
    B = np.array([[1.0, -1.0, 0.0, 1.0, -1.0, 1.0, -1.0]])
    x = np.array([[1, 0, 0.5, 0, 1, 0.5, 0.5]] * 3, np.float64)
    r = E.bce(A, B, x, 0.5, sat=True)
    inf = np.inf
    # v = +30: y = 1; v = -30: y = exp(-30) (an fp32 number, not 0); v = +-100: y = 1 / 0
    assert r["y"][0, 0] == 1 and 0 < r["y"][0, 1] < 1e-12 and r["y"][1, 0] == 1 and r["y"][1, 1] == 0
    t0 = r["term"][0]
    assert t0[0] == 0 and t0[2] == np.log(0.5) and t0[3] == -inf and t0[5] == -inf
    assert abs(t0[1]) < 1e-12 and abs(t0[4] + 30) < 1e-9 and abs(t0[6] + 15) < 1e-9
    assert list(r["term"][1]) == [0, 0, np.log(0.5), -inf, -inf, -inf, -inf]
    assert r["rowpart"][0, 0] == inf and r["rowpart"][1, 0] == inf and np.isfinite(r["rowpart"][2, 0])
    assert np.isfinite(r["du"]).all() and not np.isnan(r["term"]).any()
    assert np.array_equal(r["du"][1], (np.array([1, 0, 0.5, 1, 0, 1, 0]) - x[1]) * 0.5)
    assert not np.isnan(r["term_mag"]).any()
    with pytest.raises(AssertionError):
        E.bce(np.array([[15.0]]), np.array([[1.0]]), np.array([[1.0]]), 1.0, sat=True)
    with pytest.raises(AssertionError):
        E.check_accuracy_logits(np.array([8.5]))


def test_pack_bits_and_plane_split():
    rng = np.random.default_rng(2)
    x = (rng.random((5, 21)) < 0.5).astype(np.float32)
    bits = E.pack_bits(x)
    assert bits.shape == (5, 3) and bits.dtype == np.uint8
    for r in range(5):
        for c in range(24):
            assert (bits[r, c >> 3] >> (c & 7)) & 1 == (c < 21 and x[r, c] != 0)
    v = np.concatenate([rng.standard_normal(4000).astype(np.float32) * 3,
                        np.array([0, -0.0, 1, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, np.inf], np.float32)])
    p = E.split_planes(v, 3)
    want = torch.from_numpy(v).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(p[0], want)   # torch's conversion rounds to nearest even
    assert np.array_equal(E.split_planes(v, 1)[0], want)
    fin = np.isfinite(v)
    s = (E.bf16_to_f32(p[2]).astype(np.float64) + E.bf16_to_f32(p[1]) + E.bf16_to_f32(p[0]))[fin]
    assert np.array_equal(s.astype(np.float32), v[fin])   # three planes hold all 24 bits


@pytest.mark.parametrize("K", sorted(SCALES))
@pytest.mark.parametrize("grey", [False, True])
def test_fp32_form_is_inside_the_bar_and_a_dropped_column_is_not(K, grey):
    """The 2e-6 mag bar is not sized from the kernels: a plain fp32 evaluation of the formula sits
    well inside it (worst error / bound printed), and the same reference without the last column of
    the last block is outside it by a factor of 50 or more in every row (the smallest of the 1800 rows of
    these six cases: 97; the median row: beyond 1000)."""
    M, N = 300, 392
    A, B, x = _case(M, N, K, 100 + K, grey)
    r = E.bce(A, B, x, 1.0 / M)
    E.check_accuracy_logits(r["v"])
    e = E.bce_fp32_emulation(A, B, x, 1.0 / M)
    worst = {k: (np.abs(e[k].astype(np.float64) - r[k]) / (BAR * r[k + "_mag"])).max()
             for k in ("rowpart", "term", "du", "y")}
    print(f"EPI_EMU K={K} grey={grey} max|v|={np.abs(r['v']).max():.2f} " +
          " ".join(f"{k}={w:.3f}" for k, w in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    assert worst["rowpart"] <= 0.1 and worst["term"] <= 0.25 and worst["du"] <= 0.25
    mut = E.bce(A, B[:, :N - 1], x[:, :N - 1], 1.0 / M)
    ratio = np.abs(mut["rowpart"][:, -1] - r["rowpart"][:, -1]) / (BAR * r["rowpart_mag"][:, -1])
    print(f"EPI_EMU K={K} grey={grey} dropped column: min ratio {ratio.min():.0f} median {np.median(ratio):.0f}")
    assert ratio.min() >= 50.0 and np.median(ratio) >= 1000.0


@pytest.mark.parametrize("kind", [0, 1])
def test_act_and_dact_against_autograd(kind):
    rng = np.random.default_rng(7)
    M, N, K = 12, 10, 6
    A, B = rng.standard_normal((M, K)), rng.standard_normal((K, N)) * 0.5
    a = E.act(A, B, kind)
    v = torch.tensor(a["v"], requires_grad=True)
    out = torch.tanh(v) if kind == 0 else torch.nn.functional.elu(v)
    assert np.abs(a["out"] - out.detach().numpy()).max() <= REL
    # the dgrad through that activation, aux = its output; rows 8.. read aux rows 4.. (remap)
    g = rng.standard_normal((M, K))
    Bt = rng.standard_normal((K, N))
    aux = out.detach().numpy()[:8]
    d = E.dact(g, Bt, aux, kind, remap_split=8, remap_shift=4)
    rows = np.concatenate([np.arange(8), np.arange(4, 8)])
    assert np.array_equal(E.remap_rows(M, 8, 4), rows)
    up = torch.tensor(g @ Bt)
    vv = torch.tensor(a["v"][rows], requires_grad=True)
    oo = torch.tanh(vv) if kind == 0 else torch.nn.functional.elu(vv)
    gr, = torch.autograd.grad((oo * up).sum(), vv)
    assert np.abs(d["out"] - gr.numpy()).max() <= REL * d["mag"].max()
    assert np.array_equal(E.remap_rows(5, 0, 0), np.arange(5))
