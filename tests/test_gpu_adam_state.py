"""Adam past its first step, and resume.

* The dual Adam update (adam_kernel, adam_args, the fp32 beta powers kept by mvae_adam and
  recomputed by mvae_set_step) over eight steps and from unequal step counters, parameters AND
  moment buffers, element by element against oracle.mvae_oracle.adam in float64. The gradients
  are injected through the KIND_GRAD1 / KIND_GRAD2 views exactly as a data-parallel host's
  all-reduce writes them, so the comparison is of Adam alone and the elements can be chosen where
  an optimizer goes wrong (zeros, g^2 underflowing, cancelling first moments, 6 decades of scale).
* A checkpoint (TangoEncoder.state_dict / load_state_dict) resumes bit for bit in every precision
  mode: the interrupted model carries weight planes written inside adam_kernel, beta powers
  multiplied up step by step and a dyn-flag slot mid-alternation; the resumed one planes re-split
  by mvae_sync_params, powers recomputed by mvae_set_step and slot 0.

The bounds (u = 2^-24, s the 1-based step, G the largest |g| -- or initial |m|, sqrt(v) -- the
element has seen) are forward bounds of the three to four fp32 roundings of one update:

    m      4 s u G   + 1e-45
    v      4 s u G^2 + 1e-44
    theta  s (2 u |theta| + 1e-4 (lr1 + lr2))        (the last term: check_step's per-step bar)

test_fp32_oracle_stays_within_adam_bounds (CPU) shows a correct fp32 Adam -- the oracle's own fp32
mode -- inside them with 5x room (moments) and 4x room (parameters) on the same gradients; the
GPU's FMA contraction and its division / square-root rounding get the rest.

Only this file's GPU tests carry the gpu mark (not the module): the fp32-oracle check runs
without a GPU.
"""
import numpy as np
import pytest
import torch

from magic_amd import _lib
from magic_amd.config import preset
from oracle import mvae_oracle as O
from tests.gpu_helpers import make_inputs, make_params, oracle_cfg, to_dev
from tests.test_gpu_parity import tiny

U = 2.0 ** -24
STEPS = 8
KINDS = {"m1": _lib.KIND_M1, "v1": _lib.KIND_V1, "m2": _lib.KIND_M2, "v2": _lib.KIND_V2}

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def adam_cfg(**kw):
    return tiny("elu", "sqdiff", True, 100.0, **kw)


# ------------------------------------------------------------------ crafted gradients
def crafted_grads(shapes, steps, seed):
    """steps x {name: float32 array}. Base: magnitude 10^U(-6, 0) with a random sign, times a
    per-step factor U(0.5, 2) with 30 % sign flips. A fixed random mask puts four classes in
    places (5 % of the elements each): always 0; 0 on odd steps; +-1e-20 (g^2 underflows the fp32
    normal range); strictly alternating sign (the first moment cancels)."""
    rng = np.random.default_rng(seed)
    fixed = {}
    for n, shp in shapes.items():
        mag = 10.0 ** rng.uniform(-6.0, 0.0, size=shp)
        sign = np.where(rng.random(shp) < 0.5, -1.0, 1.0)
        cls = rng.choice(5, size=shp, p=[0.8, 0.05, 0.05, 0.05, 0.05])
        fixed[n] = (mag, sign, cls)
    out = []
    for s in range(1, steps + 1):
        gs = {}
        for n, shp in shapes.items():
            mag, sign, cls = fixed[n]
            f = rng.uniform(0.5, 2.0, size=shp)
            flip = np.where(rng.random(shp) < 0.3, -1.0, 1.0)
            g = mag * sign * f * flip
            g = np.where(cls == 1, 0.0, g)
            g = np.where((cls == 2) & (s % 2 == 1), 0.0, g)
            g = np.where(cls == 3, 1e-20 * sign * flip, g)
            g = np.where(cls == 4, mag * sign * f * (-1.0) ** s, g)
            gs[n] = g.astype(np.float32)
        out.append(gs)
    return out


def grad_recipe(oc, P, steps, seed=11):
    """g1 over every trained variable and g2 over the encoder's, drawn independently."""
    s1 = {n: P[n].shape for n in O.trained_names(oc)}
    s2 = {n: P[n].shape for n in O.encoder_names(oc)}
    return crafted_grads(s1, steps, seed), crafted_grads(s2, steps, seed + 1)


class Bounds:
    """The per-element bounds above; tracks G and the worst ratio error / bound per quantity."""

    def __init__(self, oc, m0=None, v0=None):
        """m0, v0: {(optimizer, name): initial |m|, initial v} when the moments do not start at 0."""
        self.lr = float(oc.lr[0] + oc.lr[1])
        self.G = dict(m0 or {})
        self.G2 = dict(v0 or {})
        self.worst = {"m": 0.0, "v": 0.0, "theta": 0.0}

    def see(self, o, g):
        for n, a in g.items():
            k, a = (o, n), np.abs(a.astype(np.float64))
            self.G[k] = np.maximum(self.G.get(k, 0.0), a)
            self.G2[k] = np.maximum(self.G2.get(k, 0.0), a * a)

    def check(self, s, got, ref, what, name, o=None):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        if what == "m":
            bound = 4 * s * U * self.G[(o, name)] + 1e-45
        elif what == "v":
            bound = 4 * s * U * self.G2[(o, name)] + 1e-44
        else:
            bound = s * (2 * U * np.abs(ref) + 1e-4 * self.lr)
        ratio = float((np.abs(got - ref) / bound).max())
        self.worst[what] = max(self.worst[what], ratio)
        assert ratio <= 1.0, (what, o, name, "step", s, "error / bound", ratio)


def test_fp32_oracle_stays_within_adam_bounds():
    """The oracle's fp32 mode against its float64 mode on the crafted gradients: a correct fp32
    Adam uses a fifth of the moment bounds and a quarter of the parameter bound at the most.
    Measured with this recipe: m 0.043, v 0.153, theta 0.203 of the bound. (theta's error is the
    two roundings of theta - d1 - d2 per step, up to 2 u |theta| of the per-step bound
    2 u |theta| + 1e-4 (lr1 + lr2), and adds up like a random walk: its ratio can never pass 1
    for a correct fp32 Adam, and sits near 0.2 for weights of magnitude ~0.3.)"""
    cfg = adam_cfg()
    oc = oracle_cfg(cfg)
    P = make_params(cfg)
    g1s, g2s = grad_recipe(oc, P, STEPS)
    P64 = {k: v.astype(np.float64) for k, v in P.items()}
    P32 = {k: v.copy() for k, v in P.items()}
    st64, st32 = O.adam_init(oc, P64), O.adam_init(oc, P32)
    bd = Bounds(oc)
    for s in range(1, STEPS + 1):
        g1, g2 = g1s[s - 1], g2s[s - 1]
        bd.see(1, g1)
        bd.see(2, g2)
        P64, st64 = O.adam(P64, {k: v.astype(np.float64) for k, v in g1.items()},
                           {k: v.astype(np.float64) for k, v in g2.items()}, st64, oc)
        P32, st32 = O.adam(P32, g1, g2, st32, oc, dtype=np.float32)
        assert all(v.dtype == np.float32 for v in P32.values())
        for o, g in ((1, g1), (2, g2)):
            for n in g:
                assert st32[f"m{o}"][n].dtype == np.float32
                bd.check(s, st32[f"m{o}"][n], st64[f"m{o}"][n], "m", n, o)
                bd.check(s, st32[f"v{o}"][n], st64[f"v{o}"][n], "v", n, o)
        for n in g1:
            bd.check(s, P32[n], P64[n], "theta", n)
    print("fp32 oracle / bound:", {k: round(v, 3) for k, v in bd.worst.items()})
    assert bd.worst["m"] <= 0.2 and bd.worst["v"] <= 0.2 and bd.worst["theta"] <= 0.25, bd.worst


# ------------------------------------------------------------------ GPU helpers
def _engine(cfg):
    from magic_amd.engine import Engine
    return Engine(cfg, 0)


def _host(views):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in views.items()}


def _put(views, arrays):
    for k, a in arrays.items():
        views[k].copy_(to_dev(np.asarray(a, np.float32)))


def _uncovered(eng, buf_id, kinds):
    """Indices of the flat buffer that no named view of ``kinds`` covers (row padding, the ones
    columns' slots, alignment gaps)."""
    buf = eng.buffer(buf_id)
    base = buf.data_ptr()
    covered = np.zeros(buf.numel(), bool)
    for kind in kinds:
        for name, v in eng.tensors(kind).items():
            if name in O.DEAD:  # MVAE_BUF_DEAD, not the parameter buffer
                continue
            off = (v.data_ptr() - base) // 4
            if v.dim() == 2:
                idx = off + np.arange(v.shape[0])[:, None] * v.stride(0) + np.arange(v.shape[1])[None, :]
            else:
                idx = off + np.arange(v.shape[0])
            assert idx.min() >= 0 and idx.max() < covered.size
            assert not covered[idx].any(), ("views overlap", name)
            covered[idx] = True
    return torch.from_numpy(np.flatnonzero(~covered)).to(buf.device)


def _backward_phase(eng, cfg, seed):
    """forward / metric / backward on a real batch: mvae_adam wants the backward behind it."""
    X, areas, eps = make_inputs(cfg, cfg.batch, seed=seed)
    eng.forward(to_dev(X), to_dev(eps))
    eng.metric(to_dev(areas))
    eng.backward()


def _compare_state(eng, oc, bd, s, Po, st):
    Pg = _host(eng.params())
    for tag, kind in KINDS.items():
        o = int(tag[1])
        got = _host(eng.tensors(kind))
        assert set(got) == set(st[tag])
        for n in got:
            bd.check(s, got[n], st[tag][n], tag[0], n, o)
    for n in O.trained_names(oc):
        bd.check(s, Pg[n], Po[n], "theta", n)
    return Pg


# ------------------------------------------------------------------ trajectory
@gpu
@pytest.mark.usefixtures("_need_gpu")
@pytest.mark.parametrize("opts", ["", "adam_nt=0"], ids=["nt", "plain"])
@pytest.mark.parametrize("prec", ["f32", "f32x", "bf16"])
def test_adam_trajectory_matches_float64(prec, opts):
    """Eight Adam steps on injected gradients: parameters, m1, v1, m2, v2 element by element
    within the bounds of the module docstring; step counters; dead variables and every element of
    MVAE_BUF_PARAMS / MVAE_BUF_ADAM outside the named views bitwise untouched.

    Measured on MI355X, worst error / bound: m 0.131, v 0.153, theta 0.251, the same figures in
    all six cases (the fp32 oracle on the same gradients: 0.043, 0.153, 0.203)."""
    cfg = adam_cfg(precision=prec, options=opts)
    oc = oracle_cfg(cfg)
    P = make_params(cfg)
    g1s, g2s = grad_recipe(oc, P, STEPS)
    eng = _engine(cfg)
    try:
        eng.load_params(P)
        Po = {k: v.astype(np.float64) for k, v in P.items()}
        st = O.adam_init(oc, Po)
        bd = Bounds(oc)
        gap_p = _uncovered(eng, _lib.BUF_PARAMS, [_lib.KIND_PARAM])
        gap_a = _uncovered(eng, _lib.BUF_ADAM, list(KINDS.values()))
        pad_p = eng.buffer(_lib.BUF_PARAMS)[gap_p].clone()
        pad_a = eng.buffer(_lib.BUF_ADAM)[gap_a].clone()
        for s in range(1, STEPS + 1):
            g1, g2 = g1s[s - 1], g2s[s - 1]
            _backward_phase(eng, cfg, seed=20 + s)
            _put(eng.tensors(_lib.KIND_GRAD1), g1)
            _put(eng.tensors(_lib.KIND_GRAD2), g2)
            eng.adam()
            torch.cuda.synchronize()
            bd.see(1, g1)
            bd.see(2, g2)
            Po, st = O.adam(Po, {k: v.astype(np.float64) for k, v in g1.items()},
                            {k: v.astype(np.float64) for k, v in g2.items()}, st, oc)
            Pg = _compare_state(eng, oc, bd, s, Po, st)
            assert eng.get_step() == (s, s)
            for n in O.DEAD:
                np.testing.assert_array_equal(Pg[n], P[n].astype(np.float64))
        print(f"adam {prec} {opts or 'default'} worst error / bound:",
              {k: round(v, 3) for k, v in bd.worst.items()})
        same_p = torch.equal(eng.buffer(_lib.BUF_PARAMS)[gap_p].view(torch.int32), pad_p.view(torch.int32))
        same_a = torch.equal(eng.buffer(_lib.BUF_ADAM)[gap_a].view(torch.int32), pad_a.view(torch.int32))
        assert same_p and same_a, ("elements outside the views changed", same_p, same_a,
                                   gap_p.numel(), gap_a.numel())
    finally:
        eng.close()


def _f32_power(beta, t):
    """beta^(t + 1) as t fp32 multiplies from beta (adam_init + t steps of adam)."""
    p = np.float32(beta)
    for _ in range(t):
        p = np.float32(p * np.float32(beta))
    return p


@gpu
@pytest.mark.usefixtures("_need_gpu")
def test_unequal_step_counters():
    """set_step(1000, 3), known nonzero moments, one step: each optimizer's bias correction comes
    from its own counter (swapped powers move the encoder by ~lr, orders of magnitude over the
    bound). G of the bounds is max(|g|, initial |m|) for m and max(g^2, initial v) for v: the
    roundings of m + (g - m) (1 - beta) scale with the larger of the two.

    Measured on MI355X, worst error / bound: m 0.404, v 0.298, theta 0.373."""
    cfg = adam_cfg()
    oc = oracle_cfg(cfg)
    P = make_params(cfg)
    g1s, g2s = grad_recipe(oc, P, 1, seed=31)
    g1, g2 = g1s[0], g2s[0]
    rng = np.random.default_rng(5)
    init = {}
    for tag, names in (("m1", g1), ("v1", g1), ("m2", g2), ("v2", g2)):
        init[tag] = {n: ((rng.standard_normal(P[n].shape) * 1e-3) if tag[0] == "m" else
                         10.0 ** rng.uniform(-8.0, -4.0, size=P[n].shape)).astype(np.float32) for n in names}
    eng = _engine(cfg)
    try:
        eng.load_params(P)
        eng.set_step(1000, 3)
        assert eng.get_step() == (1000, 3)
        for tag, kind in KINDS.items():
            _put(eng.tensors(kind), init[tag])
        _backward_phase(eng, cfg, seed=21)
        _put(eng.tensors(_lib.KIND_GRAD1), g1)
        _put(eng.tensors(_lib.KIND_GRAD2), g2)
        eng.adam()
        torch.cuda.synchronize()
        Po = {k: v.astype(np.float64) for k, v in P.items()}
        st = O.adam_init(oc, Po)
        for tag in KINDS:
            st[tag] = {n: a.astype(np.float64) for n, a in init[tag].items()}
        for o, t in ((1, 1000), (2, 3)):
            st[f"b1p{o}"], st[f"b2p{o}"] = _f32_power(oc.beta1, t), _f32_power(oc.beta2, t)
        bd = Bounds(oc, {(o, n): np.abs(a.astype(np.float64)) for o in (1, 2) for n, a in init[f"m{o}"].items()},
                    {(o, n): a.astype(np.float64) for o in (1, 2) for n, a in init[f"v{o}"].items()})
        bd.see(1, g1)
        bd.see(2, g2)
        Po, st = O.adam(Po, {k: v.astype(np.float64) for k, v in g1.items()},
                        {k: v.astype(np.float64) for k, v in g2.items()}, st, oc)
        _compare_state(eng, oc, bd, 1, Po, st)
        print("adam unequal counters worst error / bound:", {k: round(v, 3) for k, v in bd.worst.items()})
        assert eng.get_step() == (1001, 4)
    finally:
        eng.close()


# ------------------------------------------------------------------ resume
def _resume_cfg(case):
    if case == "f32":
        return adam_cfg(), 0.1
    if case == "f32x":  # batch % 64 == 0 and D % 8 == 0: the bits plans apply
        return preset("8c", image_size=24, batch=64, precision="f32x").replace(enc=(300, 200), latent=20), 0.1
    if case == "bf16":  # enc_chain / dec_chain at their defaults; early Adam inside train_step
        return preset("8d", image_size=24, batch=64, precision="bf16").replace(enc=(400, 300, 260), latent=16), 0.1
    from tests.test_gpu_conv import tiny_conv
    return tiny_conv("tanh", "cosine", False, 10.0, precision="bf16"), 0.3


def _dyn(vae):
    if vae.config.precision == "f32":
        return None
    return int(vae.engine.buffer(_lib.BUF_DYN).view(torch.int32).item())


def _fit(vae, batch):
    """partial_fit with internal eps -> (five losses, distances, dyn flag) as exact bit patterns."""
    out = vae.partial_fit(batch[0], batch[1])
    return np.array(out[:5], np.float64), np.asarray(out[5]).copy(), _dyn(vae)


@gpu
@pytest.mark.usefixtures("_need_gpu")
@pytest.mark.parametrize("case", ["f32", "f32x", "bf16", "conv_bf16"])
def test_resume_is_bitwise(case):
    """Model A trains on exact, grey, exact batches with get_predictions between the steps (the
    eval counter is nonzero; five de-interleaves in all, so A's dyn-flag slot is the odd one while
    a fresh context starts at slot 0), is saved, and goes on with grey, exact, exact. Model C (other
    initial weights) loads the checkpoint and runs the same three batches: losses, distances and
    the dyn flag after every step, and every parameter / moment tensor and both counter pairs at
    the end, are bitwise A's."""
    from magic_amd.vae import TangoEncoder
    cfg, density = _resume_cfg(case)
    exact = make_inputs(cfg, cfg.batch, seed=3, density=density)
    grey = make_inputs(cfg, cfg.batch, seed=4, density=density, grey=True)
    A = TangoEncoder(None, config=cfg, init_seed=0)
    C = TangoEncoder(None, config=cfg, init_seed=5)
    try:
        _fit(A, exact)
        A.get_predictions(exact[0])
        assert _fit(A, grey)[2] in (None, 1)
        A.get_predictions(grey[0])
        assert _fit(A, exact)[2] in (None, 0)
        assert A.engine.get_step() == (3, 3) and A.engine.get_rng() == (3, 2)
        sd = A.state_dict()
        C.load_state_dict(sd)
        for i, b in enumerate((grey, exact, exact)):
            la, da, fa = _fit(A, b)
            lc, dc, fc = _fit(C, b)
            assert np.isfinite(la).all()
            assert la.tobytes() == lc.tobytes(), (case, "losses, step", i, la, lc)
            assert da.tobytes() == dc.tobytes(), (case, "distances, step", i)
            assert fa == fc and fa == (None if case == "f32" else int(b is grey)), (case, "dyn flag", i, fa, fc)
        sa, sc = A.state_dict(), C.state_dict()
        assert set(sa) == set(sc)
        for k in sa:
            if k not in ("step", "rng"):
                assert torch.equal(sa[k].contiguous().view(torch.int32), sc[k].contiguous().view(torch.int32)), (case, k)
        assert A.engine.get_step() == C.engine.get_step() == (6, 6)
        assert A.engine.get_rng() == C.engine.get_rng() == (6, 2)
    finally:
        A.close()
        C.close()
