"""tests/head_ref.py (the float64 restatement the latent head's kernels are held to) checked
independently of the kernels: its four dhead row blocks against float64 torch autograd of the cost
and of training_loss as functions of ms (l2_normalize's maximum as clamp_min, whose gradient is the
tf.maximum routing; columns below L2_EPS included), and its distance / losses / column statistics
against oracle/mvae_oracle.py on a tiny configuration. Agreement to 1e-12 of each value's mag."""
import numpy as np
import pytest
import torch

from oracle import mvae_oracle as O
from tests import head_ref as H

REL = 1e-12


def _inputs(B, L, seed, dead=False):
    rng = np.random.default_rng(seed)
    ms = rng.standard_normal((3, B, 2 * L))
    ms[:, :, L:] = rng.uniform(-8, 4, (3, B, L))
    eps = rng.standard_normal((3, B, L))          # slots (lock, rot, key)
    if dead and L >= 4:
        # lock column 0 exactly zero, lock column 1 and key column 2 below L2_EPS, key column 3 zero
        for blk, slot, col, v in ((1, 0, 0, 0.0), (1, 0, 1, 1e-7), (2, 2, 2, 1e-7), (2, 2, 3, 0.0)):
            ms[blk, :, col] = v * rng.choice([-1.0, 1.0], B)
            eps[slot, :, col] = 0.0
    dzdec = rng.standard_normal((B, L)) / B
    areas = rng.uniform(-1, 1, B)
    return ms.reshape(3 * B, 2 * L), eps, dzdec, areas


def _chain(ms, eps, dzdec, areas, B, L, metric, recip, w, Bg):
    f = H.latent_fwd(ms, eps, B, L)
    zl, zk = f["z"][1], f["z"][2]
    cs = H.colsq(zl, zk)["out"]
    m = H.metric(zl, zk, f["rowfwd"], np.zeros((B, 1)), areas, cs, metric, recip, w, Bg)
    cd = H.coldot(zl, zk, cs, m["draw"])["out"] if metric == 0 else None
    b = H.latent_bwd(ms, eps, dzdec, m["draw"], cs, cd, B, L, metric, w, Bg)
    return f, cs, m, cd, b


def _autograd(ms, eps, dzdec, areas, B, L, metric, recip, w, Bg):
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    msr = t(ms).reshape(3, B, 2 * L).clone().requires_grad_(True)
    e = t(eps)[list(H.EPS_SLOT)]
    mu, s = msr[:, :, :L], msr[:, :, L:]
    z = mu + torch.sqrt(torch.exp(s)) * e
    zr, zl, zk = z[0], z[1], z[2]
    K = -0.5 * torch.sum(1 + s[1] - mu[1] ** 2 - torch.exp(s[1]), 1)
    F = w * torch.sum((zl - zr) ** 2, 1)
    cost = torch.sum(t(dzdec) * zl) + torch.sum(K + F) / Bg
    if metric == 0:
        na = zl * torch.rsqrt(torch.clamp_min(torch.sum(zl ** 2, 0, keepdim=True), H.L2_EPS))
        nb = zk * torch.rsqrt(torch.clamp_min(torch.sum(zk ** 2, 0, keepdim=True), H.L2_EPS))
        raw = torch.sum(na * nb, 1)
    else:
        raw = torch.sum((zl - zk) ** 2, 1)
    dist = 1.0 / raw if recip else raw
    T = torch.sum((dist - t(areas)) ** 2) / Bg
    g1, = torch.autograd.grad(cost, msr, retain_graph=True)
    g2, = torch.autograd.grad(T, msr)
    g1, g2 = g1.numpy(), g2.numpy()
    assert not g1[2].any() and not g2[0].any()     # the cost never sees the key, the metric never the rot
    return np.stack([g1[0], g1[1], g2[1], g2[2]]), dist.detach().numpy()


@pytest.mark.parametrize("metric,recip,w,Bgf,dead", [
    (0, 0, 10.0, 1, False), (0, 1, 10.0, 1, False), (0, 0, 100.0, 1, True), (0, 1, 10.0, 1, True),
    (1, 0, 10.0, 1, False), (1, 1, 100.0, 4, False), (1, 0, 10.0, 4, True),
])
@pytest.mark.parametrize("B,L", [(5, 6), (1, 4), (9, 1)])
def test_dhead_equals_autograd(metric, recip, w, Bgf, dead, B, L):
    Bg = B * Bgf      # (the cosine's column statistics are over the batch: its cases keep Bg = B)
    dead = dead and B >= 5   # (one row: the two live terms of raw are +-0.1 and may cancel to a 0 distance)
    ms, eps, dzdec, areas = _inputs(B, L, 11 + B + L, dead)
    f, cs, m, cd, b = _chain(ms, eps, dzdec, areas, B, L, metric, recip, w, Bg)
    if dead and L >= 4 and metric == 0:
        assert (cs < H.L2_EPS).sum() == 4 and (cs == 0).sum() == 2
    want, dist = _autograd(ms, eps, dzdec, areas, B, L, metric, recip, w, Bg)
    assert np.all(np.abs(m["dist"] - dist) <= REL * m["dist_mag"])
    err = np.abs(b["dhead"] - want)
    assert np.all(err <= REL * b["mag"]), float((err / np.maximum(b["mag"], 1e-300)).max())
    assert np.all(np.abs(b["dhead"]) <= b["mag"] * (1 + 1e-9))   # a mag bounds its value


@pytest.mark.parametrize("metric,recip", [("cosine", False), ("cosine", True), ("sqdiff", False), ("sqdiff", True)])
def test_forward_metric_losses_equal_oracle(metric, recip):
    cfg = O.OracleConfig(image_size=6, enc=(16, 12), dec=(10, 14), latent=4, act="tanh", deform_weight=10.0,
                         metric=metric, reciprocal=recip)
    B, L, Bg = 7, 4, 7
    rng = np.random.default_rng(3)
    P = O.init_params(cfg, seed=0, dtype=np.float64)
    X = (rng.random((B, 3 * cfg.D)) < 0.3).astype(np.float64)
    areas = rng.uniform(0.1, 2.0, B)
    eps = rng.standard_normal((3, B, L))
    c = O.forward(P, X, eps, cfg)
    O.metric(c, areas, cfg, Bg)
    ms = np.concatenate([np.concatenate([c[f"mu_{t}"], c[f"s_{t}"]], 1) for t in "rlk"])
    m_id = 0 if metric == "cosine" else 1
    f = H.latent_fwd(ms, eps, B, L)
    close = lambda a, b, mag: np.all(np.abs(a - b) <= REL * mag)
    for blk, t in enumerate("rlk"):
        assert close(f["z"][blk], c[f"z_{t}"], f["z_mag"][blk])
    assert close(-0.5 * f["rowfwd"][:, 0], c["K"], f["rowfwd_mag"][:, 0])
    assert close(cfg.deform_weight * f["rowfwd"][:, 1], c["F"], cfg.deform_weight * f["rowfwd_mag"][:, 1])
    cs = H.colsq(c["z_l"], c["z_k"])
    assert close(cs["out"], c["colsq"].reshape(-1), cs["mag"])
    assert close(cs["part"].sum(0), cs["out"], cs["mag"])
    m = H.metric(c["z_l"], c["z_k"], f["rowfwd"], c["R"][:, None], areas, cs["out"], m_id, recip,
                 cfg.deform_weight, Bg)
    assert close(m["dist"], c["dist"], m["dist_mag"])
    assert close(m["draw"], c["draw"], m["draw_mag"])
    assert close(m["rowvals"], np.stack([c["R"], c["K"], c["F"], c["T"]], 1), m["rowvals_mag"])
    if metric == "cosine":
        cd = H.coldot(c["z_l"], c["z_k"], cs["out"], m["draw"])
        assert close(cd["out"], c["coldot"], cd["mag"])
    lr = H.loss_reduce(m["rowvals"], Bg)
    assert close(lr["losses"], O.loss_sums(c, Bg), lr["mag"])


def test_planes_split_is_exact():
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 6, 4096)).astype(np.float32)
    p = H.planes(a, 3)
    val = lambda b: (b.astype(np.uint32) << 16).view(np.float32)
    assert np.array_equal(p[0], torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal((val(p[0]).astype(np.float64) + val(p[1]) + val(p[2])).astype(np.float32), a)
