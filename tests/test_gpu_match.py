"""``mvae_match``: the model's distance between every lock and every key embedding with a fused
top-k. Scores against a float64 reference under the fp32 summation bound, the top-k lists judged
on the GPU's own scores, fused against stored, independence from the split of M, consistency with
``get_predictions``, and the Python surface (``TangoEncoder.embed`` / ``match``, ``retrieve``, the
driver's ``--retrieve`` report)."""
import os

import numpy as np
import pytest
import torch

from magic_amd.config import MVAEConfig, preset
from tests.gpu_helpers import make_params, to_dev

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap_micro.npz")
U = 2.0 ** -24
METRICS = [("cosine", False), ("cosine", True), ("sqdiff", False), ("sqdiff", True)]
# (N, M) per L: every N and M of the issue's lists appears with every metric
SHAPES = {2: [(1, 1), (63, 64), (130, 1000)],
          20: [(65, 257), (130, 64), (1, 1000)],
          200: [(63, 257), (65, 1)],
          2000: [(130, 257), (1, 64)]}
CASES = [(m, r, L, N, M) for m, r in METRICS for L, nm in SHAPES.items() for N, M in nm]  # 40


@pytest.fixture(scope="module")
def engines():
    """One small engine per (metric, reciprocal, L): match reads only those of the context."""
    from magic_amd.engine import Engine
    made = {}

    def get(metric, recip, L):
        key = (metric, recip, L)
        if key not in made:
            made[key] = Engine(MVAEConfig(image_size=8, batch=64, enc=(40,), dec=(28, 20), latent=L, metric=metric,
                                          reciprocal=recip, precision="f32"), 0)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def galleries(N, M, L, seed=0):
    """seeded normal draws; key 0 repeats lock 0 (sqdiff raw = 0) where there is more than one key"""
    rng = np.random.default_rng(seed + 7 * N + 11 * M + L)
    zl = rng.standard_normal((N, L)).astype(np.float32)
    zk = rng.standard_normal((M, L)).astype(np.float32)
    if M > 1:
        zk[0] = zl[0]
    return zl, zk


def reference(zl, zk, metric):
    """float64 raw [N, M] and the sum of the absolute terms"""
    a, b = zl.astype(np.float64), zk.astype(np.float64)
    if metric == "cosine":
        a = a / np.sqrt(np.maximum((a * a).sum(0), 1e-12))
        b = b / np.sqrt(np.maximum((b * b).sum(0), 1e-12))
        return a @ b.T, np.abs(a) @ np.abs(b).T
    raw = np.zeros((len(a), len(b)))
    for l0 in range(0, a.shape[1], 100):  # (chunks of l: bounded temporaries)
        d = a[:, None, l0:l0 + 100] - b[None, :, l0:l0 + 100]
        raw += (d * d).sum(-1)
    return raw, raw.copy()


def check_scores(dist, raw, mag, L, recip, factor=1.0):
    """|raw_gpu - raw| <= 2 (L + 4) 2^-24 sum|terms| per entry; a reciprocal output is checked as
    1 / dist_gpu with 4 2^-24 |raw| more"""
    d = dist.astype(np.float64)
    bound = factor * 2 * (L + 4) * U * mag
    if recip:
        with np.errstate(divide="ignore"):
            d = 1.0 / d
        bound = bound + factor * 4 * U * np.abs(raw)
    err = np.abs(d - raw)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    assert (err <= bound).all(), f"worst error / bound = {worst:.3f}"
    return worst


def ranking(scores, k, order):
    """The first k of each row in the total order: by score (order +1 largest first), then by
    smaller j; NaN last. Judged on the scores given (the GPU's own)."""
    out = np.empty((scores.shape[0], k), np.int64)
    j = np.arange(scores.shape[1])
    for i, s in enumerate(scores):
        nan = np.isnan(s)
        key = np.where(nan, 0.0, -s.astype(np.float64) if order > 0 else s.astype(np.float64))
        out[i] = np.lexsort((j, key, nan))[:k]
    return out


def check_topk(val, ind, dist, k, order):
    ind = ind.astype(np.int64)
    assert ind.shape == val.shape == (dist.shape[0], k)
    assert (ind >= 0).all() and (ind < dist.shape[1]).all()
    assert all(len(set(r)) == k for r in ind.tolist())
    np.testing.assert_array_equal(val.view(np.int32), np.take_along_axis(dist, ind, 1).view(np.int32))
    # ordered by (score, smaller j) with no unselected j ahead of the last selected: the list is the
    # head of the total order
    np.testing.assert_array_equal(ind, ranking(dist, k, order))


def run_match(eng, zl, zk, k, order, dist):
    out = eng.match(to_dev(zl), to_dev(zk), k, order=order, dist=dist)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


# ------------------------------------------------------------------ 8. / 9. / 10. scores and top-k
@pytest.mark.parametrize("metric,recip,L,N,M", CASES,
                         ids=[f"{m}{'_recip' if r else ''}-L{L}-N{N}-M{M}" for m, r, L, N, M in CASES])
def test_scores_and_topk(engines, metric, recip, L, N, M):
    eng = engines(metric, recip, L)
    zl, zk = galleries(N, M, L)
    raw, mag = reference(zl, zk, metric)
    dist = None
    for k in sorted({1, min(10, M), min(M, 64)}):
        for order in (1, -1):
            val, ind, d = run_match(eng, zl, zk, k, order, True)
            if dist is None:
                dist = d
                worst = check_scores(dist, raw, mag, L, recip)
                print(f"worst error / bound {worst:.3f}")
                if metric == "sqdiff" and M > 1:
                    assert dist[0, 0] == (np.inf if recip else 0.0)
            np.testing.assert_array_equal(d.view(np.int32), dist.view(np.int32))
            check_topk(val, ind, dist, k, order)
            # fused: the same lists without the matrix
            val2, ind2 = run_match(eng, zl, zk, k, order, False)
            np.testing.assert_array_equal(val2.view(np.int32), val.view(np.int32))
            np.testing.assert_array_equal(ind2, ind)


@pytest.mark.parametrize("metric", ["cosine", "sqdiff"])
def test_equal_scores_and_nan(engines, metric):
    """Every score equal: 0 .. k - 1. A NaN row of zk sorts last for either order. (Under the
    cosine metric the NaN column sums are clamped by max(., 1e-12), as in the step's metric kernel:
    the norms stay numbers and only the NaN row's scores are NaN.)"""
    eng = engines(metric, False, 20)
    zl = np.tile(np.linspace(-1, 1, 20, dtype=np.float32), (5, 1))
    zk = np.tile(np.linspace(1, 2, 20, dtype=np.float32), (70, 1))
    for order in (1, -1):
        val, ind, dist = run_match(eng, zl, zk, 64, order, True)
        assert (dist == dist[0, 0]).all()
        np.testing.assert_array_equal(ind, np.tile(np.arange(64), (5, 1)))
    zl, zk = galleries(5, 70, 20, seed=3)
    zk[3] = np.nan
    for order in (1, -1):
        for k in (10, 64):
            val, ind, dist = run_match(eng, zl, zk, k, order, True)
            assert np.isnan(dist[:, 3]).all()
            assert np.isfinite(np.delete(dist, 3, axis=1)).all()
            check_topk(val, ind, dist, k, order)
            assert not (ind == 3).any()
        val, ind, dist = run_match(eng, zl, zk[:64], 64, order, True)
        check_topk(val, ind, dist, 64, order)
        assert (ind[:, -1] == 3).all()


def launcher_splits(N, M):
    """match_plan's rule (match.hip): workgroups for four per CU, no split under four key tiles"""
    ntn = -(-N // 64)
    s = max(1, min(-(-1024 // ntn), -(-M // 256)))
    length = -(-(-(-M // s)) // 64) * 64
    return -(-M // length)


@pytest.mark.parametrize("metric,recip", [("cosine", False), ("sqdiff", True)])
def test_many_splits(engines, metric, recip):
    """N = 4 against M = 40000 runs 157 splits of M and the merge: the lists are the head of the
    total order over the stored scores -- what one split would return -- and the fused call returns
    the same bits."""
    N, M, L = 4, 40000, 20
    assert launcher_splits(N, M) > 100 and launcher_splits(130, 1000) > 1 and launcher_splits(63, 64) == 1
    eng = engines(metric, recip, L)
    zl, zk = galleries(N, M, L)
    zk[M - 1] = zl[1]  # the best key of lock 1 is the last one, in the last (short) split
    for k, order in ((10, 1), (64, -1), (64, 1)):
        val, ind, dist = run_match(eng, zl, zk, k, order, True)
        check_topk(val, ind, dist, k, order)
        val2, ind2 = run_match(eng, zl, zk, k, order, False)
        np.testing.assert_array_equal(val2.view(np.int32), val.view(np.int32))
        np.testing.assert_array_equal(ind2, ind)
    if metric == "sqdiff":
        assert ind[1, 0] == M - 1  # (order +1 on 1 / raw: raw = 0 first)


def test_match_validation(engines):
    eng = engines("sqdiff", False, 20)
    zl, zk = (to_dev(a) for a in galleries(4, 8, 20))
    val = torch.zeros(4, 8, device="cuda")
    ind = torch.zeros(4, 8, dtype=torch.int32, device="cuda")
    for kw in (dict(k=0), dict(k=9), dict(order=0), dict(N=0), dict(M=0)):
        a = dict(N=4, M=8, k=8, order=1)
        a.update(kw)
        rc = eng.lib.mvae_match(eng.ctx, zl.data_ptr(), a["N"], zk.data_ptr(), a["M"], a["k"], a["order"], None,
                                val.data_ptr(), ind.data_ptr(), eng.stream)
        assert rc == -1 and eng.lib.mvae_last_error(eng.ctx).decode().startswith("mvae_match:"), kw
    with pytest.raises(ValueError):
        eng.match(zl, zk, 65)
    with pytest.raises(ValueError):
        eng.match(zl[:, :5].contiguous(), zk, 1)


# ------------------------------------------------------------------ 11. the existing distance
FLAVOURS = [("tanh", "cosine", False), ("tanh", "cosine", True), ("elu", "sqdiff", True),
            ("tanh", "sqdiff", False), ("elu", "cosine", False)]


@pytest.mark.parametrize("act,metric,recip", FLAVOURS)
def test_diagonal_equals_get_predictions(act, metric, recip):
    """diag(match) of embed(locks), embed(keys) against get_predictions(X, eps = 0) on the
    materialised batch (z = mu): N = M = B = 64, twice the score bound."""
    from magic_amd.engine import Engine
    from magic_amd.overlap_input import PairBatch, rotation_coefficients
    B, S, L = 64, 8, 6
    cfg = MVAEConfig(image_size=S, batch=B, enc=(40, 36, 24), dec=(28, 20), latent=L, act=act, metric=metric,
                     reciprocal=recip, precision="f32x")
    rng = np.random.default_rng(4)
    locks = ((rng.random((B, S, S)) < 0.4) * 255).astype(np.uint8)
    keys = ((rng.random((B, S, S)) < 0.4) * 255).astype(np.uint8)
    eng = Engine(cfg, 0)
    try:
        eng.load_params(make_params(cfg))
        coef = rotation_coefficients(np.zeros(B, np.float32), S, S)
        pb = PairBatch(to_dev(locks), to_dev(keys), to_dev(np.arange(B, dtype=np.int32)), to_dev(coef))
        pred = eng.predict(pb.materialize(), torch.zeros(3, B, L, device="cuda")).cpu().numpy()
        zl, zk = eng.embed(to_dev(locks)).clone(), eng.embed(to_dev(keys)).clone()
        _, _, dist = eng.match(zl, zk, 1, dist=True)
        torch.cuda.synchronize()
        raw, mag = reference(zl.cpu().numpy(), zk.cpu().numpy(), metric)
        diag = np.arange(B)
        got = dist.cpu().numpy()[diag, diag]
        r, m = raw[diag, diag], mag[diag, diag]
        # the comparison itself, in raw form (1 / x for a reciprocal flavour): the two GPU values
        # against each other at twice the score bound, its magnitudes from the float64 reference
        bound = 2.0 * (2 * (L + 4) * U * m + (4 * U * np.abs(r) if recip else 0.0))
        with np.errstate(divide="ignore"):
            g, p = ((1.0 / v.astype(np.float64)) if recip else v.astype(np.float64) for v in (got, pred))
        err = np.abs(g - p)
        print(f"diag(match) vs get_predictions: worst |difference| / (2 bound) {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), float((err / bound).max())
        # extras: each against the float64 distance of the embeddings
        check_scores(got, r, m, L, recip)
        check_scores(pred, r, m, L, recip, factor=2.0)
    finally:
        eng.close()


# ------------------------------------------------------------------ 12. Python surface
def micro_tables(n=32):
    z = np.load(GOLD)
    w = int(z["shape"][2])
    unpack = lambda a: (np.unpackbits(a[:n], axis=-1)[..., :w] * 255).astype(np.uint8)  # noqa: E731
    return unpack(z["lock_bits"]), unpack(z["key_bits"])


def test_python_surface_and_retrieve():
    from magic_amd import retrieval
    from magic_amd.vae import TangoEncoder
    locks, keys = micro_tables(32)
    S = locks.shape[1]
    cfg = preset("11a", image_size=S, batch=64, precision="bf16")
    vae = TangoEncoder(None, config=cfg, init_seed=5)
    try:
        z = vae.embed(locks)
        assert isinstance(z, np.ndarray) and z.shape == (32, cfg.latent) and z.dtype == np.float32
        zi = vae.embed(locks, idx=[3, 3, 0, 31])
        np.testing.assert_array_equal(zi, z[[3, 3, 0, 31]])
        with pytest.raises(ValueError):
            vae.embed(locks, idx=[32])
        with pytest.raises(ValueError):  # a float table is refused, not cast to 0 / 1
            vae.embed(locks.astype(np.float32) / 255)
        with pytest.raises(ValueError):
            vae.embed(torch.from_numpy(locks).float())
        val, ind = vae.match(z, vae.embed(keys), k=3)
        assert val.shape == ind.shape == (32, 3) and val.dtype == np.float32 and ind.dtype == np.int32
        val, ind, dist = vae.match(z[:5], z, k=2, order=-1, return_dist=True)
        assert dist.shape == (5, 32) and dist.dtype == np.float32
        r, dist = retrieval.retrieve(vae, locks, keys, k=32, return_dist=True)
        assert r.k == 32 and r.hit_at_k == 1.0 and 0.0 <= r.hit_at_1 <= 1.0
        assert r.hit_at_1 == float((r.indices[:, 0] == np.arange(32)).mean())
        np.testing.assert_array_equal(r.indices, ranking(dist, 32, 1))
        np.testing.assert_array_equal(r.values, np.take_along_axis(dist, r.indices.astype(np.int64), 1))
        assert "hit@32 = 1.0000" in retrieval.report(r)
    finally:
        vae.close()


def test_driver_retrieve_report():
    """main.train followed by the --retrieve report on the micro archive."""
    from magic_amd import main
    from magic_amd.overlap_input import inputs
    from magic_amd.vae import TangoEncoder
    cfg = preset("11a", image_size=200, batch=64, precision="bf16")
    vae = TangoEncoder(None, config=cfg)
    try:
        s = inputs(normalize=True, reshape=True, rotation=True, batch_size=64, image_size=200, data_dir=GOLD, seed=3,
                   fused=True)
        main.train(vae, s, 2 * 64, 1, driver="11a", eval_at=lambda epoch, i: False, log=lambda m: None)
        lines = []
        r = main.retrieve_report(vae, s, 10, log=lines.append)
        n = len(s.locks)
        assert r.indices.shape == (n, 10) and not np.isnan(r.values).any()
        assert len(lines) == 1 and "hit@1 = " in lines[0] and "hit@10 = " in lines[0]
        assert 0.0 <= r.hit_at_1 <= r.hit_at_k <= 1.0
    finally:
        vae.close()
