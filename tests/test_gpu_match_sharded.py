"""Retrieval at gallery scale: ``mvae_match_ex`` over the shards of a gallery against one
``mvae_match`` over all of it (bit for bit: lists, stored scores, any shard order, lists merged
apart), the exposed column norms against the internal ones, scores that do not depend on the other
queries of a call, ``mvae_pair_scores`` against the stored matrix, the fused count of keys before
a threshold against the full ordering of the GPU's own scores, validation, and the Python surface
(``retrieve(shard=, ranks=)``, the driver's ``--retrieve-shard`` / ``--retrieve-ranks``)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from magic_amd import _lib
from magic_amd.config import MVAEConfig, preset
from tests.gpu_helpers import to_dev
from tests.test_gpu_match import galleries, launcher_splits, micro_tables, ranking

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap_micro.npz")
METRICS = [("cosine", False), ("cosine", True), ("sqdiff", False), ("sqdiff", True)]
MID = [f"{m}{'_recip' if r else ''}" for m, r in METRICS]
SHARDS = (257, 64, 1, 678)  # of M = 1000: across the 64-row and 128-key units, one smaller than k
EMPTY = 0x7FC00000


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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same(a, b):
    np.testing.assert_array_equal(bits(a), bits(b))


def host(*ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def bases(shards):
    return np.concatenate([[0], np.cumsum(shards)[:-1]]).tolist()


def norms(eng, metric, zl, zk):
    """the reciprocal column norms of the whole galleries through the exposed pair (None for sqdiff)"""
    if metric != "cosine":
        return None, None
    return eng.match_rnorm(eng.match_colsq(zl)), eng.match_rnorm(eng.match_colsq(zk))


def sweep(eng, zl, zk, k, order, rl, rk, parts, dist=None, target=None):
    """parts: (key_base, rows) in the order fed; the lists carried from part to part"""
    val = ind = ahead = None
    for n, (b, m) in enumerate(parts):
        out = eng.match(zl, zk[b:b + m], k, order=order, rl=rl, rk=rk, key_base=b,
                        carry=None if n == 0 else (val, ind), target=target, ahead=ahead,
                        dist_out=None if dist is None else dist[:, b:b + m])
        val, ind = out[0], out[1]
        if target is not None:
            ahead = out[-1]
    return val, ind, ahead


# ------------------------------------------------------------------ 1. sharded equals one-shot
@pytest.mark.parametrize("L,N", [(2, 1), (20, 65), (200, 130), (2000, 65)])
@pytest.mark.parametrize("metric,recip", METRICS, ids=MID)
def test_sharded_equals_one_shot(engines, metric, recip, L, N):
    M = 1000
    eng = engines(metric, recip, L)
    zl, zk = (to_dev(a) for a in galleries(N, M, L))
    rl, rk = norms(eng, metric, zl, zk)
    parts = list(zip(bases(SHARDS), SHARDS))
    assert sum(SHARDS) == M
    for k in (1, 10, 64):
        for order in (1, -1):
            val, ind, dist = host(*eng.match(zl, zk, k, order=order, dist=True))  # mvae_match
            # carried, with the matrix written into the column blocks of one buffer
            d = torch.full((N, M), float("nan"), device="cuda")
            v, i, _ = sweep(eng, zl, zk, k, order, rl, rk, parts, dist=d)
            v, i, d = host(v, i, d)
            same(v, val), same(i, ind), same(d, dist)
            # the same shards in reverse order, no matrix
            v, i = host(*sweep(eng, zl, zk, k, order, rl, rk, parts[::-1])[:2])
            same(v, val), same(i, ind)
            # matched apart, then merged
            sep = [eng.match(zl, zk[b:b + m], k, order=order, rl=rl, rk=rk, key_base=b) for b, m in parts]
            sv = torch.stack([s[0] for s in sep], 1).contiguous()
            si = torch.stack([s[1] for s in sep], 1).contiguous()
            one = host(sep[2][0], sep[2][1])  # the one-key shard: one entry, then empty ones
            assert (one[1][:, 0] == parts[2][0]).all()
            if k > 1:
                assert (one[1][:, 1:] == -1).all() and (bits(one[0][:, 1:]) == EMPTY).all()
            v, i = host(*eng.match_merge(sv, si, order=order))
            same(v, val), same(i, ind)


# ------------------------------------------------------------------ 2. many splits under carry
@pytest.mark.parametrize("metric,recip", [("cosine", False), ("sqdiff", True)])
def test_many_splits_under_carry(engines, metric, recip):
    N, M, L, k = 4, 40000, 20, 64
    assert launcher_splits(N, M // 2) > 50
    eng = engines(metric, recip, L)
    a, b = galleries(N, M, L)
    b[M - 1] = a[1]
    zl, zk = to_dev(a), to_dev(b)
    rl, rk = norms(eng, metric, zl, zk)
    for order in (1, -1):
        val, ind = host(*eng.match(zl, zk, k, order=order))
        for parts in ([(0, M // 2), (M // 2, M // 2)], [(M // 2, M // 2), (0, M // 2)]):
            v, i = host(*sweep(eng, zl, zk, k, order, rl, rk, parts)[:2])
            same(v, val), same(i, ind)


# ------------------------------------------------------------------ 3. norms
@pytest.mark.parametrize("L", [2, 200])
def test_norms(engines, L):
    n = 845
    eng = engines("cosine", False, L)
    zl, zk = (to_dev(a) for a in galleries(n, n, L, seed=5))
    whole = eng.match_colsq(zk)
    acc = eng.match_colsq(zk[:512])
    eng.match_colsq(zk[512:768], out=acc, accumulate=True)
    eng.match_colsq(zk[768:], out=acc, accumulate=True)
    w, a = host(whole, acc)
    assert w.dtype == np.float64 and (w > 0).all()
    same(a, w)
    ref = (zk.cpu().numpy().astype(np.float64) ** 2).sum(0)
    assert (np.abs(w - ref) <= 2 * (n - 1) * 2.0 ** -53 * ref).all()
    # the exposed norms are the internal ones: the same cosine matrix
    rl, rk = eng.match_rnorm(eng.match_colsq(zl)), eng.match_rnorm(whole)
    _, _, dist = host(*eng.match(zl, zk, 10, dist=True))
    _, _, d = host(*eng.match(zl, zk, 10, rl=rl, rk=rk, dist=True))
    same(d, dist)
    # shards off the 256-row chunks: fp64 rounding only
    acc = eng.match_colsq(zk[:100])
    eng.match_colsq(zk[100:400], out=acc, accumulate=True)
    eng.match_colsq(zk[400:], out=acc, accumulate=True)
    a, r0, r1 = host(acc, rk, eng.match_rnorm(acc))
    rel = np.abs(a - w) / w
    print(f"colsq, other shards: worst relative difference {rel.max():.3e} (bound {2 * (n - 1) * 2.0 ** -53:.3e})")
    assert (rel <= 2 * (n - 1) * 2.0 ** -53).all()
    assert (np.abs(r1.astype(np.float64) - r0) <= np.spacing(r0)).all()


# ------------------------------------------------------------------ 4. query independence
@pytest.mark.parametrize("recip", [False, True])
def test_query_independence(engines, recip):
    N, M, L, k = 130, 257, 20, 10
    eng = engines("cosine", recip, L)
    zl, zk = (to_dev(a) for a in galleries(N, M, L))
    rl, rk = norms(eng, "cosine", zl, zk)
    val, ind, dist = host(*eng.match(zl, zk, k, rl=rl, rk=rk, dist=True))
    same(dist, host(eng.match(zl, zk, k, dist=True)[2])[0])
    for a, b in ((0, 1), (1, 64), (64, 130)):
        v, i, d = host(*eng.match(zl[a:b], zk, k, rl=rl, rk=rk, dist=True))
        same(v, val[a:b]), same(i, ind[a:b]), same(d, dist[a:b])
        # no norms given: those of the rows passed, as mvae_match on the chunk (today's behaviour)
        want = host(*eng.match(zl[a:b], zk, k, dist=True))
        got = host(*eng.match(zl[a:b], zk, k, dist_out=torch.empty(b - a, M, device="cuda")))  # both NULL
        for g, w in zip(got, want):
            same(g, w)
        v = torch.empty(b - a, k, device="cuda")
        i = torch.empty(b - a, k, device="cuda", dtype=torch.int32)
        d = torch.empty(b - a, M, device="cuda")
        rc = eng.lib.mvae_match_ex(eng.ctx, zl[a:b].data_ptr(), b - a, zk.data_ptr(), M, k, 1, None, d.data_ptr(),
                                   v.data_ptr(), i.data_ptr(), eng.stream)  # opts NULL
        assert rc == 0
        for g, w in zip(host(v, i, d), want):
            same(g, w)
    if not recip:  # a single query normalised by itself is +-1 per column: not the gallery's score
        assert not np.array_equal(host(eng.match(zl[:1], zk, k, dist=True)[2])[0], dist[:1])


# ------------------------------------------------------------------ 5. pair scores
@pytest.mark.parametrize("L", [2, 20, 200, 2000])
@pytest.mark.parametrize("metric,recip", METRICS, ids=MID)
def test_pair_scores(engines, metric, recip, L):
    M = 130
    eng = engines(metric, recip, L)
    for n in (1, 65, 300):
        a, b = galleries(n, M, L, seed=2)
        zl, zk = to_dev(a), to_dev(b)
        t = np.random.default_rng(n + L).integers(0, M, n)
        t[0] = 0  # (zk[0] = zl[0]: a zero raw distance, an infinite reciprocal)
        zkt = zk[to_dev(t)].contiguous()
        rl, rk = norms(eng, metric, zl, zk)
        dist = host(eng.match(zl, zk, 1, rl=rl, rk=rk, dist_out=torch.empty(n, M, device="cuda"))[2])[0]
        same(host(eng.pair_scores(zl, zkt, rl, rk))[0], dist[np.arange(n), t])
        # no norms given: over the n rows passed, the diagonal of mvae_match on them
        diag = host(eng.match(zl, zkt, 1, dist=True)[2])[0][np.arange(n), np.arange(n)]
        same(host(eng.pair_scores(zl, zkt))[0], diag)


# ------------------------------------------------------------------ 6. ranks
def positions(dist, t, order):
    """the place of key t[i] in row i's total order over the scores given"""
    full = ranking(dist, dist.shape[1], order)
    return np.array([int(np.nonzero(full[i] == t[i])[0][0]) for i in range(len(t))])


@pytest.mark.parametrize("metric,recip", [("cosine", False), ("sqdiff", True)])
def test_ranks(engines, metric, recip):
    N, M, L, k = 65, 1000, 20, 10
    eng = engines(metric, recip, L)
    zl, zk = (to_dev(a) for a in galleries(N, M, L))
    rl, rk = norms(eng, metric, zl, zk)
    t = np.random.default_rng(1).integers(0, M, N).astype(np.int32)
    t[0] = 0
    tv, ti = eng.pair_scores(zl, zk[to_dev(t.astype(np.int64))].contiguous(), rl, rk), to_dev(t)
    parts = list(zip(bases(SHARDS), SHARDS))
    for order in (1, -1):
        val, ind, dist, ahead = host(*eng.match(zl, zk, k, order=order, rl=rl, rk=rk, dist=True, target=(tv, ti)))
        same(host(tv)[0], dist[np.arange(N), t])
        want = positions(dist, t, order)
        np.testing.assert_array_equal(ahead, want)
        top = ahead < k
        assert (ind[top, ahead[top]] == t[top]).all()
        for p in (parts, parts[::-1]):
            v, i, a = host(*sweep(eng, zl, zk, k, order, rl, rk, p, target=(tv, ti)))
            np.testing.assert_array_equal(a, want)
            same(v, val), same(i, ind)


def test_ranks_many_splits(engines):
    """the per-split counts through the workspace, added by the merge launch"""
    N, M, L = 4, 40000, 20
    eng = engines("sqdiff", True, L)
    zl, zk = (to_dev(a) for a in galleries(N, M, L))
    t = np.array([0, 39999, 20000, 777], np.int32)
    tv, ti = eng.pair_scores(zl, zk[to_dev(t.astype(np.int64))].contiguous()), to_dev(t)
    for order in (1, -1):
        _, _, dist, ahead = host(*eng.match(zl, zk, 64, order=order, dist=True, target=(tv, ti)))
        np.testing.assert_array_equal(ahead, positions(dist, t, order))
        a = sweep(eng, zl, zk, 64, order, None, None, [(M // 2, M // 2), (0, M // 2)], target=(tv, ti))[2]
        np.testing.assert_array_equal(host(a)[0], ahead)


@pytest.mark.parametrize("metric", ["cosine", "sqdiff"])
def test_ranks_equal_scores_and_nan(engines, metric):
    eng = engines(metric, False, 20)
    zl = to_dev(np.tile(np.linspace(-1, 1, 20, dtype=np.float32), (5, 1)))
    zk = to_dev(np.tile(np.linspace(1, 2, 20, dtype=np.float32), (70, 1)))
    t = np.array([0, 69, 3, 64, 17], np.int32)
    tv = eng.pair_scores(zl, zk[:5].contiguous(), *norms(eng, metric, zl, zk))
    for order in (1, -1):
        out = eng.match(zl, zk, 10, order=order, dist=True, target=(tv, to_dev(t)))
        _, _, dist, ahead = host(*out)
        assert (dist == dist[0, 0]).all() and (host(tv)[0] == dist[0, 0]).all()
        np.testing.assert_array_equal(ahead, t)  # every score equal: the smaller indices are ahead
    a, b = galleries(5, 70, 20, seed=3)
    b[3] = np.nan
    b[40] = np.nan
    zl, zk = to_dev(a), to_dev(b)
    for order in (1, -1):
        _, _, dist = host(*eng.match(zl, zk, 10, order=order, dist=True))
        assert np.isnan(dist[:, [3, 40]]).all() and np.isfinite(np.delete(dist, [3, 40], axis=1)).all()
        for t in (np.array([0, 69, 5, 64, 17], np.int32), np.array([3, 40, 3, 40, 3], np.int32)):
            tv = to_dev(dist[np.arange(5), t])
            ahead = host(eng.match(zl, zk, 10, order=order, target=(tv, to_dev(t)))[2])[0]
            np.testing.assert_array_equal(ahead, positions(dist, t, order))
            if np.isnan(dist[0, t[0]]):  # a NaN target: the 68 finite keys, and the NaN keys before it
                np.testing.assert_array_equal(ahead, 68 + (t == 40))
            else:                        # a finite target: no NaN key is counted
                assert (ahead <= 67).all()


# ------------------------------------------------------------------ 7. validation
def test_validation(engines):
    eng = engines("sqdiff", False, 20)
    lib, M = eng.lib, 8
    zl, zk = (to_dev(a) for a in galleries(4, M, 20))
    val = torch.zeros(4, 8, device="cuda")
    ind = torch.zeros(4, 8, dtype=torch.int32, device="cuda")
    f = torch.zeros(16, device="cuda")
    i4 = torch.zeros(16, dtype=torch.int32, device="cuda")
    d8 = torch.zeros(20, dtype=torch.float64, device="cuda")

    def refused(rc, prefix):
        return rc == -1 and lib.mvae_last_error(eng.ctx).decode().startswith(prefix + ":")

    def ex(N=4, M=M, k=8, order=1, zl=zl.data_ptr(), top=val.data_ptr(), **kw):
        o = _lib.mvae_match_opts()
        for name, v in kw.items():
            setattr(o, name, v)
        return lib.mvae_match_ex(eng.ctx, zl, N, zk.data_ptr(), M, k, order, C.byref(o), None, top, ind.data_ptr(),
                                 eng.stream)

    top = 2 ** 31 - 1
    bad = [dict(key_base=-1), dict(key_base=top - M + 1), dict(key_base=top), dict(carry=2), dict(carry=-1),
           dict(dist_ld=M - 1), dict(dist_ld=-1), dict(thr_val=f.data_ptr()), dict(ahead=i4.data_ptr()),
           dict(thr_val=f.data_ptr(), thr_idx=i4.data_ptr()), dict(thr_idx=i4.data_ptr(), ahead=i4.data_ptr()),
           dict(k=0), dict(k=65), dict(order=0), dict(order=2), dict(N=0), dict(M=0), dict(zl=None), dict(top=None)]
    for kw in bad:
        assert refused(ex(**kw), "mvae_match_ex"), kw
    assert ex(key_base=top - M) == 0                     # the last index is 2^31 - 2
    torch.cuda.synchronize()
    assert (ind.cpu().numpy()[:, 0] >= top - M).all()
    assert ex(dist_ld=M, carry=1) == 0 and ex(dist_ld=0) == 0
    z = zl.data_ptr()
    assert refused(lib.mvae_match_colsq(eng.ctx, None, 4, d8.data_ptr(), 0, eng.stream), "mvae_match_colsq")
    assert refused(lib.mvae_match_colsq(eng.ctx, z, 4, None, 0, eng.stream), "mvae_match_colsq")
    assert refused(lib.mvae_match_colsq(eng.ctx, z, 0, d8.data_ptr(), 0, eng.stream), "mvae_match_colsq")
    assert refused(lib.mvae_match_colsq(eng.ctx, z, 4, d8.data_ptr(), 2, eng.stream), "mvae_match_colsq")
    assert refused(lib.mvae_match_rnorm(eng.ctx, None, f.data_ptr(), eng.stream), "mvae_match_rnorm")
    assert refused(lib.mvae_match_rnorm(eng.ctx, d8.data_ptr(), None, eng.stream), "mvae_match_rnorm")
    assert refused(lib.mvae_pair_scores(eng.ctx, z, None, 4, None, None, f.data_ptr(), eng.stream), "mvae_pair_scores")
    assert refused(lib.mvae_pair_scores(eng.ctx, z, z, 4, None, None, None, eng.stream), "mvae_pair_scores")
    assert refused(lib.mvae_pair_scores(eng.ctx, z, z, 0, None, None, f.data_ptr(), eng.stream), "mvae_pair_scores")
    mg = lambda **kw: lib.mvae_match_merge(  # noqa: E731
        eng.ctx, kw.get("vals", val.data_ptr()), ind.data_ptr(), kw.get("N", 4), kw.get("parts", 2), kw.get("k", 4),
        kw.get("order", 1), f.data_ptr(), i4.data_ptr(), eng.stream)
    for kw in (dict(vals=None), dict(N=0), dict(parts=0), dict(k=0), dict(k=65), dict(order=0)):
        assert refused(mg(**kw), "mvae_match_merge"), kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eng.match(zl, zk, 65, key_base=1)
    with pytest.raises(ValueError):
        eng.match(zl, zk, 9)  # (the plain call keeps k <= M)
    with pytest.raises(ValueError):
        eng.match(zl, zk, 4, ahead=i4[:4])


# ------------------------------------------------------------------ 8. Python surface
def host_ranks(dist, order):
    n = min(dist.shape)
    return positions(dist[:n], np.arange(n), order)


class Recorder:
    """a TangoEncoder seen through its embed calls"""

    def __init__(self, vae):
        self._vae, self.counts = vae, []

    def embed(self, table, *a, **kw):
        self.counts.append(len(table))
        return self._vae.embed(table, *a, **kw)

    def __getattr__(self, name):
        return getattr(self._vae, name)


def check_retrieve(vae, locks, keys, k, shard):
    from magic_amd import retrieval
    r0, dist = retrieval.retrieve(vae, locks, keys, k=k, return_dist=True)
    assert r0.ranks is None and r0.mrr is None and r0.median_rank is None
    line = retrieval.report(r0)
    assert line == (f"retrieval over {len(locks)} locks: hit@1 = {r0.hit_at_1:.4f}, hit@{r0.k} = {r0.hit_at_k:.4f} "
                    "(largest distance first)")
    rec = Recorder(vae)
    r1 = retrieval.retrieve(rec, locks, keys, k=k, shard=shard)
    assert rec.counts and max(rec.counts) <= shard and sum(rec.counts) == len(locks) + len(keys)
    same(r1.values, r0.values), same(r1.indices, r0.indices)
    assert (r1.hit_at_1, r1.hit_at_k, r1.k, r1.ranks) == (r0.hit_at_1, r0.hit_at_k, r0.k, None)
    assert retrieval.report(r1) == line
    for sh in (None, shard):
        r2, d2 = retrieval.retrieve(vae, locks, keys, k=k, shard=sh, ranks=True, return_dist=True)
        same(d2, dist), same(r2.values, r0.values), same(r2.indices, r0.indices)
        np.testing.assert_array_equal(r2.ranks, host_ranks(dist, 1))
        assert r2.mrr == float((1.0 / (r2.ranks + 1)).mean()) and r2.median_rank == float(np.median(r2.ranks + 1))
        assert r2.hit_at_1 == float((r2.ranks == 0).mean()) == r0.hit_at_1
        assert r2.hit_at_k == float((r2.ranks < r2.k).mean()) == r0.hit_at_k
        assert retrieval.report(r2).startswith(line + ", MRR = ")


def test_retrieve_sharded_micro():
    from magic_amd.vae import TangoEncoder
    locks, keys = micro_tables(32)
    vae = TangoEncoder(None, config=preset("11a", image_size=locks.shape[1], batch=64, precision="bf16"), init_seed=5)
    try:
        check_retrieve(vae, locks, keys, 32, 7)
    finally:
        vae.close()


def test_retrieve_sharded_cosine():
    from magic_amd.vae import TangoEncoder
    rng = np.random.default_rng(8)
    locks = ((rng.random((600, 8, 8)) < 0.4) * 255).astype(np.uint8)
    keys = ((rng.random((590, 8, 8)) < 0.4) * 255).astype(np.uint8)
    cfg = MVAEConfig(image_size=8, batch=64, enc=(40, 24), dec=(28, 20), latent=6, metric="cosine",
                     reciprocal=False, precision="f32")
    vae = TangoEncoder(None, config=cfg, init_seed=3)
    try:
        check_retrieve(vae, locks, keys, 10, 256)
        # TangoEncoder.match forwards the norms and the index base: a query batch against a slice of the
        # gallery scores as inside the full call
        eng = vae.engine
        zl, zk = vae.embed(locks), vae.embed(keys)
        rl, rk = (eng.match_rnorm(eng.match_colsq(to_dev(a))).cpu().numpy() for a in (zl, zk))
        full = vae.match(zl, zk, k=1, return_dist=True)[2]
        val, ind, d = vae.match(zl[:40], zk[100:], k=5, rl=rl, rk=rk, key_base=100, return_dist=True)
        same(d, full[:40, 100:])
        assert ind.min() >= 100
        same(val, np.take_along_axis(d, ind.astype(np.int64) - 100, 1))
    finally:
        vae.close()


def test_driver_flags(capsys):
    from magic_amd import main
    main.main(["--preset", "11a", "--image-size", "200", "--batch", "64", "--epochs", "1", "--samples-per-epoch", "64",
               "--data", GOLD, "--fused-input", "--retrieve", "10", "--retrieve-shard", "16", "--retrieve-ranks"])
    lines = [l for l in capsys.readouterr().out.splitlines() if "hit@1 = " in l]
    assert len(lines) == 1 and "hit@10 = " in lines[0] and "MRR = " in lines[0] and "median rank = " in lines[0]
