"""``mvae_rerank`` and ``mvae_overlap_place`` (``magic_amd/csrc/rerank.hip``) and their Python surface
against the CPU restatement ``tests/rerank_ref.py``: a shortlist ordered by exact overlap area, with
poses, and a key shown at its pose. Integer work: every comparison is for exact equality. The
reference of a table (every lock with every key) is computed once and shared."""
import functools

import numpy as np
import pytest
import torch

from magic_amd import _lib
from magic_amd.overlap_input import max_overlap, place, random_shapes, rerank, rotation_coefficients
from tests.overlap_ref import angle_coefficients
from tests.rerank_ref import pair_table, place_ref, rerank_ref

pytestmark = pytest.mark.gpu

NL, NK = 6, 9  # locks and keys of a table: 54 reference pairs


def dev(a, dtype=None):
    t = torch.as_tensor(np.array(a))  # a copy: the shared reference tables are read-only
    return (t.to(dtype) if dtype is not None else t).cuda().contiguous()


def shapes(n, h, w, seed):
    s = max(h, w)
    img = random_shapes(n, s, torch.Generator().manual_seed(seed), "cpu").numpy()
    return (img[:, :h, :w] * 255).astype(np.uint8)


def noise(n, h, w, seed):
    return ((np.random.default_rng(seed).random((n, h, w)) < 0.5) * 255).astype(np.uint8)


def angles(n_rot, seed=0):
    """n_rot 1: the identity (pure translation); else angle 0 and random angles (radians)."""
    return np.zeros(1) if n_rot == 1 else np.r_[0.0, np.random.default_rng(seed).uniform(0, 2 * np.pi, n_rot - 1)]


def coefs(n_rot, h, w, seed=0):
    return rotation_coefficients(angles(n_rot, seed), h, w)


@functools.lru_cache(maxsize=None)
def table(kind, h, w, n_rot):
    """(locks, keys, coef, area [NL, NK], pose [NL, NK, 3]): the shared, unchanged reference."""
    make = shapes if kind == "shapes" else noise
    L, K = make(NL, h, w, 1 + h), make(NK, h, w, 2 + h)
    coef = coefs(n_rot, h, w, seed=h)
    area, pose = pair_table(L, K, coef)
    for a in (L, K, coef, area, pose):
        a.setflags(write=False)
    return L, K, coef, area, pose


def raw_rerank(L, K, coef, cand, lock_idx=None, pose=True, src=True):
    """The C entry point itself, every output prefilled with -7 so that an unwritten slot shows."""
    lib = _lib.load()
    Ld, Kd, cf = dev(L), dev(K), dev(np.asarray(coef, np.float32))
    cd = dev(np.asarray(cand), torch.int32)
    li = dev(np.asarray(lock_idx), torch.int32) if lock_idx is not None else None
    n, r = cd.shape
    h, w = Ld.shape[1:]
    full = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")  # noqa: E731
    key, area = full(n, r), full(n, r)
    ps = full(n, r, 3) if pose else None
    fr = full(n, r) if src else None
    nbytes = lib.mvae_rerank_work_bytes(n, r, len(cf), h, w)
    assert nbytes >= lib.mvae_overlap_work_bytes(n * r, len(cf), h, w) > 0
    work = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    rc = lib.mvae_rerank(Ld.data_ptr(), Kd.data_ptr(), h, w, p(li), cd.data_ptr(), n, r, cf.data_ptr(), len(cf),
                         key.data_ptr(), area.data_ptr(), p(ps), p(fr), work.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    _lib.check(lib, None, rc)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy() if t is not None else None  # noqa: E731
    return host(key), host(area), host(ps), host(fr)


def check_rerank(tab, cand, lock_idx=None):
    L, K, coef, area, pose = tab
    got = raw_rerank(L, K, coef, cand, lock_idx)
    want = rerank_ref(cand, area, pose, lock_idx)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    return got


def draw(rng, n, r, empties=0.15):
    cand = rng.integers(0, NK, (n, r))
    cand[rng.random((n, r)) < empties] = -1
    cand[0, 0], cand[-1, -1] = 0, NK - 1  # key 0 and the last image of the table
    return cand


# ------------------------------------------------------------------ sizes, ragged groups, lists
@pytest.mark.parametrize("n_rot", [1, 8])
@pytest.mark.parametrize("hw", [(8, 8), (20, 20), (24, 40), (72, 72)])
def test_rows_of_every_length_and_count(hw, n_rot):
    """R in {1, 3, 64} and N in {1, 5, 7, 130}: one lane to a full wave, a single wave of a workgroup,
    ragged groups of four locks and more than one workgroup; empties at random, repeated keys (R
    exceeds the table), NULL and list lock_idx with repeats."""
    rng = np.random.default_rng(hw[0] + n_rot)
    for kind in ("shapes", "noise"):
        tab = table(kind, hw[0], hw[1], n_rot)
        if kind == "shapes":
            assert tab[3].max() > 0
        for n in (1, 5, 7, 130):
            for r in (1, 3, 64):
                cand = draw(rng, n, r)
                if n <= NL and (n + r) % 2 == 0:  # lock_idx NULL: lock i
                    check_rerank(tab, cand)
                else:
                    li = rng.integers(0, NL, n)
                    li[0], li[-1] = NL - 1, 0
                    check_rerank(tab, cand, li)


# ------------------------------------------------------------------ ties
def test_ties_keep_the_models_order():
    S = 20
    L, K = shapes(4, S, S, 60), shapes(5, S, S, 61)
    L[3] = 0       # an empty lock: every candidate has area 0
    K[4] = K[1]    # two identical key images at different indices
    coef = coefs(8, S, S, seed=6)
    tab = (L, K, coef) + pair_table(L, K, coef)
    cand = np.array([[1, 4, 1, 0, 2],    # the same key twice and its twin between them
                     [4, 1, 3, 4, 1],
                     [4, 3, 2, 1, 0],
                     [2, 0, 4, 1, 3]])
    key, area, pose, src = check_rerank(tab, cand, [0, 1, 3, 3])
    for i in (0, 1):
        t = [j for j in range(5) if key[i, j] in (1, 4)]  # key 1 and its twin: one area, neighbours
        assert len(t) == sum(c in (1, 4) for c in cand[i]) >= 3
        assert t == list(range(t[0], t[0] + len(t))) and len(set(area[i, t].tolist())) == 1
        assert src[i, t].tolist() == sorted(src[i, t].tolist())  # equal areas: columns in the model's order
        assert key[i, t].tolist() == [cand[i, c] for c in src[i, t]]
    for i in (2, 3):  # the empty lock: all areas 0, the row is the model's
        assert (area[i] == 0).all() and (pose[i] == 0).all()
        assert key[i].tolist() == cand[i].tolist() and src[i].tolist() == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------ empties
def test_empty_entries():
    tab = table("shapes", 20, 20, 8)
    cand = np.array([[3, -1, 5, -1, 0, 8],     # in the middle of a row
                     [-1, -1, -1, -1, -1, -1],  # a whole row
                     [-1, 8, 0, 2, 2, -5],      # at both ends; any negative value is an empty
                     [7, 6, 5, 4, 3, 2],
                     [-1, -1, -1, -1, -1, 0]])
    key, area, pose, src = check_rerank(tab, cand)
    assert key[0, 4:].tolist() == [-1, -1] and area[0, 4:].tolist() == [-1, -1] and src[0, 4:].tolist() == [1, 3]
    assert (key[1] == -1).all() and (area[1] == -1).all() and (pose[1] == 0).all()
    assert src[1].tolist() == list(range(6))
    assert key[2, 4:].tolist() == [-1, -1] and src[2, 4:].tolist() == [0, 5]
    assert key[4, 0] == 0 and src[4].tolist() == [5, 0, 1, 2, 3, 4]
    # every row empty: nothing to verify, and the tables are not read
    none = np.full((5, 3), -1)
    key, area, pose, src = check_rerank(tab, none, [5, 0, 0, 2, 5])
    assert (key == -1).all() and (area == -1).all() and (pose == 0).all()
    assert (src == np.arange(3)).all()


def test_null_pose_out_and_null_from_out():
    L, K, coef, area, pose = tab = table("noise", 24, 40, 8)
    cand = draw(np.random.default_rng(3), 5, 3)  # lock_idx NULL: at most NL rows
    want = rerank_ref(cand, area, pose)
    full = check_rerank(tab, cand)
    for kw in (dict(pose=False), dict(src=False), dict(pose=False, src=False)):
        k, a, p, s = raw_rerank(L, K, coef, cand, **kw)
        np.testing.assert_array_equal(k, want[0])
        np.testing.assert_array_equal(a, want[1])
        assert (p is None) == (not kw.get("pose", True)) and (s is None) == (not kw.get("src", True))
        if p is not None:
            np.testing.assert_array_equal(p, full[2])
        if s is not None:
            np.testing.assert_array_equal(s, full[3])


# ------------------------------------------------------------------ Python
def test_rerank_surface():
    L, K, _, _, _ = table("shapes", 20, 20, 8)
    coef = angle_coefficients(8, 20, 20)  # angles=8: the equally spaced ones
    area, pose = pair_table(L, K, coef)
    cand = draw(np.random.default_rng(9), 5, 4)
    out = rerank(dev(L), dev(K), dev(cand, torch.int32), angles=8)
    for t, shape in zip(out, ((5, 4), (5, 4), (5, 4, 3), (5, 4))):
        assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == shape
    for g, w in zip(out, rerank_ref(cand, area, pose)):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    li = [4, 4, 0, 5, 1]
    out = rerank(dev(L), dev(K), dev(cand, torch.int32), dev(li, torch.int32), angles=8)
    for g, w in zip(out, rerank_ref(cand, area, pose, li)):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    c = dev(cand, torch.int32)
    for bad in (dict(cand=c.long()), dict(cand=c.cpu()), dict(cand=c[0]), dict(cand=c.repeat(1, 17)),
                dict(locks=dev(L).float()), dict(locks=torch.from_numpy(L.copy())), dict(keys=dev(K)[:, :10]),
                dict(lock_idx=dev(li[:4], torch.int32)), dict(lock_idx=dev(li, torch.int64)),
                dict(cand=dev(draw(np.random.default_rng(1), 7, 2), torch.int32))):  # 7 rows, 6 locks, no list
        a = dict(locks=dev(L), keys=dev(K), cand=c, lock_idx=None)
        a.update(bad)
        with pytest.raises(ValueError):
            rerank(a["locks"], a["keys"], a["cand"], a["lock_idx"], angles=8)


# ------------------------------------------------------------------ placement
def raw_place(L, K, coef, lock_idx, key_idx, pose, overlay=True, stats=True):
    lib = _lib.load()
    Ld, Kd, cf = dev(L), dev(K), dev(np.asarray(coef, np.float32))
    li = dev(np.asarray(lock_idx), torch.int32) if lock_idx is not None else None
    ki = dev(np.asarray(key_idx), torch.int32) if key_idx is not None else None
    ps = dev(np.asarray(pose), torch.int32)
    n = len(ps)
    h, w = Ld.shape[1:]
    ov = torch.full((n, h, w), 0xF9, dtype=torch.uint8, device="cuda") if overlay else None
    st = torch.full((n, 4), -7, dtype=torch.int32, device="cuda") if stats else None
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    rc = lib.mvae_overlap_place(Ld.data_ptr(), Kd.data_ptr(), h, w, p(li), p(ki), n, cf.data_ptr(), len(cf),
                                ps.data_ptr(), p(ov), p(st), torch.cuda.current_stream().cuda_stream)
    _lib.check(lib, None, rc)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy() if t is not None else None  # noqa: E731
    return host(ov), host(st)


def check_place(L, K, coef, lock_idx, key_idx, pose):
    n = len(pose)
    li = lock_idx if lock_idx is not None else range(n)
    ki = key_idx if key_idx is not None else range(n)
    want = [place_ref(L[a], K[b], coef, p) for a, b, p in zip(li, ki, pose)]
    wo, ws = np.stack([o for o, _ in want]), np.stack([s for _, s in want])
    ov, st = raw_place(L, K, coef, lock_idx, key_idx, pose)
    np.testing.assert_array_equal(ov, wo)
    np.testing.assert_array_equal(st, ws)
    only_ov, none = raw_place(L, K, coef, lock_idx, key_idx, pose, stats=False)  # each output on its own
    assert none is None
    np.testing.assert_array_equal(only_ov, wo)
    none, only_st = raw_place(L, K, coef, lock_idx, key_idx, pose, overlay=False)
    assert none is None
    np.testing.assert_array_equal(only_st, ws)
    return ov, st


@pytest.mark.parametrize("n_rot", [1, 8])
@pytest.mark.parametrize("hw", [(8, 8), (20, 20), (24, 40), (72, 72)])
def test_place_at_the_poses_of_max_overlap(hw, n_rot):
    rng = np.random.default_rng(hw[1] + n_rot)
    for kind in ("shapes", "noise"):
        L, K, coef, area, pose = table(kind, hw[0], hw[1], n_rot)
        li, ki = rng.integers(0, NL, 7), rng.integers(0, NK, 7)
        li[0], ki[0], ki[-1] = NL - 1, 0, NK - 1
        a, p = max_overlap(dev(L), dev(K), dev(li, torch.int32), dev(ki, torch.int32), angles=angles(n_rot, hw[0]))
        a, p = a.cpu().numpy(), p.cpu().numpy()
        np.testing.assert_array_equal(p, pose[li, ki])  # (the table was made with these angles)
        ov, st = check_place(L, K, coef, li, ki, p)
        np.testing.assert_array_equal(st[:, 3], a)
        check_place(L, K, coef, None, None, pose[np.arange(NL), np.arange(NL)])  # both lists NULL: pair i
        some = np.stack([rng.integers(0, n_rot, 5), rng.integers(-(hw[0] - 1), hw[0], 5),
                         rng.integers(-(hw[1] - 1), hw[1], 5)], axis=1)  # any pose in range, not the best
        check_place(L, K, coef, None, ki[:5], some)


def test_place_stats_equal_the_area_of_max_overlap():
    S = 20
    L, K = shapes(6, S, S, 70), shapes(6, S, S, 71)
    Ld, Kd = dev(L), dev(K)
    area, pose = max_overlap(Ld, Kd, angles=8)
    ov, st = place(Ld, Kd, None, None, pose, angles=8)
    assert ov.is_cuda and ov.dtype == torch.uint8 and tuple(ov.shape) == (6, S, S)
    assert st.is_cuda and st.dtype == torch.int32 and tuple(st.shape) == (6, 4)
    assert torch.equal(st[:, 3], area) and area.max() > 0
    coef = angle_coefficients(8, S, S)
    for i, p in enumerate(pose.cpu().numpy()):
        wo, ws = place_ref(L[i], K[i], coef, p)
        np.testing.assert_array_equal(ov[i].cpu().numpy(), wo)
        np.testing.assert_array_equal(st[i].cpu().numpy(), ws)
    idx = dev([5, 0, 2], torch.int32)
    for bad in (dict(pose=pose.long()), dict(pose=pose[:, :2].contiguous()), dict(pose=pose.cpu()),
                dict(lock_idx=idx), dict(key_idx=idx.long()), dict(locks=Ld.float())):
        a = dict(locks=Ld, keys=Kd, lock_idx=None, key_idx=None, pose=pose)
        a.update(bad)
        with pytest.raises(ValueError):
            place(a["locks"], a["keys"], a["lock_idx"], a["key_idx"], a["pose"], angles=8)


def test_place_corners_and_poses_out_of_range():
    H, W = 24, 40
    L = np.zeros((3, H, W), np.uint8)
    K = np.zeros((3, H, W), np.uint8)
    L[0, 0, 0] = K[0, H - 1, W - 1] = 255      # opposite corners: dy = -(H - 1), dx = -(W - 1)
    L[1, H - 1, W - 1] = K[1, 0, 0] = 255      # ... and +
    L[2], K[2] = shapes(1, H, W, 80)[0], shapes(1, H, W, 81)[0]
    coef = coefs(1, H, W)
    n_rot = 1
    pose = [(0, -(H - 1), -(W - 1)), (0, H - 1, W - 1), (0, H - 1, -(W - 1)), (0, -(H - 1), W - 1)]
    ov, st = check_place(L, K, coef, [0, 1, 2, 2], [0, 1, 2, 2], pose)
    assert st[0].tolist() == [1, 1, 1, 1] and st[1].tolist() == [1, 1, 1, 1]
    assert ov[0, 0, 0] == 3 and ov[0].sum() == 3 and ov[1, H - 1, W - 1] == 3 and ov[1].sum() == 3
    bad = [(-1, 0, 0), (n_rot, 0, 0), (0, H, 0), (0, 0, -W), (0, -H, 0), (0, 0, W), (1 << 30, 3, 3)]
    lb = (L[2] >= 128).astype(np.uint8)
    ov, st = check_place(L, K, coef, [2] * len(bad), [2] * len(bad), bad)
    for o, s in zip(ov, st):
        np.testing.assert_array_equal(o, lb)              # the lock alone
        assert s.tolist() == [int(lb.sum()), -1, -1, -1]
    # with 8 angles r = 8 is the first one out of range and r = 7 the last one in
    coef8 = coefs(8, H, W, seed=2)
    ov, st = check_place(L, K, coef8, [2, 2], [2, 2], [(7, 1, -2), (8, 1, -2)])
    assert st[0, 1] > 0 and st[1].tolist() == [int(lb.sum()), -1, -1, -1]


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def gallery():
    from magic_amd import retrieval
    from magic_amd.config import MVAEConfig
    from magic_amd.vae import TangoEncoder
    rng = np.random.default_rng(8)
    locks = ((rng.random((14, 8, 8)) < 0.4) * 255).astype(np.uint8)
    keys = ((rng.random((12, 8, 8)) < 0.4) * 255).astype(np.uint8)
    cfg = MVAEConfig(image_size=8, batch=64, enc=(40, 24), dec=(28, 20), latent=6, metric="cosine",
                     reciprocal=False, precision="f32")
    vae = TangoEncoder(None, config=cfg, init_seed=3)
    truth = retrieval.overlap_matrix(locks, keys, angles=8)
    try:
        yield vae, locks, keys, truth
    finally:
        vae.close()


def test_retrieve_rerank_over_the_whole_gallery_is_the_truth(gallery):
    from magic_amd import retrieval
    vae, locks, keys, truth = gallery
    r = retrieval.retrieve(vae, locks, keys, k=3, rerank=12, rerank_angles=8, truth=truth)
    assert r.k == 3 and r.indices.shape == r.values.shape == r.areas.shape == (14, 3)
    assert r.poses.shape == (14, 3, 3) and r.shortlist.shape == (14, 12)
    np.testing.assert_array_equal(r.areas, np.take_along_axis(truth, r.indices.astype(np.int64), axis=1))
    assert (r.areas[:, :-1] >= r.areas[:, 1:]).all()
    np.testing.assert_array_equal(r.areas[:, 0], truth.max(1))
    assert r.area_regret == 0.0
    assert 0.0 <= r.moved <= 1.0 and r.moved == float((r.indices[:, 0] != r.shortlist[:, 0]).mean())
    ov, st = retrieval.placed(r, locks, keys, angles=8)
    np.testing.assert_array_equal(st[:, 3].cpu().numpy(), r.areas[:, 0])
    ov2, st2 = retrieval.placed(r, locks, keys, rank=2, angles=8)
    np.testing.assert_array_equal(st2[:, 3].cpu().numpy(), r.areas[:, 2])
    coef = angle_coefficients(8, 8, 8)
    for i in (0, 13):
        wo, ws = place_ref(locks[i], keys[r.indices[i, 0]], coef, r.poses[i, 0])
        np.testing.assert_array_equal(ov[i].cpu().numpy(), wo)
        np.testing.assert_array_equal(st[i].cpu().numpy(), ws)
    s = retrieval.report(r)
    assert "verified" in s and "model's 12 best" in s and "area regret = 0.00" in s
    # the truly best key is the first maximum of a row; among equal areas the verified list keeps the
    # model's order, so the two may name different keys of one area: judged as documented, on the list
    best = np.argmax(truth, axis=1)
    assert r.true_hit_at_1 == float((r.indices[:, 0] == best).mean())
    assert r.true_hit_at_k == float((r.indices == best[:, None]).any(1).mean())


def test_retrieve_rerank_shortlist_scores_and_plain_call(gallery):
    from magic_amd import retrieval
    vae, locks, keys, truth = gallery
    plain = retrieval.retrieve(vae, locks, keys, k=5)
    # without rerank the result is today's, field by field, and the new fields are None
    zl, zk = vae.embed(locks), vae.embed(keys)
    val, ind = vae.match(zl, zk, k=5, order=1)
    np.testing.assert_array_equal(plain.values, val)
    np.testing.assert_array_equal(plain.indices, ind)
    own = np.arange(12)[:, None]
    assert plain.hit_at_1 == float((ind[:12, :1] == own).any(1).mean())
    assert plain.hit_at_k == float((ind[:12] == own).any(1).mean())
    assert (plain.k, plain.order, plain.ranks, plain.mrr, plain.median_rank) == (5, 1, None, None, None)
    assert plain.true_hit_at_1 is None and plain.true_hit_at_k is None
    assert (plain.areas, plain.poses, plain.shortlist, plain.moved, plain.area_regret) == (None,) * 5
    assert "verified" not in retrieval.report(plain) and len(plain) == 16
    r = retrieval.retrieve(vae, locks, keys, k=3, rerank=5, rerank_angles=8)
    np.testing.assert_array_equal(r.shortlist, plain.indices)
    assert r.area_regret is None and "area regret" not in retrieval.report(r)
    for i in range(14):
        for j in range(3):
            at = np.flatnonzero(plain.indices[i] == r.indices[i, j])
            assert len(at) == 1                                 # a key of the shortlist,
            assert r.values[i, j] == plain.values[i, at[0]]     # with the model's score of it,
            assert r.areas[i, j] == truth[i, r.indices[i, j]]   # and its exact area
    want = rerank_ref(plain.indices, truth, np.zeros((14, 12, 3), np.int32))
    np.testing.assert_array_equal(r.indices, want[0][:, :3])
    np.testing.assert_array_equal(r.areas, want[1][:, :3])
    own = np.arange(12)[:, None]
    assert r.hit_at_1 == float((r.indices[:12, :1] == own).any(1).mean())  # judged on the verified list
    assert r.hit_at_k == float((r.indices[:12] == own).any(1).mean())
    # the sharded path with ranks gives the same lists
    s = retrieval.retrieve(vae, locks, keys, k=3, rerank=5, rerank_angles=8, shard=5, ranks=True)
    for f in ("indices", "areas", "poses", "shortlist"):
        np.testing.assert_array_equal(getattr(s, f), getattr(r, f))
    # (the scores of a sharded cosine match equal the one-shot ones to the rounding of the fp64 column
    # sums unless the shard is a multiple of 256: ``retrieve``'s contract)
    np.testing.assert_allclose(s.values, r.values, rtol=1e-6, atol=0)
    assert s.ranks is not None and s.moved == r.moved
    for bad in (dict(k=3, rerank=2), dict(k=3, rerank=65), dict(k=3, rerank=13)):
        with pytest.raises(ValueError):
            retrieval.retrieve(vae, locks, keys, rerank_angles=8, **bad)
    with pytest.raises(ValueError):
        retrieval.placed(plain, locks, keys)


def test_driver_retrieve_rerank(capsys):
    from magic_amd import main
    main.main(["--preset", "11a", "--image-size", "32", "--batch", "64", "--epochs", "1", "--samples-per-epoch", "64",
               "--labels", "computed", "--label-angles", "8", "--retrieve", "5", "--retrieve-rerank", "16",
               "--rerank-angles", "8"])
    lines = [l for l in capsys.readouterr().out.splitlines() if "hit@1 = " in l]
    assert len(lines) == 1 and "hit@5 = " in lines[0] and "verified" in lines[0] and "model's 16 best" in lines[0]
    with pytest.raises(SystemExit):
        main.main(["--retrieve-rerank", "16"])  # valid only with --retrieve
    capsys.readouterr()
