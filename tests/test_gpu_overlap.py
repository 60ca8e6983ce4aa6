"""``mvae_overlap_pairs`` (``magic_amd/csrc/overlap.hip``) and its Python surface against the CPU
restatement ``tests/overlap_ref.max_overlap_ref``: the maximum overlap area of a lock and a key over
rotations and integer shifts, and its pose. Integer work, so area AND pose are compared for exact
equality in every case."""
import os

import numpy as np
import pytest
import torch

from magic_amd import _lib
from magic_amd.overlap_input import (BatchStream, angle_coefficients, max_overlap, random_shapes,
                                     rotation_coefficients, synthetic_batch)
from tests.overlap_ref import max_overlap_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap_micro.npz")


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda().contiguous()


def raw(locks, keys, coef, lock_idx=None, key_idx=None, count=None, pose=True):
    """The C entry point itself (NULL index lists and a NULL pose_out are its own cases)."""
    lib = _lib.load()
    L, K, cf = dev(locks), dev(keys), dev(np.asarray(coef, np.float32))
    li = dev(lock_idx, torch.int32) if lock_idx is not None else None
    ki = dev(key_idx, torch.int32) if key_idx is not None else None
    n = count if count is not None else (len(lock_idx) if lock_idx is not None else len(locks))
    h, w = L.shape[1:]
    area = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ps = torch.full((n, 3), -7, dtype=torch.int32, device="cuda") if pose else None
    nbytes = lib.mvae_overlap_work_bytes(n, len(cf), h, w)
    assert nbytes >= 8 * n
    work = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    rc = lib.mvae_overlap_pairs(L.data_ptr(), K.data_ptr(), h, w, p(li), p(ki), n, cf.data_ptr(), len(cf),
                                area.data_ptr(), p(ps), work.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(lib, None, rc)
    torch.cuda.synchronize()
    return area.cpu().numpy(), (ps.cpu().numpy() if pose else None)


def ref(locks, keys, coef, lock_idx=None, key_idx=None, count=None):
    n = count if count is not None else (len(lock_idx) if lock_idx is not None else len(locks))
    li = lock_idx if lock_idx is not None else range(n)
    ki = key_idx if key_idx is not None else range(n)
    out = [max_overlap_ref(locks[a], keys[b], coef) for a, b in zip(li, ki)]
    return np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int32).reshape(n, 3)


def check(locks, keys, coef, **kw):
    area, pose = raw(locks, keys, coef, **kw)
    ra, rp = ref(locks, keys, coef, **kw)
    np.testing.assert_array_equal(area, ra)
    np.testing.assert_array_equal(pose, rp)
    return area, pose


def shapes(n, h, w, seed):
    s = max(h, w)
    img = random_shapes(n, s, torch.Generator().manual_seed(seed), "cpu").numpy()
    return (img[:, :h, :w] * 255).astype(np.uint8)


def noise(n, h, w, seed):
    return ((np.random.default_rng(seed).random((n, h, w)) < 0.5) * 255).astype(np.uint8)


def coefs(n_rot, h, w, seed=0):
    """n_rot 1: the identity (pure translation); else angle 0 and random angles."""
    ang = np.zeros(1) if n_rot == 1 else np.r_[0.0, np.random.default_rng(seed).uniform(0, 2 * np.pi, n_rot - 1)]
    return rotation_coefficients(ang, h, w)


# ------------------------------------------------------------------ word boundaries
@pytest.mark.parametrize("n_rot", [1, 8])
@pytest.mark.parametrize("hw", [(20, 20), (40, 40), (72, 72), (100, 100), (24, 40)])
def test_shapes_and_noise_across_word_boundaries(hw, n_rot):
    h, w = hw
    coef = coefs(n_rot, h, w, seed=h)
    area, _ = check(shapes(8, h, w, 1 + h), shapes(8, h, w, 2 + h), coef)
    assert area.max() > 0
    check(noise(8, h, w, 3 + h), noise(8, h, w, 4 + h), coef)  # ~50 % foreground: many near-ties


# ------------------------------------------------------------------ extremes
def extreme_tables(S=40):
    rng = np.random.default_rng(5)
    L = np.zeros((8, S, S), np.uint8)
    K = np.zeros((8, S, S), np.uint8)
    L[0, 0, 0] = K[0, S - 1, S - 1] = 255          # opposite corners: dy = dx = -(S - 1)
    L[1, S - 1, S - 1] = K[1, 0, 0] = 255          # ... and + (S - 1)
    L[2] = shapes(1, S, S, 9)[0]                   # empty key
    L[3] = K[3] = 255                              # both full: S^2 at shift 0
    L[4, 5:8, 5:8] = L[4, 25:28, 30:33] = 255      # two equal maxima of 9: the smaller dy wins
    K[4, 10:13, 10:13] = 255
    L[5] = rng.integers(126, 130, (S, S))          # grey bytes around the threshold
    K[5] = rng.integers(126, 130, (S, S))
    K[6] = shapes(1, S, S, 10)[0]                  # empty lock
    L[7, 3:9, 4:30] = 200                          # 127 is background, 128 foreground
    K[7, 3:9, 4:30] = 127
    K[7, 20:22, 4:10] = 128
    return L, K


def test_extremes_under_translation():
    S = 40
    L, K = extreme_tables(S)
    area, pose = check(L, K, coefs(1, S, S))
    assert area.tolist()[:5] == [1, 1, 0, S * S, 9] and area[6] == 0 and area[7] == 12
    assert pose[0].tolist() == [0, -(S - 1), -(S - 1)] and pose[1].tolist() == [0, S - 1, S - 1]
    assert pose[2].tolist() == pose[3].tolist() == pose[6].tolist() == [0, 0, 0]
    assert pose[4].tolist() == [0, -5, -5]


def test_extremes_under_rotation():
    S = 40
    L, K = extreme_tables(S)
    area, pose = check(L, K, coefs(5, S, S, seed=2))
    assert area[2] == area[6] == 0 and pose[2].tolist() == pose[6].tolist() == [0, 0, 0]
    # a quarter turn listed twice: the first of the two equal angles is the pose
    quarter = rotation_coefficients(np.array([np.pi / 2, np.pi / 2, 0.0]), S, S)
    check(L, K, quarter)


# ------------------------------------------------------------------ index lists
def test_index_lists_null_lists_counts_and_null_pose():
    S = 20
    coef = coefs(4, S, S, seed=3)
    L, K = shapes(10, S, S, 20), shapes(7, S, S, 21)
    li = [3, 3, 0, 9, 9, 1, 5, 3, 8]
    ki = [6, 0, 6, 6, 2, 2, 4, 6, 1]
    a, p = check(L, K, coef, lock_idx=li, key_idx=ki)
    assert a[0] == a[7] and p[0].tolist() == p[7].tolist()  # a repeated pair
    check(L, K, coef, count=7)                        # both lists NULL: pair i
    check(L, K, coef, lock_idx=li[:7], count=7)       # one list NULL
    check(L, K, coef, key_idx=ki[:5], count=5)
    check(L, K, coef, lock_idx=[9], key_idx=[2])      # count 1: a workgroup per angle
    a2, none = raw(L, K, coef, lock_idx=li, key_idx=ki, pose=False)
    assert none is None
    np.testing.assert_array_equal(a2, a)


def test_more_pairs_than_compute_units():
    S = 20
    rng = np.random.default_rng(11)
    L, K = shapes(40, S, S, 30), shapes(40, S, S, 31)
    li, ki = rng.integers(0, 40, 300), rng.integers(0, 40, 300)
    check(L, K, coefs(3, S, S, seed=4), lock_idx=li, key_idx=ki)


# ------------------------------------------------------------------ the reference's images
def test_fixture_pairs_at_360_angles():
    z = np.load(GOLD)
    w = int(z["shape"][2])
    unpack = lambda a: (np.unpackbits(a[[0, 5]], axis=-1)[..., :w] * 255).astype(np.uint8)  # noqa: E731
    L, K = unpack(z["lock_bits"]), unpack(z["key_bits"])
    assert L.shape == (2, 200, 200)
    area, pose = max_overlap(dev(L), dev(K), angles=360)
    ra, rp = ref(L, K, angle_coefficients(360, 200, 200))
    np.testing.assert_array_equal(area.cpu().numpy(), ra)
    np.testing.assert_array_equal(pose.cpu().numpy(), rp)
    labels = np.load(os.path.join(os.path.dirname(_lib.HERE), "magic_amd", "data", "overlap_areas.npy"))[[0, 5]]
    assert np.all(np.abs(ra / labels - 1.0) <= 0.025)  # and the recorded labels, as on the CPU


# ------------------------------------------------------------------ Python
def test_max_overlap_surface():
    S = 20
    L, K = shapes(6, S, S, 40), shapes(6, S, S, 41)
    area, pose = max_overlap(dev(L), dev(K), angles=8)
    assert area.is_cuda and area.dtype == torch.int32 and area.shape == (6,)
    assert pose.is_cuda and pose.dtype == torch.int32 and pose.shape == (6, 3)
    ra, rp = ref(L, K, angle_coefficients(8, S, S))
    np.testing.assert_array_equal(area.cpu().numpy(), ra)
    np.testing.assert_array_equal(pose.cpu().numpy(), rp)
    ang = np.array([0.3, 4.0, 1.1])  # radians
    li, ki = dev([5, 0, 2, 2], torch.int32), dev([1, 1, 4, 0], torch.int32)
    area, pose = max_overlap(dev(L), dev(K), li, ki, angles=ang)
    ra, rp = ref(L, K, rotation_coefficients(ang, S, S), [5, 0, 2, 2], [1, 1, 4, 0])
    np.testing.assert_array_equal(area.cpu().numpy(), ra)
    np.testing.assert_array_equal(pose.cpu().numpy(), rp)
    for bad in (dev(L).float(), dev(L).to(torch.int32), torch.from_numpy(L), L):
        with pytest.raises(ValueError):
            max_overlap(bad, dev(K), angles=8)
    with pytest.raises(ValueError):
        max_overlap(dev(L), dev(K), dev([0, 1], torch.int64), None, angles=8)
    with pytest.raises(ValueError):
        max_overlap(dev(L), dev(K), angles=0)


def test_batch_stream_computed_labels():
    s = BatchStream(16, 20, seed=3, synthetic_pool=48, labels="computed", label_angles=8)
    area, _ = max_overlap(s.locks, s.keys, angles=8)
    assert s.areas.dtype == torch.float32 and torch.equal(s.areas, area.float())
    L, K = s.locks.cpu().numpy(), s.keys.cpu().numpy()
    ra, _ = ref(L[:4], K[:4], angle_coefficients(8, 20, 20))
    np.testing.assert_array_equal(s.areas[:4].cpu().numpy(), ra.astype(np.float32))
    x, a = next(s)
    assert x.shape == (16, 3 * 400) and a.shape == (16,)
    assert set(a.cpu().tolist()) <= set(s.areas.cpu().tolist())
    with pytest.raises(ValueError):
        BatchStream(16, 20, synthetic_pool=48, labels="measured")
    # a PairSource's areas are replaced alike
    from magic_amd.overlap_input import PairSource
    src = PairSource.from_packed(GOLD, limit=2)
    t = BatchStream(2, 200, src, labels="computed", label_angles=4)
    assert torch.equal(t.areas, max_overlap(t.locks, t.keys, angles=4)[0].float())
    assert not torch.equal(t.areas, torch.from_numpy(src.areas).cuda())


def test_sampled_labels_are_todays():
    a = BatchStream(16, 20, seed=3, synthetic_pool=48)
    b = BatchStream(16, 20, seed=3, synthetic_pool=48, labels="sampled", label_angles=5)
    assert torch.equal(a.areas, b.areas) and torch.equal(a.locks, b.locks) and torch.equal(a.keys, b.keys)
    for _ in range(4):  # more than one epoch of the pool
        (xa, la), (xb, lb) = next(a), next(b)
        assert torch.equal(xa, xb) and torch.equal(la, lb)
    xa, la = synthetic_batch(8, 20, seed=2)
    xb, lb = synthetic_batch(8, 20, seed=2, labels="sampled")
    xc, lc = synthetic_batch(8, 20, seed=2, labels="computed", label_angles=8)
    assert torch.equal(xa, xb) and torch.equal(la, lb) and torch.equal(xa, xc)
    assert lc.dtype == torch.float32 and lc.shape == (8,) and not torch.equal(lc, la)


def test_overlap_matrix():
    from magic_amd import retrieval
    S = 20
    L, K = shapes(6, S, S, 50), shapes(5, S, S, 51)
    want = np.array([[max_overlap_ref(l, k, angle_coefficients(8, S, S))[0] for k in K] for l in L], np.int32)
    for chunk in (7, 1 << 16):
        got = retrieval.overlap_matrix(L, K, angles=8, chunk=chunk)
        assert got.shape == (6, 5) and got.dtype == np.int32
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(retrieval.overlap_matrix(dev(L), dev(K), angles=8), want)


def test_retrieve_truth_fields():
    from magic_amd import retrieval
    from magic_amd.config import MVAEConfig
    from magic_amd.vae import TangoEncoder
    rng = np.random.default_rng(8)
    locks = ((rng.random((40, 8, 8)) < 0.4) * 255).astype(np.uint8)
    keys = ((rng.random((30, 8, 8)) < 0.4) * 255).astype(np.uint8)
    cfg = MVAEConfig(image_size=8, batch=64, enc=(40, 24), dec=(28, 20), latent=6, metric="cosine",
                     reciprocal=False, precision="f32")
    vae = TangoEncoder(None, config=cfg, init_seed=3)
    try:
        r0 = retrieval.retrieve(vae, locks, keys, k=5)
        assert r0.true_hit_at_1 is None and r0.true_hit_at_k is None
        assert "truly best" not in retrieval.report(r0)
        truth = np.zeros((40, 30), np.int32)
        for i in range(40):
            if i % 4 in (0, 2):
                t = r0.indices[i, 0]       # the truly best key is returned first
            elif i % 4 == 1:
                t = r0.indices[i, 4]       # ... last of the five
            else:
                t = min(set(range(30)) - set(r0.indices[i].tolist()))  # ... not at all
            truth[i, t] = 10
            truth[i, t + 1:][::7] = 10     # equal maxima at larger indices: the smallest index counts
        r = retrieval.retrieve(vae, locks, keys, k=5, truth=truth)
        assert r.true_hit_at_1 == 0.5 and r.true_hit_at_k == 0.75
        np.testing.assert_array_equal(r.indices, r0.indices)
        assert (r.hit_at_1, r.hit_at_k, r.ranks) == (r0.hit_at_1, r0.hit_at_k, None)
        assert "truly best key: hit@1 = 0.5000, hit@5 = 0.7500" in retrieval.report(r)
        rs = retrieval.retrieve(vae, locks, keys, k=5, ranks=True, truth=torch.from_numpy(truth))
        assert (rs.true_hit_at_1, rs.true_hit_at_k) == (0.5, 0.75) and rs.ranks is not None
        with pytest.raises(ValueError):
            retrieval.retrieve(vae, locks, keys, k=5, truth=truth[:, :29])
    finally:
        vae.close()


def test_driver_computed_labels(capsys):
    from magic_amd import main
    main.main(["--preset", "11a", "--image-size", "32", "--batch", "64", "--epochs", "1", "--samples-per-epoch", "64",
               "--labels", "computed", "--label-angles", "8", "--retrieve", "10"])
    lines = [l for l in capsys.readouterr().out.splitlines() if "hit@1 = " in l]
    assert len(lines) == 1 and "hit@10 = " in lines[0]
