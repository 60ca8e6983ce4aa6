"""``overlap_input.draw_keys``, the key draw of a cross-pair batch, pinned on the CPU with fixed
seeds: which key each row takes, and exactly which random numbers the draw consumes (so that the
next batch of a stream is reproducible from the documented calls alone)."""
import numpy as np
import pytest

from magic_amd.overlap_input import BatchStream, draw_keys

B, N, M = 257, 11, 13
SEED = 12345


def lock_idx():
    return np.random.default_rng(99).integers(0, N, B)


def documented_draws(rng, m):
    """The draw order the docstring states: u = rng.random(B), then kj = rng.integers(0, m, B)."""
    u = rng.random(B)
    kj = rng.integers(0, m, B)
    return u, kj


def test_cross_0_returns_idx():
    idx = lock_idx()
    out = draw_keys(np.random.default_rng(SEED), idx, M, 0.0)
    np.testing.assert_array_equal(out, idx)
    assert out.dtype == np.int64 and out is not idx


def test_cross_1_is_the_uniform_draw():
    idx = lock_idx()
    _, kj = documented_draws(np.random.default_rng(SEED), M)
    out = draw_keys(np.random.default_rng(SEED), idx, M, 1.0)
    np.testing.assert_array_equal(out, kj)
    assert out.min() >= 0 and out.max() < M
    assert len(np.unique(out)) == M  # 257 draws over 13 keys reach every key, the last one included


def test_partial_cross_mixes_by_u():
    idx = lock_idx()
    u, kj = documented_draws(np.random.default_rng(SEED), M)
    out = draw_keys(np.random.default_rng(SEED), idx, M, 0.25)
    np.testing.assert_array_equal(out, np.where(u < 0.25, kj, idx))
    assert 0 < (u < 0.25).sum() < B  # both kinds of row occur


def test_candidates_bound_the_draw():
    """cross = 1 with candidates: row b takes candidates[idx[b], kj[b] % k], never another key."""
    idx = lock_idx()
    k = 3
    cand = np.stack([np.random.default_rng(7 + i).permutation(M)[:k] for i in range(N)])
    _, kj = documented_draws(np.random.default_rng(SEED), M)
    out = draw_keys(np.random.default_rng(SEED), idx, M, 1.0, candidates=cand)
    np.testing.assert_array_equal(out, cand[idx, kj % k])
    for b in range(B):
        assert out[b] in cand[idx[b]]
    # a row that keeps its own key ignores the candidates
    u, kj = documented_draws(np.random.default_rng(SEED), M)
    out = draw_keys(np.random.default_rng(SEED), idx, M, 0.5, candidates=cand)
    np.testing.assert_array_equal(out, np.where(u < 0.5, cand[idx, kj % k], idx))


@pytest.mark.parametrize("cross", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("mined", [False, True])
def test_draw_consumes_exactly_the_documented_calls(cross, mined):
    """Whatever ``cross`` and the candidates are, the generator ends where the two documented calls
    leave it: the stream's next batch does not depend on either."""
    idx = lock_idx()
    cand = np.zeros((N, 2), np.int64) if mined else None
    a, b = np.random.default_rng(SEED), np.random.default_rng(SEED)
    draw_keys(a, idx, M, cross, candidates=cand)
    documented_draws(b, M)
    assert a.bit_generator.state == b.bit_generator.state
    np.testing.assert_array_equal(a.random(5), b.random(5))


def test_stream_refuses_cross_pairs_without_computed_labels():
    """Checked before anything touches a device."""
    for pairs in ("cross", "mined"):
        with pytest.raises(ValueError, match="computed"):
            BatchStream(64, 20, labels="sampled", pairs=pairs, device="cpu")
    with pytest.raises(ValueError, match="pairs"):
        BatchStream(64, 20, labels="computed", pairs="all", device="cpu")
