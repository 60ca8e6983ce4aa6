"""oracle/philox_oracle.py against the published Philox4x32-10 known answers (Random123's
kat_vectors), and a sanity check of the normals it derives from them. CPU only."""
import numpy as np
import pytest

from oracle import philox_oracle as PH

# (counter words, key words, output words): Random123 kat_vectors, "philox4x32 10"
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = PH.philox4x32_10(ctr, key)
    assert tuple(int(w) for w in got) == want


def test_philox_is_vectorised():
    """All three known answers in one call (arrays broadcast element by element)."""
    ctr = [np.array([k[0][j] for k in KAT], dtype=np.uint64) for j in range(4)]
    key = [np.array([k[1][j] for k in KAT], dtype=np.uint64) for j in range(2)]
    got = PH.philox4x32_10(ctr, key)
    for n, k in enumerate(KAT):
        assert tuple(int(w[n]) for w in got) == k[2]


def test_uniform_is_formed_in_float32():
    """The largest words round to u = 1.0 exactly (radius 0), the smallest to 2^-33."""
    u = PH.uniform_f32(np.array([0, 1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF], dtype=np.uint64))
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -33) and u[1] == np.float32(1.5 * 2.0 ** -32)
    assert u[2] < 1.0 and u[3] == 1.0 and u[4] == 1.0


def test_eps_reference_layout():
    """Element (s, b, i) is lane g & 3 of block g >> 2, g = (s Bg + off + b) L + i; a shard is
    the slice of the global draw; the eval stream and another counter are other draws."""
    seed, L, Bg = 0x9E3779B97F4A7C15, 5, 7
    e = PH.eps_reference(seed, 3, Bg, L)
    assert e.shape == (3, Bg, L) and e.dtype == np.float64
    for s, b, i in [(0, 0, 0), (0, 0, 3), (1, 0, 0), (1, 2, 4), (2, 6, 4)]:
        g = (s * Bg + b) * L + i
        assert e[s, b, i] == PH.normals_of_blocks(np.array([g >> 2]), seed, 3)[0, g & 3]
    np.testing.assert_array_equal(PH.eps_reference(seed, 3, Bg, L, off=2, B=3), e[:, 2:5])
    assert not np.any(PH.eps_reference(seed, 3 | PH.EVAL_STREAM, Bg, L) == e)
    assert not np.any(PH.eps_reference(seed, (1 << 32) + 3, Bg, L) == e)
    assert not np.any(PH.eps_reference(seed & 0xFFFFFFFF, 3, Bg, L) == e)


def test_reference_normals_are_standard_normal():
    v = PH.eps_reference(2, 0, 1 << 10, 1 << 10, B=1 << 10)[0].ravel()
    assert v.size == 1 << 20
    mean, std, m4 = v.mean(), v.std(), ((v - v.mean()) ** 4).mean() / v.var() ** 2
    print(f"2^20 reference normals: mean {mean:.2e} std-1 {std - 1:.2e} m4-3 {m4 - 3:.2e}")
    assert abs(mean) < 5e-3 and abs(std - 1) < 5e-3 and abs(m4 - 3) < 0.05
