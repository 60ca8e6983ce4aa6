"""``tests/bits_ref.py`` against the ``BitMat`` comment of ``magic_amd/csrc/mvae_internal.h``
restated as a loop over single elements, and the batch operand's pieces on a hand-made batch."""
import numpy as np
import pytest

from tests import bits_ref as R


def bitmat_loop(A):
    """One element at a time, in the comment's own words: block (mt, kt) at word 512 (mt kts + kt);
    in a block, word 2 ((2 s + wm) 64 + lane) + j; bit 8 h + 4 kh + (el >> 1) + 16 (el & 1)."""
    M, K = A.shape
    kts = (K + 63) // 64
    out = [0] * (((M + 255) // 256) * kts * 512)
    for row in range(M):
        for k in range(K):
            if not A[row][k]:
                continue
            mt, r = divmod(row, 256)
            kt, kk = divmod(k, 64)
            s, r = divmod(r, 128)
            wm, r = divmod(r, 64)
            jh, l15 = divmod(r, 16)  # r = 16 (2 j + h) + (lane & 15)
            j, h = divmod(jh, 2)
            kh, kk = divmod(kk, 32)  # k = 32 kh + 8 (lane >> 4) + el
            l4, el = divmod(kk, 8)
            lane = 16 * l4 + l15
            out[512 * (mt * kts + kt) + 2 * ((2 * s + wm) * 64 + lane) + j] |= \
                1 << (8 * h + 4 * kh + (el >> 1) + 16 * (el & 1))
    return np.array(out, np.uint32)


@pytest.mark.parametrize("M,K", [(70, 65), (300, 130)])
def test_bitmat_is_the_layout_comment(M, K):
    A = (np.random.default_rng(M + K).random((M, K)) < 0.4).astype(np.uint8)
    A[M - 1, K - 1] = A[0, 0] = 1
    got = R.bitmat(A)
    assert got.dtype == np.uint32 and got.size == R.bitmat_words(M, K)
    np.testing.assert_array_equal(got, bitmat_loop(A))
    assert sum(bin(int(w)).count("1") for w in got) == int(A.sum())  # one bit per element, no more


def test_bitmat_single_elements():
    """the comment's worked positions: (row, k) -> (word, bit)"""
    for (row, k), (word, bit) in {(0, 0): (0, 0), (0, 1): (0, 16), (0, 2): (0, 1), (16, 0): (0, 8),
                                  (32, 0): (1, 0), (0, 32): (0, 4), (0, 8): (2 * 16, 0), (64, 0): (128, 0),
                                  (256, 64): (512 * 3 + 512, 0)}.items():
        A = np.zeros((300, 130), np.uint8)
        A[row, k] = 1
        w = R.bitmat(A)
        assert w[word] == 1 << bit and np.count_nonzero(w) == 1, (row, k)


def test_operand_of_a_small_batch():
    B, D, ldx, ldbits = 2, 16, 24, 16
    X = np.zeros((B, D, 3), np.float32)
    X[0, 3, 0] = 1.0       # lock of row 0, pixel 3
    X[1, 9, 1] = 1.0       # rotated lock of row 1, pixel 9
    X[1, 15, 2] = 1.0      # key of row 1, pixel 15
    o = R.operand(X.reshape(B, 3 * D), B, D, ldx, ldbits)
    A = np.zeros((3 * B, D + 1), np.uint8)
    A[:, D] = 1            # the ones column
    A[2 + 0, 3] = A[0 + 1, 9] = A[4 + 1, 15] = 1  # blocks: rot 0, lock 1, key 2
    np.testing.assert_array_equal(o["xbf"], bitmat_loop(A))
    np.testing.assert_array_equal(o["xbw"], bitmat_loop(A.T))
    xb = o["xbits"].reshape(B, ldbits)
    assert xb[0, 0] == 1 << 3 and np.count_nonzero(xb) == 1
    assert o["dyn"].tolist() == [0, 0, 0, 0] and not o["plane"].any() and not o["xs"].any()
    # a grey value that bf16 does not hold: both flags, plane 0 of every value, the asked fp32 rows
    X[0, 5, 0] = np.float32(7) / np.float32(255)
    o = R.operand(X.reshape(B, 3 * D), B, D, ldx, ldbits, f32mask=2)
    assert o["dyn"].tolist() == [1, 0, 1, 0]
    pl, xs = o["plane"].reshape(3 * B, ldx), o["xs"].reshape(3 * B, ldx)
    assert pl[2, 3] == 0x3F80 and pl[1, 9] == 0x3F80 and pl[5, 15] == 0x3F80
    assert pl[2, 5] == 0x3CE1  # 7 / 255 = 0x3CE0E0E1 rounds up
    assert np.count_nonzero(pl) == 4 and not pl[:, D:].any()
    assert xs[2, 5] == X[0, 5, 0] and xs[2, 3] == 1.0 and np.count_nonzero(xs) == 2
    # 255 at divisor 1: not binary, exact in bf16
    X[0, 5, 0] = 255.0
    assert R.operand(X.reshape(B, 3 * D), B, D, ldx, ldbits)["dyn"].tolist() == [0, 0, 1, 0]
