"""Host reference (numpy) of the layer-0 bit operand: the ``BitMat`` layout of
``magic_amd/csrc/mvae_internal.h`` and everything the batch input kernels write for a batch
``X [B][3 D]`` -- the forward and weight-gradient BitMats, the BCE target bits, the flag words and,
for a batch with a pixel other than 0 / 1, bf16 plane 0 and the fp32 rows. Written from the header's
comment, not from a kernel: ``tests/test_bits_ref.py`` holds ``bitmat`` to a per-element loop, and
``tests/test_gpu_bits.py`` holds every route's kernels to this file, word for word."""
import numpy as np

BLOCK_WORDS = 512  # a block of 256 rows x 64 k


def bitmat_kts(K):
    return (K + 63) // 64


def bitmat_words(M, K):
    return (M + 255) // 256 * bitmat_kts(K) * BLOCK_WORDS


def bitmat(A):
    """0/1 matrix [M][K] -> the words of its BitMat (uint32, bitmat_words(M, K) of them). Block
    (mt, kt) at word 512 (mt kts + kt); in a block, word 2 ((2 s + wm) 64 + lane) + j holds, for
    row 128 s + 64 wm + 16 (2 j + h) + (lane & 15) and k = 32 kh + 8 (lane >> 4) + el, bit
    8 h + 4 kh + (el >> 1) + 16 (el & 1). Rows >= M and k >= K are zero."""
    A = np.asarray(A)
    M, K = A.shape
    kts = bitmat_kts(K)
    row, k = np.nonzero(A)
    s, wm, j, h, l15 = (row >> 7) & 1, (row >> 6) & 1, (row >> 5) & 1, (row >> 4) & 1, row & 15
    kh, l4, el = (k >> 5) & 1, (k >> 3) & 3, k & 7
    lane = 16 * l4 + l15
    word = BLOCK_WORDS * ((row >> 8) * kts + (k >> 6)) + 2 * ((2 * s + wm) * 64 + lane) + j
    bit = 8 * h + 4 * kh + (el >> 1) + 16 * (el & 1)
    out = np.zeros(bitmat_words(M, K), np.uint32)
    np.bitwise_or.at(out, word, np.uint32(1) << bit.astype(np.uint32))
    return out


def stacked_rows(X, B, D):
    """X [B][3 D] (per pixel: lock, rotated lock, key) -> the stacked rows [3B][D] float32:
    blocks [rot | lock | key] from channels (1, 0, 2)"""
    x = np.asarray(X, np.float32).reshape(B, D, 3)
    return np.concatenate([x[:, :, ch] for ch in (1, 0, 2)], axis=0)


def bf16_rne(v):
    """fp32 -> the bf16 bits (uint16) rounded to nearest even (finite values)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)


def operand(X, B, D, ldx, ldbits, f32mask=0):
    """What the batch input kernels leave in zero-filled buffers for the batch X:

    xbf    bitmat(A), A [3B][D + 1] = (stacked rows != 0) with the ones column at k = D
    xbw    bitmat(A.T)
    xbits  [B][ldbits] bytes: byte c of row r = columns 8c .. 8c + 7 of the lock block, bit j
           column 8c + j
    dyn    4 ints: [0] some value is not a bf16 value (tested only in the grey pass: 0 for a 0/1
           batch), [2] some value is not 0 / 1, [1] and [3] -- the other slot -- zeroed
    plane  [3B][ldx] bf16 plane 0 of the stacked rows (columns < D), all zero for a 0/1 batch
    xs     [3B][ldx] fp32 rows of the blocks in f32mask, written with the plane (grey batch only)
    """
    R = stacked_rows(X, B, D)
    A = np.zeros((3 * B, D + 1), np.uint8)
    A[:, :D] = R != 0
    A[:, D] = 1
    lock = A[B:2 * B, :D]
    xbits = np.zeros((B, ldbits), np.uint8)
    xbits[:, :(D + 7) // 8] = np.packbits(lock, axis=1, bitorder="little")
    grey = bool(((R != 0) & (R != 1)).any())
    plane = np.zeros((3 * B, ldx), np.uint16)
    xs = np.zeros((3 * B, ldx), np.float32)
    inexact = False
    if grey:
        plane[:, :D] = bf16_rne(R)
        inexact = bool(((plane[:, :D].astype(np.uint32) << 16).view(np.float32) != R).any())
        for c in range(3):
            if f32mask >> c & 1:
                xs[c * B:(c + 1) * B, :D] = R[c * B:(c + 1) * B]
    return dict(xbf=bitmat(A), xbw=bitmat(A.T), xbits=xbits.reshape(-1),
                dyn=np.array([int(inexact), 0, int(grey), 0], np.int32), plane=plane.reshape(-1),
                xs=xs.reshape(-1))
