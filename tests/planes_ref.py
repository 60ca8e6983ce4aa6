"""Host reference (numpy) of the plane side of batch input: what each route of
``mvae_debug_input_planes`` leaves behind for a batch ``X [B][3 D]``, and which elements it writes.
Written from the comments of ``magic_amd/csrc/mvae_internal.h`` (launch_deinterleave, BitsDst, the bits
launchers) and ``magic_amd/csrc/batch_input.hip``, not from running a kernel;
``tests/test_planes_ref.py`` holds the split and the form chooser to values written out by hand, and
``tests/test_gpu_input_planes.py`` holds the kernels to this file, bit for bit.

The contract between the two ends: the producer raises the inexact flag ``dyn[slot]`` exactly when a
residual plane (1 or 2 of the exact split) is nonzero, i.e. when some value is not a bf16 value -- and
only then writes the residual planes and the fp32 rows of ``f32dyn_mask``; the GEMMs read A's residual
planes only while the flag is up (tests/test_gpu_gemm_pairs.py).

                     route 0 (plane path)                          routes 1-3 (bits path, grey pass)
  plane 0            always (np >= 1)                              batch with a value not 0 / 1
  planes 1-2 (np 3)  dyn[slot] rose                                batch with a value not 0 / 1 (zeros where exact)
  fp32 rows          f32mask: always; f32dyn_mask: dyn[slot] rose  f32dyn_mask: batch with a value not 0 / 1
  xbits              the 8-pixel form only                         always
  dyn[slot]          a value is not a bf16 value (0 with np 0)     ... in a batch with a value not 0 / 1
  dyn[2 + slot]      a value not 0 / 1 (8-pixel form); 1 (others)  a value not 0 / 1
  the other slot     zeroed                                        zeroed

Every result is a pair (values, mask): full-size arrays of the buffer's shape and a bool array of the
elements the route writes. Denormals, infinities, NaN and -0 are outside the domain.
"""
import numpy as np

from tests.bits_ref import stacked_rows
from tests.epi_ref import split_planes

OCT, QUAD, SCALAR = "8-pixel", "4-pixel", "scalar"


def form(D, ldx, x_aligned):
    """Which de-interleave kernel launch_deinterleave picks: 8 pixels per thread for D % 8 == 0, a 16-byte
    aligned x and ldx % 8 == 0; 4 for the same with 4; else one pixel per thread."""
    if D % 8 == 0 and x_aligned and ldx % 8 == 0:
        return OCT
    if D % 4 == 0 and x_aligned and ldx % 4 == 0:
        return QUAD
    return SCALAR


def _bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _rows(B, mask):
    """bool [3B]: the stacked rows of the blocks in mask (bit c: block c of B rows)"""
    return np.repeat([bool(mask >> c & 1) for c in range(3)], B)


def _lock_bits(R, B, D, ldbits):
    bits = np.zeros((B, ldbits), np.uint8)
    m = np.zeros((B, ldbits), bool)
    bits[:, :D // 8] = np.packbits(R[B:2 * B, :D // 8 * 8] != 0, axis=1, bitorder="little")
    m[:, :D // 8] = True
    return bits, m


def _result(R, B, D, ldx, ldbits, np_, plane0, residual, fp32_rows, bits, dyn):
    """The buffers' images: planes [max(np, 1)][3B][ldx] uint16, xs [3B][ldx] float32, xbits
    [B][ldbits] uint8, each with its mask; dyn [4] (every word is written or zero on entry)."""
    P = np.zeros((max(np_, 1), 3 * B, ldx), np.uint16)
    Pm = np.zeros(P.shape, bool)
    S = split_planes(R, 3)
    if np_ >= 1 and plane0:
        P[0, :, :D], Pm[0, :, :D] = S[0], True
    if np_ == 3 and residual:
        P[1:, :, :D], Pm[1:, :, :D] = S[1:], True
    xs = np.zeros((3 * B, ldx), np.float32)
    xm = np.zeros(xs.shape, bool)
    xs[fp32_rows, :D], xm[fp32_rows, :D] = R[fp32_rows], True
    xb, xbm = _lock_bits(R, B, D, ldbits)
    if not bits:
        xbm[:] = False
    return dict(planes=(P, Pm), xs=(xs, xm), xbits=(xb, xbm), dyn=np.asarray(dyn, np.int32))


def _flags(slot, inexact, not_binary):
    dyn = [0, 0, 0, 0]
    dyn[slot], dyn[2 + slot] = int(inexact), int(not_binary)
    return dyn


def inexact(R):
    """some value is not a bf16 value: a residual plane of the exact split is nonzero"""
    return bool((_bf16_value(split_planes(R, 1)[0]) != R).any())


def route0(X, B, D, ldx, ldbits, np_, f32mask, f32dyn_mask, slot, x_aligned=True):
    """launch_deinterleave on X [B][3 D]."""
    R = stacked_rows(X, B, D)
    f = form(D, ldx, x_aligned)
    rose = np_ >= 1 and inexact(R)           # (no plane image: nothing tests the values)
    grey = bool(((R != 0) & (R != 1)).any())
    rows = _rows(B, f32mask) | (_rows(B, f32dyn_mask) & (rose and np_ >= 1))
    out = _result(R, B, D, ldx, ldbits, np_, True, rose, rows, f == OCT, _flags(slot, rose, grey or f != OCT))
    out["form"] = f
    return out


def bits_route(X, B, D, ldx, ldbits, np_, f32dyn_mask, slot):
    """launch_deint_bits / launch_pairs_bits / launch_images_bits on the batch X [B][3 D] (np 1 or 3;
    D % 8 == 0): the bit operands are tests/bits_ref.py's; the grey pass runs for a batch with a value
    other than 0 / 1 and writes whole planes."""
    R = stacked_rows(X, B, D)
    grey = bool(((R != 0) & (R != 1)).any())
    rows = _rows(B, f32dyn_mask) & grey
    return _result(R, B, D, ldx, ldbits, np_, grey, grey, rows, True, _flags(slot, grey and inexact(R), grey))
