"""The GEMM epilogues of the step (gemm_common.h: EPI_BCE / EPI_BCEB, EPI_DACT / EPI_DACTB, EPI_ACT)
restated in float64 numpy from the kernel's own inputs. tests/test_epi_ref.py pins this restatement
to the oracle and to float64 torch autograd; tests/test_gpu_bce.py holds the kernels to it per
element.

Every function returns, next to each output, its magnitude ``mag`` in the project's convention (the
sum of the absolute values of the terms, taken down to the inputs: tests/head_ref.py); the fp32 bar
is ``|gpu - ref| <= 2e-6 * mag``, and a zero mag demands exactness.

The BCE head: v = A B, y = 1 / (1 + exp(-v)), the per-pixel term x log y + (1 - x) log(1 - y) with
each product taken as 0 where its factor is 0 (TF pow(0, 0) = 1, no epsilon), rowpart[r][b] = -sum of
the terms over the columns of 128-column block b, dU = (y - x) scale.

  mag(term) = |x log y| + |(1 - x) log1p(-y)| + |x - y| magv + x + (1 - x) / (1 - y)

|x - y| magv is the logit's error propagated (d term / d v = x - y). The last two exist because an
fp32 y near 1 is rounded to an absolute 2^-24: log(1 - y) sees that divided by 1 - y and log y sees
it at unit scale; any fp32 form of the formula inherits that. (Products with a zero factor are 0
here too.)

Saturation (``sat=True``): what fp32 does where y leaves (0, 1). 1 + exp(-v) rounds to 1 once
exp(-v) < 2^-24 (v > 16.7), and exp(-v) overflows fp32 for v < -88.8, where the reciprocal is 0; in
between, down to v = -88, y = exp(v) is an ordinary fp32 number (9.4e-14 at v = -30), NOT 0. The
reference then takes y = 1 for v >= 20 and y = 0 for v <= -95 and refuses logits in the bands where
the rounding depends on the implementation (12 < |v| < 20, -95 < v < -80). A term is -inf exactly
where a nonzero factor meets log 0.
"""
from __future__ import annotations

import numpy as np

f64 = lambda a: np.asarray(a, np.float64)
BLK = 128


def nblk(N):
    return (N + BLK - 1) // BLK


def logits(A, B):
    """v = A B and magv = |A| |B| (A [M][K], B [K][N])"""
    A, B = f64(A), f64(B)
    return A @ B, np.abs(A) @ np.abs(B)


def sigmoid(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-f64(v)))


def check_accuracy_logits(v):
    """accuracy cases keep every |logit| <= 8 (at 14.5 a dropped column no longer shows: the last
    two mag terms grow with 1 / (1 - y))"""
    assert np.abs(v).max() <= 8.0, np.abs(v).max()


def check_saturation_logits(v):
    a = np.abs(v)
    assert not ((a > 12) & (a < 20)).any() and not ((v > -95) & (v < -80)).any()


def _prod0(f, g):
    """f g with the product 0 where f is 0 (g may be -inf or nan there)"""
    with np.errstate(invalid="ignore"):
        return np.where(f != 0, f * np.where(f != 0, g, 0.0), 0.0)


def block_sums(t):
    """[M][N] -> [M][nblk]: sums over the columns of each 128-column block"""
    M, N = t.shape
    return np.stack([t[:, b * BLK:min((b + 1) * BLK, N)].sum(1) for b in range(nblk(N))], 1)


def bce(A, B, x, scale, sat=False):
    """The BCE head on A [M][K], B [K][N], target x [M][N] (columns beyond N already cut)."""
    v, magv = logits(A, B)
    x = f64(x)
    y = sigmoid(v)
    if sat:
        check_saturation_logits(v)
        y = np.where(v >= 20, 1.0, np.where(v <= -95, 0.0, y))
    with np.errstate(divide="ignore", invalid="ignore"):
        l1, l0 = np.log(y), np.log1p(-y)
        t1, t0 = _prod0(x, l1), _prod0(1 - x, l0)
        term = t1 + t0
        term_mag = np.abs(t1) + np.abs(t0) + np.abs(x - y) * magv + x + _prod0(1 - x, 1.0 / (1 - y))
    with np.errstate(invalid="ignore"):
        rowpart, rowpart_mag = -block_sums(term), block_sums(term_mag)
    return dict(v=v, magv=magv, y=y, y_mag=y * (1 - y) * magv + y, term=term, term_mag=term_mag,
                rowpart=rowpart, rowpart_mag=rowpart_mag, du=(y - x) * scale,
                du_mag=(y * (1 - y) * magv + y + np.abs(x)) * scale)


def act(A, B, kind):
    """EPI_ACT: act(v) with mag = act'(v) magv + |act(v)|; kind 0 tanh, 1 elu (TF: exp(v) - 1, v < 0)"""
    v, magv = logits(A, B)
    if kind == 0:
        out = np.tanh(v)
        d = 1 - out * out
    else:
        out = np.where(v < 0, np.expm1(np.minimum(v, 0)), v)
        d = np.where(v < 0, np.exp(np.minimum(v, 0)), 1.0)
    return dict(out=out, mag=d * magv + np.abs(out), v=v, magv=magv)


def remap_rows(M, remap_split, remap_shift):
    """aux row of output row r (GemmEpi::remap_split / remap_shift)"""
    r = np.arange(M)
    return np.where(r >= remap_split, r - remap_shift, r)


def dact(A, B, aux, kind, remap_split=0, remap_shift=0):
    """EPI_DACT: v act'(aux[remap(r)]) in terms of the activation OUTPUT aux (TF TanhGrad / EluGrad);
    mag = magv (1 + aux^2) with tanh, magv (1 + |aux|) with elu"""
    v, magv = logits(A, B)
    a = f64(aux)[remap_rows(v.shape[0], remap_split, remap_shift)][:, :v.shape[1]]
    if kind == 0:
        return dict(out=v * (1 - a * a), mag=magv * (1 + a * a))
    return dict(out=np.where(a < 0, v * (a + 1), v), mag=magv * (1 + np.abs(a)))


def pack_bits(x):
    """xbits of a target [M][N]: byte c of a row = columns 8c .. 8c + 7, bit j = column 8c + j nonzero
    (include/mvae.h); [M][ceil(N / 8)] uint8, the bits past N zero"""
    nz = np.asarray(x) != 0
    M, N = nz.shape
    pad = np.zeros((M, (N + 7) // 8 * 8), bool)
    pad[:, :N] = nz
    return np.packbits(pad.reshape(M, -1, 8), axis=2, bitorder="little")[:, :, 0]


def bf16_rne_bits(v32):
    """fp32 (finite or inf) -> bf16 bits, round to nearest even"""
    u = np.ascontiguousarray(v32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def split_planes(v32, n):
    """the RNE plane split of an fp32 array: plane t = bf16(residual), residual -= plane (fp32,
    exact); n = 1 round to nearest, n = 3 the exact split. [n][...] uint16"""
    r = np.ascontiguousarray(v32, np.float32).copy()
    out = []
    for _ in range(n):
        b = bf16_rne_bits(r)
        out.append(b)
        with np.errstate(invalid="ignore"):   # (inf - inf: the residual of an inf is not used)
            r = (r - bf16_to_f32(b)).astype(np.float32)
    return np.stack(out)


def bce_fp32_emulation(A, B, x, scale):
    """A plain fp32 form of the head (k-ordered fp32 accumulation, fp32 exp / log, the two-log term
    with its selects, the columns of a block summed in order): what any straightforward fp32 kernel
    computes. It sizes the bar; it is not the kernel's order of operations."""
    f = np.float32
    A, B, x = np.asarray(A, f), np.asarray(B, f), np.asarray(x, f)
    v = np.zeros((A.shape[0], B.shape[1]), f)
    for k in range(A.shape[1]):
        v = (v + A[:, k:k + 1] * B[k:k + 1, :]).astype(f)
    y = (f(1) / (f(1) + np.exp(-v, dtype=f))).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        l1, l0 = np.log(y, dtype=f), np.log((f(1) - y).astype(f), dtype=f)
        term = (np.where(x != 0, x * l1, f(0)).astype(f) + np.where(x != 1, (f(1) - x) * l0, f(0)).astype(f)).astype(f)
    rp = np.zeros((A.shape[0], nblk(B.shape[1])), f)
    for c in range(B.shape[1]):
        rp[:, c // BLK] = (rp[:, c // BLK] + term[:, c]).astype(f)
    return dict(y=y, term=term, rowpart=-rp, du=((y - x) * f(scale)).astype(f))
