"""The conv tower's four per-pixel kernels (conv_tower.hip: conv1_fwd, lrn2_pool2_fwd, pool2_bwd,
conv1_wgrad) one at a time on caller buffers (mvae_debug_tower: the step's own launchers), each
against the float64 oracle (oracle/conv_oracle.py, pinned to torch.autograd by
tests/test_conv_oracle.py) applied to the same fp32 inputs, element by element.

Bounds. A sum of products in fp32 is held to 2e-6 * sum|terms| (the bar of test_conv2_kernel and
test_gemm_layouts; 26 fused multiply-adds are provably within 26 * 2^-24 = 1.55e-6 of it). The LRN
scale s^-beta comes from the native v_log_f32 / v_exp_f32: a relative 1e-5 on that factor (the
activation bar of test_gemm_epilogues, taken relative). Every term of an LRN gradient carries one
such factor, so those are held to (2e-6 + 1e-5) * sum|terms|. Each test prints its worst
error / bound (DESIGN.md §5m records them).

Argmax rule. Where the reference's window has an exact tie at its maximum, the first position is
required (ReLU zeros, identical pixels). Where another entry is below the maximum by no more than
the two value bounds (or is a ReLU zero whose pre-activation is within its bound of zero, so the
kernel may see a small positive there), either position is accepted and the value is checked at the
position the kernel chose. Such near-ties may be at most 1e-3 of a case's elements: asserted on the
reference's own numbers."""
import numpy as np
import pytest
import torch

from oracle import conv_oracle as CV
from tests.gpu_helpers import to_dev

pytestmark = pytest.mark.gpu

C = 64
SUM_TOL, POW_TOL, NEAR_CAP = 2e-6, 1e-5, 1e-3
SENT_F, SENT_B = -7777.0, 0xEE   # prefills: fp32 buffers, every byte of the others


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _tower(mode, S, n, ld, opt=0, in0=None, in1=None, xs=None, arg_in=None, out0=None, out1=None,
           outb=None, arg_out=None):
    from magic_amd import _lib
    lib = _lib.load()
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.mvae_debug_tower(mode, S, n, ld, opt, p(in0), p(in1), p(xs), p(arg_in), p(out0), p(out1),
                              p(outb), p(arg_out), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mvae_last_error(None)


def _bf16_bits(a):
    """round-to-nearest-even bf16 bit patterns of an fp32 array"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_val(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _windows(a):
    """[N, H, W, C] -> [N, H/2, W/2, 4, C], window position dy * 2 + dx (the oracle's maxpool order)"""
    N, H, W, Ch = a.shape
    return a.reshape(N, H // 2, 2, W // 2, 2, Ch).transpose(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, Ch)


def _lrn_tol(a):
    """bound of the kernel's lrn(a) given exact fp32 a: the relative POW_TOL on s^-beta, plus the
    fp32 window sum (SUM_TOL of its terms) carried through d(a s^-beta)/ds"""
    s = CV.lrn_scale(a)
    return POW_TOL * np.abs(CV.lrn(a)) + SUM_TOL * (s - CV.LRN_BIAS) * CV.LRN_BETA * np.abs(a) * s ** (-CV.LRN_BETA - 1)


def _lrn_in_tol(a, ta):
    """first-order bound of lrn(a)'s change when a_j moves by at most ta_j"""
    s = CV.lrn_scale(a)
    cross = 2 * CV.LRN_ALPHA * CV.LRN_BETA * np.abs(a) * s ** (-CV.LRN_BETA - 1) * CV._window_sum(np.abs(a) * ta)
    return ta * s ** -CV.LRN_BETA + cross


def _check_argmax(v, tol, soft, karg, what):
    """The argmax rule of the module docstring. v, tol, soft: [N, H2, W2, 4, C] reference values,
    value bounds and the may-be-positive-in-fp32 ReLU zeros; karg [N, H2, W2, C] the kernel's
    positions. Returns (reference value, bound) at the kernel's positions and the near-tie share."""
    ref_arg = v.argmax(axis=3)
    m = np.take_along_axis(v, ref_arg[:, :, :, None, :], 3)
    tol_m = np.take_along_axis(tol, ref_arg[:, :, :, None, :], 3)
    gap = m - v
    near = ((gap > 0) | soft) & (gap <= tol + tol_m)
    share = near.any(axis=3).mean()
    assert share <= NEAR_CAP, (what, "near-tie share", share)
    assert karg.max() <= 3
    k = karg.astype(np.int64)[:, :, :, None, :]
    ok = (karg == ref_arg) | np.take_along_axis(near, k, 3)[:, :, :, 0]
    assert ok.all(), (what, "argmax", int((~ok).sum()), np.argwhere(~ok)[:4].tolist())
    moved = float((karg != ref_arg).mean())
    return np.take_along_axis(v, k, 3)[:, :, :, 0], np.take_along_axis(tol, k, 3)[:, :, :, 0], share, moved


def _ratio(got, ref, bound, what):
    """max |got - ref| / bound over the elements; an element with a zero bound must be exact"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), (what, "not finite", int((~np.isfinite(got)).sum()))
    err = np.abs(got - ref)
    assert np.all(err[bound == 0] == 0), (what, "exact zeros")
    r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    return r


def _sparse(rng, shape, keep=0.3, dead_pixels=0.25):
    """about `keep` non-zero entries, and whole pixels (all 64 channels) of zeros: the kernels'
    __ballot skip"""
    g = np.where(rng.random(shape) < keep, rng.standard_normal(shape), 0.0)
    g = g * (rng.random(shape[:-1] + (1,)) >= dead_pixels)
    return (g + 0.0).astype(np.float32)


def _pixels(rng, n, S, ld, grey):
    """[n][ld] pixel rows: binary or k/255 foreground; the padding holds NaN (never read)"""
    x = (rng.random((n, S * S)) < (0.5 if grey else 0.3)).astype(np.float32)
    if grey:
        x *= (rng.integers(1, 256, size=x.shape) / 255.0).astype(np.float32)
    buf = np.full((n, ld), np.nan, np.float32)
    buf[:, :S * S] = x
    return x, buf


def _w1(rng):
    return (rng.standard_normal((26, C)) * 0.2).astype(np.float32)


# ------------------------------------------------------------------ mode 0: conv1 + pool 1 + LRN 1
@pytest.mark.parametrize("S,B,grey", [(4, 3, False), (8, 2, True), (12, 3, False), (12, 1, True),
                                      (68, 1, True), (100, 1, False), (100, 2, True)])
def test_conv1_fwd(S, B, grey):
    """conv1_fwd_kernel: S = 4, 8 (images smaller than / as large as the staged 6-row patch needs
    zero borders on every side), 12, 68 (34 pooled columns: waves take 9, 9, 8, 8), 100 (the benched
    size: one 50-column segment). Both n1 images are requested at once."""
    rng = np.random.default_rng(S * 7 + B + 100 * grey)
    n, S1, ldx = 3 * B, S // 2, S * S + 8
    x, xbuf = _pixels(rng, n, S, ldx, grey)
    w = _w1(rng)
    shape = (n, S1, S1, C)
    p1, n1 = _full(shape, SENT_F, torch.float32), _full(shape, SENT_F, torch.float32)
    n1b, arg1 = _full(shape, 0, torch.int16), _full(shape, SENT_B, torch.uint8)
    _tower(0, S, n, ldx, in0=to_dev(xbuf), in1=to_dev(w), out0=p1, out1=n1, outb=n1b, arg_out=arg1)
    p1, n1, n1b, arg1 = p1.cpu().numpy(), n1.cpu().numpy(), _u16(n1b), arg1.cpu().numpy()

    x4 = x.astype(np.float64).reshape(n, S, S, 1)
    W, b = w[:25].astype(np.float64), w[25].astype(np.float64)
    z = _windows(CV.conv(x4, W, b))
    tol = SUM_TOL * _windows(CV.conv(np.abs(x4), np.abs(W), np.abs(b)))
    v = np.maximum(z, 0)
    p_ref, p_tol, share, moved = _check_argmax(v, tol, (z <= 0) & (z >= -tol), arg1, "arg1")
    r_p = _ratio(p1, p_ref, p_tol, "p1")
    n_ref = CV.lrn(p_ref)
    n_tol = _lrn_tol(p_ref) + _lrn_in_tol(p_ref, p_tol)
    r_n = _ratio(n1, n_ref, n_tol, "n1")
    print(f"conv1_fwd S={S} B={B} grey={grey}: p1 err/bound={r_p:.3f} n1 err/bound={r_n:.3f} "
          f"near-tie share={share:.2e} moved={moved:.2e} zero windows={float((v.max(3) == 0).mean()):.3f}")
    assert r_p <= 1, r_p
    assert r_n <= 1, r_n
    # the LRN window is clipped at the channel ends: lanes 0-4 and 59-63, against the clipped sum
    for sl in (slice(0, 5), slice(59, 64)):
        assert np.all(np.abs(n1[..., sl] - n_ref[..., sl]) <= n_tol[..., sl]), sl
    np.testing.assert_array_equal(n1b, _bf16_bits(n1))
    assert (v.max(3) == 0).any() and len(np.unique(arg1)) == 4   # ties on zeros and every position occur


# ------------------------------------------------------------------ mode 1: LRN 2 + pool 2
def _relu_maps(rng, n, S1, dup=0.3):
    """post-ReLU activations [n, S1, S1, 64] (exact zeros); in about `dup` of the 2x2 windows a
    later pixel repeats an earlier one in all 64 channels: an exact tie at a positive maximum"""
    a = np.maximum(rng.standard_normal((n, S1, S1, C)) * 1.5, 0).astype(np.float32)
    w = _windows(a).copy()
    pick = rng.random(w.shape[:3]) < dup
    src, dst = rng.integers(0, 3, size=w.shape[:3]), rng.integers(1, 4, size=w.shape[:3])
    for s in range(3):
        for d in range(s + 1, 4):
            sel = pick & (src == s) & (dst == d)
            w[sel, d] = w[sel, s]
    S2 = S1 // 2
    return np.ascontiguousarray(
        w.reshape(n, S2, S2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(n, S1, S1, C))


_POOL2_CASES = [(2, 3), (6, 1), (10, 2), (34, 1), (50, 3)]


@pytest.mark.parametrize("f32,planes", [(1, 0), (1, 1), (1, 3), (0, 1), (0, 3)])
@pytest.mark.parametrize("S1,nimg", _POOL2_CASES)
def test_lrn2_pool2_fwd(S1, nimg, f32, planes):
    """lrn2_pool2_fwd_kernel, two pooled pixels per wave, four waves per workgroup. Pooled pixels
    NP = nimg S2^2: (2, 3) NP 3, (6, 1) NP 9, (34, 1) NP 289, (50, 3) NP 1875 are odd (the last
    wave's second pixel is the tail duplicate); waves ceil(NP / 2) = 2, 5, 25 (S1 = 10, nimg 2), 145,
    938 all leave the last workgroup with idle waves. Every output combination of the step:
    fp32 only (f32 / f32x's fp32 image), fp32 + 1 or 3 bf16 planes, planes alone. The row stride is
    wider than a row: the padding, and every buffer the flags leave unrequested, keep the prefill."""
    rng = np.random.default_rng(S1 * 3 + nimg)
    S2 = S1 // 2
    F, ldf = S2 * S2 * C, S2 * S2 * C + 24
    a2 = _relu_maps(rng, nimg, S1)
    xf = _full((nimg, ldf), SENT_F, torch.float32)
    xfp = _full((3, nimg, ldf), 0, torch.int16)
    xfp.view(torch.uint8).fill_(SENT_B)
    arg2 = _full((nimg, S2, S2, C), SENT_B, torch.uint8)
    _tower(1, 2 * S1, nimg, ldf, opt=f32 | (planes << 1), in0=to_dev(a2), out0=xf, outb=xfp, arg_out=arg2)
    xf, xfp, arg2 = xf.cpu().numpy(), _u16(xfp), arg2.cpu().numpy()
    sent_h = SENT_B * 0x101

    a = a2.astype(np.float64)
    v, tol = _windows(CV.lrn(a)), _windows(_lrn_tol(a))
    ref, bound, share, moved = _check_argmax(v, tol, np.zeros(v.shape, bool), arg2, "arg2")
    ref, bound = ref.reshape(nimg, F), bound.reshape(nimg, F)
    ties = int(((v == v.max(3, keepdims=True)).sum(3) > 1)[v.max(3) > 0].sum())
    if S1 >= 6:   # exact ties at a positive maximum, and on zeros
        assert ties > 0 and (v.max(3) == 0).any()

    assert np.all(xf[:, F:] == SENT_F) and np.all(xfp[:, :, F:] == sent_h) and np.all(xfp[planes:] == sent_h)
    if f32:
        val = xf[:, :F]
    else:
        assert np.all(xf == SENT_F)
        val = None
    if planes == 3:
        tot = _bf16_val(xfp[:, :, :F]).sum(0)   # three bf16 values: exact in float64
        if val is not None:
            np.testing.assert_array_equal(tot, val.astype(np.float64))
        else:
            assert np.all(tot == tot.astype(np.float32))
            val = tot.astype(np.float32)
        np.testing.assert_array_equal(xfp[0, :, :F], _bf16_bits(val))   # plane 0 leads the split
    r = None
    if val is not None:
        r = _ratio(val, ref, bound, "xf")
        assert r <= 1, r
        if planes == 1:
            np.testing.assert_array_equal(xfp[0, :, :F], _bf16_bits(val))
    else:   # one plane alone: the RNE image of a value within the bound (half a bf16 ulp more)
        got = _bf16_val(xfp[0, :, :F])
        assert np.all(np.abs(got - ref) <= bound + 2.0 ** -8 * np.abs(ref) * (1 + 1e-4))
    print(f"lrn2_pool2 S1={S1} nimg={nimg} f32={f32} planes={planes}: err/bound={r} "
          f"near-tie share={share:.2e} moved={moved:.2e} positive ties={ties}")


def test_lrn2_pool2_one_plane_is_rne_of_fp32():
    """The single bf16 plane written without the fp32 image equals the RNE bf16 of the fp32 image a
    second launch writes (the kernel is deterministic), bit for bit."""
    rng = np.random.default_rng(5)
    S1, nimg = 10, 3
    S2 = S1 // 2
    ldf = S2 * S2 * C + 8
    a2 = to_dev(_relu_maps(rng, nimg, S1))
    xf = _full((nimg, ldf), SENT_F, torch.float32)
    xfp = _full((1, nimg, ldf), 0, torch.int16)
    arg_a, arg_b = (_full((nimg, S2, S2, C), SENT_B, torch.uint8) for _ in range(2))
    _tower(1, 2 * S1, nimg, ldf, opt=1, in0=a2, out0=xf, arg_out=arg_a)
    _tower(1, 2 * S1, nimg, ldf, opt=1 << 1, in0=a2, outb=xfp, arg_out=arg_b)
    F = S2 * S2 * C
    np.testing.assert_array_equal(_u16(xfp)[0, :, :F], _bf16_bits(xf.cpu().numpy()[:, :F]))
    assert torch.equal(arg_a, arg_b)


# ------------------------------------------------------------------ mode 2: pool 2 + LRN 2 + ReLU backward
@pytest.mark.parametrize("S1,B", [(2, 2), (6, 1), (10, 2), (34, 1), (50, 2), (50, 1)])
def test_pool2_bwd(S1, B):
    """pool2_bwd_kernel, four (backward image, pooled pixel) pairs per wave: 4B S2^2 = 8, 36, 200,
    1156, 5000, 2500 pairs (S1 = 2: two waves; 6: nine waves, the last workgroup one wave). B = 2
    has two images in each of the four backward row groups, forward image j < 2B ? j : j - B; arg2
    is the test's own, every position present. Off the argmax and on dead pixels the result is an
    exact zero; da2b is the RNE bf16 image of da2."""
    rng = np.random.default_rng(S1 * 5 + B)
    S2 = S1 // 2
    F, ldf = S2 * S2 * C, S2 * S2 * C + 40
    a2 = _relu_maps(rng, 3 * B, S1, dup=0)
    arg2 = rng.integers(0, 4, size=(3 * B, S2, S2, C)).astype(np.uint8)
    g = _sparse(rng, (4 * B, S2, S2, C))
    g[0, 0, 0] = g[-1, -1, -1] = 0   # a dead pooled pixel in the first and the last wave, at any size
    dxf = np.full((4 * B, ldf), np.nan, np.float32)
    dxf[:, :F] = g.reshape(4 * B, F)
    da2 = _full((4 * B, S1, S1, C), SENT_F, torch.float32)
    da2b = _full((4 * B, S1, S1, C), 0, torch.int16)
    _tower(2, 2 * S1, B, ldf, in0=to_dev(dxf), in1=to_dev(a2), arg_in=to_dev(arg2), out0=da2, outb=da2b)
    da2, da2b = da2.cpu().numpy(), _u16(da2b)

    fwd = np.array([j if j < 2 * B else j - B for j in range(4 * B)])
    a = a2.astype(np.float64)[fwd]
    dn = CV.unpool(g.astype(np.float64), arg2.astype(np.int64)[fwd], a.shape)
    ref = CV.lrn_bwd(a, dn) * (a > 0)
    bound = (SUM_TOL + POW_TOL) * CV.lrn_bwd(a, dn, np.abs) * (a > 0)
    r = _ratio(da2, ref, bound, "da2")
    print(f"pool2_bwd S1={S1} B={B}: err/bound={r:.3f} exact zeros={float((bound == 0).mean()):.3f}")
    assert r <= 1, r
    np.testing.assert_array_equal(da2b, _bf16_bits(da2))
    assert len(np.unique(arg2)) == 4 and (bound == 0).mean() > 0.5
    dead = ~dn.any(axis=-1)   # pixels no channel routes a gradient to
    assert dead.any() and np.all(da2[dead] == 0)


def test_pool2_bwd_single_outputs():
    """fp32 alone (f32 / f32x) and bf16 alone (bf16 mode) equal the two written together."""
    rng = np.random.default_rng(11)
    S1, B = 6, 2
    S2 = S1 // 2
    F = S2 * S2 * C
    ins = dict(in0=to_dev(_sparse(rng, (4 * B, F))), in1=to_dev(_relu_maps(rng, 3 * B, S1, dup=0)),
               arg_in=to_dev(rng.integers(0, 4, size=(3 * B, F)).astype(np.uint8)))
    shape = (4 * B, S1, S1, C)
    both = _full(shape, SENT_F, torch.float32), _full(shape, 0, torch.int16)
    f_only, h_only = _full(shape, SENT_F, torch.float32), _full(shape, 0, torch.int16)
    _tower(2, 2 * S1, B, F, out0=both[0], outb=both[1], **ins)
    _tower(2, 2 * S1, B, F, out0=f_only, **ins)
    _tower(2, 2 * S1, B, F, outb=h_only, **ins)
    assert torch.equal(both[0].view(torch.int32), f_only.view(torch.int32))
    assert torch.equal(both[1], h_only)


# ------------------------------------------------------------------ mode 3: conv1 weight gradient
@pytest.mark.parametrize("S,B,chunks,grey", [(4, 3, 0, False), (12, 3, 4, True), (12, 5, 4, False),
                                             (64, 2, 0, True), (68, 2, 3, False), (68, 1, 0, True),
                                             (100, 1, 1, False), (100, 2, 3, True)])
def test_conv1_wgrad(S, B, chunks, grey):
    """conv1_wgrad_kernel walks (image, pooled row, 32-column segment) with the next segment
    prefetched. Segments: S = 4, 12 one short segment (2 / 6 columns); 64 exactly one of 32; 68 a
    second of 2 columns (nq < 4: two waves idle); 100 a second of 18. Chunks (ipc = ceil(2B / n)):
      (4, 3, 0)    n = 6, ipc 1                       (64, 2, 0)   n = 4, ipc 1
      (12, 3, 4)   ipc 2: 2, 2, 2 images, one empty   (68, 2, 3)   ipc 2: 2, 2 images, one empty
      (12, 5, 4)   ipc 3: 3, 3, 3 and a last of 1     (68, 1, 0)   n = 2, ipc 1
      (100, 1, 1)  ipc 2: the prefetch crosses from an image's last 18-column segment to the next image
      (100, 2, 3)  ipc 2, one empty chunk
    The debug entry prefills the slab with NaN bits (an empty chunk must write zeros). Run twice:
    bitwise equal."""
    rng = np.random.default_rng(S * 13 + B + chunks)
    S1, ldx = S // 2, S * S + 8
    x, xbuf = _pixels(rng, 3 * B, S, ldx, grey)
    p1 = np.maximum(rng.standard_normal((3 * B, S1, S1, C)) * 1.5, 0).astype(np.float32)
    arg1 = rng.integers(0, 4, size=p1.shape).astype(np.uint8)
    dn1 = _sparse(rng, (4 * B, S1, S1, C))
    ins = dict(in0=to_dev(dn1), in1=to_dev(p1), xs=to_dev(xbuf), arg_in=to_dev(arg1))
    outs = []
    for _ in range(2):
        g1, g2 = _full((26, C), SENT_F, torch.float32), _full((26, C), SENT_F, torch.float32)
        _tower(3, S, B, ldx, opt=chunks, out0=g1, out1=g2, **ins)
        outs.append(np.stack([g1.cpu().numpy(), g2.cpu().numpy()]))
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))

    pf, af = p1.astype(np.float64), arg1.astype(np.int64)
    worst = 0.0
    for grp in range(2):
        ref, mag = np.zeros((26, C)), np.zeros((26, C))
        for r in range(2 * B):
            j = 2 * B * grp + r
            f = j if j < 2 * B else j - B
            a, d = pf[f:f + 1], dn1[j:j + 1].astype(np.float64)
            cols = CV.im2col(x[f].astype(np.float64).reshape(1, S, S, 1)).reshape(-1, 25)
            for acc, A in ((ref, lambda t: t), (mag, np.abs)):
                d1 = CV.unpool(CV.lrn_bwd(a, d, A) * (a > 0), af[f:f + 1], (1, S, S, C)).reshape(-1, C)
                acc[:25] += cols.T @ d1
                acc[25] += d1.sum(0)
        worst = max(worst, _ratio(outs[0][grp], ref, (SUM_TOL + POW_TOL) * mag, f"g{grp + 1}"))
    print(f"conv1_wgrad S={S} B={B} chunks={chunks} grey={grey}: err/bound={worst:.3f}")
    assert worst <= 1, worst
    assert len(np.unique(arg1)) == 4 and (p1 == 0).any()
