"""The latent head's kernels (mvae_kernels.hip: latent_fwd, colstats_part / colstats_final, metric,
loss_reduce, latent_bwd) one at a time on caller buffers (mvae_debug_head: the step's own launchers),
each output element against tests/head_ref.py (float64, pinned to torch.autograd and the oracle by
tests/test_head_ref.py) computed from the kernel's OWN inputs: the column statistics from the fp32
z they read, the metric from the fp32 colsq it read, and so on, so one kernel's error never excuses
the next.

Bound: |gpu - ref| <= 2e-6 * mag, mag the sum of |terms| head_ref.py returns next to every output
(zero mag: the output must be exact). Inputs keep s in [-8, 4], where the fp32 product s log2(e) / 2
and v_exp_f32 / __expf / rsqrt stay well inside that bar. Every test prints its worst error / bound
(DESIGN.md 5n records them).

Buffers are prefilled with NaN bit patterns (fp32 0x7FC12345, bf16 planes 0x7FC1) and carry a guard
row behind the last one; everything a kernel does not own must come back bit-identical: pad columns,
the rot rows of z, rows the zmask deselects, rows >= B.

Dead columns (cosine): lock column 0 and key column 3 exactly zero, lock column 1 and key column 2
tiny (B z^2 ~ 1e-13 < L2_EPS), whenever L >= 6; asserted on the reference: no column's sum of squares
lies within 1e-3 relative of L2_EPS, so the branch is unambiguous."""
import ctypes

import numpy as np
import pytest
import torch

from magic_amd import _lib
from oracle import philox_oracle as PH
from tests import head_ref as H

pytestmark = pytest.mark.gpu

TOL = 2e-6
NAN32, NAN16 = 0x7FC12345, 0x7FC1
EPS_BAR = 1e-3          # the sampler's structural bar (tests/test_gpu_sampler.py)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    for k in sorted(WORST):
        print(f"head worst error / bound: {k} = {WORST[k]:.3f}")


def round8(n):
    return (n + 7) & ~7


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def nan32(*shape):
    return torch.full(shape, NAN32, dtype=torch.int32, device="cuda")


def nan16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device="cuda")


def bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a.view(np.uint32)


def f32(t):
    return t.cpu().numpy().view(np.float32)


def head(mode, **kw):
    lib = _lib.load()
    a = _lib.mvae_head_args()
    a.mode = mode
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    rc = lib.mvae_debug_head(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, lib.mvae_last_error(None))


def ratio(got, ref, mag, kernel, what, abs_=0.0):
    """max |got - ref| / (TOL mag + abs_) over the elements; an element with a zero bound must be exact"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (what, "not finite", int((~np.isfinite(got)).sum()))
    err, bound = np.abs(got - ref), TOL * np.asarray(mag, np.float64) + abs_
    assert np.all(err[bound == 0] == 0), (what, "inexact at a zero bound")
    r = float((err / np.where(bound == 0, 1.0, bound)).max()) if err.size else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    return r


def check(got, ref, mag, kernel, what, abs_=0.0):
    r = ratio(got, ref, mag, kernel, what, abs_)
    print(f"{kernel} {what}: worst error / bound {r:.3f}")
    assert r <= 1.0, (kernel, what, r)


def untouched(t, owned, what):
    """every element outside the boolean mask `owned` still holds the prefill"""
    b = bits(t)
    pat = NAN16 if b.dtype == np.uint16 else NAN32
    bad = (b != pat) & ~owned
    assert not bad.any(), (what, "written outside what the kernel owns", np.argwhere(bad)[:4].tolist())
    assert (b[owned] != pat).all(), (what, "an owned element still holds the prefill")


def tiny(B):
    return np.sqrt(1e-13 / B)


def dead_ok(cs):
    cs = np.asarray(cs, np.float64)
    assert not (np.abs(cs - H.L2_EPS) <= 1e-3 * H.L2_EPS).any()


# ------------------------------------------------------------------------- inputs
def make_ms(B, L, seed, dead=True, recip=False):
    """ms [3B][2L] and eps [3][B][L] (fp32); dead: the module docstring's columns (mu as given, eps 0).
    recip: the correlated family (key mu = lock mu + 0.1 noise, |mu| >= 0.5, s in [-8, -4])."""
    rng = np.random.default_rng(seed)
    ms = rng.standard_normal((3, B, 2 * L))
    ms[:, :, L:] = rng.uniform(-8, 4, (3, B, L))
    eps = rng.standard_normal((3, B, L))
    if recip:
        base = rng.uniform(0.5, 1.5, (B, L)) * rng.choice([-1.0, 1.0], (B, L))
        ms[1, :, :L] = base
        ms[2, :, :L] = base + 0.1 * rng.standard_normal((B, L))
        ms[:, :, L:] = rng.uniform(-8, -4, (3, B, L))
    if dead and L >= 6:
        sg = np.sign(ms[1, :, :L]) if recip else rng.choice([-1.0, 1.0], (B, L))
        t = tiny(B) * rng.uniform(0.5, 1.0, B)
        ms[1, :, 0], ms[1, :, 1], ms[2, :, 2], ms[2, :, 3] = 0.0, sg[:, 1] * t, sg[:, 2] * t, 0.0
        if recip:
            ms[2, :, 1], ms[1, :, 2] = sg[:, 1] * np.abs(ms[2, :, 1]), sg[:, 2] * np.abs(ms[1, :, 2])
        eps[0, :, :2] = 0.0
        eps[2, :, 2:4] = 0.0
    return ms.reshape(3 * B, 2 * L).astype(np.float32), eps.astype(np.float32)


def make_z(B, L, ldz, seed, recip=False):
    """an fp32 z buffer [3B][ldz] (pad columns NaN) with the dead columns, and its lock / key rows"""
    ms, eps = make_ms(B, L, seed, recip=recip)
    z = H.reparam(ms, eps, B, L)["z"].astype(np.float32)
    buf = np.full((3 * B, ldz), np.nan, np.float32)
    buf[:, :L] = z.reshape(3 * B, L)
    return buf, z[1], z[2]


# ------------------------------------------------------------------------- latent_fwd
FWD_FORMS = [(zm, n) for zm in (0, 2, 6) for n in (0, 1, 3)]


def run_fwd(ms_d, B, L, ldz, zmask, n, eps_d=None, **regen):
    z, rf = nan32(3 * B + 1, ldz), nan32(B + 1, 4)
    # (planes of the step's stride 3B ldz: a contiguous [n][3B][ldz] image, so the guard is a tail)
    zp = nan16(max(n, 1) * 3 * B * ldz + ldz)
    head(_lib.HEAD_FWD, B=B, L=L, Bg=regen.get("Bg", B), ldz=ldz, zmask=zmask, z_planes=n, ms=ms_d, eps=eps_d,
         z=z, zp=zp if n else None, rowfwd=rf, off=regen.get("off", 0), seed=regen.get("seed", 0),
         counter=regen.get("counter", 0))
    return z, zp, rf


def check_fwd(ref, B, L, ldz, zmask, n, out, zfull, what):
    z, zp, rf = out
    zb, own = f32(z), np.zeros((3 * B + 1, ldz), bool)
    for bit, blk in ((2, 1), (4, 2)):
        if zmask & bit:
            own[blk * B:(blk + 1) * B, :L] = True
            check(zb[blk * B:(blk + 1) * B, :L], ref["z"][blk], ref["z_mag"][blk], "latent_fwd", what + f" z[{blk}]")
    untouched(z, own, what + " z")
    r = f32(rf)
    check(r[:B, :3], ref["rowfwd"], ref["rowfwd_mag"], "latent_fwd", what + " rowfwd")
    assert np.all(bits(rf)[:B, 3] == 0), what
    rown = np.zeros((B + 1, 4), bool)
    rown[:B] = True
    untouched(rf, rown, what + " rowfwd")
    pb = bits(zp)
    pown = np.zeros(pb.shape, bool)
    if n:
        img = pb[:n * 3 * B * ldz].reshape(n, 3 * B, ldz)
        want = H.planes(zfull[B:2 * B, :L], n)      # the split of the kernel's own fp32 lock rows
        assert np.array_equal(img[:, B:2 * B, :L], want), (what, "planes")
        po = np.zeros((n, 3 * B, ldz), bool)
        po[:, B:2 * B, :L] = True
        pown[:n * 3 * B * ldz] = po.reshape(-1)
    untouched(zp, pown, what + " planes")


@pytest.mark.parametrize("L", [1, 2, 5, 6, 20, 63, 64, 100, 1020, 1024, 1028, 2000])
def test_latent_fwd(L):
    """scalar form (L % 4), the 4-wide one-wave form to its limit (1020), the four-wave form with
    exactly one pass (1024), a one-quad second pass (1028) and C5's ragged row (2000)"""
    for B in (1, 3, 4, 5, 130):
        ms, eps = make_ms(B, L, 100 * L + B)
        ref = H.latent_fwd(ms, eps, B, L)
        ms_d, eps_d = dev(ms), dev(eps)
        ld0 = round8(L + 1)
        full = run_fwd(ms_d, B, L, ld0, 6, 3, eps_d)
        again = run_fwd(ms_d, B, L, ld0, 6, 3, eps_d)
        for a, b in zip(full, again):
            assert torch.equal(a, b), "two launches differ"
        for ldz, forms in ((ld0, FWD_FORMS), (ld0 + 8, [(6, 3), (0, 1), (2, 0)])):
            zfull = f32(run_fwd(ms_d, B, L, ldz, 6, 0, eps_d)[0])
            for zmask, n in forms:
                out = run_fwd(ms_d, B, L, ldz, zmask, n, eps_d)
                check_fwd(ref, B, L, ldz, zmask, n, out, zfull, f"B={B} L={L} ldz={ldz} zmask={zmask} np={n}")


def test_latent_fwd_odd_stride_takes_scalar_form():
    """L = 8 at a stride of 9 (and of 16: the 4-wide form) give the same bits"""
    B, L = 5, 8
    ms, eps = make_ms(B, L, 7)
    ref = H.latent_fwd(ms, eps, B, L)
    ms_d, eps_d = dev(ms), dev(eps)
    outs = {}
    for ldz in (9, 16):
        zfull = f32(run_fwd(ms_d, B, L, ldz, 6, 0, eps_d)[0])
        for zmask, n in ((6, 3), (2, 1), (0, 3)):
            out = run_fwd(ms_d, B, L, ldz, zmask, n, eps_d)
            check_fwd(ref, B, L, ldz, zmask, n, out, zfull, f"B={B} L={L} ldz={ldz} zmask={zmask} np={n}")
        outs[ldz] = zfull
    assert np.array_equal(outs[9][:, :L].view(np.uint32)[B:], outs[16][:, :L].view(np.uint32)[B:])


def gpu_eps(B, L, Bg, off, seed, counter):
    """The eps [3][B][L] the kernels regenerate for (seed, counter, Bg, off), read back bit for bit: with
    mu = 0 and s = 0 the forward's lock row is 0 + 1 * eps, and slot sl of the stream is slot 0 of the
    rank whose first row is sl Bg + off."""
    ms_d = dev(np.zeros((3 * B, 2 * L)))
    ldz = round8(L + 1)
    e = [f32(run_fwd(ms_d, B, L, ldz, 2, 0, None, Bg=3 * Bg, off=sl * Bg + off, seed=seed, counter=counter)[0])
         [B:2 * B, :L] for sl in range(3)]
    return np.stack(e)


@pytest.mark.parametrize("L", [5, 8])
def test_latent_regenerated_eps(L):
    """eps regenerated in registers (a rank of a larger batch: Bg = 4B, off = B): the draw is
    oracle/philox_oracle.py's, and the forward and the backward give the bits of the same launch fed
    that draw as a buffer; both are then held to the float64 reference of that draw."""
    B, seed, counter = 6, 0x9E3779B97F4A7C15, 2 ** 32 + 5
    Bg, off = 4 * B, B
    eps = gpu_eps(B, L, Bg, off, seed, counter)
    want = PH.eps_reference(seed, counter, Bg, L, off, B)
    assert np.abs(eps - want).max() <= EPS_BAR
    ms, _ = make_ms(B, L, 9, dead=False)
    ms_d, eps_d, ldz = dev(ms), dev(eps), round8(L + 1)
    reg = dict(Bg=Bg, off=off, seed=seed, counter=counter)
    a = run_fwd(ms_d, B, L, ldz, 6, 3, None, **reg)
    b = run_fwd(ms_d, B, L, ldz, 6, 3, eps_d, Bg=Bg)
    for x, y in zip(a, b):
        assert torch.equal(x, y), "regenerated eps differs from the buffer"
    check_fwd(H.latent_fwd(ms, eps, B, L), B, L, ldz, 6, 3, a, f32(a[0]), f"regenerated B={B} L={L}")
    rng = np.random.default_rng(4)
    ins = bwd_inputs(ms, eps, B, L, Bg, rng)
    ldh = round8(2 * L)
    for metric in (0, 1):
        x = run_bwd(ins, B, L, Bg, ldh, metric, True, 3, eps_d)
        y = run_bwd(ins, B, L, Bg, ldh, metric, True, 3, None, off=off, seed=seed, counter=counter)
        for p, q in zip(x, y):
            assert torch.equal(p, q), "regenerated eps differs from the buffer (backward)"
        check_bwd(bwd_ref(ins, ms, eps, B, L, Bg, metric), B, L, ldh, True, 3, y, f32(y[0]),
                  f"regenerated B={B} L={L} metric={metric}")


# ------------------------------------------------------------------------- column statistics
def run_cs(mode, z_d, B, L, ldz, one, colsq=None, draw=None, cnt=None):
    ncols = 2 * L if mode == 0 else L
    nchunk = (B + 127) // 128
    part, out = nan32(nchunk * ncols + 8), nan32(ncols + 8)
    head(_lib.HEAD_COLSTATS, B=B, L=L, Bg=B, ldz=ldz, cs_mode=mode, z=z_d, colsq=colsq, draw=draw, part=part,
         out=out, cnt=cnt if one else None)
    return part, out


@pytest.mark.parametrize("B", [1, 127, 128, 129, 1000, 8192, 8193, 8320])
def test_colstats(B):
    """both statistics in both forms: one to 65 row chunks (8193 and 8320: the second round of the
    one-launch form's 64-chunk staging loop), a last chunk of one row, 2L = 66 (a column block of 2)"""
    for L in (1, 6, 32, 33, 100):
        what = f"B={B} L={L}"
        ldz = round8(L + 1)
        zbuf, zl, zk = make_z(B, L, ldz, 1000 * L + B)
        z_d = dev(zbuf)
        rng = np.random.default_rng(B + L)
        draw = (rng.standard_normal(B) * 10.0 ** rng.uniform(-2, 1, B)).astype(np.float32)
        draw_d = dev(draw)
        nchunk = (B + 127) // 128
        colsq_d = None
        for mode in (0, 1):
            ncols = 2 * L if mode == 0 else L
            if mode == 0:
                ref = H.colsq(zl, zk)
                dead_ok(ref["out"])
                if L >= 6:
                    assert (ref["out"] < H.L2_EPS).sum() == 4 and (ref["out"] == 0).sum() == 2
            else:
                ref = H.coldot(zl, zk, f32(colsq_d)[:2 * L], draw)
            nb = (ncols + 63) // 64
            cnt = torch.zeros(nb + 1, dtype=torch.int32, device="cuda")
            p2, o2 = run_cs(mode, z_d, B, L, ldz, False, colsq_d, draw_d)
            p1, o1 = run_cs(mode, z_d, B, L, ldz, True, colsq_d, draw_d, cnt)
            assert not cnt.any().item(), (what, mode, "counters not back at zero")
            p1b, o1b = run_cs(mode, z_d, B, L, ldz, True, colsq_d, draw_d, cnt)
            assert not cnt.any().item(), (what, mode, "counters not back at zero (second launch)")
            assert torch.equal(o1, o2) and torch.equal(p1, p2), (what, mode, "one launch != two launches")
            assert torch.equal(o1, o1b) and torch.equal(p1, p1b), (what, mode, "second launch differs")
            own = np.zeros(ncols + 8, bool)
            own[:ncols] = True
            untouched(o2, own, what + " out")
            pown = np.zeros(nchunk * ncols + 8, bool)
            pown[:nchunk * ncols] = True
            untouched(p2, pown, what + " part")
            k = "colsq" if mode == 0 else "coldot"
            check(f32(o2)[:ncols], ref["out"], ref["mag"], k, what)
            check(f32(p2)[:nchunk * ncols].reshape(nchunk, ncols), ref["part"], ref["part_mag"], k, what + " partials")
            if mode == 0:
                colsq_d = o2


# ------------------------------------------------------------------------- metric
METRIC_L = [(6, 8), (60, 64), (64, 72), (64, 65), (68, 72), (100, 104), (256, 264), (260, 264), (2000, 2008)]


@pytest.mark.parametrize("L,ldz", METRIC_L)
def test_metric(L, ldz):
    """cosine and squared difference x reciprocal x areas given / NULL; the float4 / scalar dispatch of
    the cosine (L = 60 scalar, 64 and 68 float4, 64 at a stride of 65 scalar); every row checked"""
    for i, B in enumerate((1, 3, 4, 5, 257)):
        nblk = (1, 3, 64, 65, 79)[(i + L) % 5]
        Bg = B if (i + L) % 2 else 4 * B
        rng = np.random.default_rng(L * 7 + B)
        rowpart = (rng.standard_normal((B, nblk)) * 10.0 ** rng.uniform(-2, 2, (B, nblk))).astype(np.float32)
        rowfwd = np.stack([rng.standard_normal(B) * 30, rng.uniform(0, 50, B), rng.uniform(0.5, 5, B),
                           np.zeros(B)], 1).astype(np.float32)
        areas = rng.uniform(0.1, 2.0, B).astype(np.float32)
        w = 10.0
        for recip in (0, 1):
            zbuf, zl, zk = make_z(B, L, ldz, L + 31 * B, recip=bool(recip))
            cs = H.colsq(zl, zk)["out"].astype(np.float32)
            dead_ok(cs)
            z_d, cs_d, rp_d, rf_d, ar_d = dev(zbuf), dev(cs), dev(rowpart), dev(rowfwd), dev(areas)
            for metric in (0, 1):
                for ar in (ar_d, None):
                    what = f"B={B} L={L} ldz={ldz} nblk={nblk} Bg={Bg} metric={metric} recip={recip} areas={ar is not None}"
                    ref = H.metric(zl, zk, rowfwd, rowpart, areas if ar is not None else None, cs, metric, recip,
                                   w, Bg)
                    if recip:   # raw must not cancel: its bound is then a bound on 1 / raw
                        assert np.all(np.abs(ref["raw"]) >= 0.5 * ref["raw_mag"]), what
                    rv, di, dr = nan32(B + 1, 4), nan32(B + 1), nan32(B + 1)
                    head(_lib.HEAD_METRIC, B=B, L=L, Bg=Bg, ldz=ldz, nblk=nblk, metric=metric, recip=recip, w=w,
                         z=z_d, rowfwd=rf_d, rowpart=rp_d, areas=ar, colsq=cs_d, rowvals=rv, dist=di, draw=dr)
                    check(f32(rv)[:B], ref["rowvals"], ref["rowvals_mag"], "metric", what + " rowvals")
                    check(f32(di)[:B], ref["dist"], ref["dist_mag"], "metric", what + " dist")
                    check(f32(dr)[:B], ref["draw"], ref["draw_mag"], "metric", what + " draw")
                    for t, nm in ((rv, "rowvals"), (di, "dist"), (dr, "draw")):
                        own = np.zeros(tuple(t.shape), bool)
                        own[:B] = True
                        untouched(t, own, what + " " + nm)


# ------------------------------------------------------------------------- loss_reduce
@pytest.mark.parametrize("B", [1, 255, 256, 257, 2047, 2048, 2049, 4100])
def test_loss_reduce(B):
    """the 8-row unrolled loop (from 1793 rows on), its tail and the one-row remainder"""
    rng = np.random.default_rng(B)
    rv = (rng.standard_normal((B, 4)) * 10.0 ** rng.uniform(-3, 3, (B, 4))).astype(np.float32)
    rv_d = dev(rv)
    for Bg in (B, 4 * B):
        ref = H.loss_reduce(rv, Bg)
        losses = nan32(8)
        head(_lib.HEAD_LOSS, B=B, Bg=Bg, L=1, rowvals=rv_d, losses=losses)
        check(f32(losses)[:5], ref["losses"], ref["mag"], "loss_reduce", f"B={B} Bg={Bg}")
        own = np.zeros(8, bool)
        own[:5] = True
        untouched(losses, own, "losses")


# ------------------------------------------------------------------------- latent_bwd
def bwd_inputs(ms, eps, B, L, Bg, rng):
    """dzdec, draw and the cosine's colsq / coldot (of this batch's own z, rounded to fp32)"""
    z = H.reparam(ms, eps, B, L)["z"]
    dzdec = (rng.standard_normal((B, L)) / Bg).astype(np.float32)
    draw = (rng.standard_normal(B) * 10.0 ** rng.uniform(-2, 1, B) / Bg).astype(np.float32)
    cs = H.colsq(z[1], z[2])["out"].astype(np.float32)
    dead_ok(cs)
    cd = H.coldot(z[1], z[2], cs, draw)["out"].astype(np.float32)
    return dict(ms=dev(ms), dzdec=dev(dzdec), draw=dev(draw), colsq=dev(cs), coldot=dev(cd),
                host=(dzdec, draw, cs, cd))


def bwd_ref(ins, ms, eps, B, L, Bg, metric, w=10.0):
    dzdec, draw, cs, cd = ins["host"]
    return H.latent_bwd(ms, eps, dzdec, draw, cs, cd, B, L, metric, w, Bg)


def run_bwd(ins, B, L, Bg, ldh, metric, fp32, n, eps_d, w=10.0, **regen):
    dh = nan32(4 * B + 1, ldh)
    hp = nan16(max(n, 1) * 4 * B * ldh + ldh)
    head(_lib.HEAD_BWD, B=B, L=L, Bg=Bg, ldh=ldh, metric=metric, w=w, h_planes=n, ms=ins["ms"], eps=eps_d,
         dzdec=ins["dzdec"], draw=ins["draw"], colsq=ins["colsq"], coldot=ins["coldot"],
         dhead=dh if fp32 else None, hp=hp if n else None, off=regen.get("off", 0), seed=regen.get("seed", 0),
         counter=regen.get("counter", 0))
    return dh, hp


def check_bwd(ref, B, L, ldh, fp32, n, out, dfull, what):
    dh, hp = out
    own = np.zeros((4 * B + 1, ldh), bool)
    if fp32:
        own[:4 * B, :2 * L] = True
        d = f32(dh)[:4 * B, :2 * L].reshape(4, B, 2 * L)
        for q, row in enumerate(("rot g1", "lock g1", "lock g2", "key g2")):
            for h, col in enumerate(("dmu", "ds")):
                sl = slice(h * L, (h + 1) * L)
                check(d[q][:, sl], ref["dhead"][q][:, sl], ref["mag"][q][:, sl], "latent_bwd", f"{what} {row} {col}")
        # printed, not asserted: the g2 rows under magnitudes that take |z| for mag(z) (head_ref.py)
        e = np.abs(d[2:4] - ref["dhead"][2:4])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(e == 0, 0.0, e / (TOL * ref["g2_mag_abs_z"])).max())
        k = "latent_bwd g2 rows under |z| magnitudes (not a bound)"
        WORST[k] = max(WORST.get(k, 0.0), r)
    untouched(dh, own, what + " dhead")
    pb = bits(hp)
    pown = np.zeros(pb.shape, bool)
    if n:
        img = pb[:n * 4 * B * ldh].reshape(n, 4 * B, ldh)
        assert np.array_equal(img[:, :, :2 * L], H.planes(dfull[:4 * B, :2 * L], n)), (what, "planes")
        po = np.zeros((n, 4 * B, ldh), bool)
        po[:, :, :2 * L] = True
        pown[:n * 4 * B * ldh] = po.reshape(-1)
    untouched(hp, pown, what + " planes")


BWD_FORMS = [(True, 0), (False, 1), (False, 3), (True, 3), (True, 1)]   # fp32 only, planes only, both


@pytest.mark.parametrize("L", [1, 5, 6, 8, 20, 100, 2000])
def test_latent_bwd(L):
    """all eight blocks ([4 rows] x [dmu | ds]) per element, both metrics, the three output forms; B L
    and B L / 4 are no multiples of 256 (the last workgroup is partial); Bg = B and 4B in turn"""
    for i, B in enumerate((1, 3, 65, 300)):
        Bg = B if (i + L) % 2 else 4 * B
        ms, eps = make_ms(B, L, 50 * L + B)
        rng = np.random.default_rng(L + B)
        ins = bwd_inputs(ms, eps, B, L, Bg, rng)
        eps_d = dev(eps)
        ld0 = round8(2 * L)
        for metric in (0, 1):
            ref = bwd_ref(ins, ms, eps, B, L, Bg, metric)
            for ldh, forms in ((ld0, BWD_FORMS), (ld0 + 8, [(True, 3), (False, 1)])):
                dfull = f32(run_bwd(ins, B, L, Bg, ldh, metric, True, 0, eps_d)[0])
                for fp32, n in forms:
                    out = run_bwd(ins, B, L, Bg, ldh, metric, fp32, n, eps_d)
                    check_bwd(ref, B, L, ldh, fp32, n, out, dfull,
                              f"B={B} L={L} Bg={Bg} ldh={ldh} metric={metric} fp32={fp32} np={n}")
        if B == 65:   # the backward's recomputed z is the forward's: both within the bar of one reference
            ldz = round8(L + 1)
            z = f32(run_fwd(ins["ms"], B, L, ldz, 6, 0, eps_d)[0])
            for blk in (1, 2):
                check(z[blk * B:(blk + 1) * B, :L], ref["z"][blk], ref["z_mag"][blk], "latent_fwd",
                      f"B={B} L={L} forward z[{blk}] against the backward's reference")
