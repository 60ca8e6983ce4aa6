"""The fused GEMM epilogues of the step, one launch at a time on caller buffers (mvae_debug_epi:
gemm_run on the GemmDesc the step's wiring would build), per element against tests/epi_ref.py
(float64 from the kernel's own inputs). The bar is the project's 2e-6 mag for every fp32 output
(a zero mag demands exactness); tests/test_epi_ref.py shows that a plain fp32 evaluation of the same
formulas sits at 0.03-0.12 of it and a single dropped column at 50 times it or more.

Every output buffer is prefilled with NaN bits (fp32 0x7FC12345, bf16 0x7FC1) and carries a guard
row and columns beyond the stride's use: what a launch owns must not hold the prefill, everything
else must come back bit-identical. Buffers a target form must not read hold NaN.

Shapes are the smallest at which each path can go wrong: M 1 / 70 / 257 / 300 / 520,
N 128 / 136 / 260 / 300 / 392 / 516 (648 for the split), K 21 / 65 / 200 with lda = round8(K).
Each kernel family gets the whole M x N sweep at K = 65 and K = 21 / 200 at two shapes.

Saturation: v = -30 gives y = exp(-30) = 9.4e-14 in fp32 (and in float64), not 0, so there y and dU
are held to the bound and x = 1 contributes the finite 30; y is exactly 1 at v = +30 / +100 and
exactly 0 at v = -100, where the terms are +inf or exactly 0 (tests/epi_ref.py, sat=True).

Worst error / bound measured on an MI355X (a record; the assertions' bound is 1; run with -s for the
EPI_WORST lines): rowpart 0.025-0.037, dU and y 0.058-0.068 in bf16, 0.144 in fp32, 0.176-0.252 in
f32x; DACT 0.054-0.157, ACT / DACT with padw 0.117-0.171; the finite saturation blocks 0.027. The
216 tests take 7 s together, the slowest (the fp32 family sweep, which also builds the float64
references the others share) 1 s.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from magic_amd import _lib
from tests import epi_ref as E

pytestmark = pytest.mark.gpu

BAR = 2e-6
NANF, NANH = 0x7FC12345, 0x7FC1
SCALES = {21: 0.25, 65: 0.15, 200: 0.1}   # of B: largest |logit| 5.5-6.7 (asserted <= 8 on the reference)
MS, NS = (1, 70, 257, 300, 520), (128, 136, 260, 300, 392, 516)
# (prec, variant, x3): fp32 128x128; per plane mode the 128x128 plane kernel, the ring kernel at tile N
# 128 / 256, the ring kernel on the C/D epilogue, the eight-phase kernel, the planner's pick; the
# plane-stacked kernel
FAMILIES = [(0, 0, 0)] + [(p, v, 0) for p in (1, 2) for v in (4, 11, 12, 10, 13, 0)] + [(2, 11, 1)]
PLANE_FAMILIES = [f for f in FAMILIES if f[0]]
FID = lambda f: f"prec{f[0]}_v{f[1]}" + ("_x3" if f[2] else "")  # noqa: E731
WORST = {}   # (test, output) -> worst error / bound seen in this session (printed as EPI_WORST lines)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    for k in sorted(WORST):
        print(f"EPI_WORST {k[0]} {k[1]} {WORST[k]:.4f}")


def r8(n):
    return (n + 7) // 8 * 8


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bf16_exact(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


# ------------------------------------------------------------------ inputs and references (shared)
@functools.lru_cache(maxsize=None)
def operands(M, N, K, exact):
    """A [M][K], B [K][N] fp32 (host); exact: values bf16 holds (the bf16 mode's operand rounding is
    then the identity, as in test_gpu_bf16_exact.py)"""
    rng = np.random.default_rng(M * 7 + N * 13 + K * 29)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = (rng.standard_normal((K, N)) * SCALES[K]).astype(np.float32)
    return (bf16_exact(A), bf16_exact(B)) if exact else (A, B)


@functools.lru_cache(maxsize=None)
def target(M, N, kind):
    """bin: 0/1; grey: k/255 foreground (no bf16 values) with exact 0 and 1 inside; grey16: j/128 (bf16
    values) with exact 0 and 1 inside; mixed: rows 0-63 binary, the rest grey -- so the waves of one
    launch take the one-logarithm and the two-logarithm form"""
    rng = np.random.default_rng(M * 3 + N * 5 + len(kind))
    fg = rng.random((M, N)) < 0.3
    x = fg.astype(np.float32)
    if kind == "bin":
        return x
    g = (rng.integers(1, 256, size=x.shape) / 255.0).astype(np.float32)
    if kind == "grey16":
        g = (rng.integers(1, 129, size=x.shape) / 128.0).astype(np.float32)
    xg = x * g
    xg[:, 5 % N] = 1.0
    xg[:, 6 % N] = 0.0
    if kind == "mixed":
        xg[:64] = x[:64]
    return xg


@functools.lru_cache(maxsize=None)
def reference(M, N, K, exact, kind):
    A, B = operands(M, N, K, exact)
    r = E.bce(A, B, target(M, N, kind), 1.0 / M)
    E.check_accuracy_logits(r["v"])
    return {k: dev(r[k]) for k in ("rowpart", "rowpart_mag", "du", "du_mag", "y", "y_mag")}


def padded(a, ld, rows=None, fill=0.0):
    """host [m][n] -> device fp32 [rows][ld], the rest `fill`"""
    m, n = a.shape
    t = torch.full((rows or m, ld), fill, dtype=torch.float32)
    t[:m, :n] = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return t.cuda()


def nan_f32(rows, ld):
    return torch.full((rows, ld), NANF, dtype=torch.int32, device="cuda").view(torch.float32)


def nan_bf16(*shape):
    return torch.full(shape, NANH, dtype=torch.int16, device="cuda")


def bits_f32(t):
    return t.view(torch.int32)


def hold(test, name, got, ref, mag):
    """|got - ref| <= 2e-6 mag per element (mag 0: exact); records the worst error / bound"""
    err = (got.double() - ref).abs()
    bound = BAR * mag
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, 0.0, float("inf")).double())
    w = float(ratio.max()) if ratio.numel() else 0.0
    WORST[(test, name)] = max(WORST.get((test, name), 0.0), w)
    bad = ~(err <= bound)
    assert not bad.any(), (test, name, w, [tuple(i) for i in bad.nonzero()[:5].tolist()])
    return w


def call(a):
    lib = _lib.load()
    rc = lib.mvae_debug_epi(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mvae_last_error(None)


def owned(bits, M, N, prefill, what):
    """rows < M and columns < N written, everything else the prefill"""
    assert not (bits[..., :M, :N] == prefill).any(), what + ": an owned element holds the prefill"
    rest = bits.clone()
    rest[..., :M, :N] = prefill
    assert (rest == prefill).all(), what + ": written outside the launch's rows / columns"


def run_bce(A, B, x, *, prec, variant, x3=0, form="f32", du=True, ncp=0, y=True, mis="", rp=(2, 1), split_c0=0):
    """One BCE head on host A [M][K], B [K][N], x [M][N]. form: f32 (the fp32 target alone) | plane
    (dyn = {0,0,1,0}) | allbin (dyn = 0, no bits) | bits (dyn = 0, bits; the plane NaN) | dyn1 (dyn[0]
    = 1 with a NaN plane: the fp32 rows) | stalebits (plane, with the complement of the bits given).
    The fp32 target holds NaN wherever the form must not read it (plane modes). mis: which of ldc /
    ldx / ldy is odd. rp = (rp_ld - nblk, rp_off), or None for rp_ld = 0. Returns the device buffers
    after the ownership checks."""
    M, K = A.shape
    N = B.shape[1]
    nb = E.nblk(N)
    ld = {k: r8(N) + 8 + (1 if k in mis.split(",") else 0) for k in ("ldc", "ldx", "ldy")}
    reads_x = prec == 0 or form in ("f32", "dyn1")
    a = _lib.mvae_epi_args()
    keep = [padded(A, r8(K)), padded(B, r8(N))]
    a.M, a.N, a.K, a.lda, a.ldb = M, N, K, r8(K), r8(N)
    a.A, a.B = keep[0].data_ptr(), keep[1].data_ptr()
    a.prec, a.variant, a.x3, a.epi, a.scale = prec, variant, x3, _lib.EPI_BCE, 1.0 / M
    xf = padded(x, ld["ldx"], M + 1, float("nan")) if reads_x else nan_f32(M + 1, ld["ldx"])
    a.x, a.ldx = xf.data_ptr(), ld["ldx"]
    keep.append(xf)
    if form != "f32":
        dyn = {"plane": (0, 0, 1, 0), "allbin": (0, 0, 0, 0), "bits": (0, 0, 0, 0), "dyn1": (1, 0, 1, 0),
               "stalebits": (0, 0, 1, 0)}[form]
        dynt = torch.tensor(dyn, dtype=torch.int32, device="cuda")
        if form in ("plane", "allbin", "stalebits"):
            xp = padded(x, ld["ldx"], M + 1, float("nan")).bfloat16().view(torch.int16)
            assert torch.equal(xp.view(torch.bfloat16).float()[:M, :N].cpu(), torch.from_numpy(x)), "target not bf16"
        else:
            xp = nan_bf16(M + 1, ld["ldx"])
        a.xp, a.dyn = xp.data_ptr(), dynt.data_ptr()
        keep += [dynt, xp]
        if form in ("bits", "stalebits"):   # stalebits: the complement, which dyn[2] != 0 forbids reading
            ldbits = (N + 7) // 8 + 3
            xb = torch.full((M + 1, ldbits), 0xFF, dtype=torch.uint8)
            xb[:M, :(N + 7) // 8] = torch.from_numpy(E.pack_bits(x) ^ (0xFF if form == "stalebits" else 0))
            xb = xb.cuda()
            a.xbits, a.ldbits = xb.data_ptr(), ldbits
            keep.append(xb)
    out = {}
    a.ldc = ld["ldc"]
    if du:
        out["du"] = nan_f32(M + 1, a.ldc)
        a.du = out["du"].data_ptr()
    if ncp:
        out["planes"] = nan_bf16(ncp, M + 1, a.ldc)
        a.cp, a.ncp, a.pc = out["planes"].data_ptr(), ncp, (M + 1) * a.ldc
    if y:
        out["y"] = nan_f32(M + 1, ld["ldy"])
        a.y, a.ldy = out["y"].data_ptr(), ld["ldy"]
    rp_ld, rp_off = (nb + rp[0], rp[1]) if rp else (nb, 0)
    out["rowpart"] = nan_f32(M + 1, rp_ld)
    a.rowpart, a.rp_ld, a.rp_off = out["rowpart"].data_ptr(), (rp_ld if rp else 0), rp_off
    a.split_c0 = split_c0
    call(a)
    if du:
        owned(bits_f32(out["du"]), M, N, NANF, "du")
    if ncp:
        owned(out["planes"], M, N, NANH, "planes")
    if y:
        owned(bits_f32(out["y"]), M, N, NANF, "y")
    rpb = bits_f32(out["rowpart"])
    owned(rpb[:, rp_off:rp_off + nb], M, nb, NANF, "rowpart")
    assert (rpb[:, :rp_off] == NANF).all() and (rpb[:, rp_off + nb:] == NANF).all(), "rowpart outside its blocks"
    out["rp"] = out["rowpart"][:M, rp_off:rp_off + nb]
    return out


def planes_are_the_split(out, M, N):
    """every plane image the bit-exact RNE split of the stored fp32 value"""
    r = out["du"][:M, :N].clone()
    for t in range(out["planes"].shape[0]):
        b = r.bfloat16()
        assert torch.equal(out["planes"][t, :M, :N], b.view(torch.int16)), f"plane {t}"
        r = r - b.float()


def planes_value(out, M, N):
    p = out["planes"][:, :M, :N].view(torch.bfloat16).double()
    return sum(p[t] for t in reversed(range(p.shape[0])))


def hold_all(test, out, ref, M, N):
    w = {"rowpart": hold(test, "rowpart", out["rp"], ref["rowpart"], ref["rowpart_mag"])}
    if "du" in out:
        w["du"] = hold(test, "du", out["du"][:M, :N], ref["du"], ref["du_mag"])
    if "y" in out:
        w["y"] = hold(test, "y", out["y"][:M, :N], ref["y"], ref["y_mag"])
    return w


def same_bits(a, b, keys=("du", "planes", "y", "rowpart")):
    """[(key, count of differing elements)] over the buffers both runs have"""
    diff = []
    for k in keys:
        if k in a and k in b:
            u, v = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a[k], b[k]))
            if not torch.equal(u, v):
                diff.append((k, int((u != v).sum()), [tuple(i) for i in (u != v).nonzero()[:3].tolist()]))
    return diff


def ncp_of(prec):
    return (0, 1, 3)[prec]


# ------------------------------------------------------------------ kernel families
@pytest.mark.parametrize("fam", FAMILIES, ids=FID)
def test_bce_kernel_families(fam):
    """Every output element of every kernel family against float64, over M x N at K = 65 and at K = 21
    / 200 on two shapes: a mixed target (binary rows beside grey rows) as fp32, the fp32 dU with its
    planes (each the RNE split of the stored value) and y. rowpart alternates between a wider row
    (rp_ld = nblk + 2, rp_off = 1) and the launch's own (rp_ld = 0)."""
    prec, variant, x3 = fam
    test = "families_" + FID(fam)
    shapes = [(M, N, 65) for M in MS for N in NS] + [(M, N, K) for K in (21, 200) for M, N in ((300, 392), (257, 260))]
    for i, (M, N, K) in enumerate(shapes):
        A, B = operands(M, N, K, prec == 1)
        out = run_bce(A, B, target(M, N, "mixed"), prec=prec, variant=variant, x3=x3, ncp=ncp_of(prec),
                      rp=(2, 1) if i % 2 else None)
        hold_all(test, out, reference(M, N, K, prec == 1, "mixed"), M, N)
        if prec:
            planes_are_the_split(out, M, N)


@pytest.mark.parametrize("fam", [f for f in PLANE_FAMILIES if f[1] in (11, 12, 13, 0)], ids=FID)
@pytest.mark.parametrize("mis", ["ldc", "ldx", "ldy", "ldc,ldx,ldy"])
def test_bce_misaligned_strides(fam, mis):
    """ldc, ldx or ldy odd: the ring kernel falls back to the C/D epilogue and the eight-phase kernel
    to element-wise accesses; the same bound, the same ownership."""
    prec, variant, x3 = fam
    for M, N in ((300, 392), (257, 260), (520, 516)):
        A, B = operands(M, N, 65, prec == 1)
        out = run_bce(A, B, target(M, N, "mixed"), prec=prec, variant=variant, x3=x3, ncp=ncp_of(prec), mis=mis)
        hold_all("misaligned_" + FID(fam), out, reference(M, N, 65, prec == 1, "mixed"), M, N)
        planes_are_the_split(out, M, N)


@pytest.mark.parametrize("M,N", [(300, 392), (257, 260), (520, 516), (300, 136)])
def test_bce_planner_pick(M, N):
    """Variant 0 runs one of the forced kernels: its outputs are bitwise those of variant 4, 11, 12 or
    13 (the matches are printed: which kernel the planner picked per shape)."""
    for prec in (1, 2):
        A, B = operands(M, N, 65, prec == 1)
        x = target(M, N, "mixed")
        base = run_bce(A, B, x, prec=prec, variant=0, ncp=ncp_of(prec))
        match = [v for v in (4, 11, 12, 13)
                 if not same_bits(base, run_bce(A, B, x, prec=prec, variant=v, ncp=ncp_of(prec)))]
        print(f"EPI_PICK prec={prec} {M}x{N}x65 variant 0 bitwise equal to variants {match}")
        assert match, (prec, M, N)


# ------------------------------------------------------------------ target forms
@pytest.mark.parametrize("fam", FAMILIES, ids=FID)
def test_bce_target_forms_binary(fam):
    """One binary target as fp32 only, as its plane with the not-binary word set, as its plane with
    both words clear (no per-pixel test) and as bits (the plane then NaN): the four runs of one kernel
    give the same bits in every output. The fp32 rows hold NaN wherever they must not be read. (The
    fp32 kernels always read the fp32 rows.) Each run is also held to float64."""
    prec, variant, x3 = fam
    for M, N in ((300, 392), (257, 260), (70, 136)):
        A, B = operands(M, N, 65, prec == 1)
        x = target(M, N, "bin")
        ref = reference(M, N, 65, prec == 1, "bin")
        runs = {}
        for form in ("f32", "plane", "allbin", "bits"):
            runs[form] = run_bce(A, B, x, prec=prec, variant=variant, x3=x3, form=form, ncp=ncp_of(prec))
            hold_all("forms_binary_" + FID(fam), runs[form], ref, M, N)
        for form in ("plane", "allbin", "bits"):
            d = same_bits(runs["f32"], runs[form])
            if d:
                print(f"EPI_FORMS {FID(fam)} {M}x{N} {form} differs from f32 in {d}")
            assert not d, (form, d)


@pytest.mark.parametrize("fam", PLANE_FAMILIES, ids=FID)
def test_bce_target_forms_grey(fam):
    """dyn[0] = 1 with a NaN plane: the fp32 rows are used. A grey target of bf16 values through its
    plane (the fp32 rows NaN) equals the run on the fp32 rows bit for bit. The mixed target through
    the plane: the waves of the binary rows take the one-logarithm form beside the others; stale bits
    given with the not-binary word set change nothing."""
    prec, variant, x3 = fam
    kw = dict(prec=prec, variant=variant, x3=x3, ncp=ncp_of(prec))
    test = "forms_grey_" + FID(fam)
    for M, N in ((300, 392), (257, 260)):
        A, B = operands(M, N, 65, prec == 1)
        hold_all(test, run_bce(A, B, target(M, N, "grey"), form="dyn1", **kw), reference(M, N, 65, prec == 1, "grey"), M, N)
        x16 = target(M, N, "grey16")
        ref16 = reference(M, N, 65, prec == 1, "grey16")
        a, b = run_bce(A, B, x16, form="f32", **kw), run_bce(A, B, x16, form="plane", **kw)
        hold_all(test, a, ref16, M, N)
        hold_all(test, b, ref16, M, N)
        assert not same_bits(a, b), same_bits(a, b)
        xm = bf16_exact(target(M, N, "mixed"))
        rm = E.bce(A, B, xm, 1.0 / M)
        rm = {k: dev(rm[k]) for k in ("rowpart", "rowpart_mag", "du", "du_mag", "y", "y_mag")}
        pm = run_bce(A, B, xm, form="plane", **kw)
        hold_all(test, pm, rm, M, N)
        # bits left over from a binary batch are not read while the not-binary word is set
        assert not same_bits(pm, run_bce(A, B, xm, form="stalebits", **kw))


def test_bce_bits_from_the_producer():
    """xbits, ldbits and dyn as mvae_debug_pairs_bits writes them (mode 0, S = 12, B = 64): the lock
    block fed to the head equals the run on the fp32 lock rows, bit for bit, on every plane family;
    the Python packer agrees with the producer."""
    from tests.test_gpu_pairs import dev as pdev, draws, tables
    lib = _lib.load()
    S, Bt = 12, 64
    D = S * S
    L, K = tables(S, 255, seed=S)
    idx, coef = draws(Bt, S, seed=Bt + S)
    ldx, ldbits = D + 8, (D // 8 + 15) // 16 * 16
    ceil = lambda a, b: (a + b - 1) // b  # noqa: E731
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    xbf, xbw = z(ceil(3 * Bt, 256) * ceil(D + 1, 64) * 512, torch.int32), z(ceil(D + 1, 256) * ceil(3 * Bt, 64) * 512, torch.int32)
    xbits, dyn, plane, xi = z(Bt * ldbits, torch.uint8), z(4, torch.int32), z(3 * Bt * ldx, torch.int16), z(Bt * 3 * D, torch.float32)
    t = [pdev(L), pdev(K), pdev(idx), pdev(coef)]
    rc = lib.mvae_debug_pairs_bits(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), Bt, S, 255.0, 0, 0,
                                   xi.data_ptr(), xbf.data_ptr(), xbw.data_ptr(), xbits.data_ptr(), ldbits,
                                   dyn.data_ptr(), plane.data_ptr(), ldx, torch.cuda.current_stream().cuda_stream)
    _lib.check(lib, None, rc)
    lock = xi.view(Bt, D, 3)[:, :, 0].contiguous().cpu().numpy()   # channel 0 of the interleaved pixels
    assert dyn.cpu().tolist()[0] == 0 and dyn.cpu().tolist()[2] == 0 and lock.any()
    assert np.array_equal(xbits.view(Bt, ldbits)[:, :D // 8].cpu().numpy(), E.pack_bits(lock))
    M, N, Kk = Bt, D, 65
    for prec, variant, x3 in PLANE_FAMILIES:
        A, B = operands(M, N, Kk, prec == 1)
        base = run_bce(A, B, lock, prec=prec, variant=variant, x3=x3, ncp=ncp_of(prec), rp=None)
        a = _lib.mvae_epi_args()
        keep = [padded(A, r8(Kk)), padded(B, r8(N)), nan_f32(M + 1, ldx), nan_f32(M + 1, ldx), nan_bf16(ncp_of(prec), M + 1, ldx),
                nan_f32(M + 1, ldx), nan_f32(M + 1, E.nblk(N)), nan_bf16(M + 1, ldx)]
        a.M, a.N, a.K, a.lda, a.ldb, a.A, a.B = M, N, Kk, r8(Kk), r8(N), keep[0].data_ptr(), keep[1].data_ptr()
        a.prec, a.variant, a.x3, a.epi, a.scale = prec, variant, x3, _lib.EPI_BCE, 1.0 / M
        a.x, a.ldx, a.du, a.ldc, a.cp, a.ncp, a.pc = keep[2].data_ptr(), ldx, keep[3].data_ptr(), ldx, keep[4].data_ptr(), ncp_of(prec), (M + 1) * ldx
        a.y, a.ldy, a.rowpart = keep[5].data_ptr(), ldx, keep[6].data_ptr()
        a.xp, a.dyn, a.xbits, a.ldbits = keep[7].data_ptr(), dyn.data_ptr(), xbits.data_ptr(), ldbits
        call(a)
        got = dict(du=keep[3][:M, :N], planes=keep[4][:, :M, :N], y=keep[5][:M, :N], rowpart=keep[6][:M])
        want = dict(du=base["du"][:M, :N], planes=base["planes"][:, :M, :N], y=base["y"][:M, :N], rowpart=base["rowpart"][:M])
        got, want = ({k: v.contiguous() for k, v in d.items()} for d in (got, want))
        assert not same_bits(got, want), (FID((prec, variant, x3)), same_bits(got, want))


# ------------------------------------------------------------------ output forms
@pytest.mark.parametrize("fam", FAMILIES, ids=FID)
def test_bce_output_forms(fam):
    """fp32 only, planes only (their sum within the bound; one RN plane adds half a bf16 ulp, at most
    2^-8 of the value), both, y on and off: the outputs every form shares are bitwise the same."""
    prec, variant, x3 = fam
    test = "outputs_" + FID(fam)
    for M, N in ((300, 392), (257, 260)):
        A, B = operands(M, N, 65, prec == 1)
        x, ref = target(M, N, "mixed"), reference(M, N, 65, prec == 1, "mixed")
        kw = dict(prec=prec, variant=variant, x3=x3)
        full = run_bce(A, B, x, ncp=ncp_of(prec), **kw)
        hold_all(test, full, ref, M, N)
        forms = [dict(du=True, ncp=0, y=False), dict(du=True, ncp=0, y=True)]
        if prec:
            forms += [dict(du=False, ncp=ncp_of(prec), y=False), dict(du=False, ncp=ncp_of(prec), y=True),
                      dict(du=True, ncp=ncp_of(prec), y=False)]
        for f in forms:
            out = run_bce(A, B, x, **f, **kw)
            hold_all(test, out, ref, M, N)
            assert not same_bits(full, out), (f, same_bits(full, out))
            if f["ncp"] and not f["du"]:
                mag = ref["du_mag"] + ((ref["du"].abs() + BAR * ref["du_mag"]) * 2.0 ** -8 / BAR if f["ncp"] == 1 else 0)
                hold(test, "planes_sum", planes_value(out, M, N), ref["du"], mag)


# ------------------------------------------------------------------ row partials
@pytest.mark.parametrize("fam", [f for f in PLANE_FAMILIES if f[1] in (11, 12, 13, 0)], ids=FID)
@pytest.mark.parametrize("N", [516, 648])
def test_bce_split_head(fam, N):
    """split_c0 = 256: columns [0, 256) on the requested kernel and the rest on the ring kernel at tile
    N 128, as the step's split head -- against float64 per block, and against the one-launch run. With
    a binary target (every form) the two are bitwise equal in bf16, and within twice the bound in f32x
    (both are within it; the eight-phase kernel sums the plane pairs in another order). With grey
    rows the waves of the two tilings hold other sets of pixels, so the wave-uniform choice between
    the one-logarithm and the two-logarithm form can differ per wave: the same values, not the same
    bits -- twice the bound in both precisions. The same launch twice gives the same bits."""
    prec, variant, x3 = fam
    M, K = 300, 65
    test = "split_" + FID(fam)
    A, B = operands(M, N, K, prec == 1)
    kw = dict(prec=prec, variant=variant, x3=x3, ncp=ncp_of(prec))
    for kind, form in (("bin", "f32"), ("bin", "plane"), ("bin", "bits"), ("mixed", "f32"), ("mixed", "plane")):
        x = target(M, N, kind)
        ref = reference(M, N, K, prec == 1, kind)
        if kind == "mixed" and form == "plane":
            x = bf16_exact(x)
            rr = E.bce(A, B, x, 1.0 / M)
            ref = {k: dev(rr[k]) for k in ("rowpart", "rowpart_mag", "du", "du_mag", "y", "y_mag")}
        one = run_bce(A, B, x, form=form, **kw)
        two = run_bce(A, B, x, form=form, split_c0=256, **kw)
        again = run_bce(A, B, x, form=form, split_c0=256, **kw)
        hold_all(test, one, ref, M, N)
        hold_all(test, two, ref, M, N)
        planes_are_the_split(two, M, N)
        assert not same_bits(two, again), same_bits(two, again)
        if prec == 1 and kind == "bin":
            assert not same_bits(one, two), (form, same_bits(one, two))
        else:
            hold(test, "rowpart_vs_one", two["rp"], one["rp"].double(), 2 * ref["rowpart_mag"])
            hold(test, "du_vs_one", two["du"][:M, :N], one["du"][:M, :N].double(), 2 * ref["du_mag"])
            hold(test, "y_vs_one", two["y"][:M, :N], one["y"][:M, :N].double(), 2 * ref["y_mag"])


@pytest.mark.parametrize("fam", FAMILIES, ids=FID)
def test_bce_same_launch_twice(fam):
    prec, variant, x3 = fam
    M, N = 520, 516
    A, B = operands(M, N, 200, prec == 1)
    kw = dict(prec=prec, variant=variant, x3=x3, ncp=ncp_of(prec), form="f32")
    a, b = run_bce(A, B, target(M, N, "mixed"), **kw), run_bce(A, B, target(M, N, "mixed"), **kw)
    hold_all("twice_" + FID(fam), a, reference(M, N, 200, prec == 1, "mixed"), M, N)
    assert not same_bits(a, b), same_bits(a, b)


# ------------------------------------------------------------------ saturation
@functools.lru_cache(maxsize=None)
def saturated(M, N, K, grey):
    """A with one nonzero (30 or 100) per row and B of +-1 / 0: v in {+-30, +-100, 0} exactly. Per (row,
    128-column block) either `safe` -- x = (v > 0), or any grey value where v = 0: every term finite --
    or a random target, which meets log 0 somewhere."""
    rng = np.random.default_rng(11 + grey)
    A = np.zeros((M, K), np.float32)
    A[np.arange(M), np.arange(M) % K] = rng.choice([30.0, 100.0], M)
    B = rng.choice([-1.0, 0.0, 1.0], (K, N)).astype(np.float32)
    v = A.astype(np.float64) @ B
    x = (rng.random((M, N)) < 0.5).astype(np.float32)
    if grey:
        x = (x * rng.integers(0, 129, size=x.shape) / 128.0).astype(np.float32)
        x[:, 3] = 1.0
    blk = np.arange(N) // 128
    safe = ((np.arange(M)[:, None] + blk[None, :]) % 3) == 0
    xs = (v > 0).astype(np.float32)
    if grey:
        xs = np.where(v == 0, x, xs).astype(np.float32)
    x = np.where(safe, xs, x).astype(np.float32)
    r = E.bce(A, B, x, 1.0 / M, sat=True)
    ref = {k: dev(r[k]) for k in ("rowpart", "rowpart_mag", "du", "du_mag", "y", "y_mag", "v")}
    return A, B, x, ref


@pytest.mark.parametrize("fam", FAMILIES, ids=FID)
@pytest.mark.parametrize("grey", [0, 1], ids=["binary", "grey"])
def test_bce_saturation(fam, grey):
    """No epsilon, pow(0, 0) = 1: rowpart is +inf exactly for the (row, block) pairs the reference
    names and finite and in bound in every other block of the same rows; dU is finite and within the
    bound, bitwise (y - x) scale wherever y is exactly 0 or 1; y is exactly 1 at v = 30 / 100 and
    exactly 0 at v = -100; no NaN anywhere. Every target form."""
    prec, variant, x3 = fam
    M, N, K = 300, 392, 21
    A, B, x, ref = saturated(M, N, K, grey)
    inf = torch.isinf(ref["rowpart"])
    assert inf.any() and (~inf).any() and ((~inf).sum(1) > 0).all() and (inf.sum(1) > 0).all()
    forms = ("f32", "plane") if grey else ("f32", "plane", "allbin", "bits")
    scale = torch.tensor(1.0 / M, dtype=torch.float32, device="cuda")
    xt = dev(x)
    for form in forms:
        out = run_bce(A, B, x, prec=prec, variant=variant, x3=x3, form=form, ncp=ncp_of(prec))
        rp, du, y = out["rp"], out["du"][:M, :N], out["y"][:M, :N]
        for k, t in (("rowpart", rp), ("du", du), ("y", y)):
            assert not torch.isnan(t).any(), (form, k)
        assert torch.equal(torch.isinf(rp) & (rp > 0), inf), form
        fin = ~inf
        hold("saturation", "rowpart", rp[fin], ref["rowpart"][fin], ref["rowpart_mag"][fin])
        assert torch.isfinite(du).all()
        hold("saturation", "du", du, ref["du"], ref["du_mag"])
        hold("saturation", "y", y, ref["y"], ref["y_mag"])
        one, zero = ref["v"] >= 30, ref["v"] <= -100
        assert (y[one] == 1).all() and (y[zero] == 0).all()
        ex = one | zero
        assert torch.equal(du[ex], ((one.float() - xt) * scale)[ex])
        if prec:
            planes_are_the_split(out, M, N)


# ------------------------------------------------------------------ DACT / ACT
def run_out(a, M, N, ldc, ncp, keep):
    du, pl = nan_f32(M + 1, ldc), (nan_bf16(ncp, M + 1, ldc) if ncp else None)
    a.du, a.ldc = du.data_ptr(), ldc
    if ncp:
        a.cp, a.ncp, a.pc = pl.data_ptr(), ncp, (M + 1) * ldc
    keep += [du, pl]
    call(a)
    return du, pl


DACT_FAMILIES = [(0, 0), (1, 4), (1, 11), (1, 13), (2, 4), (2, 12), (2, 13)]


@pytest.mark.parametrize("prec,variant", DACT_FAMILIES, ids=[f"prec{p}_v{v}" for p, v in DACT_FAMILIES])
@pytest.mark.parametrize("act", [0, 1], ids=["tanh", "elu"])
@pytest.mark.parametrize("Bp", [37, 75])
def test_epi_dact_remap(prec, variant, act, Bp):
    """The encoder dgrads' row remap: M = 4 B' output rows read 3 B' aux rows (rows >= 2 B' read row r -
    B'); the boundary falls inside a 32-row block and inside a band. B as [N][K] (bt). fp32 aux, and in
    bf16 mode its bf16 image alone (aux NULL). Every aux row is distinct, and the buffer holds M + 1
    rows, so a launch without the remap reads other values, not other memory."""
    M, N, K = 4 * Bp, 260, 65
    rng = np.random.default_rng(Bp * 7 + act)
    A = rng.standard_normal((M, K)).astype(np.float32)
    Bt = (rng.standard_normal((N, K)) * 0.15).astype(np.float32)
    pre = rng.standard_normal((M + 1, N)) * 1.5
    aux = (np.tanh(pre) if act == 0 else np.where(pre < 0, np.expm1(pre), pre)).astype(np.float32)
    if prec == 1:
        A, Bt, aux = bf16_exact(A), bf16_exact(Bt), bf16_exact(aux)
    r = E.dact(A, Bt.T, aux[:3 * Bp], act, remap_split=2 * Bp, remap_shift=Bp)
    ref, mag = dev(r["out"]), dev(r["mag"])
    ld = r8(N) + 8
    for use_plane in ((False, True) if prec == 1 else (False,)):
        a = _lib.mvae_epi_args()
        keep = [padded(A, r8(K)), padded(Bt, r8(K)), padded(aux, ld, M + 1, float("nan"))]
        a.M, a.N, a.K, a.lda, a.ldb, a.bt, a.A, a.B = M, N, K, r8(K), r8(K), 1, keep[0].data_ptr(), keep[1].data_ptr()
        a.prec, a.variant, a.epi, a.act = prec, variant, _lib.EPI_DACT, act
        a.ld_aux, a.remap_split, a.remap_shift = ld, 2 * Bp, Bp
        if use_plane:
            keep.append(keep[2].bfloat16().view(torch.int16))
            a.auxp = keep[3].data_ptr()
        else:
            a.aux = keep[2].data_ptr()
        du, pl = run_out(a, M, N, ld, ncp_of(prec), keep)
        owned(bits_f32(du), M, N, NANF, "du")
        hold("dact", f"prec{prec}_v{variant}", du[:M, :N], ref, mag)
        if pl is not None:
            owned(pl, M, N, NANH, "planes")
            planes_are_the_split(dict(du=du, planes=pl), M, N)


ROW_MAJOR = {(1, 11), (1, 12), (1, 13), (2, 11), (2, 12), (2, 13)}   # the 16-B row-major epilogue runs


@pytest.mark.parametrize("prec,variant", [(0, 0), (1, 4), (1, 10), (1, 11), (1, 12), (1, 13), (2, 11), (2, 13)])
@pytest.mark.parametrize("padw", [1, 2])
@pytest.mark.parametrize("epi", [_lib.EPI_ACT, _lib.EPI_DACT], ids=["act", "dact"])
def test_epi_act_padding_columns(prec, variant, padw, epi):
    """padw 1 / 2 at N % 8 != 0: each padding column [N, round8(N)) holds its constant (1.0 at column N
    with padw 2, else 0) wherever the 16-B row-major epilogue runs, and that constant or the prefill
    wherever another epilogue runs; columns from round8(N) on, and the guard row, are untouched. At N %
    8 = 0 nothing past N is written. The values are held to float64."""
    M, K = 300, 65
    for N in (260, 301, 392):
        rng = np.random.default_rng(N + padw)
        A = rng.standard_normal((M, K)).astype(np.float32)
        B = (rng.standard_normal((K, N)) * 0.15).astype(np.float32)
        aux = np.tanh(rng.standard_normal((M, N))).astype(np.float32)
        if prec == 1:
            A, B, aux = bf16_exact(A), bf16_exact(B), bf16_exact(aux)
        r = E.act(A, B, 0) if epi == _lib.EPI_ACT else E.dact(A, B, aux, 0)
        ld = r8(N) + 8
        a = _lib.mvae_epi_args()
        keep = [padded(A, r8(K)), padded(B, r8(N)), padded(aux, ld, M + 1)]   # (aux padding: zeros, as the step's)
        a.M, a.N, a.K, a.lda, a.ldb, a.A, a.B = M, N, K, r8(K), r8(N), keep[0].data_ptr(), keep[1].data_ptr()
        a.prec, a.variant, a.epi, a.act, a.padw = prec, variant, epi, 0, padw
        if epi == _lib.EPI_DACT:
            a.aux, a.ld_aux = keep[2].data_ptr(), ld
        du, pl = run_out(a, M, N, ld, ncp_of(prec), keep)
        hold("padw", f"prec{prec}_v{variant}", du[:M, :N], dev(r["out"]), dev(r["mag"]))
        want = torch.zeros(M, r8(N) - N, device="cuda")
        if padw == 2 and N % 8:
            want[:, 0] = 1.0
        bufs = [(bits_f32(du), want.view(torch.int32), NANF)]
        if pl is not None:
            planes_are_the_split(dict(du=du, planes=pl), M, N)
            wp = torch.zeros(pl.shape[0], M, r8(N) - N, dtype=torch.int16, device="cuda")
            wp[0] = want.bfloat16().view(torch.int16)
            bufs.append((pl, wp, NANH))
        for b, w, pre in bufs:
            assert not (b[..., :M, :N] == pre).any()
            pad = b[..., :M, N:r8(N)]
            if (prec, variant) in ROW_MAJOR:
                assert torch.equal(pad, w), "padding columns"
            else:
                assert ((pad == w) | (pad == pre)).all(), "padding columns"
            assert (b[..., :M, r8(N):] == pre).all() and (b[..., M:, :] == pre).all()
