"""The plane side of batch input, pinned bit for bit (mvae_debug_input_planes against the host reference
of tests/planes_ref.py): the plane path's three de-interleave forms with residual_planes_kernel, and the
grey pass of the three bits routes. Everything a route writes -- bf16 planes 0-2, the fp32 rows of both
masks, the target bits, the four flag ints (and the routes' BitMats, against tests/bits_ref.py) --
equals the reference; everything else comes back as it went in.

Every output buffer is prefilled with the NaN bit patterns of tests/test_gpu_head.py (fp32 0x7FC12345,
bf16 0x7FC1), xbits with 0xA5, and carries a guard tail and a gap between the planes: columns D .. ldx,
blocks outside the masks, the residual planes of an exact batch, the unused flag slot's junk (which the
launch has to zero) are all compared. All comparisons are exact: the kernels move bits and round to
nearest even.

Shapes are the smallest that reach each branch: one and two workgroups of each form, the
alignment and stride fallbacks, residual_planes_kernel's grid stride (B D = 524 680 > 2048 x 256
threads) and the grey pass's (65 600 octets > 256 x 256 threads). Values: 0/1; exact grey (multiples of
2^-7; 255); every byte over 255; a 0/1 batch with a single inexact value at the first and at the last
element (the flag's ballot with one lane); the rounding ties of tests/test_planes_ref.py; full-mantissa
values of both signs in [2^-20, 2^20]. Denormals, infinities, NaN and -0 are outside the pinned domain.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from magic_amd import _lib
from oracle import input_oracle
from tests import bits_ref, planes_ref
from tests.test_planes_ref import TIES

pytestmark = pytest.mark.gpu

NAN32, NAN16, FILL8, GUARD, GAP = 0x7FC12345, 0x7FC1, 0xA5, 64, 24
# (np, f32mask, f32dyn_mask): the step's masks -- the BCE target on the flag (plane modes), always (the
# conv tower's), every block (fp32), none (the bits head)
MASKS = [(0, 2), (2, 0), (7, 0), (0, 0)]
CONFIGS = [(n, fm, fdm) for n in (1, 3) for fm, fdm in MASKS] + [(0, 7, 0)]
BITS_CONFIGS = [(n, 0, fdm) for n in (1, 3) for fdm in (2, 0)]
SEVENTH = np.float32(7) / np.float32(255)

# name -> (B, D, ldx, x_off floats past a 16-byte boundary, the form)
ROUTE0 = {"oct_3x8": (3, 8, 16, 0, planes_ref.OCT), "oct_2x64": (2, 64, 72, 0, planes_ref.OCT),
          "oct_2x2304": (2, 2304, 2312, 0, planes_ref.OCT),            # 288 octets: a second, partly filled workgroup
          "quad_3x4": (3, 4, 8, 0, planes_ref.QUAD), "quad_2x100": (2, 100, 104, 0, planes_ref.QUAD),
          "quad_2x1028": (2, 1028, 1032, 0, planes_ref.QUAD),          # 257 quads
          "quad_2x64_ldx68": (2, 64, 68, 0, planes_ref.QUAD),
          "scalar_3x1": (3, 1, 4, 0, planes_ref.SCALAR), "scalar_2x25": (2, 25, 28, 0, planes_ref.SCALAR),
          "scalar_2x259": (2, 259, 262, 0, planes_ref.SCALAR),
          "scalar_2x64_x_off1": (2, 64, 72, 1, planes_ref.SCALAR), "scalar_2x64_ldx65": (2, 64, 65, 0, planes_ref.SCALAR),
          "stride_65x8072": (65, 8072, 8080, 0, planes_ref.OCT)}       # residual_planes_kernel strides
BIG = {"stride_65x8072": (("bytes255", "one_last", "bin"), [(3, 0, 2), (1, 0, 2), (3, 7, 0)])}
BITS_SHAPES = [(64, 8, 8), (64, 12, 12), (128, 20, 20), (64, 82, 100)]   # the last: the grey pass strides
X_VALUES = ("bin", "grey_exact", "255", "bytes255", "one_first", "one_last", "ties", "full")
TABLE_VALUES = ("bin", "grey_exact", "255", "bytes255", "one_first", "one_last")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared batches are read-only)


# ------------------------------------------------------------------ batches

@functools.lru_cache(maxsize=None)
def x_batch(B, D, values):
    """X [B][3 D] float32 of a value class (read-only)."""
    rng = np.random.default_rng(7919 * B + D)
    n = B * 3 * D
    binary = (rng.random(n) < 0.3).astype(np.float32)
    if values == "bin":
        x = binary
    elif values == "grey_exact":
        x = rng.integers(0, 256, n).astype(np.float32) * np.float32(2.0 ** -7)
    elif values == "255":
        x = binary * np.float32(255)
    elif values == "bytes255":
        x = ((np.arange(n) * 37 + rng.integers(0, 256)) % 256).astype(np.float32) / np.float32(255)
    elif values == "one_first":     # the first pixel of row 0's lock
        x = binary
        x[0] = SEVENTH
    elif values == "one_last":      # the last pixel of the last row's key
        x = binary
        x[-1] = SEVENTH
    elif values == "ties":
        t = np.array(list(TIES), np.uint32).view(np.float32)
        x = t[(np.arange(n) * 5 + 3) % len(t)]
    else:
        assert values == "full"
        x = (np.exp2(rng.uniform(-20, 20, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    x = np.ascontiguousarray(x.reshape(B, 3 * D), np.float32)
    x.setflags(write=False)
    return x


def check_class(values, R):
    """the batch is what its name says (on the reference's side)"""
    grey, inexact = bool(((R != 0) & (R != 1)).any()), planes_ref.inexact(R)
    assert grey == (values != "bin") and inexact == (values not in ("bin", "grey_exact", "255")), values
    if values in ("one_first", "one_last"):
        assert int(((R != 0) & (R != 1)).sum()) in (1, 2)   # (2: a rotated lock samples the lock's pixel)
    if values == "bytes255" and R.size >= 3 * 256:
        assert len(np.unique(R)) == 256


@functools.lru_cache(maxsize=None)
def table_batch(B, H, W, values):
    """One batch in the three bits routes' forms, built on the host as tests/test_gpu_bits.py builds its
    own: the uint8 lock / key tables with (idx, key_idx, coef) -- every image used once, so a single
    changed byte is a single value of the batch (and of its rotation) --; the stacked rows' images,
    shuffled, as one table with its idx [3B]; the host's X."""
    rng = np.random.default_rng(1000 * B + 10 * H + W)
    hi, div = (255, 1.0) if values == "255" else (255, 128.0) if values == "grey_exact" else (255, 255.0)
    if values in ("grey_exact", "bytes255"):
        L = rng.integers(0, 256, (B, H, W)).astype(np.uint8)
        K = rng.integers(0, 256, (B, H, W)).astype(np.uint8)
        K.reshape(-1)[:256] = np.arange(256)
    else:
        L = ((rng.random((B, H, W)) < 0.3) * hi).astype(np.uint8)
        K = ((rng.random((B, H, W)) < 0.3) * hi).astype(np.uint8)
    idx, kidx = rng.permutation(B).astype(np.int32), rng.permutation(B).astype(np.int32)
    if values == "one_first":
        L[idx[0], 0, 0] = 7
    if values == "one_last":
        K[kidx[B - 1], H - 1, W - 1] = 7
    coef = input_oracle.rotation_coefficients(rng.uniform(0, 2 * np.pi, B).astype(np.float32), H, W)
    x = input_oracle.make_batch(L[idx], K[kidx], np.arange(B), coef, scale_div=div)
    rows = np.concatenate([np.stack([input_oracle.rotate_nearest(L[i], c) for i, c in zip(idx, coef)]),
                           L[idx], K[kidx]])  # [3B][H][W] uint8: rot | lock | key
    perm = rng.permutation(3 * B)
    out = dict(L=L, K=K, idx=idx, kidx=kidx, coef=coef, x=x, table=rows[perm], tidx=np.argsort(perm).astype(np.int32),
               div=div)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------ buffers and the call

class Layout:
    def __init__(self, B, D, ldx, ldbits, bits):
        self.B, self.D, self.ldx, self.ldbits, self.bits = B, D, ldx, ldbits, bits
        self.rows = 3 * B * ldx
        self.ps = self.rows + GAP

    def fresh(self, slot):
        """Prefilled device buffers: three planes' room whatever np, the used flag slot zero and junk in
        the other one, zeroed BitMats."""
        full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device="cuda")  # noqa: E731
        dyn = [0, 0, 0, 0]
        dyn[1 - slot], dyn[3 - slot] = 5, 9
        b = dict(planes=full(2 * self.ps + self.rows + GUARD, NAN16, torch.int16),
                 xs=full(self.rows + GUARD, NAN32, torch.int32),
                 xbits=full(self.B * self.ldbits + GUARD, FILL8, torch.uint8),
                 dyn=torch.tensor(dyn, dtype=torch.int32, device="cuda"))
        if self.bits:
            b["xbf"] = full(bits_ref.bitmat_words(3 * self.B, self.D + 1), 0, torch.int32)
            b["xbw"] = full(bits_ref.bitmat_words(self.D + 1, 3 * self.B), 0, torch.int32)
        return b

    def apply(self, images, ref, np_):
        """The buffers' host images after a call that writes `ref` over `images`."""
        out = {k: v.copy() for k, v in images.items()}
        P, Pm = ref["planes"]
        for t in range(np_):
            v = out["planes"][t * self.ps: t * self.ps + self.rows].reshape(3 * self.B, self.ldx)
            v[Pm[t]] = P[t][Pm[t]]
        xs, xm = ref["xs"]
        v = out["xs"][:self.rows].reshape(3 * self.B, self.ldx)
        v[xm] = xs.view(np.uint32)[xm]
        xb, xbm = ref["xbits"]
        v = out["xbits"][:self.B * self.ldbits].reshape(self.B, self.ldbits)
        v[xbm] = xb[xbm]
        out["dyn"] = ref["dyn"].copy()
        for k in ("xbf", "xbw"):
            if k in ref:
                out[k] = ref[k].copy()
        return out


VIEW = dict(planes=np.uint16, xs=np.uint32, xbits=np.uint8, dyn=np.int32, xbf=np.uint32, xbw=np.uint32)


def host(bufs):
    return {k: v.cpu().numpy().view(VIEW[k]) for k, v in bufs.items()}


def call(route, lay, H, W, np_, fm, fdm, slot, bufs, x=None, tb=None):
    """One call of the entry on the device buffers `bufs`; x: a device tensor view (routes 0, 1)."""
    lib = _lib.load()
    a = _lib.mvae_input_args()
    a.route, a.B, a.H, a.W, a.ldx, a.np = route, lay.B, H, W, lay.ldx, np_
    a.f32mask, a.f32dyn_mask, a.ldbits, a.no_xbw, a.slot = fm, fdm, lay.ldbits, 0, slot
    a.plane_stride, a.planes_elems = lay.ps, bufs["planes"].numel() - GUARD
    a.xs_elems, a.xbits_elems = lay.rows, lay.B * lay.ldbits
    for k in ("planes", "xs", "xbits", "dyn", "xbf", "xbw"):
        if k in bufs:
            setattr(a, k, bufs[k].data_ptr())
    keep = []
    if route <= 1:
        a.x, a.x_elems = x.data_ptr(), x.numel()
    elif route == 2:
        keep = [dev(tb[k]) for k in ("L", "K", "idx", "kidx", "coef")]
        a.locks, a.keys, a.idx, a.key_idx, a.coef = (t.data_ptr() for t in keep)
        a.divisor = tb["div"]
    else:
        keep = [dev(tb["table"]), dev(tb["tidx"])]
        a.locks, a.idx = (t.data_ptr() for t in keep)
        a.divisor = tb["div"]
    rc = lib.mvae_debug_input_planes(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mvae_last_error(None)
    torch.cuda.synchronize()


def x_dev(x, off=0):
    """x on the device, `off` floats past a 16-byte boundary"""
    t = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[off: off + x.size]
    v.copy_(torch.from_numpy(x.reshape(-1).copy()))   # (a copy: the shared batches are read-only)
    return v


def same(got, want, what):
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


# ------------------------------------------------------------------ route 0: the plane path

R0_CASES = [(s, v) for s in ROUTE0 for v in (BIG[s][0] if s in BIG else X_VALUES)]


@pytest.mark.parametrize("shape,values", R0_CASES, ids=[f"{s}-{v}" for s, v in R0_CASES])
def test_plane_path_writes_the_reference_and_nothing_else(shape, values):
    B, D, ldx, off, form = ROUTE0[shape]
    x = x_batch(B, D, values)
    check_class(values, bits_ref.stacked_rows(x, B, D))
    xd = x_dev(x, off)
    lay = Layout(B, D, ldx, D // 8 + 3, bits=False)
    for i, (np_, fm, fdm) in enumerate(BIG[shape][1] if shape in BIG else CONFIGS):
        for slot in ((i & 1,) if shape in BIG else (0, 1)):
            ref = planes_ref.route0(x, B, D, ldx, lay.ldbits, np_, fm, fdm, slot, x_aligned=off % 4 == 0)
            assert ref["form"] == form
            bufs = lay.fresh(slot)
            before = host(bufs)
            call(0, lay, 1, D, np_, fm, fdm, slot, bufs, x=xd)
            same(host(bufs), lay.apply(before, ref, np_), (shape, values, np_, fm, fdm, slot))
            # the case is what it says: the flag and the residual planes go together
            rose = bool(ref["dyn"][slot])
            assert rose == (np_ >= 1 and values not in ("bin", "grey_exact", "255"))
            assert bool(ref["planes"][1][1:].any()) == (rose and np_ == 3)
            assert ref["dyn"][2 + slot] == int(values != "bin" or form != planes_ref.OCT)


def test_plane_path_without_target_bits():
    """xbits is optional on the plane path: a NULL pointer changes nothing else."""
    B, D, ldx, _, _ = ROUTE0["oct_2x64"]
    x = x_batch(B, D, "bytes255")
    lay = Layout(B, D, ldx, D // 8 + 3, bits=False)
    bufs = lay.fresh(0)
    before = host(bufs)
    ref = planes_ref.route0(x, B, D, ldx, lay.ldbits, 3, 0, 2, 0)
    ref["xbits"] = (ref["xbits"][0], np.zeros_like(ref["xbits"][1]))
    xb = bufs.pop("xbits")
    call(0, lay, 1, D, 3, 0, 2, 0, bufs, x=x_dev(x))
    bufs["xbits"] = xb
    same(host(bufs), lay.apply(before, ref, 3), "no xbits")


# ------------------------------------------------------------------ routes 1-3: the grey pass

def _bits_ref(x, lay, np_, fdm, slot):
    ref = planes_ref.bits_route(x, lay.B, lay.D, lay.ldx, lay.ldbits, np_, fdm, slot)
    return ref


@functools.lru_cache(maxsize=None)
def _bitmats(B, H, W, values):
    tb = table_batch(B, H, W, values)
    o = bits_ref.operand(tb["x"], B, H * W, H * W + 8, H * W // 8 + 3)
    return o["xbf"], o["xbw"]


BITS_CASES = [(b, h, w, v) for b, h, w in BITS_SHAPES
              for v in (("bin", "bytes255", "one_last") if h * w > 4096 else TABLE_VALUES)]


@pytest.mark.parametrize("route", [1, 2, 3], ids=["x", "pairs", "images"])
@pytest.mark.parametrize("B,H,W,values", BITS_CASES, ids=[f"B{b}_{h}x{w}-{v}" for b, h, w, v in BITS_CASES])
def test_bits_routes_write_the_reference_and_nothing_else(B, H, W, values, route):
    D = H * W
    tb = table_batch(B, H, W, values)
    check_class(values, bits_ref.stacked_rows(tb["x"], B, D))
    lay = Layout(B, D, D + 8, D // 8 + 3, bits=True)
    xd = x_dev(tb["x"]) if route == 1 else None
    xbf, xbw = _bitmats(B, H, W, values)
    for i, (np_, fm, fdm) in enumerate(BITS_CONFIGS):
        for slot in ((i & 1,) if D > 4096 else (0, 1)):
            ref = dict(_bits_ref(tb["x"], lay, np_, fdm, slot), xbf=xbf, xbw=xbw)
            bufs = lay.fresh(slot)
            before = host(bufs)
            call(route, lay, H, W, np_, fm, fdm, slot, bufs, x=xd, tb=tb)
            same(host(bufs), lay.apply(before, ref, np_), (route, B, H, W, values, np_, fdm, slot))
            grey = values != "bin"
            assert ref["dyn"].tolist()[slot::2] == [int(values not in ("bin", "grey_exact", "255")), int(grey)]
            assert bool(ref["planes"][1].any()) == grey


X_ONLY = [(64, 8, 8, "ties"), (64, 12, 12, "full"), (128, 20, 20, "ties"), (128, 20, 20, "full")]


@pytest.mark.parametrize("B,H,W,values", X_ONLY, ids=[f"B{b}_{h}x{w}-{v}" for b, h, w, v in X_ONLY])
def test_grey_pass_splits_ties_and_full_mantissas(B, H, W, values):
    D = H * W
    x = x_batch(B, D, values)
    lay = Layout(B, D, D + 8, D // 8 + 3, bits=True)
    o = bits_ref.operand(x, B, D, lay.ldx, lay.ldbits)
    xd = x_dev(x)
    for np_, fm, fdm in BITS_CONFIGS:
        for slot in (0, 1):
            ref = dict(_bits_ref(x, lay, np_, fdm, slot), xbf=o["xbf"], xbw=o["xbw"])
            assert ref["dyn"].tolist()[slot::2] == [1, 1]
            bufs = lay.fresh(slot)
            before = host(bufs)
            call(1, lay, H, W, np_, fm, fdm, slot, bufs, x=xd)
            same(host(bufs), lay.apply(before, ref, np_), (B, H, W, values, np_, fdm, slot))


# ------------------------------------------------------------------ the sequence: stale residue stays

@pytest.mark.parametrize("shape", ["oct_2x64", "oct_2x2304", "quad_2x100", "scalar_2x25"])
def test_plane_path_leaves_the_residual_planes_of_the_batch_before(shape):
    """A grey inexact batch in slot 0, then a 0/1 batch in slot 1 on the same buffers: plane 0 is the
    second batch's, the flags read zero (the 8-pixel form; the others keep the not-binary word up), and
    planes 1-2 and the f32dyn_mask rows are still the first batch's -- what the GEMM gate must not read."""
    B, D, ldx, off, form = ROUTE0[shape]
    lay = Layout(B, D, ldx, D // 8 + 3, bits=False)
    first, second = x_batch(B, D, "bytes255"), x_batch(B, D, "bin")
    bufs = lay.fresh(0)
    img0 = host(bufs)
    call(0, lay, 1, D, 3, 0, 2, 0, bufs, x=x_dev(first, off))
    img1 = lay.apply(img0, planes_ref.route0(first, B, D, ldx, lay.ldbits, 3, 0, 2, 0), 3)
    same(host(bufs), img1, "first")
    call(0, lay, 1, D, 3, 0, 2, 1, bufs, x=x_dev(second, off))
    ref2 = planes_ref.route0(second, B, D, ldx, lay.ldbits, 3, 0, 2, 1)
    got = host(bufs)
    same(got, lay.apply(img1, ref2, 3), "second")
    assert got["dyn"].tolist() == [0, 0, 0, int(form != planes_ref.OCT)]
    rows = lay.rows
    p0 = got["planes"][:rows].reshape(3 * B, ldx)[:, :D]
    assert np.array_equal(p0, ref2["planes"][0][0][:, :D]) and set(np.unique(p0)) <= {0, 0x3F80}
    assert np.array_equal(got["planes"][lay.ps:], img1["planes"][lay.ps:])
    stale = got["planes"][lay.ps: lay.ps + rows].reshape(3 * B, ldx)[:, :D]
    assert (stale != NAN16).all() and stale.any()
    assert np.array_equal(got["xs"], img1["xs"]) and (got["xs"][:rows].reshape(3 * B, ldx)[B:2 * B, :D] != NAN32).all()


@pytest.mark.parametrize("route", [1, 2, 3], ids=["x", "pairs", "images"])
def test_bits_routes_leave_the_planes_of_the_batch_before(route):
    """The same on a bits route: the 0/1 batch writes its bit operands and zeroed flags, and no plane."""
    B, H, W = 64, 8, 8
    D = H * W
    lay = Layout(B, D, D + 8, D // 8 + 3, bits=True)
    first, second = table_batch(B, H, W, "bytes255"), table_batch(B, H, W, "bin")
    bufs = lay.fresh(0)
    img = host(bufs)
    for slot, tb, values in ((0, first, "bytes255"), (1, second, "bin")):
        xbf, xbw = _bitmats(B, H, W, values)
        ref = dict(_bits_ref(tb["x"], lay, 3, 2, slot), xbf=xbf, xbw=xbw)
        # (the BitMats' padding is never written and both batches fill the same words)
        call(route, lay, H, W, 3, 0, 2, slot, bufs, x=x_dev(tb["x"]) if route == 1 else None, tb=tb)
        prev, img = img, lay.apply(img, ref, 3)
        same(host(bufs), img, values)
    assert img["dyn"].tolist() == [0, 0, 0, 0]
    assert np.array_equal(img["planes"], prev["planes"]) and np.array_equal(img["xs"], prev["xs"])
    assert (img["planes"][: lay.rows].reshape(3 * B, lay.ldx)[:, :D] != NAN16).all()
