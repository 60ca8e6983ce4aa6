"""The f32x plane pairs, pinned bit for bit (mvae_debug_gemm_ex over tests/gemm_cases.py PAIR_CASES;
tests/test_abi_gemm_ex.py shows on the CPU that the cases reach the plane kernel, the ring kernel at 256
and 192 rows, both plane-stacked forms, the eight-phase kernel and both of its bits forms, each unsplit and
with a partial last k-tile in its own slice).

f32x sums the plane products (i, j), i + j < 3, in the order (0,0) (0,1) (0,2) (1,1) (1,0) (2,0). The
tolerance tests cannot see a lost pair: planes 1 and 2 weigh 2^-9 and 2^-17 and the bar 2e-6 |A||B| grows
with K (DESIGN 5u has the figures). Here every output element is ONE product, so that nothing hides it:
 * pairs (i, 0): A has one nonzero per row, at k0(m) = (7 m + 3 + 11 b) % K -- the nonzeros walk the k
   positions, the partial last k-tile and every split-K slice among them --, full-mantissa normals; B
   holds +-2^e, e in -3..3: C[m][n] = A[m][k0] B[k0][n] needs A's three planes against B's plane 0;
 * pairs (0, j): the mirror image, B with one nonzero per column;
 * pair (1, 1): one nonzero per row of A and per column of B, values with 12-bit significands (plane 1
   nonzero, plane 2 zero): the 24-bit product is the sum of exactly the four pairs i, j <= 1;
 * the gate: A one-hot of 0/1 values against a dense full-mantissa B, with no flag on A, a flag word of 0
   (the kernels then run only the leading pairs with A's plane 0: the step's path for 0/1 pixels) and a
   word of 1; and A as bits (npairs_a0).
The float64 product is an fp32 number and every order of fp32 summation of the plane products is exact,
so C must equal it bit for bit: full-mantissa values are kept only where all six orders of summing their
three planes in fp32 give the value back (the rest, under 1 % of the draws, are left out), and a sum with
zeros is exact. Everything outside the batch windows' [M][:N] must still hold the NaN prefill.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from magic_amd import _lib
from tests import gemm_cases as G
from tests.epi_ref import split_planes

pytestmark = pytest.mark.gpu

PLAIN = [c for c in G.PAIR_CASES if not c["bits"]]
BITS = [c for c in G.PAIR_CASES if c["bits"]]
ids = lambda cs: [c["name"] for c in cs]  # noqa: E731
STATS = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ values

def plane_values(v):
    """the three planes of v as fp32 values [3][...]"""
    return (split_planes(v, 3).astype(np.uint32) << 16).view(np.float32)


def full_mantissa(rng, n, what):
    """n normals whose planes sum back exactly in fp32 in all six orders: the first n such of a pool of
    draws (at least 4096, so that the fraction means something for a one-hot operand of a few hundred
    values); asserts that the filter takes at most 1 % of the pool and that at least 90 % of the values
    kept reach plane 2"""
    pool = rng.standard_normal(max(2 * n, 4096)).astype(np.float32)
    p = plane_values(pool)
    ok = np.ones(len(pool), bool)
    for a, b, c in itertools.permutations(range(3)):
        ok &= ((p[a] + p[b]).astype(np.float32) + p[c]).astype(np.float32) == pool
    v, p2 = pool[ok][:n], p[2][ok][:n]
    dropped, deep = 1.0 - ok.mean(), (p2 != 0).mean()
    STATS[what] = (n, dropped, deep)
    assert len(v) == n and dropped <= 0.01 and deep >= 0.90, (what, dropped, deep)
    return v


def pow2(rng, n):
    return (rng.choice([-1.0, 1.0], n) * np.exp2(rng.integers(-3, 4, n))).astype(np.float32)


def twelve_bit(rng, n):
    """+-s 2^e with s in [2048, 4000], s % 16 != 0: plane 0 is s rounded to a multiple of 16, plane 1 the
    rest (|.| <= 8), plane 2 zero; (|p0| + |p1|)^2 < 2^24, so every partial sum of the four plane products
    of two such values is an integer of fewer than 24 bits times a power of two"""
    s = rng.integers(2048, 4001, n)
    s += (s % 16 == 0)
    v = (s * rng.choice([-1.0, 1.0], n) * np.exp2(rng.integers(-14, -7, n))).astype(np.float32)
    p = split_planes(v, 3)
    assert p[1].all() and not p[2].any()
    return v


def k_of(i, K, b):
    return (7 * i + 3 + 11 * b) % K


def one_hot(n, K, b, vals):
    """[n][K] with vals[i] at column k_of(i)"""
    out = np.zeros((n, K), np.float32)
    out[np.arange(n), k_of(np.arange(n), K, b)] = vals
    return out


def logical(c, kind, b, rng):
    """(A [M][K], B [K][N]) of batch element b for a kind of case"""
    M, N, K = c["M"], c["N"], c["K"]
    if kind == "i0":
        return one_hot(M, K, b, full_mantissa(rng, M, "A one-hot")), pow2(rng, K * N).reshape(K, N)
    if kind == "0j":
        return pow2(rng, M * K).reshape(M, K), one_hot(N, K, b, full_mantissa(rng, N, "B one-hot")).T.copy()
    if kind == "11":
        return one_hot(M, K, b, twelve_bit(rng, M)), one_hot(N, K, b, twelve_bit(rng, N)).T.copy()
    assert kind == "gate"
    return one_hot(M, K, b, np.ones(M, np.float32)), full_mantissa(rng, K * N, "B dense").reshape(K, N)


_BUILT = {}


def build(c, kind):
    """The case's device buffers (zero padding, each batch window's values) and its float64 products,
    built once."""
    key = (c["name"], kind)
    if key in _BUILT:
        return _BUILT[key]
    rng = np.random.default_rng([c["M"], c["N"], c["K"], c["at"], c["bt"], ("i0", "0j", "11", "gate").index(kind)])
    A, B, refs = np.zeros(c["a_elems"], np.float32), np.zeros(c["b_elems"], np.float32), []
    (ar, ac), (br, bc) = G.a_shape(c), G.b_shape(c)
    for b in range(c["batch"]):
        a, bm = logical(c, kind, b, rng)
        # the nonzeros reach every k-tile, the partial last one included
        nz = np.nonzero(np.abs(a).sum(0) * np.abs(bm).sum(1))[0]
        assert set(nz // 64) == set(range(-(-c["K"] // 64))), (c["name"], kind)
        A[b * c["sA"]: b * c["sA"] + ar * c["lda"]].reshape(ar, c["lda"])[:, :ac] = a.T if c["at"] else a
        B[b * c["sB"]: b * c["sB"] + br * c["ldb"]].reshape(br, c["ldb"])[:, :bc] = bm.T if c["bt"] else bm
        ref = a.astype(np.float64) @ bm.astype(np.float64)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)     # an fp32 number
        assert (np.count_nonzero(a, 1).max() <= 1 or np.count_nonzero(bm, 0).max() <= 1)  # one product each
        if kind == "11":
            pa, pb = plane_values(a).astype(np.float64), plane_values(bm).astype(np.float64)
            assert np.array_equal(sum(pa[i] @ pb[j] for i in (0, 1) for j in (0, 1)), ref)
            assert np.count_nonzero(pa[1] @ pb[1]) == np.count_nonzero(ref) >= 60   # pair (1, 1) in every element
        refs.append(torch.from_numpy(ref.astype(np.float32)).cuda())
    _BUILT[key] = (torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), refs)
    return _BUILT[key]


def launch(c, A, B, **over):
    lib = _lib.load()
    c = {**c, **over}
    C = torch.full((c["c_elems"],), float("nan"), device="cuda")
    a = G.fill_args(_lib.mvae_gemm_args(), c, A=A.data_ptr(), B=B.data_ptr(), C=C.data_ptr())
    o = _lib.mvae_plan_out()
    rc = lib.mvae_debug_gemm_ex(ctypes.byref(a), ctypes.byref(o), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (c["name"], lib.mvae_last_error(None))
    torch.cuda.synchronize()
    return C, {f[0]: getattr(o, f[0]) for f in _lib.mvae_plan_out._fields_}


def window(c, buf, b):
    return buf[b * c["sC"]: b * c["sC"] + c["M"] * c["ldc"]].view(c["M"], c["ldc"])[:, :c["N"]]


def check(c, kind, **over):
    A, B, refs = build(c, kind)
    buf, plan = launch(c, A, B, **over)
    inside = torch.zeros(c["c_elems"], dtype=torch.bool, device="cuda")
    for b, ref in enumerate(refs):
        got = window(c, buf, b)
        wrong = (got != ref) | torch.isnan(got)
        assert not wrong.any(), (c["name"], kind, over, b, int(wrong.sum()),
                                 (got.double() - ref.double()).abs().max().item())
        window(c, inside, b).fill_(True)
    assert torch.isnan(buf[~inside]).all(), c["name"]
    return plan


def expected_plan(c, **over):
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    a, o = G.plan_args(_lib.mvae_plan_args(), {**c, **over}, (ctypes.addressof(buf) + 15) & ~15), _lib.mvae_plan_out()
    assert lib.mvae_debug_plan(ctypes.byref(a), ctypes.byref(o)) == 0
    return {k: getattr(o, k) for k in ("kernel", "tm", "tn", "ntm", "ntn", "split", "kchunk")}


def same_plan(c, plan, **over):
    want = expected_plan(c, **over)
    assert {k: plan[k] for k in want} == want, (c["name"], over, plan, want)


# ------------------------------------------------------------------ the pins

@pytest.mark.parametrize("kind", ["i0", "0j", "11"])
@pytest.mark.parametrize("c", PLAIN, ids=ids(PLAIN))
def test_every_plane_pair_reaches_the_output(c, kind):
    same_plan(c, check(c, kind))


@pytest.mark.parametrize("a_dyn", [0, 1, 2])
@pytest.mark.parametrize("c", PLAIN, ids=ids(PLAIN))
def test_gate_on_a_binary_operand_changes_nothing(c, a_dyn):
    """A of 0/1 values: its residual planes are zero, so the pairs the flag word 0 skips add nothing."""
    same_plan(c, check(c, "gate", a_dyn=a_dyn), a_dyn=a_dyn)


@pytest.mark.parametrize("a_dyn", [0, 1])
@pytest.mark.parametrize("c", BITS, ids=ids(BITS))
def test_bits_paths_run_every_pair_of_b(c, a_dyn):
    """A as a BitMat: the eight-phase kernel's bits path runs the leading pairs with A's plane 0."""
    plan = check(c, "gate", a_dyn=a_dyn)
    same_plan(c, plan, a_dyn=a_dyn)
    assert plan["kernel"] == G.E8


def test_the_filter_keeps_almost_everything():
    """(after the cases above ran) 99.93 % of normals qualify and 96.5 % of those reach plane 2, counted
    on 200 000 draws; each operand asserts <= 1 % dropped and >= 90 % with a plane 2."""
    full_mantissa(np.random.default_rng(5), 200_000, "200000 draws")
    n, dropped, deep = STATS["200000 draws"]
    print(f"PAIRS_FILTER dropped {dropped:.5f} plane2 {deep:.4f}")
    assert dropped <= 0.002 and deep >= 0.95
