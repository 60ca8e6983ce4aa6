"""The GEMMs' batch, split-K slice and tile-order indexing, pinned per element (mvae_debug_gemm_ex over the
cases of tests/gemm_cases.py; tests/test_abi_gemm_ex.py shows on the CPU that the cases reach every
kernel family, ring tile, empty and one-k-tile last slice, ragged band and alignment fallback).

Operands are built on the host from a seed: bf16-representable normals (A of 0/1 values where it is also
given as bits), zero row padding, so the fp32, bf16 and f32x modes answer to one bar; C is a buffer of
NaN with ldc > N and, where the case allows, a gap between the batch windows. For every case and every
batch element:
 * float64: |C_b - A_b B_b| <= 2e-6 max(|A_b| |B_b|) + 1e-6 (+ 1e-5 behind an activation), the product
   taken over that element's views, overlapping windows included (the bar of test_gpu_bf16_exact.py);
 * nothing else written: outside the batch windows' [M][:N] the buffer is still NaN, inside finite;
 * batched == one at a time, bitwise, with the same forces, and the two plans agree;
 * the tile order changes nothing, bitwise; two runs of a split are bitwise equal;
 * the bits paths equal the plane path (bitwise in bf16, 1e-6 mag + 1e-7 in f32x), the shared BitMat
   the per-element ones, bitwise.
The entry fills its split-K workspace with NaN bits before the launch, so the zero slab of an empty
slice is the kernel's own.
"""
import ctypes

import pytest
import torch

from magic_amd import _lib
from tests import gemm_cases as G
from tests.gemm_cases import E8, F32, PLANE, RING, VALU, X3

pytestmark = pytest.mark.gpu

# worst error / bound on an MI355X (gfx950) over the batched cases of each kernel family (a record, not
# used by the assertions: the bound is 1)
RATIOS_MEASURED = {"f32": 0.0316, "valu": 0.0316, "plane": 0.0428, "ring": 0.0376, "x3": 0.0367, "e8": 0.0376,
                   "e8_bits": 0.0087}

FORCED = [c for c in G.CASES if c["variant"] != 0 and c["split"] > 0]
GROUPED = [c for c in G.CASES if c["group"] > 0]
SPLIT = [c for c in G.CASES if c["split"] > 1]
BITS = [c for c in G.CASES if c["bits"] and c["variant"] == 13]
SHARED = [c for c in G.CASES if c["bits_shared"]]
ids = lambda cs: [c["name"] for c in cs]  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _values(rows, cols, g, binary):
    if binary:
        return (torch.rand(rows, cols, generator=g) < 0.37).float()
    return torch.randn(rows, cols, generator=g).bfloat16().float()


def _operand(n, batch, stride, rows, cols, ld, g, binary=False):
    """A zeroed host buffer of n floats with every batch window's [rows][:cols] filled (overlapping
    windows share their rows: the later fill stands)."""
    buf = torch.zeros(n)
    for b in range(batch):
        buf[b * stride: b * stride + rows * ld].view(rows, ld)[:, :cols] = _values(rows, cols, g, binary)
    return buf


_OPERANDS, _RUNS, _REFS = {}, {}, {}


def _operands(c):
    """(A, B) device buffers of the case, built once from the seed its shape gives."""
    key = c["name"]
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(1000003 * c["M"] + 1009 * c["N"] + c["K"] + 7 * c["batch"] + c["at"])
        (ar, ac), (br, bc) = G.a_shape(c), G.b_shape(c)
        A = _operand(c["a_elems"], c["batch"], c["sA"], ar, ac, c["lda"], g, binary=c["bits"] != 0)
        B = _operand(c["b_elems"], c["batch"], c["sB"], br, bc, c["ldb"], g)
        _OPERANDS[key] = (A.cuda(), B.cuda())
    return _OPERANDS[key]


def _launch(c, A, B):
    """One call of the entry on device buffers A, B: (the NaN-prefilled C buffer, the reported plan)."""
    lib = _lib.load()
    C = torch.full((c["c_elems"],), float("nan"), device="cuda")
    a = G.fill_args(_lib.mvae_gemm_args(), c, A=A.data_ptr(), B=B.data_ptr(), C=C.data_ptr())
    o = _lib.mvae_plan_out()
    rc = lib.mvae_debug_gemm_ex(ctypes.byref(a), ctypes.byref(o), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (c["name"], lib.mvae_last_error(None))
    torch.cuda.synchronize()
    return C, {f[0]: getattr(o, f[0]) for f in _lib.mvae_plan_out._fields_}


def _run(c, **over):
    """The case (with fields overridden) on its operands, run once and kept."""
    key = (c["name"], tuple(sorted(over.items())))
    if key not in _RUNS:
        _RUNS[key] = _launch({**c, **over}, *_operands(c))
    return _RUNS[key]


def _window(c, buf, b):
    return buf[b * c["sC"]: b * c["sC"] + c["M"] * c["ldc"]].view(c["M"], c["ldc"])[:, :c["N"]]


def _views(c, b):
    """float64 A_b [M][K] and B_b [K][N] of batch element b, from the device buffers."""
    A, B = _operands(c)
    (ar, ac), (br, bc) = G.a_shape(c), G.b_shape(c)
    Ab = A[b * c["sA"]: b * c["sA"] + ar * c["lda"]].view(ar, c["lda"])[:, :ac].double()
    Bb = B[b * c["sB"]: b * c["sB"] + br * c["ldb"]].view(br, c["ldb"])[:, :bc].double()
    return (Ab.T if c["at"] else Ab), (Bb.T if c["bt"] else Bb)


def _ref(c, b):
    """(float64 reference, max |A_b| |B_b|) of batch element b, computed once."""
    key = (c["name"], b)
    if key not in _REFS:
        Ab, Bb = _views(c, b)
        acc = Ab @ Bb
        if c["epi"] == 1:
            acc = torch.tanh(acc) if c["act"] == 0 else torch.where(acc < 0, torch.expm1(acc), acc)
        _REFS[key] = (acc, (Ab.abs() @ Bb.abs()).max().item())
    return _REFS[key]


@pytest.mark.parametrize("c", G.CASES, ids=ids(G.CASES))
def test_batch_elements_match_float64_and_nothing_else_is_written(c):
    buf, plan = _run(c)
    inside = torch.zeros(c["c_elems"], dtype=torch.bool, device="cuda")
    worst = 0.0
    for b in range(c["batch"]):
        ref, mag = _ref(c, b)
        bound = 2e-6 * mag + (1e-5 if c["epi"] == 1 else 1e-6)
        got = _window(c, buf, b)
        assert torch.isfinite(got).all(), (c["name"], b)
        worst = max(worst, (got.double() - ref).abs().max().item() / bound)
        _window(c, inside, b).fill_(True)
    print(f"GEMMB_RATIO {_lib.KERNEL_NAMES[plan['kernel']]} {c['name']} {plan['tm']}x{plan['tn']} split "
          f"{plan['split']} kchunk {plan['kchunk']} group {plan['group']} vec {plan['vec_epilogue']} ratio={worst:.4f}")
    assert worst <= 1.0, (c["name"], worst)
    assert torch.isnan(buf[~inside]).all(), c["name"]
    if c["split"] > 0:
        assert plan["split"] == c["split"]
    if c["group"] > 0 and plan["kernel"] in (RING, X3, E8):
        assert plan["group"] == c["group"]


@pytest.mark.parametrize("c", FORCED, ids=ids(FORCED))
def test_batched_equals_one_at_a_time_bitwise(c):
    """Element b alone, as a batch of one on its own views (the same forces; its plane images in the
    alignment class they have inside the batch): the same plan, the same bits."""
    buf, plan = _run(c)
    A, B = _operands(c)
    (ar, _), (br, _) = G.a_shape(c), G.b_shape(c)
    for b in range(c["batch"]):
        one = dict(c, batch=1, sA=0, sB=0, sC=0, a_elems=ar * c["lda"], b_elems=br * c["ldb"],
                   c_elems=c["M"] * c["ldc"], bits_shared=0,
                   a_off=(c["a_off"] + b * c["sA"]) % 8, b_off=(c["b_off"] + b * c["sB"]) % 8)
        # a 256-row kernel the batch strides alone kept the batch from (sA, sB % 8: read only when batch
        # > 1): the one-element call names the kernel the batch ran on
        if plan["kernel"] == PLANE and c["variant"] != 4 and one["a_off"] == 0 and one["b_off"] == 0:
            one["variant"] = 4
        got, p1 = _launch(one, A[b * c["sA"]:], B[b * c["sB"]:])
        for k in ("kernel", "tm", "tn", "split", "kchunk"):
            assert p1[k] == plan[k], (c["name"], b, k, p1, plan)
        assert torch.equal(_window(one, got, 0), _window(c, buf, b)), (c["name"], b)


@pytest.mark.parametrize("c", GROUPED, ids=ids(GROUPED))
def test_tile_order_changes_nothing_bitwise(c):
    (banded, pb), (rows, pr) = _run(c), _run(c, group=-1)
    assert pb["group"] == c["group"] and pr["group"] == 0
    assert pb["ntm"] % c["group"] != 0 or c["group"] == 1, "the last band is ragged"
    for k in ("kernel", "tm", "tn", "ntm", "ntn", "split", "kchunk"):
        assert pb[k] == pr[k], (k, pb, pr)
    assert torch.equal(torch.nan_to_num(banded, nan=-7.0), torch.nan_to_num(rows, nan=-7.0))


@pytest.mark.parametrize("c", SPLIT, ids=ids(SPLIT))
def test_split_runs_are_bitwise_repeatable(c):
    """The slabs are summed in a fixed order: a second launch (a fresh workspace of NaN bits) gives the
    same bits. With an empty last slice the sum reads that slice's slab: zeros the kernel wrote."""
    first, plan = _run(c)
    again, _ = _launch(c, *_operands(c))
    assert plan["split"] == c["split"] and plan["ws_elems"] == c["batch"] * c["split"] * c["M"] * c["N"]
    assert torch.equal(torch.nan_to_num(first, nan=-7.0), torch.nan_to_num(again, nan=-7.0))


@pytest.mark.parametrize("c", BITS, ids=ids(BITS))
def test_bits_paths_equal_the_plane_path(c):
    """A as a BitMat against the same case on A's planes: the same products in the same order in bf16
    (bitwise); in f32x the bits path walks a k-tile's plane pairs innermost, the plane path k-tiles in
    pairs -- 1e-6 mag + 1e-7, the relations test_gpu_r6.py holds at batch 1."""
    (bits, pb), (planes, pp) = _run(c), _run(c, bits=0, bits_shared=0)
    for k in ("kernel", "tm", "tn", "ntm", "ntn", "group", "split", "kchunk"):
        assert pb[k] == pp[k] and pb["kernel"] == E8, (k, pb, pp)
    for b in range(c["batch"]):
        x, y = _window(c, bits, b), _window(c, planes, b)
        if c["prec"] == G.PREC_BF16:
            assert torch.equal(x, y), (c["name"], b)
        else:
            assert (x.double() - y.double()).abs().max().item() <= 1e-6 * _ref(c, b)[1] + 1e-7, (c["name"], b)


@pytest.mark.parametrize("c", SHARED, ids=ids(SHARED))
def test_shared_bitmat_equals_one_per_element_bitwise(c):
    """One BitMat of the whole stored A, a batch element a k-tile offset into every strip (the step's
    layer-0 weight gradient), against one BitMat per element: the same bits read, the same result."""
    (shared, ps), (each, pe) = _run(c), _run(c, bits_shared=0)
    assert ps == pe and ps["kernel"] == E8
    assert torch.equal(torch.nan_to_num(shared, nan=-7.0), torch.nan_to_num(each, nan=-7.0))


def test_cases_cover_every_family_on_this_device():
    """The plans the entry reports on the device are the ones the CPU test asked mvae_debug_plan for."""
    seen = {}
    for c in G.CASES:
        if c["batch"] >= 2:
            _, p = _run(c)
            seen.setdefault(p["kernel"], set()).add((p["tm"], p["tn"], p["split"] > 1))
    assert set(seen) == {F32, VALU, PLANE, RING, X3, E8}
    assert {(tm, tn) for tm, tn, _ in seen[RING]} == {(256, 256), (256, 128), (192, 256), (192, 128)}
    assert all({s for _, _, s in v} == {False, True} for v in seen.values())
