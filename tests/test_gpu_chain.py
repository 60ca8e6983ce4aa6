"""The fused hidden-layer chain (enc_chain.hip) on caller buffers (mvae_debug_chain), each layer
against float64, element by element.

The chain's operands are bf16 already, so the float64 product of one layer's own input (the
kernel's previous output plane, or x) with its weights is exact; the kernel may differ from
act(H W) only by its fp32 accumulation, its activation approximation and one round-to-nearest:

    |gpu - ref| <= 0.5 ulp_bf16(ref) + 2e-6 (|H| |W|)[i, j] + 1e-5,   ulp_bf16(r) = 2^(floor(log2 |r|) - 7)

(the last two terms are the fp32-GEMM and activation bars of test_gemm_layouts / test_gemm_epilogues).
A lost k-step, a stale weight stage, a mis-swizzled 8-column chunk or a wrong padding column is
hundreds of ulps. Worst error / bound measured on an MI355X over every case of test_chain_layers
and test_chain_step_stride, per rows per workgroup (RATIOS_MEASURED): 0.993 (16, 32, 48 and auto),
0.994 (64), 0.995 (80, 96); the CPU emulation in fp32 with 32-row partial sums gives 0.996. The
chain's planes are bit-identical to mvae_debug_gemm's on all 72 layers of
test_chain_matches_gemm_per_layer (ratio 0 of its bound).
"""
import ctypes as C
import functools

import pytest
import torch

from magic_amd import _lib

EINVAL = -1
FILL = 0x7FC1  # a bf16 NaN pattern no kernel writes: the prefill of every output buffer

# K0; N of each layer (K[l] = N[l-1] + 1, as in the step)
SHAPES = {
    "c3": (501, (500, 500, 500, 500)),   # C3's chain, the maximum nl
    "limits": (512, (511, 511)),         # 16 k-steps; the ones column is column 511, the block's last
    "ragged": (33, (65, 127, 1)),        # a k-step of one row; one column past a wave's 64; K = 128; N = 1
    "tiny": (3, (8, 16)),                # fewer k-steps than weight stages; ones column opens a chunk
    "dec": (21, (500, 500)),             # the C2 / C3 decoder chain
    "onestep": (32, (63, 64)),           # exactly one k-step; N + 1 = 64; K = 64
    "narrow": (300, (7,)),               # one layer narrower than a chunk
}
ROWS = (16, 32, 48, 64, 80, 96)
MMAX = 2 * 96 + 1

# worst error / bound on an MI355X (gfx950), all shapes, layers and M of test_chain_layers, by rows
# (a record, not used by the assertions: the bound is 1)
RATIOS_MEASURED = {0: 0.9928, 16: 0.9935, 32: 0.9935, 48: 0.9935, 64: 0.9944, 80: 0.9954, 96: 0.9954}

gpu = pytest.mark.gpu


@pytest.fixture
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def round8(n):
    return (n + 7) // 8 * 8


def ulp_bf16(r):
    """2^(floor(log2 |r|) - 7); 0 at r = 0."""
    return torch.exp2(torch.floor(torch.log2(r.abs())) - 7)


def layer_K(K0, Ns):
    return [K0] + [n + 1 for n in Ns[:-1]]


@functools.lru_cache(maxsize=None)
def operands(shape):
    """x [MMAX][round8(K0)] and the layers' weights [K][round8(N) + 8] (bf16, zero padding): built
    once per shape, never written."""
    K0, Ns = SHAPES[shape]
    g = torch.Generator(device="cuda").manual_seed(1000 + K0 + 7 * len(Ns) + Ns[0])
    x = torch.zeros(MMAX, round8(K0), device="cuda", dtype=torch.bfloat16)
    x[:, :K0 - 1] = torch.tanh(torch.randn(MMAX, K0 - 1, device="cuda", generator=g)).bfloat16()
    x[:, K0 - 1] = 1.0  # the bias input
    ws = []
    for K, N in zip(layer_K(K0, Ns), Ns):
        w = torch.zeros(K, round8(N) + 8, device="cuda", dtype=torch.bfloat16)
        w[:, :N] = (torch.randn(K, N, device="cuda", generator=g) * (2.0 / (K + N)) ** 0.5).bfloat16()
        ws.append(w)
    return x, tuple(ws)


def run_chain(shape, M, rows, act=0, tight=False, ws=None):
    """One launch on fresh FILL-prefilled output buffers of M + 96 rows; ldo = round8(N + 1) + 8, or
    the step's own round8(N + 1) (tight). Returns the out tensors (bf16)."""
    lib = _lib.load()
    K0, Ns = SHAPES[shape]
    x, w0 = operands(shape)
    ws = w0 if ws is None else ws
    Ks, nl = layer_K(K0, Ns), len(Ns)
    outs = [torch.full((M + 96, round8(N + 1) + (0 if tight else 8)), FILL, device="cuda",
                       dtype=torch.int16).view(torch.bfloat16) for N in Ns]
    IA, PA = C.c_int * nl, C.c_void_p * nl
    rc = lib.mvae_debug_chain(M, nl, IA(*Ks), IA(*Ns), act, rows, x.data_ptr(), x.shape[1],
                              PA(*[w.data_ptr() for w in ws]), IA(*[w.shape[1] for w in ws]),
                              PA(*[o.data_ptr() for o in outs]), IA(*[o.shape[1] for o in outs]),
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mvae_last_error(None)
    return outs


def reference(H, W, act):
    """float64 act(H W) and the fp32-accumulation / activation slack 2e-6 |H| |W| + 1e-5."""
    pre = H @ W
    ref = torch.tanh(pre) if act == 0 else torch.where(pre < 0, torch.expm1(pre), pre)
    return ref, 2e-6 * (H.abs() @ W.abs()) + 1e-5


def check_layers(shape, M, rows, act, outs, tag):
    K0, Ns = SHAPES[shape]
    x, ws = operands(shape)
    worst = 0.0
    for l, (K, N) in enumerate(zip(layer_K(K0, Ns), Ns)):
        H = (x if l == 0 else outs[l - 1])[:M, :K].double()
        ref, slack = reference(H, ws[l][:, :N].double(), act)
        got = outs[l][:M, :N].double()
        assert torch.isfinite(got).all(), (tag, l)
        ratio = ((got - ref).abs() / (0.5 * ulp_bf16(ref) + slack)).max().item()
        worst = max(worst, ratio)
        print(f"CHAIN_RATIO {tag} rows={rows} M={M} layer={l} ratio={ratio:.4f}")
        bits = outs[l].view(torch.int16)
        n8 = round8(N + 1)
        assert (bits[:M, N] == 0x3F80).all(), (tag, l, "ones column")
        assert (bits[:M, N + 1:n8] == 0).all(), (tag, l, "zero padding")
        assert (bits[:M, n8:] == FILL).all(), (tag, l, "written past round8(N + 1)")
        assert (bits[M:] == FILL).all(), (tag, l, "written past row M")
        assert ratio <= 1.0, (tag, l, ratio)
    return worst


CASES = [(s, r, m, 0) for s in SHAPES for r in ROWS for m in (1, r + 1, 2 * r)]
CASES += [(s, 0, 2 * 96 + 1, 0) for s in SHAPES]
CASES += [(s, r, m, 1) for s in list(SHAPES)[:3] for r in ROWS for m in (1, r + 1, 2 * r)]


@gpu
@pytest.mark.parametrize("shape,rows,M,act", CASES, ids=lambda v: str(v))
def test_chain_layers(need_gpu, shape, rows, M, act):
    """Every (shape, rows per workgroup, M in {1, rows + 1, 2 rows}) with tanh, rows = 0 (auto) once
    per shape, elu on the first three shapes: each layer within half a bf16 ulp (plus the fp32
    slack) of float64 on its own input, the row padding exact, nothing written elsewhere."""
    check_layers(shape, M, rows, act, run_chain(shape, M, rows, act), f"{shape}/act{act}")


@gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_chain_step_stride(need_gpu, shape):
    """ldo = round8(N + 1), the step's own stride: the last stored chunk ends the row."""
    check_layers(shape, 97, 48, 0, run_chain(shape, 97, 48, 0, tight=True), f"{shape}/tight")


@gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("shape", ["ragged", "c3"])
def test_chain_ignores_weight_padding(need_gpu, shape, rows):
    """Weight columns [N, ldw) reach only output columns >= N, which the epilogue overwrites with
    constants: NaN there leaves every output bit where the zero-padded run put it."""
    _, ws = operands(shape)
    poisoned = []
    for w, N in zip(ws, SHAPES[shape][1]):
        p = w.clone()
        p[:, N:] = float("nan")
        poisoned.append(p)
    M = rows + 1
    a = run_chain(shape, M, rows)
    b = run_chain(shape, M, rows, ws=poisoned)
    for l, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u.view(torch.int16), v.view(torch.int16)), (shape, rows, l)


@gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("shape", ["c3", "dec"])
def test_chain_matches_gemm_per_layer(need_gpu, shape, rows):
    """Each layer through mvae_debug_gemm (bf16, ACT epilogue, planes out, planner's kernel) on the
    chain's own input widened to fp32: two roundings of two fp32 accumulations of the same exact
    products, so |chain - gemm| <= ulp_bf16(ref) + 2 slack per element."""
    lib = _lib.load()
    K0, Ns = SHAPES[shape]
    x, ws = operands(shape)
    M = 2 * rows + 1
    outs = run_chain(shape, M, rows)
    for l, (K, N) in enumerate(zip(layer_K(K0, Ns), Ns)):
        src = x if l == 0 else outs[l - 1]
        A = src[:M].float().contiguous()
        Bm = ws[l].float().contiguous()
        Cm = torch.zeros(M, N, device="cuda")
        rc = lib.mvae_debug_gemm(M, N, K, A.data_ptr(), A.shape[1], 0, Bm.data_ptr(), Bm.shape[1], 0,
                                 Cm.data_ptr(), N, 1 | (1 << 4) | (1 << 12), 0, None, 0,
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mvae_last_error(None)
        ref, slack = reference(src[:M, :K].double(), ws[l][:, :N].double(), 0)
        d = (outs[l][:M, :N].double() - Cm.double()).abs()
        ratio = (d / (ulp_bf16(ref) + 2 * slack)).max().item()
        print(f"CHAIN_GEMM_RATIO {shape} rows={rows} layer={l} ratio={ratio:.4f}")
        assert ratio <= 1.0, (shape, rows, l, ratio)


@gpu
@pytest.mark.parametrize("rows", ROWS)
def test_chain_deterministic(need_gpu, rows):
    a = run_chain("c3", 2 * rows + 1, rows)
    b = run_chain("c3", 2 * rows + 1, rows)
    for l, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u.view(torch.int16), v.view(torch.int16)), (rows, l)


# ------------------------------------------------------------------ validation (no GPU work)
def _call(lib, M=4, nl=2, K=(24, 17), N=(16, 9), act=0, rows=0, x=0x1000, ldx=24, w=(0x2000, 0x3000),
          ldw=(16, 16), out=(0x4000, 0x5000), ldo=(24, 16), arrays=True):
    n = max(len(K), 1)
    IA, PA = C.c_int * n, C.c_void_p * n
    if not arrays:
        return lib.mvae_debug_chain(M, nl, None, None, act, rows, x, ldx, None, None, None, None, None)
    return lib.mvae_debug_chain(M, nl, IA(*K), IA(*N), act, rows, x, ldx, PA(*w), IA(*ldw), PA(*out), IA(*ldo),
                                None)


@pytest.mark.parametrize("kw", [
    dict(nl=0), dict(nl=5, K=(8,) * 5, N=(7,) * 5, w=(0x2000,) * 5, ldw=(8,) * 5, out=(0x4000,) * 5, ldo=(8,) * 5),
    dict(M=0), dict(M=-3),
    dict(K=(0, 17)), dict(K=(24, 513)), dict(K=(32, 17), ldx=24),
    dict(N=(0, 9)), dict(N=(16, 512), ldw=(16, 512), ldo=(24, 520)),
    dict(ldx=20), dict(ldx=0), dict(ldw=(12, 16)), dict(ldw=(16, 8)), dict(ldo=(24, 12)), dict(ldo=(16, 16)),
    dict(ldo=(24, 8)),
    dict(x=0), dict(x=0x1008), dict(w=(0, 0x3000)), dict(w=(0x2000, 0x3004)), dict(out=(0x4000, 0)),
    dict(out=(0x4002, 0x5000)), dict(arrays=False),
    dict(act=2), dict(act=-1),
    dict(rows=8), dict(rows=24), dict(rows=112), dict(rows=-16),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items())[:40])
def test_chain_rejects_bad_arguments(kw):
    """Every argument the kernel's addressing relies on is refused with MVAE_EINVAL and a message
    before any HIP call (the pointers here are not device memory: nothing may touch them)."""
    lib = _lib.load()
    assert _call(lib, **kw) == EINVAL
    msg = lib.mvae_last_error(None)
    assert msg and msg.startswith(b"mvae_debug_chain: "), msg
