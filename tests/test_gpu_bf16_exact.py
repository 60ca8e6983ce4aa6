"""bf16-precision GEMMs with operands that are bf16 values already.

The other bf16 GEMM tests (test_gemm_layouts, test_gemm_wide_kernel, test_gemm_e8_kernel,
test_gemm_tile192 and the *_epilogues tests) bound the error by 1e-2 |A| |B|, because their float64
reference does not round the operands. Here the kernel's operand rounding is the identity, the
float64 product of the same values is exact, and the kernels are held to the f32x bar,
2e-6 |A| |B| + 1e-6: what remains is fp32 accumulation, 5000 times tighter. Worst error / bound
measured on an MI355X (RATIOS_MEASURED): 0.013 to 0.042 for every fp32 store, 0.973 to 0.996 where
the output is one RN bf16 plane (the half ulp is the whole of the error there).
"""
import pytest
import torch

from magic_amd import _lib
from tests.test_gpu_chain import ulp_bf16

pytestmark = pytest.mark.gpu

BF16 = 1  # MVAE_PREC_BF16
T192 = "t192"  # the ring kernel's 192-row tiles (epi bit 13) in the variant lists below

# worst error / bound on an MI355X (gfx950) over the cases of each test (a record, not used by the
# assertions: the bound is 1)
RATIOS_MEASURED = {"layouts": 0.021, "forced_kernels": 0.013, "forced_kernels_t192": 0.042,
                   "epilogues_fp32": 0.036, "epilogues_plane": 0.9962}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _padded_bf16(rows, cols, g, scale=1.0):
    """[rows, cols] of bf16-representable normals inside a zero-padded [rows, round8(cols)] fp32
    buffer (test_gpu_parity._padded with values that bf16 holds exactly)."""
    buf = torch.zeros(rows, (cols + 7) // 8 * 8, device="cuda")
    buf[:, :cols] = (torch.randn(rows, cols, device="cuda", generator=g) * scale).bfloat16().float()
    return buf


def _sel(variant):
    return (1 << 13) if variant == T192 else (variant << 8)


def _plain(at, bt, M, N, K, variant):
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(M * 5 + N * 11 + K)
    A = _padded_bf16(K, M, g) if at else _padded_bf16(M, K, g)
    Bm = _padded_bf16(N, K, g) if bt else _padded_bf16(K, N, g)
    Cm = torch.full((M, N), float("nan"), device="cuda")
    rc = lib.mvae_debug_gemm(M, N, K, A.data_ptr(), A.shape[1], at, Bm.data_ptr(), Bm.shape[1], bt,
                             Cm.data_ptr(), N, (BF16 << 4) | _sel(variant), 0, None, 0,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mvae_last_error(None)
    Ad = A[:, :M].double().T if at else A[:, :K].double()
    Bd = Bm[:, :K].double().T if bt else Bm[:, :N].double()
    ref = Ad @ Bd
    err = (Cm.double() - ref).abs().max().item()
    bound = 2e-6 * (Ad.abs() @ Bd.abs()).max().item() + 1e-6
    print(f"BF16X_RATIO plain variant={variant} at={at} bt={bt} {M}x{N}x{K} ratio={err / bound:.4f}")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("at,bt", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(37, 53, 29), (300, 517, 1001), (129, 40, 8193)])
def test_gemm_exact_operands_layouts(at, bt, M, N, K):
    """The planner's kernel on every operand layout: ragged small, wide, and split-K skinny."""
    _plain(at, bt, M, N, K, 0)


@pytest.mark.parametrize("at", [0, 1])
@pytest.mark.parametrize("M,N,K,variant",
                         [(M, N, K, v) for v in (3, 6, 7, 8, 11, 12, 13, 14, T192)
                          for M, N, K in ((300, 517, 1001), (1000, 600, 4099))] + [(193, 500, 501, T192)])
def test_gemm_exact_operands_forced_kernels(at, M, N, K, variant):
    """Every forced 256-row kernel form (ring 3 / 6 / 7, two-stage 8, tile N 128 / 256, eight-phase
    13 / 14) and the 192-row tiles, A row- and column-major, ragged edges and split-K (K 4099)."""
    _plain(at, 0, M, N, K, variant)


@pytest.mark.parametrize("epi,act", [(1, 0), (1, 1), (2, 0), (2, 1), (4, 0)])
@pytest.mark.parametrize("M,N,ldc", [(513, 257, 264), (280, 300, 301)])
@pytest.mark.parametrize("variant", [0, 11, 12, 13, 14])
@pytest.mark.parametrize("planes", [0, 1])
def test_gemm_exact_operands_epilogues(epi, act, M, N, ldc, variant, planes):
    """Fused ACT / DACT / SIGMOID epilogues on exact operands (aux too): 2e-6 |A| |B| + 1e-5 per
    tensor; planes = 1 writes one RN bf16 plane, half an ulp of the reference more per element.
    Nothing written past column N."""
    lib = _lib.load()
    K = 304
    g = torch.Generator(device="cuda").manual_seed(M + 7 * N + 31 * epi + act + variant)
    A = _padded_bf16(M, K, g, 0.3)
    Bm = _padded_bf16(K, N, g, 0.3)
    ld_aux = (N + 7) // 8 * 8
    pre = torch.randn(M, ld_aux, device="cuda", generator=g)
    aux = (torch.tanh(pre) if act == 0 else torch.nn.functional.elu(pre)).bfloat16().float()
    Cm = torch.full((M, ldc), float("nan"), device="cuda")
    rc = lib.mvae_debug_gemm(M, N, K, A.data_ptr(), A.shape[1], 0, Bm.data_ptr(), Bm.shape[1], 0, Cm.data_ptr(),
                             ldc, epi | (BF16 << 4) | (variant << 8) | (planes << 12), act,
                             aux.data_ptr(), ld_aux, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mvae_last_error(None)
    Ad, Bd = A[:, :K].double(), Bm[:, :N].double()
    acc = Ad @ Bd
    a = aux[:, :N].double()
    if epi == 1:
        ref = torch.tanh(acc) if act == 0 else torch.where(acc < 0, torch.expm1(acc), acc)
    elif epi == 2:
        ref = acc * (1 - a * a) if act == 0 else torch.where(a < 0, acc * (a + 1), acc)
    else:
        ref = torch.sigmoid(acc)
    bound = 2e-6 * (Ad.abs() @ Bd.abs()).max().item() + 1e-5
    err = (Cm[:, :N].double() - ref).abs()
    ratio = (err / (bound + (0.5 * ulp_bf16(ref) if planes else 0.0))).max().item()
    print(f"BF16X_RATIO epi={epi} act={act} variant={variant} planes={planes} {M}x{N} ld {ldc} ratio={ratio:.4f}")
    assert ratio <= 1.0, (ratio, err.max().item(), bound)
    if ldc > N and not planes:
        assert torch.isnan(Cm[:, N:]).all()
