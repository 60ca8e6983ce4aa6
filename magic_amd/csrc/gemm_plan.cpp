// The GEMM planner: pure host arithmetic over a GemmDesc (shapes, strides, alignments, the epilogue's
// operands, the caller's GemmForce) -> the GemmPlan gemm_run launches. No kernels and no HIP calls
// here; the cost models' constants are measurements (the profiles named beside them).
#include "mvae_internal.h"

#include <cmath>
#include <cstdint>

namespace mvae {
namespace {

bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
bool bce_mode(int m) { return m == EPI_BCE || m == EPI_BCEB; }
// epilogues that never split K (their reduction is not the slabs')
bool fixed_split(int m) { return bce_mode(m) || m == EPI_SIGMOID; }

// The 256-row bf16-plane kernels (ring, plane-stacked, eight-phase) serve d: shape and alignment.
bool wide_shape(const GemmDesc& d) {
  const GemmForce& f = d.force;
  if (d.prec == GEMM_F32 || f.kernel == K_PLANE) return false;  // (K_PLANE: the 128x128 register-staged kernel)
  const bool any = (f.kernel == K_RING || f.kernel == K_E8) && f.any_shape;
  // output dimensions >= 128 (the thin decoder / latent-head GEMMs of C3-C5: a 256-row ring
  // tile ran them 1.6-1.7x faster than the 128x128 register-staged kernel, profiles/r4/README.md)
  if (!any && (d.M < 128 || d.N < 128)) return false;
  // one k-tile and under a CU's worth of 256x256 tiles (dec layer 1: K = L + 1; the head's
  // dgrad: K = 2L): epilogue-bound on few CUs, the 128x128 kernels spread it wider
  const long long t256 = (long long)((d.M + 255) / 256) * ((d.N + 255) / 256) * d.batch;
  if (!any && !f.late_256 && d.K <= 64 && t256 < 256) return false;
  auto a8 = [](long long v) { return (v & 7) == 0; };
  if (!a8(d.lda) || !a8(d.ldb) || !a8(d.pA) || !a8(d.pB)) return false;
  if (d.batch > 1 && (!a8(d.sA) || !a8(d.sB))) return false;
  if ((reinterpret_cast<uintptr_t>(d.Ap) | reinterpret_cast<uintptr_t>(d.Bp)) & 15) return false;
  return true;
}

// Joint choice of the kernel (256 x 256 eight-phase kernel; 256 x 256 / 256 x 128 / 192 x 256 /
// 192 x 128 ring kernels) and split-K: each kernel's time is its rounds of resident workgroups
// (one per CU) x (k-tiles + fixed prologue/epilogue cost) x its time per k-tile; split-K adds the
// fp32 slab round trip and the reduction launch.
void plan_wide(const GemmDesc& d, size_t max_ws, GemmPlan& pl) {
  const GemmForce& f = d.force;
  const bool fixed = fixed_split(d.epi.mode);
  const int kt = (d.K + 63) / 64;
  const bool x3 = d.x3 && d.prec == GEMM_F32X && d.nA == 3 && d.nB == 3;
  const int T = d.nA > d.nB ? d.nA : d.nB;
  int np = 0;
  for (int i = 0; i < d.nA; ++i)
    for (int j = 0; j < d.nB; ++j) np += i + j < T;
  if (d.dynA) np = (np + (d.nB < T ? d.nB : T)) / 2;  // A's residual planes often all zero
  const bool big = d.M >= 256 && d.N >= 256;
  const bool small = d.M < 128 || d.N < 128;  // (here under any_shape only)
  // the eight-phase kernel where it measured faster than the ring kernels (profiles/r4): enough
  // 256x256 tiles to fill the chip, or a long k-loop over >= 32 tiles; its (k-tile, pair)
  // iterations copy both operand images (the ring kernel reuses an unchanged image)
  const long long t256 = (long long)((d.M + 255) / 256) * ((d.N + 255) / 256) * d.batch;
  // 192-row ring tiles: k-contiguous A, epilogues other than the BCE head / sigmoid
  const bool t192 = !d.at && !fixed;
  const long long tl192 = (long long)((d.M + 191) / 192) * ((d.N + 255) / 256) * d.batch;
  // ... except (in-step A/B, profiles/r4/README.md) single-product GEMMs where one round of
  // 192-row ring tiles keeps >= 4/3 as many CUs busy (C3 layer-0 forward: 256 vs 192 workgroups,
  // 0.255 vs 0.276 ms; hidden forward 31.7 vs 32.7 us)
  // (a real one-round fill: not a tile count split-K multiplies anyway -- the C3 decoder-output
  // dgrad, 86 vs 64 tiles, stays on the eight-phase kernel: 0.107 vs 0.115 ms in r4n)
  const bool ring_fills = t192 && np == 1 && tl192 > 128 && tl192 <= 256 && 3 * tl192 >= 4 * t256;
  const bool e8_rule = big && t256 >= 32 && (t256 >= 256 || (long long)np * kt >= 64) && !ring_fills;
  // the eight-phase kernel addresses an operand plane by 32-bit per-lane element offsets
  const long long ea = (long long)(d.at ? d.K : d.M) * d.lda, eb = (long long)(d.bt ? d.N : d.K) * d.ldb;
  const bool e8_fits = ea < (1LL << 32) && eb < (1LL << 32);
  // A as bits (a 0/1 operand): the eight-phase kernel, whose bits path reads it (its plane path
  // runs the rare batch with another pixel value)
  const bool free_choice = f.kernel == K_AUTO && !f.no_e8;
  const bool e8_only = e8_fits && (f.kernel == K_E8 || (free_choice && (e8_rule || d.Abits)));
  double best = 1e30;
  pl.kernel = K_RING; pl.tm = pl.tn = 256; pl.split = 1;  // (no candidate left: the unsplit 256x256 ring tile)
  for (int cand = 0; cand < 5; ++cand) {
    // candidates: ring 256x256, 256x128, eight-phase 256x256, ring 192x256, 192x128
    const bool e8 = cand == 2;
    const int w = cand == 1 || cand == 4 ? 128 : 256;
    const int tmr = cand >= 3 ? 192 : 256;
    if (e8 != e8_only) continue;
    if (cand >= 3 && !t192) continue;
    if ((f.tile_m == 192 && t192 && cand < 3) || (f.tile_m == 256 && cand >= 3)) continue;
    if (!e8 && f.tile_n && w != f.tile_n) continue;
    if (!e8 && small && f.ring_from_128) continue;
    const long long tiles = (long long)((d.M + tmr - 1) / tmr) * ((d.N + w - 1) / w) * d.batch;
    // ring kernels, measured: 4096^3 at 1.06 PF/s = 1.94 us per 256x256 k-tile per CU; the
    // 256x128 tile does half the MFMA work per k-tile in ~1.5 us (profiles/r2/gemm_ab_tile_n.txt);
    // 192-row tiles interpolated (a fixed ~1.1 us per k-tile plus ~0.1 us per 32x32 block).
    // eight-phase kernel: per 256x256 k-tile (gemm_bf16e.hip)
    double t_kt = e8 ? 1.35e-6 : tmr == 192 ? (w == 256 ? 1.7e-6 : 1.4e-6) : (w == 256 ? 1.9e-6 : 1.5e-6);
    // the plane-stacked kernel (option x3) serves the six-pair f32x ring plans at tile N 128:
    // C2 hidden forward 60 -> 50 us, hidden dgrad 72 -> 67 us in the region pass (r6zi)
    if (x3 && !e8 && w == 128) t_kt *= 0.88;
    const double fix = 3.0;
    for (int s = 1; s <= (fixed ? 1 : 32); ++s) {
      if (s > 1 && kt / s < 2) break;
      if (s > 1 && (size_t)d.batch * s * d.M * d.N > max_ws) break;
      const double rounds = std::ceil(tiles * s / 256.0);
      double t = rounds * (np * std::ceil((double)kt / s) + fix) * t_kt;
      // split-K: the slabs' write + read and the reduction launch (8 us fixed: C2's f32x hidden
      // forward, 12288 x 500 x 501, ran 65.6 us at 192x256 split 2 against 61.0 us as one round
      // of 192x128 tiles unsplit, where the model with 4 us preferred the split, r5zq)
      if (s > 1) t += (double)d.batch * s * d.M * d.N * 8.0 / 4.5e12 + 8e-6;
      if (t < best * 0.97) { best = t; pl.split = s; pl.kernel = e8 ? K_E8 : K_RING; pl.tn = w; pl.tm = tmr; }
    }
  }
  if (f.late_256) pl.tm = pl.tn = 256;
}

// split-K of the 128x128 kernels
int split_128(const GemmDesc& d, size_t max_ws) {
  const int ntm = (d.M + PLAN_T128 - 1) / PLAN_T128, ntn = (d.N + PLAN_T128 - 1) / PLAN_T128;
  const long long tiles = (long long)ntm * ntn * d.batch;
  const int ktiles = (d.K + PLAN_BK_F32 - 1) / PLAN_BK_F32;
  // Throughput model: each CU works through ceil(WGs/256) workgroups (two co-resident WGs
  // overlap each other's stalls but share the MFMA pipes), each WG costs its k-tiles plus a
  // fixed prologue/epilogue; split-K adds the slab round trip and one reduction launch.
  const double cus = 256.0;
  // one 128x128x32 k-tile per CU: fp32 MFMA rate; bf16 / 3-term split are load-bound
  const double t_ktile = d.prec == GEMM_F32 ? 1.75e-6 : (d.prec == GEMM_BF16 ? 0.3e-6 : 0.5e-6);
  double best = 1e30;
  int best_s = 1;
  for (int s = 1; s <= 32; ++s) {
    if (s > 1 && ktiles / s < 4) break;
    if (s > 1 && (size_t)d.batch * s * d.M * d.N > max_ws) break;
    const double rounds = std::ceil(tiles * s / cus);
    double t = rounds * ((double)ktiles / s + 2.0) * t_ktile;
    if (s > 1) t += (double)d.batch * s * d.M * d.N * 8.0 / 4.5e12 + 4e-6;
    if (t < best * 0.97) { best = t; best_s = s; }
  }
  return best_s;
}

int split_valu(const GemmDesc& d, size_t max_ws) {
  const long long tiles = (long long)((d.M + PLAN_VT - 1) / PLAN_VT) * ((d.N + PLAN_VT - 1) / PLAN_VT) * d.batch;
  const int chunks = (d.K + PLAN_VKC - 1) / PLAN_VKC;
  // latency-bound small kernels: aim at >= 4 waves per SIMD (1024 workgroups of 4 waves), at
  // least 2 chunks per slice, at most 16 slices (the ordered reduction reads them serially)
  int s = 1;
  while (s * 2 <= 16 && s * 2 <= chunks / 2 && tiles * s < 1024 &&
         (size_t)d.batch * 2 * s * d.M * d.N <= max_ws)
    s *= 2;
  return s;
}

// the row-major 16-B epilogue applies: bases and strides keep every 8-column chunk of every
// operand it touches 16-B aligned. slabs: the launch writes split-K slabs (fp32 rows of N at the
// workspace, no planes) instead of the output
bool epi_vec_ok(const GemmDesc& d, bool slabs, bool ws_aligned) {
  const GemmEpi& e = d.epi;
  const bool c_al = slabs ? ws_aligned : al16(d.C);
  const long long ldc = slabs ? d.N : d.ldc, sC = slabs ? (long long)d.M * d.N : d.sC;
  if ((slabs || e.c32) && (!c_al || (ldc & 3) || (sC & 3))) return false;
  if (!slabs && e.cp && (!al16(e.cp) || (ldc & 7) || (sC & 7) || (e.pc & 7))) return false;
  if (e.mode == EPI_DACT && !e.auxp && (!al16(e.aux) || (e.ld_aux & 3))) return false;
  if (e.mode == EPI_DACT && e.auxp && (!al16(e.auxp) || (e.ld_aux & 7))) return false;
  if (bce_mode(e.mode)) {
    if (e.x && (!al16(e.x) || (e.ldx & 3))) return false;
    if (e.xp && (!al16(e.xp) || (e.ldx & 7))) return false;
    if (e.y && (!al16(e.y) || (e.ldy & 3))) return false;
  }
  return true;
}

}  // namespace

bool gemm_valu_fits(const GemmDesc& d) {
  if (d.force.names_kernel()) return false;
  if (bce_mode(d.epi.mode)) return false;
  // skinny K, or a skinny output with a short K (the long-K weight gradients of the latent head
  // and decoder layer 1 stay on the fp32 MFMA kernel: measured faster, profiles/r2)
  const int lo = d.M < d.N ? d.M : d.N;
  return d.K <= 64 || (lo <= 64 && d.K <= 1024);
}

GemmPlan gemm_plan(const GemmDesc& d, size_t max_ws, bool ws_aligned) {
  const GemmForce& f = d.force;
  GemmPlan pl;
  const bool fixed = fixed_split(d.epi.mode);
  int bk = d.prec == GEMM_F32 ? PLAN_BK_F32 : PLAN_BK_PLANE;  // k-tile of the kernel that runs
  if (f.kernel == K_VALU) {
    pl.kernel = K_VALU;
    pl.tm = pl.tn = PLAN_VT;
    pl.split = fixed ? 1 : split_valu(d, max_ws);
    bk = PLAN_VKC;
  } else if (wide_shape(d)) {
    plan_wide(d, max_ws, pl);
  } else {
    pl.kernel = d.prec == GEMM_F32 ? K_F32 : K_PLANE;
    pl.split = fixed ? 1 : split_128(d, max_ws);
  }
  if (f.split > 0) pl.split = f.split;
  const bool slabs = pl.split > 1;
  pl.ntm = (d.M + pl.tm - 1) / pl.tm;
  pl.ntn = (d.N + pl.tn - 1) / pl.tn;
  pl.kchunk = (((d.K + bk - 1) / bk + pl.split - 1) / pl.split) * bk;
  pl.ws_elems = slabs ? (size_t)d.batch * pl.split * d.M * d.N : 0;
  // the kernel instantiation: slabs are plain stores (the reduction runs the epilogue); the BCE
  // head with a bf16-plane target chooses the target's form at run time (EPI_BCEB); the 256-row
  // kernels have an instantiation of their own for a bf16 aux (EPI_DACTB)
  const bool wide = gemm_wide_kernel(pl.kernel);
  pl.epi_launched = d.epi.mode;
  if (slabs) pl.epi_launched = EPI_STORE;
  else if (pl.kernel >= K_PLANE && d.epi.mode == EPI_BCE && d.epi.xp && d.epi.xdyn) pl.epi_launched = EPI_BCEB;
  else if (wide && d.epi.mode == EPI_DACT && d.epi.auxp) pl.epi_launched = EPI_DACTB;
  if (!wide) {
    if (pl.kernel != K_VALU && pl.epi_launched == EPI_STORE) pl.staging = f.staging;
    return pl;
  }
  // tile order: bands of 8 m-tiles walked n by n when a row has >= 8 n-tiles, so the 32 tiles
  // an XCD holds at once share 8 A and 4 B tiles in its L2 (C5 latent-head forward
  // 24576 x 4000 x 501: 0.177 -> 0.161 ms; neutral on the BCE head and the other shapes,
  // profiles/r4/r4u_tile_group.txt); GemmDesc::group >= 0 overrides (A/B: mvae_bench_gemm)
  pl.group = d.group >= 0 ? d.group : (pl.ntn >= 8 ? 8 : 0);
  // The 256-row kernels' epilogue goes through LDS (row-major 16-B stores) when the tile writes
  // bf16 planes or is the BCE head (2-B plane stores and 4-B target loads per element otherwise),
  // and stays in the C/D layout for fp32-only outputs (split-K slabs: 128-B row segments already,
  // where the LDS round trip measured 5-10 % slower); the eight-phase kernel's accumulators are
  // not in the C/D row-segment order, so its epilogue always goes through LDS: 16-B accesses
  // where aligned, else element-wise
  const bool vec = epi_vec_ok(d, slabs, ws_aligned);
  if (pl.kernel == K_E8) {
    pl.lds_epilogue = true;
    pl.vec_epilogue = vec;
    return pl;
  }
  pl.lds_epilogue = pl.vec_epilogue =
      ((d.epi.cp && !slabs) || bce_mode(pl.epi_launched)) && !f.cd_epilogue && vec;
  // The plane-stacked kernel serves this ring plan: option x3, the six f32x pairs of three-plane
  // operands, tile N 128 (or 256x256 with x3 >= 2; its BCE instantiations spill there: the head
  // keeps the eight-phase / ring kernels). nA == nB == 3 is the whole pair condition: the pair
  // order gemm_bf16_launch builds for (3, 3) -- (0,0) (0,1) (0,2) (1,1) (1,0) (2,0) -- is the
  // kernel's own table x3_pa / x3_pb at (3, 3), no other (nA, nB) has six pairs i + j < max(nA, nB)
  // with A planes 0 0 0 1 1 2, and with a run-time flag on A (dynA) the leading pairs with A plane 0
  // are then the three its three-pair loop runs
  const bool x3_tile = pl.tn == 128 || (pl.tm == 256 && d.x3 >= 2 && !bce_mode(d.epi.mode));
  if (d.x3 && d.nA == 3 && d.nB == 3 && x3_tile) pl.kernel = K_X3;
  return pl;
}

size_t gemm_workspace_elems(const GemmDesc& d) { return gemm_plan(d, ~size_t(0)).ws_elems; }

}  // namespace mvae
