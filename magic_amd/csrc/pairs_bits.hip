// The layer-0 bit operands of a 0/1 batch straight from the uint8 lock / key tables (gfx950): the
// batch producer (make_batch_kernel, mvae_kernels.hip) and the de-interleave to bits
// (deint_bits_kernel) in one pass, without the fp32 X [B, 3 D] between them. A batch is described
// by (tables, idx, kidx, rotation coefficients): row b is lock idx[b] and key kidx[b] (the own pair
// passes idx for both), its rotated lock gathered by make_batch_kernel's arithmetic. Per pixel
// triple the pass reads 2 table bytes (plus the gathers, which stay in cache: the rotated image is
// the lock image just read) and writes the ~1.1 bits of the BitMats and target bits, where the two
// kernels write and read back 12 bytes of X.
//
// The 24 values of an octet are formed as the producer forms them, (float)byte / div, and the bit
// and the not-binary test derived from that float by deint_octet: the not-binary word rises for
// exactly the batches it rises for through X, for div 255 and div 1 alike. From the three bytes
// per octet on, everything is deint_bits.h's (LDS byte image, BitMat words, target bits, ones
// column, flag slots); the grey pass shares deint_grey_octet with deint_grey_kernel.
#include "deint_bits.h"

// No FMA contraction anywhere in this file: the gather coordinates are unfused mul / add / sub, as
// in make_batch_kernel (whose comment tells what contraction did to them once).
#pragma clang fp contract(off)

namespace mvae {
namespace {

// one batch row's sources
struct PairRow {
  const unsigned char* L;  // its lock image
  const unsigned char* K;  // its key image
  float4 cf;               // (cos, sin, x_off, y_off) of its rotation
};
__device__ __forceinline__ PairRow pair_row(const unsigned char* __restrict__ locks,
                                            const unsigned char* __restrict__ keys, int HW,
                                            const int* __restrict__ idx, const int* __restrict__ kidx,
                                            const float4* __restrict__ coef, int b) {
  PairRow r;
  r.L = locks + (size_t)idx[b] * HW;
  r.K = keys + (size_t)kidx[b] * HW;
  r.cf = coef[b];
  return r;
}

// the raw bytes of pixels [pix, pix + 8) of a row: lock and key (one 8-byte load each; pix % 8 == 0,
// HW % 8 == 0 and 8-byte aligned tables) and the rotated lock (8 byte gathers from the lock image
// at make_batch_kernel's coordinates; a sample outside the image is 0, its load clamped to pixel 0),
// eight bytes per uint2, pixel j in byte j
struct PairBytes {
  uint2 l, k, r;
};
__device__ __forceinline__ PairBytes pair_load(const PairRow& row, int H, int W, int pix) {
#pragma clang fp contract(off)
  PairBytes o;
  o.l = *reinterpret_cast<const uint2*>(row.L + pix);
  o.k = *reinterpret_cast<const uint2*>(row.K + pix);
  int yy = pix / W, xx = pix - yy * W;
  unsigned rb[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float fx = (float)xx, fy = (float)yy;
    const float xin = (row.cf.x * fx - row.cf.y * fy) + row.cf.z;  // unfused: fp contract(off)
    const float yin = (row.cf.y * fx + row.cf.x * fy) + row.cf.w;
    const float xr = roundf(xin), yr = roundf(yin);
    const bool ok = xr >= 0.f && xr <= (float)(W - 1) && yr >= 0.f && yr <= (float)(H - 1);
    const unsigned v = row.L[ok ? (int)yr * W + (int)xr : 0];
    rb[j >> 2] |= (ok ? v : 0u) << (8 * (j & 3));
    if (++xx == W) { xx = 0; ++yy; }
  }
  o.r = make_uint2(rb[0], rb[1]);
  return o;
}
// ... and the octet's 24 values as X would store them: per pixel (lock, rotated lock, key) / div
__device__ __forceinline__ void pair_values(const PairBytes& p, float div, float (&e)[24]) {
  deint_byte_values(p.l, p.r, p.k, div, e);
}

// deint_bits_kernel<2, 256, 72>'s task (64 batch rows x 128 pixels per workgroup; thread tid owns
// octet tid % 16 of rows tid / 16 + 16 i) with the octets' values from the tables. NOW: no
// weight-gradient words (the xbw_split schedule: launch_bits_transpose writes them).
template <bool NOW>
__global__ __launch_bounds__(256) void pairs_bits_kernel(const unsigned char* __restrict__ locks,
                                                         const unsigned char* __restrict__ keys, int H, int W,
                                                         const int* __restrict__ idx,
                                                         const int* __restrict__ kidx,
                                                         const float4* __restrict__ coef, float div, int B, int D,
                                                         int kts_f, int kts_w, unsigned* __restrict__ xbf,
                                                         unsigned* __restrict__ xbw,
                                                         unsigned char* __restrict__ xbits, int ldbits,
                                                         int* __restrict__ dyn, int* __restrict__ dyn_next) {
  constexpr int PB = 2, NT = 256, OS = 72;
  using S = DeintShape<PB, NT>;
  if (dyn_next && (blockIdx.x | blockIdx.y | threadIdx.x) == 0) dyn_next[0] = dyn_next[2] = 0;
  __shared__ __attribute__((aligned(16))) DeintLds<PB, OS> bt;
  const int tid = threadIdx.x, bx = blockIdx.x, by = blockIdx.y;
  const int b0 = by * 64, o = tid % S::NO, pix = bx * 64 * PB + 8 * o;
  const bool in = pix + 8 <= D;  // (D % 8 == 0: an octet is whole inside the image or whole outside)
  const unsigned pad = deint_pad(pix, D);
  PairBytes pb[S::NR] = {};
  if (in) {  // every row's loads before the first use
    PairRow row[S::NR];
#pragma unroll
    for (int i = 0; i < S::NR; ++i)
      row[i] = pair_row(locks, keys, D, idx, kidx, coef, b0 + tid / S::NO + S::RPP * i);
#pragma unroll
    for (int i = 0; i < S::NR; ++i) pb[i] = pair_load(row[i], H, W, pix);
  }
  bool nb = false;
#pragma unroll
  for (int i = 0; i < S::NR; ++i) {
    const int r = tid / S::NO + S::RPP * i;
    float e[24];
    pair_values(pb[i], div, e);
    nb |= deint_octet_put<PB, OS>(in, pad, e, xbits + (size_t)(b0 + r) * ldbits + (pix >> 3), bt, o, r);
  }
  auto none = [] {};
  deint_tail<PB, NT, OS, decltype(none)&, decltype(none)&, NOW>(nb, B, D, kts_f, kts_w, xbf, xbw, dyn, bx, by, bt,
                                                                none, none);
}

// deint_grey_kernel's pass (only after pairs_bits_kernel raised the not-binary word; else every
// workgroup returns at once) with each octet's 24 values rebuilt from the tables
__global__ void pairs_grey_kernel(const unsigned char* __restrict__ locks, const unsigned char* __restrict__ keys,
                                  int H, int W, const int* __restrict__ idx, const int* __restrict__ kidx,
                                  const float4* __restrict__ coef, float div, float* __restrict__ xs,
                                  unsigned short* __restrict__ xp, long long ps, int np, int f32mask,
                                  int* __restrict__ dyn, int B, int D, int ldx) {
  if (dyn[2] == 0) return;
  const int nq = D / 8;
  const size_t n = (size_t)B * nq;
  bool nz = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / nq), q = (int)(i % nq);
    float e[24];
    pair_values(pair_load(pair_row(locks, keys, D, idx, kidx, coef, b), H, W, 8 * q), div, e);
    const float4 v[6] = {make_float4(e[0], e[1], e[2], e[3]),     make_float4(e[4], e[5], e[6], e[7]),
                         make_float4(e[8], e[9], e[10], e[11]),   make_float4(e[12], e[13], e[14], e[15]),
                         make_float4(e[16], e[17], e[18], e[19]), make_float4(e[20], e[21], e[22], e[23])};
    nz |= deint_grey_octet(v, xs, xp, ps, np, f32mask, B, b, q, ldx);
  }
  if (__ballot(nz) != 0 && (threadIdx.x & 63) == 0) atomicOr(dyn, 1);
}

}  // namespace

bool pairs_bits_fits(const unsigned char* locks, const unsigned char* keys, const float* coef, int B, int D) {
  return (D % 8) == 0 && (B % 64) == 0 && (reinterpret_cast<uintptr_t>(locks) % 8) == 0 &&
         (reinterpret_cast<uintptr_t>(keys) % 8) == 0 && (reinterpret_cast<uintptr_t>(coef) % 16) == 0;
}

hipError_t launch_pairs_bits(const unsigned char* locks, const unsigned char* keys, int H, int W, const int* idx,
                             const int* kidx, const float* coef, float div, int B, unsigned* xbf, int kts_f,
                             unsigned* xbw, int kts_w, unsigned char* xbits, int ldbits, int* dyn, int* dyn_next,
                             float* xs, const Planes& xp, int ldx, int f32dyn_mask, bool no_xbw, hipStream_t st) {
  const long long HW = (long long)H * W;
  if (H <= 0 || W <= 0 || HW > (1 << 30) || B <= 0) return hipErrorInvalidValue;
  const int D = (int)HW;
  if (!pairs_bits_fits(locks, keys, coef, B, D) || !locks || !keys || !idx || !coef || (ldx % 8) || !dyn || !xp.p ||
      !xbf || !xbits || (!no_xbw && !xbw) || kts_f != bitmat_kts(D + 1) || kts_w != bitmat_kts(3 * B) ||
      ldbits < D / 8)
    return hipErrorInvalidValue;
  if (!kidx) kidx = idx;  // the own pair
  const float4* c4 = reinterpret_cast<const float4*>(coef);
  const dim3 g((kts_f + 1) / 2, B / 64);
  if (no_xbw)
    hipLaunchKernelGGL(pairs_bits_kernel<true>, g, dim3(256), 0, st, locks, keys, H, W, idx, kidx, c4, div, B, D,
                       kts_f, kts_w, xbf, xbw, xbits, ldbits, dyn, dyn_next);
  else
    hipLaunchKernelGGL(pairs_bits_kernel<false>, g, dim3(256), 0, st, locks, keys, H, W, idx, kidx, c4, div, B, D,
                       kts_f, kts_w, xbf, xbw, xbits, ldbits, dyn, dyn_next);
  // (256 workgroups striding, as launch_deint_grey: for a 0/1 batch every one returns at once)
  hipLaunchKernelGGL(pairs_grey_kernel, dim3(256), dim3(256), 0, st, locks, keys, H, W, idx, kidx, c4, div, xs,
                     xp.p, xp.stride, xp.n, f32dyn_mask, dyn, B, D, ldx);
  return hipGetLastError();
}

}  // namespace mvae
