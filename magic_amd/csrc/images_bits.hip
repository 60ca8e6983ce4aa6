// The layer-0 operand of an embedding pass (mvae_embed_images) from one uint8 image table (gfx950).
// A pass encodes 3 B independent images: image t of the pass is row t of the stacked operand, i.e.
// the three byte octets of a batch row b come from the images b (block 0, where a training batch
// has the rotated lock), B + b (block 1, the lock) and 2 B + b (block 2, the key). Image t of the
// pass is table image idx[t] (or t when idx is null) for t < nvalid and an all-zero image past
// that: idx and the table are not read for those rows.
//
// images_bits_kernel has the task and tiling of pairs_bits_kernel (pairs_bits.hip) with three plain
// 8-byte loads per octet and no coordinate arithmetic; from the three bytes per octet on everything
// is deint_bits.h's, the (float)byte / div values included, so the not-binary word rises exactly as
// it would through X. The grey twin shares deint_grey_octet. images_x_kernel is the materialising
// path's producer: the same pass as a [B, 3 D] fp32 X.
#include "deint_bits.h"

namespace mvae {
namespace {

// image t of the pass: its first byte, or null for a row past the last wanted image
__device__ __forceinline__ const unsigned char* image_of(const unsigned char* __restrict__ table, int HW,
                                                         const int* __restrict__ idx, int nvalid, int t) {
  if (t >= nvalid) return nullptr;
  return table + (size_t)(idx ? idx[t] : t) * HW;
}
// pixels [pix, pix + 8) of an image (pix % 8 == 0, HW % 8 == 0, 8-byte aligned table)
__device__ __forceinline__ uint2 image_octet(const unsigned char* img, int pix) {
  return img ? *reinterpret_cast<const uint2*>(img + pix) : make_uint2(0u, 0u);
}

// channel ch of X (0 lock, 1 rotated lock, 2 key) is block (1, 0, 2)[ch] of the stacked rows
__device__ __forceinline__ int block_of_channel(int ch) { return ch == 0 ? 1 : (ch == 1 ? 0 : 2); }

// pairs_bits_kernel's task (64 batch rows x 128 pixels per workgroup; thread tid owns octet
// tid % 16 of rows tid / 16 + 16 i). NOW: no weight-gradient words (an evaluation pass reads none).
template <bool NOW>
__global__ __launch_bounds__(256) void images_bits_kernel(const unsigned char* __restrict__ table,
                                                          const int* __restrict__ idx, int nvalid, float div,
                                                          int B, int D, int kts_f, int kts_w,
                                                          unsigned* __restrict__ xbf, unsigned* __restrict__ xbw,
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
  uint2 by8[S::NR][3] = {};  // [row pass][block]
  if (in) {  // every row's loads before the first use
    const unsigned char* img[S::NR][3];
#pragma unroll
    for (int i = 0; i < S::NR; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) img[i][c] = image_of(table, D, idx, nvalid, c * B + b0 + tid / S::NO + S::RPP * i);
#pragma unroll
    for (int i = 0; i < S::NR; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) by8[i][c] = image_octet(img[i][c], pix);
  }
  bool nb = false;
#pragma unroll
  for (int i = 0; i < S::NR; ++i) {
    const int r = tid / S::NO + S::RPP * i;
    float e[24];
    deint_byte_values(by8[i][1], by8[i][0], by8[i][2], div, e);
    nb |= deint_octet_put<PB, OS>(in, pad, e, xbits + (size_t)(b0 + r) * ldbits + (pix >> 3), bt, o, r);
  }
  auto none = [] {};
  deint_tail<PB, NT, OS, decltype(none)&, decltype(none)&, NOW>(nb, B, D, kts_f, kts_w, xbf, xbw, dyn, bx, by, bt,
                                                                none, none);
}

// deint_grey_kernel's pass (only after images_bits_kernel raised the not-binary word; else every
// workgroup returns at once) with each octet's 24 values rebuilt from the table
__global__ void images_grey_kernel(const unsigned char* __restrict__ table, const int* __restrict__ idx, int nvalid,
                                   float div, float* __restrict__ xs, unsigned short* __restrict__ xp, long long ps,
                                   int np, int f32mask, int* __restrict__ dyn, int B, int D, int ldx) {
  if (dyn[2] == 0) return;
  const int nq = D / 8;
  const size_t n = (size_t)B * nq;
  bool nz = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / nq), q = (int)(i % nq);
    uint2 c3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) c3[c] = image_octet(image_of(table, D, idx, nvalid, c * B + b), 8 * q);
    float e[24];
    deint_byte_values(c3[1], c3[0], c3[2], div, e);
    const float4 v[6] = {make_float4(e[0], e[1], e[2], e[3]),     make_float4(e[4], e[5], e[6], e[7]),
                         make_float4(e[8], e[9], e[10], e[11]),   make_float4(e[12], e[13], e[14], e[15]),
                         make_float4(e[16], e[17], e[18], e[19]), make_float4(e[20], e[21], e[22], e[23])};
    nz |= deint_grey_octet(v, xs, xp, ps, np, f32mask, B, b, q, ldx);
  }
  if (__ballot(nz) != 0 && (threadIdx.x & 63) == 0) atomicOr(dyn, 1);
}

// The pass as X: x[b, 3 p + ch] = (float)image(block(ch) B + b)[p] / div (any D, any alignment)
__global__ void images_x_kernel(const unsigned char* __restrict__ table, const int* __restrict__ idx, int nvalid,
                                float div, int B, int D, float* __restrict__ x) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= D) return;
  float* o = x + (size_t)b * 3 * D + 3 * (size_t)p;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const unsigned char* img = image_of(table, D, idx, nvalid, block_of_channel(ch) * B + b);
    o[ch] = img ? (float)img[p] / div : 0.f;
  }
}

}  // namespace

bool images_bits_fits(const unsigned char* table, int B, int D) {
  return (D % 8) == 0 && (B % 64) == 0 && (reinterpret_cast<uintptr_t>(table) % 8) == 0;
}

hipError_t launch_images_bits(const unsigned char* table, int H, int W, const int* idx, int nvalid, float div, int B,
                              unsigned* xbf, int kts_f, unsigned* xbw, int kts_w, unsigned char* xbits, int ldbits,
                              int* dyn, int* dyn_next, float* xs, const Planes& xp, int ldx, int f32dyn_mask,
                              bool no_xbw, hipStream_t st) {
  const long long HW = (long long)H * W;
  if (H <= 0 || W <= 0 || HW > (1 << 30) || B <= 0 || B > (1 << 28)) return hipErrorInvalidValue;
  const int D = (int)HW;
  if (!table || !images_bits_fits(table, B, D) || nvalid < 1 || nvalid > 3 * B || (ldx % 8) || !dyn || !xp.p || !xbf ||
      !xbits || (!no_xbw && !xbw) || kts_f != bitmat_kts(D + 1) || kts_w != bitmat_kts(3 * B) || ldbits < D / 8)
    return hipErrorInvalidValue;
  const dim3 g((kts_f + 1) / 2, B / 64);
  if (no_xbw)
    hipLaunchKernelGGL(images_bits_kernel<true>, g, dim3(256), 0, st, table, idx, nvalid, div, B, D, kts_f, kts_w, xbf,
                       xbw, xbits, ldbits, dyn, dyn_next);
  else
    hipLaunchKernelGGL(images_bits_kernel<false>, g, dim3(256), 0, st, table, idx, nvalid, div, B, D, kts_f, kts_w,
                       xbf, xbw, xbits, ldbits, dyn, dyn_next);
  // (256 workgroups striding, as launch_deint_grey: for a 0/1 table every one returns at once)
  hipLaunchKernelGGL(images_grey_kernel, dim3(256), dim3(256), 0, st, table, idx, nvalid, div, xs, xp.p, xp.stride,
                     xp.n, f32dyn_mask, dyn, B, D, ldx);
  return hipGetLastError();
}

hipError_t launch_images_x(const unsigned char* table, int H, int W, const int* idx, int nvalid, float div, int B,
                           float* x, hipStream_t st) {
  const long long HW = (long long)H * W;
  if (!table || !x || H <= 0 || W <= 0 || HW > (1 << 30) || B <= 0 || B > 65535 || nvalid < 1 || nvalid > 3 * B)
    return hipErrorInvalidValue;
  const int D = (int)HW;
  hipLaunchKernelGGL(images_x_kernel, dim3((D + 255) / 256, B), dim3(256), 0, st, table, idx, nvalid, div, B, D, x);
  return hipGetLastError();
}

}  // namespace mvae
