// Batch input (gfx950): everything that turns a batch into the layer-0 operand.
//
//   plane path   deinterleave_*_kernel + residual_planes_kernel: X [B][3 D] -> the stacked rows
//                [rot | lock | key] as bf16 planes (and fp32 rows where something reads them)
//   bits path    deint_bits_kernel<Src, NOW> + deint_grey_kernel<Src>: a 0/1 batch as the eight-phase
//                kernel's BitMats (mvae_internal.h) -- xbf = A of the forward (stacked rows x pixels,
//                the ones column at k = D), xbw = A of the weight gradient (pixels x stacked rows, the
//                ones row at pixel D) -- plus the BCE target (the lock block) as bits per row
//                (GemmEpi::xbits): 1.1 bits written per pixel triple instead of the 48 of the bf16
//                plane. bits_transpose_kernel makes xbw from xbf (the xbw_split schedule).
//   producers    make_batch*_kernel (a pairs batch as X), images_x_kernel (an embedding pass as X):
//                the materialising routes, and the ABI's mvae_make_batch*.
//
// The bits path reads a batch through an octet source (XSrc, PairsSrc, ImagesSrc below): the fp32 X,
// the uint8 lock / key tables with (idx, kidx, rotation coefficients), or one uint8 image table. The
// table sources form an octet's 24 values as the producers form them, (float)byte / div, and the
// bit and the not-binary test derive from that float: the flags rise for exactly the batches they
// rise for through X, for div 255 and div 1 alike.
//
// Row order of every stacked buffer: [rotated lock | lock | key] (3B rows) <- X's channels (1, 0, 2).
// Padding outside the written BitMat blocks (rows past 3B, pixel quarters past D) is zero from the
// buffers' creation.
#include "mvae_internal.h"

namespace mvae {
namespace {

inline unsigned nblocks(size_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// bf16 bits of v rounded to nearest even, and the exact remainder v - bf16(v)
__device__ __forceinline__ unsigned short bf16_rn(float v, float& rem) {
  const unsigned short b = __builtin_bit_cast(unsigned short, __float2bfloat16(v));
  rem = v - __uint_as_float((unsigned)b << 16);
  return b;
}
__device__ __forceinline__ uint2 pack4(unsigned short a, unsigned short b, unsigned short c,
                                       unsigned short d) {
  return make_uint2((unsigned)a | (unsigned)b << 16, (unsigned)c | (unsigned)d << 16);
}

// 4 NQ pixels (3 NQ float4 of x in v, pixel order) of row b from column col -> the fp32 rows
// of the blocks in f32mask and bf16 plane 0 (16-B stores); returns whether a pixel is inexact
template <int NQ>
__device__ __forceinline__ bool deint_put(const float4* v, float* __restrict__ xs,
                                          unsigned short* __restrict__ xp, int B, int b,
                                          size_t col, int ldx, int f32mask) {
  static_assert(NQ % 2 == 0, "whole 16-B plane stores");
  constexpr int NP = 4 * NQ;
  bool nz = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int ch = c == 0 ? 1 : (c == 1 ? 0 : 2);  // block c (rot, lock, key) <- channel ch
    float f[NP];
#pragma unroll
    for (int h = 0; h < NQ; ++h) {
      const float4 a = v[3 * h], bb = v[3 * h + 1], cc = v[3 * h + 2];
      const float e[12] = {a.x, a.y, a.z, a.w, bb.x, bb.y, bb.z, bb.w, cc.x, cc.y, cc.z, cc.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) f[4 * h + j] = e[3 * j + ch];
    }
    const size_t o = (size_t)(c * B + b) * ldx + col;
    if (f32mask >> c & 1) {
#pragma unroll
      for (int h = 0; h < NQ; ++h)
        *reinterpret_cast<float4*>(xs + o + 4 * h) = make_float4(f[4 * h], f[4 * h + 1], f[4 * h + 2], f[4 * h + 3]);
    }
    if (xp) {
#pragma unroll
      for (int h = 0; h < NQ; h += 2) {
        float r[8];
        unsigned short h16[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) h16[j] = bf16_rn(f[4 * h + j], r[j]);
        const uint2 lo = pack4(h16[0], h16[1], h16[2], h16[3]), hi = pack4(h16[4], h16[5], h16[6], h16[7]);
        *reinterpret_cast<uint4*>(xp + o + 4 * h) = make_uint4(lo.x, lo.y, hi.x, hi.y);
#pragma unroll
        for (int j = 0; j < 8; ++j) nz |= r[j] != 0.f;
      }
    }
  }
  return nz;
}

// ---------------------------------------------------------------- plane de-interleave
// x[b][p*3 + c] (c: 0 lock, 1 rotated lock, 2 key; 11a/overlap_input.py:117-119,201)
//  -> xs[(blk*B + b)][p], blk = {rot:0, lock:1, key:2}. Each thread moves 4 pixels:
// three 16-B loads, three 16-B stores (coalesced both ways).

// [B, D, 3] interleaved (lock, rotated, key) -> row blocks [rot | lock | key] of the layer-0
// operand: fp32 rows for the blocks in f32mask (bit c: block c; plane modes keep only the lock
// block, the BCE target) and the RN bf16 plane 0 (8-byte stores). In the exact-split mode the
// residual planes are NOT written here: the kernel only raises *dyn when some pixel is not
// exact in bf16, and residual_planes_kernel then writes planes 1 and 2 (binary shape images
// never pay for them; the GEMMs read the residual planes only when *dyn != 0).
__global__ void deinterleave_vec_kernel(const float4* __restrict__ x, float* __restrict__ xs,
                                        unsigned short* __restrict__ xp, int* __restrict__ dyn,
                                        int B, int D, int ldx, int f32mask, int* __restrict__ dyn_next) {
  // the other slot of the flags, for the next de-interleave (no per-step memset launch); this
  // form does not test for 0/1 pixels: it raises the not-binary word (dyn[2]) unconditionally
  if ((blockIdx.x | blockIdx.y | threadIdx.x) == 0) {
    if (dyn_next) dyn_next[0] = dyn_next[2] = 0;
    if (dyn) atomicOr(dyn + 2, 1);
  }
  const int b = blockIdx.y;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;  // pixel quad
  bool nz = false;
  if (q * 4 < D) {
    const float4* src = x + ((size_t)b * 3 * D) / 4 + 3 * q;
    const float4 v0 = src[0], v1 = src[1], v2 = src[2];
    // pixels p0..p3: (l,r,k) = (v0.x v0.y v0.z) (v0.w v1.x v1.y) (v1.z v1.w v2.x) (v2.y v2.z v2.w)
    const float4 vv[3] = {make_float4(v0.y, v1.x, v1.w, v2.z),   // rot
                          make_float4(v0.x, v0.w, v1.z, v2.y),   // lock
                          make_float4(v0.z, v1.y, v2.x, v2.w)};  // key
    const size_t col = 4 * (size_t)q;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t o = (size_t)(c * B + b) * ldx + col;
      if (f32mask >> c & 1) *reinterpret_cast<float4*>(xs + o) = vv[c];
      if (xp) {
        float r0, r1, r2, r3;
        const uint2 w = pack4(bf16_rn(vv[c].x, r0), bf16_rn(vv[c].y, r1), bf16_rn(vv[c].z, r2),
                              bf16_rn(vv[c].w, r3));
        *reinterpret_cast<uint2*>(xp + o) = w;
        nz |= (r0 != 0.f) | (r1 != 0.f) | (r2 != 0.f) | (r3 != 0.f);
      }
    }
  }
  if (dyn && __ballot(nz) != 0 && (threadIdx.x & 63) == 0) atomicOr(dyn, 1);
}

// The same for 4 NQ pixels per thread (D % (4 NQ) == 0): 3 NQ 16-B loads (48 NQ contiguous
// bytes) issued together, then per block NQ / 2 16-B plane stores. 8 pixels per thread measured
// 0.305 -> 0.287 ms at C3 (profiles/r4/r4y_deinterleave.txt)
template <int NQ>
__global__ void deinterleave_vecn_kernel(const float4* __restrict__ x, float* __restrict__ xs,
                                         unsigned short* __restrict__ xp, int* __restrict__ dyn,
                                         int B, int D, int ldx, int f32mask, int* __restrict__ dyn_next,
                                         unsigned char* __restrict__ xbits, int ldbits) {
  // the other slot of the flags, for the next de-interleave (no per-step memset launch)
  if (dyn_next && (blockIdx.x | blockIdx.y | threadIdx.x) == 0) dyn_next[0] = dyn_next[2] = 0;
  constexpr int NP = 4 * NQ;  // pixels per thread
  const int b = blockIdx.y;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  bool nz = false, nb = false;
  if (q * NP < D) {
    const float4* src = x + ((size_t)b * 3 * D) / 4 + 3 * NQ * q;
    float4 v[3 * NQ];
#pragma unroll
    for (int i = 0; i < 3 * NQ; ++i) v[i] = src[i];
    // some value of the three channels neither 0 nor 1 (the BCE target is one of them)
#pragma unroll
    for (int i = 0; i < 3 * NQ; ++i) {
      const float e[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) nb |= (e[j] != 0.f) & (e[j] != 1.f);
    }
    nz = deint_put<NQ>(v, xs, xp, B, b, (size_t)NP * q, ldx, f32mask);
    if (xbits) {  // the lock channel (element 3 j of pixel j) as bits, 8 pixels per byte
      static_assert(NQ == 2, "one byte per thread");
      const float e[24] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                           v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w,
                           v[4].x, v[4].y, v[4].z, v[4].w, v[5].x, v[5].y, v[5].z, v[5].w};
      unsigned byte = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) byte |= (e[3 * j] != 0.f ? 1u : 0u) << j;
      xbits[(size_t)b * ldbits + q] = (unsigned char)byte;
    }
  }
  if (dyn) {  // (the ballots with every lane of the wave active)
    const bool anz = __ballot(nz) != 0, anb = __ballot(nb) != 0;
    if ((threadIdx.x & 63) == 0) {
      if (anz) atomicOr(dyn, 1);
      if (anb) atomicOr(dyn + 2, 1);
    }
  }
}

__global__ void deinterleave_scalar_kernel(const float* __restrict__ x, float* __restrict__ xs,
                                           unsigned short* __restrict__ xp, int* __restrict__ dyn,
                                           int B, int D, int ldx, int f32mask, int* __restrict__ dyn_next) {
  // the other slot of the flags (see deinterleave_vec_kernel: no 0/1 test here)
  if ((blockIdx.x | blockIdx.y | threadIdx.x) == 0) {
    if (dyn_next) dyn_next[0] = dyn_next[2] = 0;
    if (dyn) atomicOr(dyn + 2, 1);
  }
  const int b = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  bool nz = false;
  if (p < D) {
    const float* src = x + (size_t)b * 3 * D + 3 * (size_t)p;
    const float v[3] = {src[1], src[0], src[2]};  // rot, lock, key
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t o = (size_t)(c * B + b) * ldx + p;
      if (f32mask >> c & 1) xs[o] = v[c];
      if (xp) {
        float r;
        xp[o] = bf16_rn(v[c], r);
        nz |= r != 0.f;
      }
    }
  }
  if (dyn && __ballot(nz) != 0 && (threadIdx.x & 63) == 0) atomicOr(dyn, 1);
}

// Only when *dyn != 0 (some pixel of the batch is not a bf16 value): planes 1 and 2 of the
// exact split of the layer-0 operand (3-plane mode), and the fp32 rows of the blocks in
// f32mask (the BCE target, read from bf16 plane 0 while every pixel is exact).
__global__ void residual_planes_kernel(const float* __restrict__ x, float* __restrict__ xs,
                                       unsigned short* __restrict__ xp, long long ps, int np,
                                       int f32mask, const int* __restrict__ dyn, int B, int D,
                                       int ldx) {
  if (*dyn == 0) return;
  const size_t n = (size_t)B * D;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / D, p = i - b * D;
    const float* src = x + b * 3 * D + 3 * p;
    const float v[3] = {src[1], src[0], src[2]};  // rot, lock, key
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t o = (size_t)(c * B + b) * ldx + p;
      if (f32mask >> c & 1) xs[o] = v[c];
      if (np == 3) {
        float r1, r2, r3;
        (void)bf16_rn(v[c], r1);
        xp[ps + o] = bf16_rn(r1, r2);
        xp[2 * ps + o] = bf16_rn(r2, r3);
      }
    }
  }
}

// ---------------------------------------------------------------- the rotated lock's gather
// tf.contrib.image.rotate semantics (11a/overlap_input.py:127-261): output pixel (xx, yy) samples
// the lock at ((c*x - s*y) + x_off, (s*x + c*y) + y_off), NEAREST = roundf, zero fill; cf = (c, s,
// x_off, y_off), per example, precomputed in fp32 on the host. Gives the rounded sample position (xr, yr);
// rot_inside / rot_at: whether it lies in the image and its pixel index there. No FMA contraction, so the
// gather indices match the host restatement bit for bit (hipcc contracts even the *_rn intrinsics into
// FMAs unless contraction is off -- their bodies are outside -- and a few pixels per batch then
// sampled a neighbour; caught by tests/test_input_pipeline.py's grey-value tables). The only place
// this arithmetic is written: the producers and the pairs source call it.
__device__ __forceinline__ void rot_sample(const float4& cf, int xx, int yy, float& xr, float& yr) {
#pragma clang fp contract(off)
  const float fx = (float)xx, fy = (float)yy;
  const float xin = (cf.x * fx - cf.y * fy) + cf.z;  // unfused: fp contract(off) above
  const float yin = (cf.y * fx + cf.x * fy) + cf.w;
  xr = roundf(xin);
  yr = roundf(yin);
}
// whether the rounded sample (xr, yr) lies in the H x W image, and its pixel index there
__device__ __forceinline__ bool rot_inside(float xr, float yr, int H, int W) {
  return xr >= 0.f && xr <= (float)(W - 1) && yr >= 0.f && yr <= (float)(H - 1);
}
__device__ __forceinline__ int rot_at(float xr, float yr, int W) { return (int)yr * W + (int)xr; }

// ---------------------------------------------------------------- octet sources
// Where the bits path reads a [B][D] batch from: a POD passed by value as the kernel argument.
//   Row row(b, B, D)      what batch row b's loads start from (may load the row's indices)
//   Raw load(row, pix)    the raw data of its pixels [pix, pix + 8) x 3 channels (pix % 8 == 0)
//   values(raw, e)        those 24 values as X would store them: per pixel (lock, rotated lock, key)
//   CLAMPED               loads are unconditional, of a pixel clamped into the image (else they are
//                         guarded: only octets whole inside the image are loaded)
// row and load are apart so that deint_bits_kernel issues every row's index loads, then every row's
// pixel loads, before the first use.

// fp32 X [B][3 D], 16-B aligned
struct XSrc {
  // (unconditional loads -- octets past D read the row's last one, unused -- so the values need no
  // merge with a not-loaded path, whose register copies would wait for every load at once)
  static constexpr bool CLAMPED = true;
  const float4* x;
  struct Row { int b, D; };  // (nothing to load for a row)
  struct Raw { float4 v[6]; };
  __device__ __forceinline__ Row row(int b, int, int D) const { return {b, D}; }
  __device__ __forceinline__ Raw load(const Row& r, int pix) const {
    const float4* src = x + ((size_t)r.b * 3 * r.D + 3 * (size_t)pix) / 4;
    Raw o;
#pragma unroll
    for (int k = 0; k < 6; ++k) o.v[k] = src[k];
    return o;
  }
  __device__ __forceinline__ void values(const Raw& r, float (&e)[24]) const {
#pragma unroll
    for (int k = 0; k < 6; ++k) { e[4 * k] = r.v[k].x; e[4 * k + 1] = r.v[k].y; e[4 * k + 2] = r.v[k].z; e[4 * k + 3] = r.v[k].w; }
  }
};

// An octet's 24 values as X would store them, from the raw bytes of its 8 pixels in the three
// channels (eight bytes per uint2, pixel j in byte j): per pixel (lock, rotated lock, key) / div, the
// producers' (float)byte / div
__device__ __forceinline__ void byte_values(const uint2& l, const uint2& r, const uint2& k, float div,
                                            float (&e)[24]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int sh = 8 * (j & 3);
    e[3 * j] = (float)(((j < 4 ? l.x : l.y) >> sh) & 0xFFu) / div;
    e[3 * j + 1] = (float)(((j < 4 ? r.x : r.y) >> sh) & 0xFFu) / div;
    e[3 * j + 2] = (float)(((j < 4 ? k.x : k.y) >> sh) & 0xFFu) / div;
  }
}

// The uint8 lock / key tables (8-byte aligned, D = H W % 8 == 0): row b is lock idx[b], its rotation
// by coef[b] (rot_sample: 8 byte gathers from the lock image, which stay in cache -- it was just
// read; a sample outside the image is 0, its load clamped to pixel 0) and key kidx[b]
struct PairsSrc {
  static constexpr bool CLAMPED = false;
  const unsigned char* locks;
  const unsigned char* keys;
  int H, W;
  const int* idx;
  const int* kidx;
  const float4* coef;
  float div;
  struct Row {
    const unsigned char* L;  // its lock image
    const unsigned char* K;  // its key image
    float4 cf;               // (cos, sin, x_off, y_off) of its rotation
  };
  struct Raw { uint2 l, k, r; };  // lock, key, rotated lock
  __device__ __forceinline__ Row row(int b, int, int D) const {
    return {locks + (size_t)idx[b] * D, keys + (size_t)kidx[b] * D, coef[b]};
  }
  __device__ __forceinline__ Raw load(const Row& row, int pix) const {
    Raw o;
    o.l = *reinterpret_cast<const uint2*>(row.L + pix);
    o.k = *reinterpret_cast<const uint2*>(row.K + pix);
    int yy = pix / W, xx = pix - yy * W;
    unsigned rb[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float xr, yr;
      rot_sample(row.cf, xx, yy, xr, yr);
      const bool ok = rot_inside(xr, yr, H, W);
      const unsigned v = row.L[ok ? rot_at(xr, yr, W) : 0];
      rb[j >> 2] |= (ok ? v : 0u) << (8 * (j & 3));
      if (++xx == W) { xx = 0; ++yy; }
    }
    o.r = make_uint2(rb[0], rb[1]);
    return o;
  }
  __device__ __forceinline__ void values(const Raw& p, float (&e)[24]) const { byte_values(p.l, p.r, p.k, div, e); }
};

// One uint8 image table (8-byte aligned, D % 8 == 0), an embedding pass of 3B independent images:
// image t of the pass is row t of the stacked operand, i.e. the three byte octets of batch row b
// come from the images b (block 0, where a training batch has the rotated lock), B + b (block 1, the
// lock) and 2 B + b (block 2, the key). Image t is table image idx[t] (t when idx is null) for
// t < nvalid and an all-zero image past that: idx and the table are not read for those rows.
struct ImagesSrc {
  static constexpr bool CLAMPED = false;
  const unsigned char* table;
  const int* idx;
  int nvalid;
  float div;
  // image t of the pass: its first byte, or null for a row past the last wanted image
  __device__ __forceinline__ const unsigned char* image(int t, int D) const {
    if (t >= nvalid) return nullptr;
    return table + (size_t)(idx ? idx[t] : t) * D;
  }
  struct Row { const unsigned char* img[3]; };  // [block]
  struct Raw { uint2 c[3]; };                   // [block]
  __device__ __forceinline__ Row row(int b, int B, int D) const {
    return {{image(b, D), image(B + b, D), image(2 * B + b, D)}};
  }
  __device__ __forceinline__ Raw load(const Row& row, int pix) const {
    Raw o;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o.c[c] = row.img[c] ? *reinterpret_cast<const uint2*>(row.img[c] + pix) : make_uint2(0u, 0u);
    return o;
  }
  __device__ __forceinline__ void values(const Raw& p, float (&e)[24]) const {
    byte_values(p.c[1], p.c[0], p.c[2], div, e);
  }
};

// ---------------------------------------------------------------- de-interleave to bits
// One workgroup of BITS_NT threads per task of 64 batch rows x 64 BITS_PB pixels: thread tid owns
// octet tid % BITS_NO of rows tid / BITS_NO + BITS_RPP i. Each thread reads its octets (X: 4 x 96
// contiguous bytes, as the plane kernel), writes one byte per block into LDS ([block][octet][row]:
// a row-contiguous 8 x 8 bit block is one u64), then the workgroup assembles the forward words four
// at a time (one 16-B store) and the weight-gradient words one at a time.
constexpr int BITS_PB = 2, BITS_NT = 256;
constexpr int BITS_OS = 72;                  // LDS bytes per octet row (the 16 octets of a write land on 16 banks)
constexpr int BITS_NO = 8 * BITS_PB;         // octets per row
constexpr int BITS_RPP = BITS_NT / BITS_NO;  // rows per pass
constexpr int BITS_NR = 64 / BITS_RPP;       // row passes per thread
static_assert(BITS_NT % BITS_NO == 0 && 64 % BITS_RPP == 0, "whole rows per pass");
using BitsLds = unsigned char[3][BITS_NO][BITS_OS];  // a task's bytes: [block][octet][row]

// bits el = 0..7 of b -> positions 0..3 (even el) and 16..19 (odd el): a BitMat word's layout
__device__ __forceinline__ unsigned bits_spread(unsigned b) {
  unsigned e = b & 0x55u, o = (b >> 1) & 0x55u;
  e = (e | (e >> 1)) & 0x33u; e = (e | (e >> 2)) & 0x0Fu;
  o = (o | (o >> 1)) & 0x33u; o = (o | (o >> 2)) & 0x0Fu;
  return e | (o << 16);
}

// one row's 8 pixels x 3 channels (interleaved, as X stores them) -> the byte of each block
// (bit j = pixel j nonzero; block c: rot, lock, key <- channels 1, 0, 2); true if a value is not
// 0 / 1
__device__ __forceinline__ bool deint_octet(const float (&e)[24], unsigned (&by3)[3]) {
  bool nb = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int ch = c == 0 ? 1 : (c == 1 ? 0 : 2);
    unsigned byte = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = e[3 * j + ch];
      byte |= (f != 0.f ? 1u : 0u) << j;
      nb |= (f != 0.f) & (f != 1.f);
    }
    by3[c] = byte;
  }
  return nb;
}

// the task's BitMat words from its LDS bytes: the forward words four at a time (lanes 2 q, 2 q + 1
// of the fragment layout, words j = 0 / 1 each: rows 16 (2 j + h) + (lane & 15), k-octet 8 kk +
// 4 kh + (lane >> 4); one 16-B store), the weight-gradient words one at a time (pixel 64 kk +
// 16 (2 j + h) + (lane & 15), rows 32 kh + 8 (lane >> 4) + 0..7: bit (pixel & 7) of 8 row bytes of
// one octet). NOW: no weight-gradient words.
template <bool NOW>
__device__ __forceinline__ void deint_words(int B, int D, int kts_f, int kts_w, unsigned* __restrict__ xbf,
                                            unsigned* __restrict__ xbw, int bx, int by, const BitsLds& bt) {
  constexpr int PB = BITS_PB;
  const int b0 = by * 64, p0 = bx * 64 * PB;
  for (int wq = threadIdx.x; wq < 3 * PB * 32; wq += BITS_NT) {
    const int c = wq / (PB * 32), kk = (wq / 32) % PB, wl0 = 4 * (wq & 31);
    const int kt = PB * bx + kk;
    if (kt >= kts_f) continue;
    const int grow = c * B + b0;  // first stacked row of this task's 64
    unsigned w4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int wl = wl0 + q, lane = wl >> 1, j = wl & 1;
      unsigned w = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
          w |= bits_spread(bt[c][8 * kk + 4 * kh + (lane >> 4)][16 * (2 * j + h) + (lane & 15)]) << (8 * h + 4 * kh);
      w4[q] = w;
    }
    unsigned* dst = xbf + ((size_t)(grow >> 8) * kts_f + kt) * BITMAT_BLOCK_WORDS + ((grow >> 6) & 3) * 128 + wl0;
    *reinterpret_cast<uint4*>(dst) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
  }
  for (int wi = threadIdx.x; wi < (NOW ? 0 : 3 * PB * 128); wi += BITS_NT) {  // (NOW: no xbw)
    const int c = wi / (PB * 128), kk = (wi / 128) % PB, wl = wi & 127, lane = wl >> 1, j = wl & 1;
    const int grow = c * B + b0;
    const int pq = p0 + 64 * kk;
    if (pq > D) continue;
    unsigned w = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        const int pr = 64 * kk + 16 * (2 * j + h) + (lane & 15);
        const unsigned long long rows =
            *reinterpret_cast<const unsigned long long*>(&bt[c][pr >> 3][32 * kh + 8 * (lane >> 4)]);
        const unsigned long long col = (rows >> (pr & 7)) & 0x0101010101010101ull;
        const unsigned byte = (unsigned)((col * 0x0102040810204080ull) >> 56);  // bit i = row i
        w |= bits_spread(byte) << (8 * h + 4 * kh);
      }
    xbw[((size_t)(pq >> 8) * kts_w + (grow >> 6)) * BITMAT_BLOCK_WORDS + ((pq >> 6) & 3) * 128 + wl] = w;
  }
}

// The rest of a task once every thread has put its octets (nb: this thread saw a value not 0 / 1):
// the not-binary word, the workgroup's synchronisation, the BitMat words
template <bool NOW>
__device__ __forceinline__ void bits_tail(bool nb, int B, int D, int kts_f, int kts_w, unsigned* __restrict__ xbf,
                                          unsigned* __restrict__ xbw, int* __restrict__ dyn, int bx, int by,
                                          const BitsLds& bt) {
  const int tid = threadIdx.x;
  if (dyn) {
    const bool anb = __ballot(nb) != 0;
    if ((tid & 63) == 0 && anb) atomicOr(dyn + 2, 1);
  }
  __syncthreads();
  deint_words<NOW>(B, D, kts_f, kts_w, xbf, xbw, bx, by, bt);
}

// One octet of one task row into the task's LDS bytes: its three block bytes from the 24 values e
// (an octet inside the image, `in`; then also the row's target byte into xbits) or the padding byte
// `pad`; returns whether a value is not 0 / 1
__device__ __forceinline__ bool octet_put(bool in, unsigned pad, const float (&e)[24],
                                          unsigned char* __restrict__ xbits_at, BitsLds& bt, int o, int r) {
  bool nb = false;
  unsigned by3[3] = {pad, pad, pad};
  if (in) {
    nb = deint_octet(e, by3);
    *xbits_at = (unsigned char)by3[1];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) bt[c][o][r] = (unsigned char)by3[c];
  return nb;
}
// the ones column (pixel D) and zeros of an octet at pixel pix that is not whole inside the image
__device__ __forceinline__ unsigned octet_pad(int pix, int D) {
  return (pix <= D && D < pix + 8) ? 1u << (D - pix) : 0u;
}

// this thread's octet, at pixel pix, of its BITS_NR rows of the task from batch row b0: every row's
// index loads, then every row's pixel loads, before the first use
template <class Src>
__device__ __forceinline__ void bits_load(const Src& src, int B, int D, int b0, int pix,
                                          typename Src::Raw (&raw)[BITS_NR]) {
  const int tid = threadIdx.x;
  typename Src::Row row[BITS_NR];
#pragma unroll
  for (int i = 0; i < BITS_NR; ++i) row[i] = src.row(b0 + tid / BITS_NO + BITS_RPP * i, B, D);
#pragma unroll
  for (int i = 0; i < BITS_NR; ++i) raw[i] = src.load(row[i], pix);
}

// Task (blockIdx.x, blockIdx.y): pixels [128 bx, +128), batch rows [64 by, +64). Raises the
// not-binary word (dyn[2]) when a pixel is neither 0 nor 1: the step then runs deint_grey_kernel
// (the planes) and the GEMMs read the planes. NOW: no weight-gradient words (the xbw_split schedule:
// launch_bits_transpose writes them; an evaluation pass reads none).
template <class Src, bool NOW>
__global__ __launch_bounds__(BITS_NT) void deint_bits_kernel(Src src, int B, int D, int kts_f, int kts_w,
                                                             unsigned* __restrict__ xbf, unsigned* __restrict__ xbw,
                                                             unsigned char* __restrict__ xbits, int ldbits,
                                                             int* __restrict__ dyn, int* __restrict__ dyn_next) {
  // the other slot of the flags, for the next pass (no per-step memset launch)
  if (dyn_next && (blockIdx.x | blockIdx.y | threadIdx.x) == 0) dyn_next[0] = dyn_next[2] = 0;
  __shared__ __attribute__((aligned(16))) BitsLds bt;
  typename Src::Raw raw[BITS_NR] = {};
  if (Src::CLAMPED)  // (loads first, of the row's last octet for an octet past D)
    bits_load(src, B, D, (int)blockIdx.y * 64, min((int)blockIdx.x * 64 * BITS_PB + 8 * ((int)threadIdx.x % BITS_NO), D - 8), raw);
  const int tid = threadIdx.x, bx = blockIdx.x, by = blockIdx.y;
  const int b0 = by * 64, o = tid % BITS_NO, pix = bx * 64 * BITS_PB + 8 * o;
  const bool in = pix + 8 <= D;  // (D % 8 == 0: an octet is whole inside the image or whole outside)
  const unsigned pad = octet_pad(pix, D);
  if (!Src::CLAMPED && in) bits_load(src, B, D, b0, pix, raw);
  bool nb = false;
#pragma unroll
  for (int i = 0; i < BITS_NR; ++i) {
    const int r = tid / BITS_NO + BITS_RPP * i;
    float e[24];
    src.values(raw[i], e);
    nb |= octet_put(in, pad, e, xbits + (size_t)(b0 + r) * ldbits + (pix >> 3), bt, o, r);
  }
  bits_tail<NOW>(nb, B, D, kts_f, kts_w, xbf, xbw, dyn, bx, by, bt);
}

// The weight gradient's BitMat (pixels x stacked rows) from the forward's (stacked rows x
// pixels): one wave per 64 x 64 bit tile -- a quarter of a block on either side -- its 128 words in,
// the tile as [8 pixel octets][64 rows] bytes in LDS, its 128 transposed words out (the 8 x 8 bit
// transpose of deint_words). The de-interleave then writes only the forward words (no_xbw): the
// transpose runs on the side stream beside the layer-0 forward, whose 192 tiles (C3) leave CUs free,
// and the layer-0 weight gradient waits for it.
__device__ __forceinline__ unsigned bits_compact(unsigned s) {  // inverse of bits_spread (low byte)
  unsigned e = s & 0xFu, o = (s >> 16) & 0xFu;
  e = (e | (e << 2)) & 0x33u; e = (e | (e << 1)) & 0x55u;
  o = (o | (o << 2)) & 0x33u; o = (o | (o << 1)) & 0x55u;
  return e | (o << 1);
}
__global__ __launch_bounds__(256) void bits_transpose_kernel(const unsigned* __restrict__ xbf, int kts_f,
                                                             unsigned* __restrict__ xbw, int kts_w, int nrow64) {
  __shared__ __attribute__((aligned(16))) unsigned char tb[4][8][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + wave;
  const bool ok = tile < nrow64 * kts_f;
  const int a = ok ? tile % nrow64 : 0, b = ok ? tile / nrow64 : 0;  // stacked-row tile, pixel tile
  if (ok) {
    const uint2 w = *reinterpret_cast<const uint2*>(xbf + ((size_t)(a >> 2) * kts_f + b) * BITMAT_BLOCK_WORDS +
                                                    (a & 3) * 128 + 2 * lane);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
          tb[wave][4 * kh + (lane >> 4)][16 * (2 * j + h) + (lane & 15)] =
              (unsigned char)bits_compact((j ? w.y : w.x) >> (8 * h + 4 * kh));
  }
  __syncthreads();
  if (!ok) return;
  unsigned out[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    unsigned wo = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        const int p = 16 * (2 * j + h) + (lane & 15);
        const unsigned long long rows =
            *reinterpret_cast<const unsigned long long*>(&tb[wave][p >> 3][32 * kh + 8 * (lane >> 4)]);
        const unsigned long long col = (rows >> (p & 7)) & 0x0101010101010101ull;
        wo |= bits_spread((unsigned)((col * 0x0102040810204080ull) >> 56)) << (8 * h + 4 * kh);
      }
    out[j] = wo;
  }
  *reinterpret_cast<uint2*>(xbw + ((size_t)(b >> 2) * kts_w + a) * BITMAT_BLOCK_WORDS + (b & 3) * 128 + 2 * lane) =
      make_uint2(out[0], out[1]);
}

// The plane image of a batch with a pixel other than 0 or 1 (after deint_bits_kernel raised the
// not-binary word; else every workgroup returns at once): bf16 plane 0 (planes 1-2 of the exact
// split too when np == 3), the fp32 rows of the blocks in f32mask, and the inexact flag (*dyn) --
// what the plane path's GEMMs and the BCE epilogue read. Workgroups stride over the 8-pixel groups,
// each octet's 24 values read again through the source.
template <class Src>
__global__ void deint_grey_kernel(Src src, float* __restrict__ xs, unsigned short* __restrict__ xp, long long ps,
                                  int np, int f32mask, int* __restrict__ dyn, int B, int D, int ldx) {
  if (dyn[2] == 0) return;
  const int nq = D / 8;
  const size_t n = (size_t)B * nq;
  bool nz = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / nq), q = (int)(i % nq);
    float e[24];
    src.values(src.load(src.row(b, B, D), 8 * q), e);
    const float4 v[6] = {make_float4(e[0], e[1], e[2], e[3]),     make_float4(e[4], e[5], e[6], e[7]),
                         make_float4(e[8], e[9], e[10], e[11]),   make_float4(e[12], e[13], e[14], e[15]),
                         make_float4(e[16], e[17], e[18], e[19]), make_float4(e[20], e[21], e[22], e[23])};
    nz |= deint_put<2>(v, xs, xp, B, b, (size_t)8 * q, ldx, f32mask);
    if (np == 3) {  // the exact split's residual planes of the 24 values
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int ch = c == 0 ? 1 : (c == 1 ? 0 : 2);
        const size_t o = (size_t)(c * B + b) * ldx + (size_t)8 * q;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float r1, r2, r3;
          (void)bf16_rn(e[3 * j + ch], r1);
          xp[ps + o + j] = bf16_rn(r1, r2);
          xp[2 * ps + o + j] = bf16_rn(r2, r3);
        }
      }
    }
  }
  if (__ballot(nz) != 0 && (threadIdx.x & 63) == 0) atomicOr(dyn, 1);
}

// ---------------------------------------------------------------- batch producers
// The reference's input pipeline for one batch (11a/overlap_input.py:127-261): lock and key
// images from uint8 tables, the lock rotated (rot_sample), concatenated per pixel as
// (lock, rotated, key) and divided by 255 -> X [B, H*W*3].
// Row b is lock idx[b], its rotation, and key kidx[b] (the own pair passes idx for both).
__global__ void make_batch_kernel(const unsigned char* __restrict__ locks,
                                  const unsigned char* __restrict__ keys, int H, int W,
                                  const int* __restrict__ idx, const int* __restrict__ kidx,
                                  const float4* __restrict__ coef, float div, float* __restrict__ x) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int HW = H * W;
  if (p >= HW) return;
  const int id = idx[b], kid = kidx[b];
  const float4 cf = coef[b];
  // (the row's three scalar loads in flight together and waited for once: left to itself the
  // scheduler issues the key's index or the coefficients only after waiting for the lock's index, a
  // second round trip at the head of a short workgroup)
  asm volatile("" ::"s"(id), "s"(kid), "s"(cf.x), "s"(cf.y), "s"(cf.z), "s"(cf.w));
  const int yy = p / W, xx = p - yy * W;
  float xr, yr;
  rot_sample(cf, xx, yy, xr, yr);
  const unsigned char* L = locks + (size_t)id * HW;
  float rot = 0.f;
  if (rot_inside(xr, yr, H, W)) rot = (float)L[rot_at(xr, yr, W)];
  float* o = x + (size_t)b * 3 * HW + 3 * (size_t)p;
  o[0] = (float)L[p] / div;
  o[1] = rot / div;
  o[2] = (float)keys[(size_t)kid * HW + p] / div;
}

// The same batch (bit for bit) at 4 pixels per thread for H*W % 4 == 0 and a 16-B aligned x:
// one 4-B load each of the lock and key bytes, the 12 output floats of a thread written to LDS,
// and the workgroup's 1024-pixel segment of the output row (12 KB, contiguous in x) stored back
// with 16-B stores that are contiguous across each wave (3 per thread). The per-pixel store of
// make_batch_kernel (three 4-B stores at a 12-B lane stride) ran at ~2.1-2.5 TB/s.
constexpr int MB_PIX = 4 * 256;  // pixels per workgroup
__global__ __launch_bounds__(256) void make_batch4_kernel(const unsigned char* __restrict__ locks,
                                                          const unsigned char* __restrict__ keys, int H,
                                                          int W, const int* __restrict__ idx,
                                                          const int* __restrict__ kidx,
                                                          const float4* __restrict__ coef, float div,
                                                          float* __restrict__ x) {
  __shared__ __attribute__((aligned(16))) float seg[3 * MB_PIX];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int HW = H * W;
  const int s0 = blockIdx.x * MB_PIX;  // first pixel of the segment
  const int p0 = s0 + 4 * tid;
  const int id = idx[b], kid = kidx[b];
  const float4 cf = coef[b];
  // (the row's three scalar loads in flight together, as make_batch_kernel)
  asm volatile("" ::"s"(id), "s"(kid), "s"(cf.x), "s"(cf.y), "s"(cf.z), "s"(cf.w));
  const unsigned char* L = locks + (size_t)id * HW;
  if (p0 < HW) {
    const uchar4 lv = *reinterpret_cast<const uchar4*>(L + p0);
    const uchar4 kv = *reinterpret_cast<const uchar4*>(keys + (size_t)kid * HW + p0);
    const unsigned char l[4] = {lv.x, lv.y, lv.z, lv.w}, k[4] = {kv.x, kv.y, kv.z, kv.w};
    float v[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = p0 + j;
      const int yy = p / W, xx = p - yy * W;
      float xr, yr;
      rot_sample(cf, xx, yy, xr, yr);
      float rot = 0.f;
      if (rot_inside(xr, yr, H, W)) rot = (float)L[rot_at(xr, yr, W)];
      v[3 * j] = (float)l[j] / div;
      v[3 * j + 1] = rot / div;
      v[3 * j + 2] = (float)k[j] / div;
    }
    float4* d = reinterpret_cast<float4*>(seg + 12 * tid);
    d[0] = make_float4(v[0], v[1], v[2], v[3]);
    d[1] = make_float4(v[4], v[5], v[6], v[7]);
    d[2] = make_float4(v[8], v[9], v[10], v[11]);
  }
  __syncthreads();
  const int nf = 3 * min(MB_PIX, HW - s0);  // floats of this segment (a multiple of 12)
  float4* o = reinterpret_cast<float4*>(x + (size_t)b * 3 * HW + 3 * (size_t)s0);
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int f = 4 * (tid + 256 * s);
    if (f < nf) o[tid + 256 * s] = *reinterpret_cast<const float4*>(seg + f);
  }
}

// An embedding pass (ImagesSrc) as X: x[b, 3 p + ch] = (float)image((1, 0, 2)[ch] B + b)[p] / div
// (any D, any alignment)
__global__ void images_x_kernel(ImagesSrc src, int B, int D, float* __restrict__ x) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= D) return;
  float* o = x + (size_t)b * 3 * D + 3 * (size_t)p;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const unsigned char* img = src.image((ch == 0 ? 1 : (ch == 1 ? 0 : 2)) * B + b, D);
    o[ch] = img ? (float)img[p] / src.div : 0.f;
  }
}

// the bits kernel (with or without the weight-gradient words), then the gated grey pass (256
// workgroups striding: for a 0/1 batch every one returns at once, and fewer cost less)
template <class Src>
hipError_t launch_bits(const Src& src, int B, int D, const BitsDst& d, int* dyn, int* dyn_next, bool no_xbw,
                       hipStream_t st) {
  const dim3 grid((d.kts_f + 1) / 2, B / 64);
  if (no_xbw)
    hipLaunchKernelGGL((deint_bits_kernel<Src, true>), grid, dim3(BITS_NT), 0, st, src, B, D, d.kts_f, d.kts_w, d.xbf,
                       d.xbw, d.xbits, d.ldbits, dyn, dyn_next);
  else
    hipLaunchKernelGGL((deint_bits_kernel<Src, false>), grid, dim3(BITS_NT), 0, st, src, B, D, d.kts_f, d.kts_w, d.xbf,
                       d.xbw, d.xbits, d.ldbits, dyn, dyn_next);
  hipLaunchKernelGGL(deint_grey_kernel<Src>, dim3(256), dim3(256), 0, st, src, d.xs, d.xp.p, d.xp.stride, d.xp.n,
                     d.f32dyn_mask, dyn, B, D, d.ldx);
  return hipGetLastError();
}

// what every route asks of the destination for a [B][D] batch
bool dst_serves(const BitsDst& d, int B, int D, const int* dyn, bool no_xbw) {
  return (d.ldx % 8) == 0 && dyn && d.xp.p && d.xbf && d.xbits && (no_xbw || d.xbw) && d.kts_f == bitmat_kts(D + 1) &&
         d.kts_w == bitmat_kts(3 * B) && d.ldbits >= D / 8;
}

}  // namespace

hipError_t launch_deinterleave(const float* x, float* xs, const Planes& xp, int* dyn, int* dyn_next,
                               int B, int D, int ldx, int f32mask, int f32dyn_mask, hipStream_t st,
                               unsigned char* xbits, int ldbits) {
  // 8 pixels per thread (4 and 16 measured slower, profiles/r4/r4y_deinterleave.txt; an LDS-staged
  // form with lane-contiguous loads too, r4an_deinterleave_lds_rejected.txt); 4 when D % 8 != 0
  const bool al = (reinterpret_cast<uintptr_t>(x) % 16) == 0;
  if ((D % 8) == 0 && al && (ldx % 8) == 0) {
    dim3 g(nblocks(D / 8, 256), B);
    hipLaunchKernelGGL(deinterleave_vecn_kernel<2>, g, dim3(256), 0, st,
                       reinterpret_cast<const float4*>(x), xs, xp.p, dyn, B, D, ldx, f32mask, dyn_next,
                       xbits, ldbits);
  } else if ((D % 4) == 0 && (reinterpret_cast<uintptr_t>(x) % 16) == 0 && (ldx % 4) == 0) {
    dim3 g(nblocks(D / 4, 256), B);
    hipLaunchKernelGGL(deinterleave_vec_kernel, g, dim3(256), 0, st,
                       reinterpret_cast<const float4*>(x), xs, xp.p, dyn, B, D, ldx, f32mask, dyn_next);
  } else {
    dim3 g(nblocks(D, 256), B);
    hipLaunchKernelGGL(deinterleave_scalar_kernel, g, dim3(256), 0, st, x, xs, xp.p, dyn, B, D, ldx,
                       f32mask, dyn_next);
  }
  f32dyn_mask &= ~f32mask;
  if (dyn && xp.p && (xp.n == 3 || f32dyn_mask))
    hipLaunchKernelGGL(residual_planes_kernel, dim3(2048), dim3(256), 0, st, x, xs, xp.p, xp.stride,
                       xp.n, f32dyn_mask, dyn, B, D, ldx);
  return hipGetLastError();
}

hipError_t launch_deint_bits(const XBatch& s, const BitsDst& d, int* dyn, int* dyn_next, bool no_xbw,
                             hipStream_t st) {
  if ((s.D % 8) || (s.B % 64) || (reinterpret_cast<uintptr_t>(s.x) % 16) || (d.ldx % 8) || !dyn || !d.xp.p ||
      d.kts_f != bitmat_kts(s.D + 1) || d.kts_w != bitmat_kts(3 * s.B))
    return hipErrorInvalidValue;
  return launch_bits(XSrc{reinterpret_cast<const float4*>(s.x)}, s.B, s.D, d, dyn, dyn_next, no_xbw, st);
}

hipError_t launch_bits_transpose(const unsigned* xbf, int kts_f, unsigned* xbw, int kts_w, int B, hipStream_t st) {
  if (B % 64 || kts_f <= 0 || kts_w != bitmat_kts(3 * B)) return hipErrorInvalidValue;
  const int nrow64 = 3 * B / 64;
  const long long tiles = (long long)nrow64 * kts_f;
  hipLaunchKernelGGL(bits_transpose_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, st, xbf, kts_f, xbw,
                     kts_w, nrow64);
  return hipGetLastError();
}

bool pairs_bits_fits(const unsigned char* locks, const unsigned char* keys, const float* coef, int B, int D) {
  return (D % 8) == 0 && (B % 64) == 0 && (reinterpret_cast<uintptr_t>(locks) % 8) == 0 &&
         (reinterpret_cast<uintptr_t>(keys) % 8) == 0 && (reinterpret_cast<uintptr_t>(coef) % 16) == 0;
}

hipError_t launch_pairs_bits(const PairsBatch& s, const BitsDst& d, int* dyn, int* dyn_next, bool no_xbw,
                             hipStream_t st) {
  const long long HW = (long long)s.H * s.W;
  if (s.H <= 0 || s.W <= 0 || HW > (1 << 30) || s.B <= 0) return hipErrorInvalidValue;
  const int D = (int)HW;
  if (!pairs_bits_fits(s.locks, s.keys, s.coef, s.B, D) || !s.locks || !s.keys || !s.idx || !s.coef ||
      !dst_serves(d, s.B, D, dyn, no_xbw))
    return hipErrorInvalidValue;
  const PairsSrc src{s.locks, s.keys, s.H, s.W, s.idx, s.kidx ? s.kidx : s.idx /* the own pair */,
                     reinterpret_cast<const float4*>(s.coef), s.div};
  return launch_bits(src, s.B, D, d, dyn, dyn_next, no_xbw, st);
}

bool images_bits_fits(const unsigned char* table, int B, int D) {
  return (D % 8) == 0 && (B % 64) == 0 && (reinterpret_cast<uintptr_t>(table) % 8) == 0;
}

hipError_t launch_images_bits(const ImagesBatch& s, const BitsDst& d, int* dyn, int* dyn_next, bool no_xbw,
                              hipStream_t st) {
  const long long HW = (long long)s.H * s.W;
  if (s.H <= 0 || s.W <= 0 || HW > (1 << 30) || s.B <= 0 || s.B > (1 << 28)) return hipErrorInvalidValue;
  const int D = (int)HW;
  if (!s.table || !images_bits_fits(s.table, s.B, D) || s.nvalid < 1 || s.nvalid > 3 * s.B ||
      !dst_serves(d, s.B, D, dyn, no_xbw))
    return hipErrorInvalidValue;
  return launch_bits(ImagesSrc{s.table, s.idx, s.nvalid, s.div}, s.B, D, d, dyn, dyn_next, no_xbw, st);
}

hipError_t launch_images_x(const ImagesBatch& s, float* x, hipStream_t st) {
  const long long HW = (long long)s.H * s.W;
  if (!s.table || !x || s.H <= 0 || s.W <= 0 || HW > (1 << 30) || s.B <= 0 || s.B > 65535 || s.nvalid < 1 ||
      s.nvalid > 3 * s.B)
    return hipErrorInvalidValue;
  const int D = (int)HW;
  hipLaunchKernelGGL(images_x_kernel, dim3((D + 255) / 256, s.B), dim3(256), 0, st,
                     ImagesSrc{s.table, s.idx, s.nvalid, s.div}, s.B, D, x);
  return hipGetLastError();
}

hipError_t launch_make_batch(const unsigned char* locks, const unsigned char* keys, int H, int W,
                             const int* idx, const int* kidx, const float* coef, int B, float div, float* x,
                             hipStream_t st) {
  if (!kidx) kidx = idx;  // the own pair
  const size_t hw = (size_t)H * W;
  if (hw % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    dim3 g(nblocks(hw, MB_PIX), B);
    hipLaunchKernelGGL(make_batch4_kernel, g, dim3(256), 0, st, locks, keys, H, W, idx, kidx,
                       reinterpret_cast<const float4*>(coef), div, x);
    return hipGetLastError();
  }
  dim3 g(nblocks(hw, 256), B);
  hipLaunchKernelGGL(make_batch_kernel, g, dim3(256), 0, st, locks, keys, H, W, idx, kidx,
                     reinterpret_cast<const float4*>(coef), div, x);
  return hipGetLastError();
}

}  // namespace mvae
