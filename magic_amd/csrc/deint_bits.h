// The de-interleave to bits, one task (64 batch rows x 64 PB pixels): the body of
// deint_bits_kernel (mvae_kernels.hip). Writes the layer-0 pixel operand of a 0/1 batch as the
// eight-phase kernel's BitMats (mvae_internal.h): xbf = A of the forward (rows [rot | lock | key] x
// pixels, the ones column at k = D), xbw = A of the weight gradient (pixels x rows, the ones row at
// pixel D), plus the BCE target (the lock block) as bits per row (GemmEpi::xbits) -- 1.1 bits
// written per pixel triple instead of the 48 of the bf16 plane. Each thread reads 4 x 96
// contiguous bytes (8 pixels of one row, as the plane kernel), writes one byte per block into LDS
// ([block][octet][row]: a row-contiguous 8 x 8 bit block is one u64), then assembles the forward
// words four at a time (one 16-B store) and the weight-gradient words one at a time.
// Raises the not-binary word (dyn[2]) when a pixel is neither 0 nor 1. Padding outside the
// written blocks (rows past 3B, pixel quarters past D) is zero from the buffers' creation.
#pragma once
#include "mvae_internal.h"

namespace mvae {

// bits el = 0..7 of b -> positions 0..3 (even el) and 16..19 (odd el): a BitMat word's layout
__device__ __forceinline__ unsigned bits_spread(unsigned b) {
  unsigned e = b & 0x55u, o = (b >> 1) & 0x55u;
  e = (e | (e >> 1)) & 0x33u; e = (e | (e >> 2)) & 0x0Fu;
  o = (o | (o >> 1)) & 0x33u; o = (o | (o >> 2)) & 0x0Fu;
  return e | (o << 16);
}

// LDS of one task: [3 blocks][8 PB octets][OS bytes per octet row] (OS 72: the 16 octets of a
// write land on 16 banks)
template <int PB, int OS>
using DeintLds = unsigned char[3][8 * PB][OS];

// task (bx, by): pixels [64 PB bx, +64 PB), batch rows [64 by, +64), NT threads. Its loads
// (deint_load: 4 x 96 contiguous bytes of NR rows per thread into v) and the rest (deint_finish;
// `written` runs once v is consumed -- this thread's LDS bytes written, v free for the next task's
// loads -- and `synced` once the workgroup has synchronised after everyone's LDS writes)
template <int PB, int NT>
struct DeintShape {
  static constexpr int NO = 8 * PB;    // octets per row
  static constexpr int RPP = NT / NO;  // rows per pass
  static constexpr int NR = 64 / RPP;  // row passes per thread
  static_assert(NT % NO == 0 && 64 % RPP == 0, "whole rows per pass");
};
template <int PB, int NT>
__device__ __forceinline__ void deint_load(const float4* __restrict__ x, int D, int bx, int by,
                                           float4 (&v)[DeintShape<PB, NT>::NR][6]) {
  using S = DeintShape<PB, NT>;
  const int tid = threadIdx.x;
  // (unconditional loads -- octets past D read the row's last one, unused -- so the values need no
  // merge with a not-loaded path, whose register copies would wait for every load at once)
  const int b0 = by * 64, pix = min(bx * 64 * PB + 8 * (tid % S::NO), D - 8);
#pragma unroll
  for (int i = 0; i < S::NR; ++i) {
    const float4* src = x + ((size_t)(b0 + tid / S::NO + S::RPP * i) * 3 * D + 3 * (size_t)pix) / 4;
#pragma unroll
    for (int k = 0; k < 6; ++k) v[i][k] = src[k];
  }
}
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

// The grey pass's work on pixel octet q of batch row b (v: its 24 values as X stores them): bf16
// plane 0 and the fp32 rows of the blocks in f32mask (deint_put), planes 1-2 of the exact split
// when np == 3; returns whether a pixel is inexact in bf16. Shared by deint_grey_kernel (v read
// from X) and pairs_grey_kernel (v rebuilt from the uint8 tables).
__device__ __forceinline__ bool deint_grey_octet(const float4 (&v)[6], float* __restrict__ xs,
                                                 unsigned short* __restrict__ xp, long long ps, int np,
                                                 int f32mask, int B, int b, int q, int ldx) {
  const bool nz = deint_put<2>(v, xs, xp, B, b, (size_t)8 * q, ldx, f32mask);
  if (np == 3) {  // the exact split's residual planes of the 24 values
    const float e[24] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                         v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w,
                         v[4].x, v[4].y, v[4].z, v[4].w, v[5].x, v[5].y, v[5].z, v[5].w};
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
  return nz;
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

// An octet's 24 values as X would store them, from the raw bytes of its 8 pixels in the three
// channels (eight bytes per uint2, pixel j in byte j): per pixel (lock, rotated lock, key) / div,
// the producer's (float)byte / div. Shared by the kernels that read the uint8 tables
// (pairs_bits.hip, images_bits.hip).
__device__ __forceinline__ void deint_byte_values(const uint2& l, const uint2& r, const uint2& k, float div,
                                                  float (&e)[24]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int sh = 8 * (j & 3);
    e[3 * j] = (float)(((j < 4 ? l.x : l.y) >> sh) & 0xFFu) / div;
    e[3 * j + 1] = (float)(((j < 4 ? r.x : r.y) >> sh) & 0xFFu) / div;
    e[3 * j + 2] = (float)(((j < 4 ? k.x : k.y) >> sh) & 0xFFu) / div;
  }
}

// the task's BitMat words from its LDS bytes, by threads t0, t0 + nt, ...: the forward words four
// at a time (lanes 2 q, 2 q + 1 of the fragment layout, words j = 0 / 1 each: rows 16 (2 j + h) +
// (lane & 15), k-octet 8 kk + 4 kh + (lane >> 4); one 16-B store), the
// weight-gradient words one at a time (pixel 64 kk + 16 (2 j + h) + (lane & 15), rows 32 kh +
// 8 (lane >> 4) + 0..7: bit (pixel & 7) of 8 row bytes of one octet)
template <int PB, int OS, bool NOW = false>
__device__ __forceinline__ void deint_words(int t0, int nt, int B, int D, int kts_f, int kts_w,
                                            unsigned* __restrict__ xbf, unsigned* __restrict__ xbw, int bx,
                                            int by, const DeintLds<PB, OS>& bt) {
  const int b0 = by * 64, p0 = bx * 64 * PB;
  for (int wq = t0; wq < 3 * PB * 32; wq += nt) {
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
  for (int wi = t0; wi < (NOW ? 0 : 3 * PB * 128); wi += nt) {  // (NOW: no xbw)
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

// One octet of one task row into the task's LDS bytes: its three block bytes from the 24 values e
// (an octet inside the image, `in`; then also the row's target byte into xbits) or the padding byte
// `pad` (the ones column at pixel D, zeros past it); returns whether a value is not 0 / 1. Where
// the 24 values come from is the caller's business: X (deint_finish) or the uint8 tables
// (pairs_bits.hip).
template <int PB, int OS>
__device__ __forceinline__ bool deint_octet_put(bool in, unsigned pad, const float (&e)[24],
                                                unsigned char* __restrict__ xbits_at, DeintLds<PB, OS>& bt, int o,
                                                int r) {
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
__device__ __forceinline__ unsigned deint_pad(int pix, int D) {
  return (pix <= D && D < pix + 8) ? 1u << (D - pix) : 0u;
}
// The rest of a task once every thread has put its octets (nb: this thread saw a value not 0 / 1):
// the not-binary word, the workgroup's synchronisation, the BitMat words
template <int PB, int NT, int OS, class FW, class FS, bool NOW = false>
__device__ __forceinline__ void deint_tail(bool nb, int B, int D, int kts_f, int kts_w, unsigned* __restrict__ xbf,
                                           unsigned* __restrict__ xbw, int* __restrict__ dyn, int bx, int by,
                                           const DeintLds<PB, OS>& bt, FW&& written, FS&& synced) {
  const int tid = threadIdx.x;
  written();
  if (dyn) {
    const bool anb = __ballot(nb) != 0;
    if ((tid & 63) == 0 && anb) atomicOr(dyn + 2, 1);
  }
  __syncthreads();
  synced();
  deint_words<PB, OS, NOW>(tid, NT, B, D, kts_f, kts_w, xbf, xbw, bx, by, bt);
}

template <int PB, int NT, int OS, class FW, class FS, bool NOW = false>
__device__ __forceinline__ void deint_finish(int B, int D, int kts_f, int kts_w, unsigned* __restrict__ xbf,
                                             unsigned* __restrict__ xbw, unsigned char* __restrict__ xbits,
                                             int ldbits, int* __restrict__ dyn, int bx, int by,
                                             const float4 (&v)[DeintShape<PB, NT>::NR][6], DeintLds<PB, OS>& bt,
                                             FW&& written, FS&& synced) {
  using S = DeintShape<PB, NT>;
  constexpr int NO = S::NO, RPP = S::RPP, NR = S::NR;
  const int tid = threadIdx.x;
  const int b0 = by * 64, p0 = bx * 64 * PB;
  const int o = tid % NO, pix = p0 + 8 * o;
  const bool in = pix + 8 <= D;
  bool nb = false;
  const unsigned pad = deint_pad(pix, D);
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int r = tid / NO + RPP * i;
    const float e[24] = {v[i][0].x, v[i][0].y, v[i][0].z, v[i][0].w, v[i][1].x, v[i][1].y, v[i][1].z, v[i][1].w,
                         v[i][2].x, v[i][2].y, v[i][2].z, v[i][2].w, v[i][3].x, v[i][3].y, v[i][3].z, v[i][3].w,
                         v[i][4].x, v[i][4].y, v[i][4].z, v[i][4].w, v[i][5].x, v[i][5].y, v[i][5].z, v[i][5].w};
    nb |= deint_octet_put<PB, OS>(in, pad, e, xbits + (size_t)(b0 + r) * ldbits + (pix >> 3), bt, o, r);
  }
  deint_tail<PB, NT, OS, FW, FS, NOW>(nb, B, D, kts_f, kts_w, xbf, xbw, dyn, bx, by, bt, written, synced);
}

// the whole task (the standalone kernel's workgroup)
template <int PB, int NT, int OS, bool NOW = false>
__device__ __forceinline__ void deint_bits_task(const float4* __restrict__ x, int B, int D, int kts_f, int kts_w,
                                                unsigned* __restrict__ xbf, unsigned* __restrict__ xbw,
                                                unsigned char* __restrict__ xbits, int ldbits,
                                                int* __restrict__ dyn, int bx, int by, DeintLds<PB, OS>& bt) {
  float4 v[DeintShape<PB, NT>::NR][6];
  deint_load<PB, NT>(x, D, bx, by, v);
  auto none = [] {};
  deint_finish<PB, NT, OS, decltype(none)&, decltype(none)&, NOW>(B, D, kts_f, kts_w, xbf, xbw, xbits, ldbits, dyn, bx,
                                                                  by, v, bt, none, none);
}

}  // namespace mvae
