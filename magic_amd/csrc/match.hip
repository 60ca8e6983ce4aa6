// All-pairs distance between two galleries of embeddings with a fused top-k (mvae_match, gfx950).
// score(i, j) is the context's distance between lock embedding i and key embedding j:
//   sqdiff  raw = sum_l (zl[i,l] - zk[j,l])^2, summed in that difference form (a reciprocal preset
//           returns 1 / raw: the norm expansion's cancellation error is unbounded relative to a
//           small raw),
//   cosine  raw = sum_l (zl[i,l] rl[l]) (zk[j,l] rk[l]), rl / rk the reciprocal column norms over the
//           gallery's rows (the axis-0 l2_normalize of 11a/vae.py:444-458 with the gallery as batch).
// match_kernel: a workgroup owns 64 lock rows and one split of the key rows, walks its split in
// tiles of 128 keys and L in tiles of MT_K through LDS (4 x 8 scores per thread as packed fp32
// pairs, each summed by one thread over l = 0 .. L - 1 in order: a score does not depend on the
// tiling or the split), then hands the 64 x 128 scores through LDS to the top-k pass: wave w keeps
// the running lists of rows 16 w .. 16 w + 15 in registers, lane r holding entry r. A row's
// candidates, 64 at a time, are tested against its k-th entry by one ballot and the few that pass
// are inserted one by one.
// The order is total -- (score, smaller j), NaN last for either direction -- so the k best of a row
// are one list whatever the split; merge_kernel pushes the per-split lists through the same
// insertion. No atomics; with dist_out null no N x M buffer exists.
// Sharded galleries (mvae_match_ex): the key index a list holds is key_base + j, the order breaks
// ties on that global index, and merge_kernel can start from the caller's list of earlier shards --
// the k best over a union of disjoint key ranges are one list whatever the shards (a carried call
// also seeds every workgroup's threshold with the k-th entry so far). The CNT
// instantiations also count, per lock row, the keys strictly before a caller's threshold entry
// (one more ballot and popcount per row and 64 candidates; lane r of a wave holds row r's
// threshold and count, as the lists do); splits write their counts to the workspace and the merge
// launch adds them in split order. pair_scores_kernel gives the row-aligned score with the very
// operations of match_kernel's sums.
#include "mvae_internal.h"

namespace mvae {
namespace {

constexpr int MT = 64;        // lock rows per workgroup (and the unit a split of M is rounded to)
constexpr int MTM = 128;      // key rows per tile
constexpr int MTM_LD = MTM + 4;
constexpr int MT_K = 32;      // l per LDS tile
constexpr int MT_LD = MT + 4; // LDS row stride of the [l][row] operand tiles (16-B aligned rows)
constexpr float L2_EPS = 1e-12f;  // tf.nn.l2_normalize default

// The order as one integer: a better entry has the larger key. Scores ascend through the usual
// sign-magnitude map (-0 counted as +0, so +-0 tie by index), complemented when smaller is better;
// NaN maps below every number for either direction; the smaller j wins a tie. An empty list entry
// (NaN, j = ~0) is key 0, below every real one.
__device__ __forceinline__ unsigned long long match_key(float v, unsigned j, int order) {
  const unsigned u = __float_as_uint(v == 0.f ? 0.f : v);
  const unsigned a = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  const unsigned o = (v != v) ? 0u : (order > 0 ? a : ~a);
  return ((unsigned long long)o << 32) | (unsigned)~j;
}

// One wave's list of a row (lane r: entry r, best first) takes the wave's 64 candidates (lane:
// score s, key index jc, `valid`). Lanes >= k hold entries pushed out of the first k: unused.
__device__ __forceinline__ void topk_push(float& lv, unsigned& lj, float s, unsigned jc, bool valid, int k,
                                          int order) {
  const int lane = threadIdx.x & 63;
  const unsigned long long ck = valid ? match_key(s, jc, order) : 0ull;
  unsigned long long lk = match_key(lv, lj, order);
  unsigned long long thr = match_key(__shfl(lv, k - 1), __shfl(lj, k - 1), order);
  unsigned long long mask = __ballot(ck > thr);
  while (mask) {
    const int src = __ffsll((long long)mask) - 1;
    const float xs = __shfl(s, src);
    const unsigned xj = __shfl(jc, src);
    const unsigned long long xk = match_key(xs, xj, order);
    const int pos = __popcll(__ballot(lk > xk));  // entries better than x: lanes 0 .. pos - 1
    const float pv = __shfl_up(lv, 1);
    const unsigned pj = __shfl_up(lj, 1);
    if (lane > pos) { lv = pv; lj = pj; }
    else if (lane == pos) { lv = xs; lj = xj; }
    lk = match_key(lv, lj, order);
    thr = match_key(__shfl(lv, k - 1), __shfl(lj, k - 1), order);
    mask &= mask - 1;
    mask &= __ballot(ck > thr);
  }
}

// reciprocal column norms of a gallery, in a fixed order: part[chunk][l] = sum of z^2 over the
// chunk's 256 rows (four row quarters per column summed in turn, then the quarters in order) ...
__global__ __launch_bounds__(256) void colnorm_part_kernel(const float* __restrict__ z, long long n, int L,
                                                           double* __restrict__ part) {
  __shared__ double q[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.y * 256 + 64 * g;
  double s = 0.0;
  if (c < L)
    for (long long r = r0; r < r0 + 64 && r < n; ++r) {
      const double v = (double)z[r * L + c];
      s += v * v;
    }
  q[g][threadIdx.x & 63] = s;
  __syncthreads();
  const int t = threadIdx.x;
  if (g == 0 && c < L) part[(size_t)blockIdx.y * L + c] = ((q[0][t] + q[1][t]) + q[2][t]) + q[3][t];
}
// ... and r[l] = 1 / sqrt(max(sum over the chunks in order, 1e-12)), the sum rounded to fp32 first
__global__ void colnorm_final_kernel(const double* __restrict__ part, int nchunk, int L, float* __restrict__ r) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= L) return;
  double s = 0.0;
  for (int i = 0; i < nchunk; ++i) s += part[(size_t)i * L + c];
  r[c] = (float)(1.0 / sqrt((double)fmaxf((float)s, L2_EPS)));
}

struct MatchArgs {
  const float* zl; const float* zk;
  long long N, M;
  int L, k, order, metric, recip;
  const float* rl; const float* rk;  // cosine: the reciprocal column norms
  long long split_len;               // key rows per split (a multiple of MT)
  int splits;
  float* dist;                       // [N][dist_ld] or null
  float* out_val; int* out_idx;      // [N][splits][k]
  long long dist_ld;                 // row stride of dist (>= M)
  unsigned key_base;                 // global index of key row 0 (key_base + M < 2^31)
  const float* thr_val; const int* thr_idx;  // CNT: [N] threshold entries (global indices)
  int* out_cnt;                      // CNT: [N][splits] keys of the split strictly before the threshold
  const float* seed_val; const int* seed_idx;  // carry: the list of earlier calls [N][k], else null
};

typedef float f2 __attribute__((ext_vector_type(2)));

template <bool COS, bool CNT>
__global__ __launch_bounds__(256) void match_kernel(MatchArgs a) {
  // the operand tiles [l][row] during the k-loop, then the tile's scores [lock row][key]
  constexpr int A_WORDS = MT_K * MT_LD, B_WORDS = MT_K * MTM_LD, S_WORDS = MT * (MTM + 1);
  __shared__ __attribute__((aligned(16))) float smem[A_WORDS + B_WORDS > S_WORDS ? A_WORDS + B_WORDS : S_WORDS];
  float (*As)[MT_LD] = reinterpret_cast<float (*)[MT_LD]>(smem);
  float (*Bs)[MTM_LD] = reinterpret_cast<float (*)[MTM_LD]>(smem + A_WORDS);
  float (*Sc)[MTM + 1] = reinterpret_cast<float (*)[MTM + 1]>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = tid >> 4, tx = tid & 15;  // lock rows 4 ty + i; keys 4 tx + j and 64 + 4 tx + j
  const long long n0 = (long long)blockIdx.x * MT;
  const long long mbeg = (long long)blockIdx.y * a.split_len;
  const long long mend = mbeg + a.split_len < a.M ? mbeg + a.split_len : a.M;
  const int L = a.L;
  float lv[16];
  unsigned lj[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { lv[r] = __uint_as_float(0x7FC00000u); lj[r] = ~0u; }
  // carry: a key scoring worse than the k-th entry of the list so far cannot be among the k best of
  // the union, so the lists start as k copies of that score with the empty index: the test against
  // the k-th entry then drops such keys from the first tile on, and the copies (index -1) never
  // enter the merge. A list so far with fewer than k entries seeds nothing.
  if (a.seed_val) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = n0 + 16 * wave + r;
      if (row < a.N && a.seed_idx[(size_t)row * a.k + a.k - 1] != -1) lv[r] = a.seed_val[(size_t)row * a.k + a.k - 1];
    }
  }
  // CNT: lane r < 16 holds the threshold key and the running count of row 16 wave + r. The lists
  // and the threshold index are local to this call's keys inside the kernel (the order on j is the
  // order on key_base + j); a threshold index before / past the call's range is clamped to 0 /
  // 2^31 - 1: no / every key of the call precedes it on a tie.
  unsigned long long tkey = ~0ull;
  int cnt = 0;
  if (CNT) {
    const long long row = n0 + 16 * wave + (lane & 15);
    if (row < a.N) {
      const long long t = (long long)a.thr_idx[row] - (long long)a.key_base;
      tkey = match_key(a.thr_val[row], (unsigned)(t < 0 ? 0 : t > 0x7FFFFFFFll ? 0x7FFFFFFFll : t), a.order);
    }
  }

  for (long long m0 = mbeg; m0 < mend; m0 += MTM) {
    f2 acc[4][4];  // [lock row i][key pair: 4 tx + {0,1}, {2,3}, 64 + 4 tx + {0,1}, {2,3}]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f2){0.f, 0.f};
    for (int l0 = 0; l0 < L; l0 += MT_K) {
      const int kmax = L - l0 < MT_K ? L - l0 : MT_K;
      __syncthreads();  // the last tile's readers (of the operands, of the scores) are done
      // 64 lock rows and 128 keys x MT_K columns, lanes along l. Every load is issued before the
      // first LDS write, at an address clamped into its gallery (no branch around a load); what
      // lies past the gallery or past L is then written as 0.
      const int c = tid % MT_K, l = l0 + c, lc = l < L ? l : L - 1;
      const float sl = COS ? a.rl[lc] : 1.f, sk = COS ? a.rk[lc] : 1.f;
      float va[(MT * MT_K) / 256], vb[(MTM * MT_K) / 256];
#pragma unroll
      for (int i = 0; i < (MT * MT_K) / 256; ++i) {
        const long long row = n0 + tid / MT_K + (256 / MT_K) * i;
        va[i] = a.zl[(row < a.N ? row : a.N - 1) * L + lc];
      }
#pragma unroll
      for (int i = 0; i < (MTM * MT_K) / 256; ++i) {
        const long long row = m0 + tid / MT_K + (256 / MT_K) * i;
        vb[i] = a.zk[(row < mend ? row : mend - 1) * L + lc];
      }
#pragma unroll
      for (int i = 0; i < (MT * MT_K) / 256; ++i) {
        const int r = tid / MT_K + (256 / MT_K) * i;
        const float v = (l < L && n0 + r < a.N) ? va[i] : 0.f;
        As[c][r] = COS ? v * sl : v;
      }
#pragma unroll
      for (int i = 0; i < (MTM * MT_K) / 256; ++i) {
        const int r = tid / MT_K + (256 / MT_K) * i;
        const float v = (l < L && m0 + r < mend) ? vb[i] : 0.f;
        Bs[c][r] = COS ? v * sk : v;
      }
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < kmax; ++kk) {
        const float4 av = *reinterpret_cast<const float4*>(&As[kk][4 * ty]);
        const float4 b0 = *reinterpret_cast<const float4*>(&Bs[kk][4 * tx]);
        const float4 b1 = *reinterpret_cast<const float4*>(&Bs[kk][64 + 4 * tx]);
        const float ar[4] = {av.x, av.y, av.z, av.w};
        const f2 bp[4] = {(f2){b0.x, b0.y}, (f2){b0.z, b0.w}, (f2){b1.x, b1.y}, (f2){b1.z, b1.w}};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f2 ai = (f2){ar[i], ar[i]};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (COS) {
              acc[i][j] = __builtin_elementwise_fma(ai, bp[j], acc[i][j]);
            } else {
              const f2 d = ai - bp[j];
              acc[i][j] = __builtin_elementwise_fma(d, d, acc[i][j]);
            }
          }
        }
      }
    }
    __syncthreads();  // every wave is done with the operand tiles the scores overwrite
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = (j >> 1) * 64 + 4 * tx + 2 * (j & 1);
        Sc[4 * ty + i][col] = a.recip ? 1.f / acc[i][j].x : acc[i][j].x;
        Sc[4 * ty + i][col + 1] = a.recip ? 1.f / acc[i][j].y : acc[i][j].y;
      }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long jc = m0 + 64 * h + lane;
      const bool jin = jc < mend;
      if (m0 + 64 * h >= mend) break;  // (uniform: the split ends in this tile's first half)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 16 * wave + r;
        const float s = Sc[row][64 * h + lane];
        const bool valid = jin && n0 + row < a.N;
        if (valid && a.dist) a.dist[(n0 + row) * a.dist_ld + jc] = s;
        if (CNT) {
          const unsigned long long tk = __shfl(tkey, r);
          const int c = __popcll(__ballot(valid && match_key(s, (unsigned)jc, a.order) > tk));
          if (lane == r) cnt += c;
        }
        topk_push(lv[r], lj[r], s, (unsigned)jc, valid, a.k, a.order);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long row = n0 + 16 * wave + r;
    if (row < a.N && lane < a.k) {
      const size_t o = ((size_t)row * a.splits + blockIdx.y) * a.k + lane;
      a.out_val[o] = lv[r];
      a.out_idx[o] = lj[r] == ~0u ? -1 : (int)(a.key_base + lj[r]);  // (the global index leaves here)
    }
  }
  if (CNT) {
    const long long row = n0 + 16 * wave + lane;
    if (lane < 16 && row < a.N) a.out_cnt[(size_t)row * a.splits + blockIdx.y] = cnt;
  }
}

// one wave per lock row: the caller's list of earlier calls first (carry: [N][k]), then the row's
// splits * k entries, 64 at a time in split order, through the same insertion (empty entries,
// j = -1, never enter). cnt [N][splits]: ahead[row] = (add ? ahead[row] : 0) + the counts in split order.
__global__ __launch_bounds__(256) void merge_kernel(const float* __restrict__ val, const int* __restrict__ idx,
                                                    long long N, int splits, int k, int order, int carry,
                                                    const int* __restrict__ cnt, int add, float* top_val,
                                                    int* top_idx, int* ahead) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  float lv = __uint_as_float(0x7FC00000u);
  unsigned lj = ~0u;
  if (carry) {
    const bool in = lane < k;
    const float s = in ? top_val[(size_t)row * k + lane] : 0.f;
    const unsigned j = in ? (unsigned)top_idx[(size_t)row * k + lane] : ~0u;
    topk_push(lv, lj, s, j, in && j != ~0u, k, order);
  }
  const long long n = (long long)splits * k;
  const float* v = val + (size_t)row * n;
  const int* ix = idx + (size_t)row * n;
  for (long long c0 = 0; c0 < n; c0 += 64) {
    const bool in = c0 + lane < n;
    const float s = in ? v[c0 + lane] : 0.f;
    const unsigned j = in ? (unsigned)ix[c0 + lane] : ~0u;
    topk_push(lv, lj, s, j, in && j != ~0u, k, order);
  }
  if (lane < k) {
    top_val[(size_t)row * k + lane] = lv;
    top_idx[(size_t)row * k + lane] = (int)lj;
  }
  if (cnt && lane == 0) {
    int c = add ? ahead[row] : 0;
    for (int i = 0; i < splits; ++i) c += cnt[(size_t)row * splits + i];
    ahead[row] = c;
  }
}

// colsq[l] = (accumulate ? colsq[l] : 0) + the chunk sums in order: colnorm_final_kernel's sum, kept
__global__ void colsq_sum_kernel(const double* __restrict__ part, int nchunk, int L, int accumulate,
                                 double* __restrict__ colsq) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= L) return;
  double s = accumulate ? colsq[c] : 0.0;
  for (int i = 0; i < nchunk; ++i) s += part[(size_t)i * L + c];
  colsq[c] = s;
}
// ... and its last line
__global__ void rnorm_kernel(const double* __restrict__ colsq, int L, float* __restrict__ r) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= L) return;
  r[c] = (float)(1.0 / sqrt((double)fmaxf((float)colsq[c], L2_EPS)));
}

// out[i] = score(zl[i], zk[i]): one thread per row, l = 0 .. L - 1 in order, with match_kernel's
// operations -- cosine: the rounded products v * r, then one fma per l; sqdiff: d = a - b, then
// fma(d, d, acc); reciprocal: 1.f / acc.
template <bool COS>
__global__ __launch_bounds__(64) void pair_scores_kernel(const float* __restrict__ zl, const float* __restrict__ zk,
                                                         long long n, int L, int recip,
                                                         const float* __restrict__ rl, const float* __restrict__ rk,
                                                         float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float* a = zl + (size_t)i * L;
  const float* b = zk + (size_t)i * L;
  float acc = 0.f;
  for (int l = 0; l < L; ++l) {
    if (COS) {
      const float x = a[l] * rl[l], y = b[l] * rk[l];
      acc = __builtin_fmaf(x, y, acc);
    } else {
      const float d = a[l] - b[l];
      acc = __builtin_fmaf(d, d, acc);
    }
  }
  out[i] = recip ? 1.f / acc : acc;
}

}  // namespace

// Key rows per split and the number of splits: enough workgroups for four per CU where M allows,
// no split shorter than four key tiles, a whole number of tiles per split.
void match_plan(long long N, long long M, long long* split_len, int* splits) {
  const long long ntn = (N + MT - 1) / MT;
  long long s = (1024 + ntn - 1) / ntn;
  const long long smax = (M + 4 * MT - 1) / (4 * MT);
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  long long len = (M + s - 1) / s;
  len = (len + MT - 1) / MT * MT;
  *split_len = len;
  *splits = (int)((M + len - 1) / len);
}

int match_colnorm_chunks(long long n) { return (int)((n + 255) / 256); }

hipError_t launch_colnorm(const float* z, long long n, int L, double* part, float* r, hipStream_t st) {
  const int nchunk = match_colnorm_chunks(n);
  hipLaunchKernelGGL(colnorm_part_kernel, dim3((L + 63) / 64, nchunk), dim3(256), 0, st, z, n, L, part);
  hipLaunchKernelGGL(colnorm_final_kernel, dim3((L + 255) / 256), dim3(256), 0, st, part, nchunk, L, r);
  return hipGetLastError();
}

hipError_t launch_colsq(const float* z, long long n, int L, double* part, double* colsq, int accumulate,
                        hipStream_t st) {
  const int nchunk = match_colnorm_chunks(n);
  hipLaunchKernelGGL(colnorm_part_kernel, dim3((L + 63) / 64, nchunk), dim3(256), 0, st, z, n, L, part);
  hipLaunchKernelGGL(colsq_sum_kernel, dim3((L + 255) / 256), dim3(256), 0, st, part, nchunk, L, accumulate, colsq);
  return hipGetLastError();
}

hipError_t launch_rnorm(const double* colsq, int L, float* r, hipStream_t st) {
  hipLaunchKernelGGL(rnorm_kernel, dim3((L + 255) / 256), dim3(256), 0, st, colsq, L, r);
  return hipGetLastError();
}

hipError_t launch_pair_scores(const float* zl, const float* zk, long long n, int L, int metric, int recip,
                              const float* rl, const float* rk, float* out, hipStream_t st) {
  if (!zl || !zk || !out || n < 1 || L < 1 || (metric == 0 && (!rl || !rk)) || (n + 63) / 64 > 0x7FFFFFFFll)
    return hipErrorInvalidValue;
  const dim3 g((unsigned)((n + 63) / 64));
  if (metric == 0)
    hipLaunchKernelGGL(pair_scores_kernel<true>, g, dim3(64), 0, st, zl, zk, n, L, recip, rl, rk, out);
  else
    hipLaunchKernelGGL(pair_scores_kernel<false>, g, dim3(64), 0, st, zl, zk, n, L, recip, rl, rk, out);
  return hipGetLastError();
}

hipError_t launch_match_merge(const float* vals, const int* idx, long long N, int parts, int k, int order,
                              int carry, const int* cnt, int add, float* top_val, int* top_idx, int* ahead,
                              hipStream_t st) {
  if (!vals || !idx || !top_val || !top_idx || N < 1 || parts < 1 || k < 1 || k > 64 || (cnt && !ahead) ||
      (N + 3) / 4 > 0x7FFFFFFFll)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, vals, idx, N, parts, k, order,
                     carry, cnt, add, top_val, top_idx, ahead);
  return hipGetLastError();
}

hipError_t launch_match_ex(const float* zl, long long N, const float* zk, long long M, int L, int k, int order,
                           int metric, int recip, const float* rl, const float* rk, long long split_len, int splits,
                           float* dist, long long dist_ld, long long key_base, int carry, const float* thr_val,
                           const int* thr_idx, int* ahead, float* ws_val, int* ws_idx, int* ws_cnt,
                           float* top_val, int* top_idx, hipStream_t st) {
  const bool merge = splits > 1 || carry, count = thr_val != nullptr;
  if (!zl || !zk || N < 1 || M < 1 || L < 1 || k < 1 || k > 64 || splits < 1 || split_len % MT ||
      split_len * splits < M || (merge && (!ws_val || !ws_idx)) || !top_val || !top_idx ||
      (metric == 0 && (!rl || !rk)) || (N + MT - 1) / MT > 0x7FFFFFFFll || splits > 65535 ||
      key_base < 0 || key_base + M > 0x7FFFFFFFll || dist_ld < M ||
      (count && (!thr_idx || !ahead || (merge && !ws_cnt))))
    return hipErrorInvalidValue;
  MatchArgs a{zl, zk, N, M, L, k, order, metric, recip, rl, rk, split_len, splits, dist,
              merge ? ws_val : top_val, merge ? ws_idx : top_idx, dist_ld, (unsigned)key_base,
              thr_val, thr_idx, merge ? ws_cnt : ahead, carry ? top_val : nullptr, carry ? top_idx : nullptr};
  const dim3 g((unsigned)((N + MT - 1) / MT), splits);
  if (metric == 0) {
    if (count) hipLaunchKernelGGL((match_kernel<true, true>), g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((match_kernel<true, false>), g, dim3(256), 0, st, a);
  } else {
    if (count) hipLaunchKernelGGL((match_kernel<false, true>), g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((match_kernel<false, false>), g, dim3(256), 0, st, a);
  }
  if (merge)
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, ws_val, ws_idx, N, splits, k,
                       order, carry, count ? ws_cnt : nullptr, carry, top_val, top_idx, ahead);
  return hipGetLastError();
}

hipError_t launch_match(const float* zl, long long N, const float* zk, long long M, int L, int k, int order,
                        int metric, int recip, const float* rl, const float* rk, long long split_len, int splits,
                        float* dist, float* ws_val, int* ws_idx, float* top_val, int* top_idx, hipStream_t st) {
  if (k > M) return hipErrorInvalidValue;
  return launch_match_ex(zl, N, zk, M, L, k, order, metric, recip, rl, rk, split_len, splits, dist, M, 0, 0, nullptr,
                         nullptr, nullptr, ws_val, ws_idx, nullptr, top_val, top_idx, st);
}

}  // namespace mvae
