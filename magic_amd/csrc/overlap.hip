// Maximum overlap of a lock and a key over rotations and integer shifts (mvae_overlap_pairs, gfx950):
// the quantity the model's latent distance is trained to predict, computed from the uint8 tables.
//   Lb, Kb      foreground = table byte >= 128
//   Kr_r        the key rotated by coef[r] = (cos, sin, x_off, y_off) with make_batch_kernel's
//               arithmetic (batch_input.hip rot_sample: output (x, y) samples ((c x - s y) + x_off,
//               (s x + c y) + y_off), unfused fp32, roundf, zero fill), bit for bit
//   ov(r, dy, dx) = sum_{y,x} Lb[y, x] Kr_r[y - dy, x - dx],  |dy| <= H - 1, |dx| <= W - 1
//   area = max ov;  pose = the lexicographically smallest (r, dy, dx) reaching it; (0, 0, 0) when
//   the area is 0.
// Everything is integer work on bit matrices, so the result is exact.
//
// overlap_kernel: one workgroup per (pair, chunk of angles). The lock is packed once to 32-bit
// row words in LDS, stored word-major ([word][row], zero rows before and after) so that the rows
// y .. y + 7 of one word are neighbours; the key is packed unrotated once, and for each angle its
// rotation is gathered from those bits (a lane per output pixel, a ballot per 64 pixels) into a
// second packed image (a zero word on each side of a row, zero rows after the last: the reads of the
// loop below need no test). The rotated images never reach HBM.
// A work item is (dx, eight consecutive dy). Its thread walks the key rows that can meet the lock
// under one of the eight dy; per key row and lock word it builds the shifted key word once (two
// LDS words, one funnel shift by the item's constant amount), loads ONE new lock word into an
// eight-deep register window (the window of row y' + 1 is the window of row y' moved by one), and
// does eight and + popcount-accumulate. That is 3 unconditional LDS words per 8 word products; the
// loop is bound by the 17 VALU operations.
// Pruning: with the bounding boxes of Lb (once) and Kr_r (per angle, from the ballots), only
// dy in [ly0 - ky1, ly1 - ky0], dx in [lx0 - kx1, lx1 - kx0], the rows and the words where both
// can be non-zero are visited. Everything skipped is exactly 0, and a pose of a positive maximum is
// never skipped, so area and pose are those of the definition.
// The candidate (area, pose) is one 64-bit key, area << 42 | ~(r, dy + H - 1, dx + W - 1): the
// largest key is the largest area at the smallest pose. Threads, waves and the workgroup reduce by
// integer max; each workgroup writes one partial to the caller's work buffer and overlap_finish
// takes the max of a pair's partials in chunk order. No atomics on HBM.
#include <algorithm>

#include "mvae_internal.h"

namespace mvae {
namespace {

constexpr int OV_MAX = 256;              // largest height / width
constexpr int OV_T = 256;                // threads per workgroup
constexpr int OV_WAVES = OV_T / 64;
constexpr int OV_WORDS = OV_MAX / 32;    // 32-bit words per packed row, at most
constexpr int DYT = 8;                   // dy per work item = depth of the lock-word window
constexpr int PADT = DYT;                // zero rows before row 0 of the word-major lock
constexpr int HP = OV_MAX + 3 * DYT;     // its rows per word: PADT + H + (2 DYT - 2) are touched
constexpr int KROWS = OV_MAX + DYT;      // rows of the rotated key: H + DYT - 1 are touched
constexpr int KWORDS = OV_WORDS + 2;     // ... and its words per row, at most: one zero word on each side
constexpr int POSE_BITS = 42;            // r: 24 bits, dy + H - 1 and dx + W - 1: 9 bits each
constexpr unsigned long long POSE_MASK = (1ull << POSE_BITS) - 1;
constexpr int OV_TARGET_WGS = 2048;      // workgroups a call aims for (256 CUs, several each)

struct Box {  // of the foreground: rows y0 .. y1 (y0 > y1: empty), column words OR-ed over the rows
  int y0, y1;
  unsigned col[OV_WORDS];
};

__device__ __forceinline__ void box_columns(const unsigned* col, int nw, int& x0, int& x1) {
  x0 = 0x7fffffff;
  x1 = -1;
  for (int j = 0; j < nw; ++j) {
    const unsigned c = col[j];
    if (c) {
      if (x1 < 0) x0 = 32 * j + __builtin_ctz(c);
      x1 = 32 * j + 31 - __builtin_clz(c);
    }
  }
}

__global__ __launch_bounds__(OV_T) void overlap_kernel(
    const unsigned char* __restrict__ locks, const unsigned char* __restrict__ keys, int H, int W,
    const int* __restrict__ lock_idx, const int* __restrict__ key_idx, long long pair0,
    const float4* __restrict__ coef, int n_rot, int nchunks, int per_chunk,
    unsigned long long* __restrict__ work) {
#pragma clang fp contract(off)  // the gather coordinates are unfused mul / add / sub (make_batch_kernel)
  __shared__ unsigned Lp[OV_WORDS * HP];      // lock, [word][PADT + row]
  __shared__ unsigned Ks[OV_MAX * OV_WORDS];  // key as stored, [row][word]
  __shared__ unsigned Kp[KROWS * KWORDS];     // key rotated by the current angle, [row][1 + word]: a
                                              // zero word before and after each row, zero rows from H on
  __shared__ Box lbox, kbox;
  __shared__ unsigned long long red[OV_WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long pair = pair0 + blockIdx.x / nchunks;
  const int chunk = blockIdx.x % nchunks;
  const int nseg = (W + 63) >> 6;  // 64-pixel segments per row
  const int WS = 2 * nseg;         // words per packed row
  const int KS = WS + 2;           // row stride of Kp
  const size_t HW = (size_t)H * W;
  // an empty shortlist entry (mvae_rerank: a negative key index) indexes no table: a zero partial,
  // before the first barrier and for the whole workgroup alike
  if (key_idx && key_idx[pair] < 0) {
    if (tid == 0) work[(size_t)pair * nchunks + chunk] = 0ull;
    return;
  }
  const unsigned char* L = locks + (size_t)(lock_idx ? lock_idx[pair] : pair) * HW;
  const unsigned char* K = keys + (size_t)(key_idx ? key_idx[pair] : pair) * HW;

  for (int i = tid; i < OV_WORDS * HP; i += OV_T) Lp[i] = 0u;
  for (int i = tid; i < KROWS * KWORDS; i += OV_T) Kp[i] = 0u;  // the angles write rows < H, words 1 .. WS
  if (tid < OV_WORDS) lbox.col[tid] = 0u;
  if (tid == 0) { lbox.y0 = 0x7fffffff; lbox.y1 = -1; }
  __syncthreads();
  // pack both images: a wave per (row, 64-pixel segment), a lane per pixel
  for (int task = wave; task < H * nseg; task += OV_WAVES) {
    const int y = task / nseg, sg = task - y * nseg;
    const int x = 64 * sg + lane;
    const bool in = x < W;
    const unsigned long long ml = __ballot(in && L[(size_t)y * W + x] >= 128);
    const unsigned long long mk = __ballot(in && K[(size_t)y * W + x] >= 128);
    if (lane == 0) {
      const unsigned lo = (unsigned)ml, hi = (unsigned)(ml >> 32);
      Lp[(2 * sg) * HP + PADT + y] = lo;
      Lp[(2 * sg + 1) * HP + PADT + y] = hi;
      Ks[y * WS + 2 * sg] = (unsigned)mk;
      Ks[y * WS + 2 * sg + 1] = (unsigned)(mk >> 32);
      if (ml) {
        atomicMin(&lbox.y0, y);
        atomicMax(&lbox.y1, y);
        if (lo) atomicOr(&lbox.col[2 * sg], lo);
        if (hi) atomicOr(&lbox.col[2 * sg + 1], hi);
      }
    }
  }
  __syncthreads();
  const int ly0 = lbox.y0, ly1 = lbox.y1;
  int lx0, lx1;
  box_columns(lbox.col, WS, lx0, lx1);

  unsigned long long best = 0ull;
  const int r_begin = chunk * per_chunk;
  const int r_end = ly0 > ly1 ? r_begin : min(n_rot, r_begin + per_chunk);  // an empty lock: area 0
  for (int r = r_begin; r < r_end; ++r) {
    __syncthreads();  // the previous angle's readers of Kp and kbox are done
    if (tid < OV_WORDS) kbox.col[tid] = 0u;
    if (tid == 0) { kbox.y0 = 0x7fffffff; kbox.y1 = -1; }
    __syncthreads();
    const float4 cf = coef[r];
    for (int task = wave; task < H * nseg; task += OV_WAVES) {
      const int y = task / nseg, sg = task - y * nseg;
      const int x = 64 * sg + lane;
      const float fx = (float)x, fy = (float)y;
      const float xin = (cf.x * fx - cf.y * fy) + cf.z;  // unfused: fp contract(off) above
      const float yin = (cf.y * fx + cf.x * fy) + cf.w;
      const float xr = roundf(xin), yr = roundf(yin);
      bool bit = false;
      if (x < W && xr >= 0.f && xr <= (float)(W - 1) && yr >= 0.f && yr <= (float)(H - 1)) {
        const int xi = (int)xr, yi = (int)yr;
        bit = (Ks[yi * WS + (xi >> 5)] >> (xi & 31)) & 1u;
      }
      const unsigned long long m = __ballot(bit);
      if (lane == 0) {
        const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
        Kp[y * KS + 1 + 2 * sg] = lo;
        Kp[y * KS + 2 + 2 * sg] = hi;
        if (m) {
          atomicMin(&kbox.y0, y);
          atomicMax(&kbox.y1, y);
          if (lo) atomicOr(&kbox.col[2 * sg], lo);
          if (hi) atomicOr(&kbox.col[2 * sg + 1], hi);
        }
      }
    }
    __syncthreads();
    const int ky0 = kbox.y0, ky1 = kbox.y1;
    if (ky0 > ky1) continue;  // the rotated key is empty (uniform: every thread reads the same box)
    int kx0, kx1;
    box_columns(kbox.col, WS, kx0, kx1);
    const int dymin = ly0 - ky1, dxmin = lx0 - kx1;
    const int ndy = (ly1 - ky0) - dymin + 1, ndx = (lx1 - kx0) - dxmin + 1;
    const int nitems = ndx * ((ndy + DYT - 1) / DYT);
    for (int it = tid; it < nitems; it += OV_T) {
      const int c = it / ndx;
      const int dx = dxmin + (it - c * ndx), d0 = dymin + c * DYT;
      // key rows that meet the lock under one of d0 .. d0 + DYT - 1, lock words the shifted key reaches
      const int ya = max(ky0, ly0 - d0 - (DYT - 1)), yb = min(ky1, ly1 - d0);
      const int ja = max(lx0, kx0 + dx) >> 5, jb = min(lx1, kx1 + dx) >> 5;
      if (ya > yb || ja > jb) continue;
      const int q = dx >> 5, s = dx & 31;  // dx = 32 q + s, 0 <= s < 32 (floor for negative dx)
      unsigned acc[DYT];
#pragma unroll
      for (int t = 0; t < DYT; ++t) acc[t] = 0u;
      for (int jw = ja; jw <= jb; ++jw) {
        // word jw of the key shifted by dx = bits of key words jw - q (high part) and jw - q - 1. Word jw
        // holds a column the shifted key's box reaches, so one of the two is a word of the key and the
        // other at worst its zero neighbour: Kp words jw - q and jw - q + 1 of the padded row. Rows
        // past yb (up to DYT - 1 of them, below H + DYT - 1) are either past the key's box, hence
        // zero, or meet lock rows past the lock's box: no test on the row either.
        const unsigned* kp = Kp + (jw - q);
        // lock word jw of row y' + d0 + t sits at lw[y' + t]: from PADT - (DYT - 1) + ... >= 1 up to
        // PADT + (H - 1) + 2 DYT - 2 < HP, rows outside the image being zero
        const unsigned* lw = Lp + jw * HP + PADT + d0;
        unsigned w[DYT];
#pragma unroll
        for (int t = 0; t < DYT - 1; ++t) w[t] = lw[ya + t];
        for (int y0 = ya; y0 <= yb; y0 += DYT) {
#pragma unroll
          for (int u = 0; u < DYT; ++u) {
            const int yk = y0 + u;
            w[(u + DYT - 1) % DYT] = lw[yk + DYT - 1];
            const unsigned lo = kp[yk * KS], hi = kp[yk * KS + 1];
            const unsigned kw = (unsigned)(((((unsigned long long)hi << 32) | lo) << s) >> 32);
#pragma unroll
            for (int t = 0; t < DYT; ++t) acc[t] += __popc(w[(u + t) % DYT] & kw);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < DYT; ++t) {
        if (acc[t]) {
          const unsigned long long pose = ((unsigned long long)r << 18) |
                                          ((unsigned long long)(d0 + t + H - 1) << 9) |
                                          (unsigned long long)(dx + W - 1);
          const unsigned long long cand = ((unsigned long long)acc[t] << POSE_BITS) | (~pose & POSE_MASK);
          best = cand > best ? cand : best;
        }
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off);
    best = o > best ? o : best;
  }
  if (lane == 0) red[wave] = best;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < OV_WAVES; ++i) best = red[i] > best ? red[i] : best;
    work[(size_t)pair * nchunks + chunk] = best;
  }
}

__global__ void overlap_finish(const unsigned long long* __restrict__ work, long long count, int nchunks,
                               int H, int W, int* __restrict__ area_out, int* __restrict__ pose_out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  unsigned long long best = 0ull;
  for (int c = 0; c < nchunks; ++c) {
    const unsigned long long v = work[(size_t)i * nchunks + c];
    best = v > best ? v : best;
  }
  const int area = (int)(best >> POSE_BITS);
  area_out[i] = area;
  if (pose_out) {
    const unsigned long long pose = ~best & POSE_MASK;
    pose_out[3 * i + 0] = area ? (int)(pose >> 18) : 0;
    pose_out[3 * i + 1] = area ? (int)((pose >> 9) & 511) - (H - 1) : 0;
    pose_out[3 * i + 2] = area ? (int)(pose & 511) - (W - 1) : 0;
  }
}

// angles per workgroup and workgroups per pair: about OV_TARGET_WGS workgroups in all
void overlap_split(long long count, int n_rot, int& nchunks, int& per_chunk) {
  const long long want = (OV_TARGET_WGS + count - 1) / count;
  const int nc = (int)std::min<long long>(n_rot, std::max<long long>(1, want));
  per_chunk = (n_rot + nc - 1) / nc;
  nchunks = (n_rot + per_chunk - 1) / per_chunk;
}

}  // namespace

size_t overlap_work_bytes(long long count, int n_rot) {
  int nchunks, per_chunk;
  overlap_split(count, n_rot, nchunks, per_chunk);
  return (size_t)count * nchunks * sizeof(unsigned long long);
}

hipError_t launch_overlap_pairs(const unsigned char* locks, const unsigned char* keys, int H, int W,
                                const int* lock_idx, const int* key_idx, long long count, const float* coef,
                                int n_rot, int* area_out, int* pose_out, void* work, hipStream_t st) {
  if (H < 1 || H > OV_MAX || W < 1 || W > OV_MAX || count < 1 || n_rot < 1 || n_rot > OVERLAP_MAX_ROT)
    return hipErrorInvalidValue;
  int nchunks, per_chunk;
  overlap_split(count, n_rot, nchunks, per_chunk);
  unsigned long long* wk = static_cast<unsigned long long*>(work);
  const long long slice = 0x7fffffffll / nchunks;  // pairs per launch: the grid's x is below 2^31
  for (long long p0 = 0; p0 < count; p0 += slice) {
    const long long np = std::min(slice, count - p0);
    hipLaunchKernelGGL(overlap_kernel, dim3((unsigned)(np * nchunks)), dim3(OV_T), 0, st, locks, keys, H, W,
                       lock_idx, key_idx, p0, reinterpret_cast<const float4*>(coef), n_rot, nchunks, per_chunk, wk);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const long long fb = (count + 255) / 256;
  if (fb > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(overlap_finish, dim3((unsigned)fb), dim3(256), 0, st, wk, count, nchunks, H, W, area_out,
                     pose_out);
  return hipGetLastError();
}

}  // namespace mvae
