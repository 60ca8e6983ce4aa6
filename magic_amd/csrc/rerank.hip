// Verified retrieval (mvae_rerank, mvae_overlap_place, gfx950): the exact overlap of each lock with
// the keys of its shortlist, the shortlist ordered by that area, and a key shown at its pose.
//
// mvae_rerank = three steps on one stream, all in the caller's work buffer:
//   rerank_expand   pair p = i R + c: lock lock_idx[i] (NULL: i), key cand[i][c], two int32 lists
//   overlap_kernel / overlap_finish (overlap.hip) on those N R pairs: area and pose of the definition
//                   there; a negative key index is an empty entry, which overlap_kernel leaves at once
//   rerank_order    one wave per lock, four locks per workgroup. Lane e holds entry e of the row
//                   (empties: area -1) and counts, over R shuffles, the entries that come before it:
//                   rank = #{e' : area' > area, or area' == area and e' < e}. Every pair of entries is
//                   ordered one way, so the ranks are a permutation of 0 .. R - 1 and each lane writes
//                   its own slot: larger area first, ties in the shortlist's order, empties last.
// rerank_place: one workgroup per pair and a loop over the pixels, 256 at a time. A lane computes its
// lock bit, the rotated key's bit at its own pixel (for |Kr_r|) and at the shifted one (for P), writes
// the overlay byte; the four counts are popcounts of ballots, wave-uniform, added up per wave and then
// over the workgroup's four waves in LDS. No HBM atomics. The rotation is overlap.hip's and
// make_batch_kernel's: unfused fp32 (fp contract(off)), roundf, zero fill, foreground = byte >= 128.
#include <algorithm>

#include "mvae_internal.h"

namespace mvae {
namespace {

constexpr int RR_T = 256;  // threads per workgroup: four waves = four locks (order), one pair (place)
constexpr int RR_WAVES = RR_T / 64;

__global__ __launch_bounds__(RR_T) void rerank_expand(const int* __restrict__ lock_idx,
                                                      const int* __restrict__ cand, long long count, int R,
                                                      int* __restrict__ li, int* __restrict__ ki) {
  const long long p = (long long)blockIdx.x * RR_T + threadIdx.x;
  if (p >= count) return;
  const long long i = p / R;
  li[p] = lock_idx ? lock_idx[i] : (int)i;
  ki[p] = cand[p];
}

__global__ __launch_bounds__(RR_T) void rerank_order(const int* __restrict__ cand, const int* __restrict__ area_in,
                                                     const int* __restrict__ pose_in, long long N, int R,
                                                     int* __restrict__ key_out, int* __restrict__ area_out,
                                                     int* __restrict__ pose_out, int* __restrict__ from_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * RR_WAVES + wave;
  if (i >= N) return;  // the ragged last group: whole waves leave, and there is no barrier below
  const size_t row = (size_t)i * R;
  const bool have = lane < R;
  const int key = have ? cand[row + lane] : -1;
  const bool empty = key < 0;
  const int area = have ? (empty ? -1 : area_in[row + lane]) : -2;
  int rank = 0;
  for (int e = 0; e < R; ++e) {  // R is uniform: every lane takes part in every shuffle
    const int a = __shfl(area, e);
    rank += (a > area || (a == area && e < lane)) ? 1 : 0;
  }
  if (!have) return;
  const size_t o = row + rank;  // rank < R: at most R - 1 entries come before this one
  key_out[o] = empty ? -1 : key;
  area_out[o] = area;
  if (pose_out) {
    pose_out[3 * o + 0] = empty ? 0 : pose_in[3 * (row + lane) + 0];
    pose_out[3 * o + 1] = empty ? 0 : pose_in[3 * (row + lane) + 1];
    pose_out[3 * o + 2] = empty ? 0 : pose_in[3 * (row + lane) + 2];
  }
  if (from_out) from_out[o] = lane;
}

// bit (x, y) of the key rotated by cf: make_batch_kernel's gather
__device__ __forceinline__ bool rotated_bit(const unsigned char* __restrict__ K, int H, int W, float4 cf, int x,
                                            int y) {
#pragma clang fp contract(off)  // the gather coordinates are unfused mul / add / sub
  const float fx = (float)x, fy = (float)y;
  const float xin = (cf.x * fx - cf.y * fy) + cf.z;
  const float yin = (cf.y * fx + cf.x * fy) + cf.w;
  const float xr = roundf(xin), yr = roundf(yin);
  if (!(xr >= 0.f && xr <= (float)(W - 1) && yr >= 0.f && yr <= (float)(H - 1))) return false;
  return K[(size_t)(int)yr * W + (int)xr] >= 128;
}

__global__ __launch_bounds__(RR_T) void rerank_place(
    const unsigned char* __restrict__ locks, const unsigned char* __restrict__ keys, int H, int W,
    const int* __restrict__ lock_idx, const int* __restrict__ key_idx, long long pair0,
    const float4* __restrict__ coef, int n_rot, const int* __restrict__ pose,
    unsigned char* __restrict__ overlay_out, int* __restrict__ stats_out) {
#pragma clang fp contract(off)
  __shared__ int red[RR_WAVES][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long pair = pair0 + blockIdx.x;
  const int HW = H * W;  // at most 65536
  const unsigned char* L = locks + (size_t)(lock_idx ? lock_idx[pair] : pair) * HW;
  const unsigned char* K = keys + (size_t)(key_idx ? key_idx[pair] : pair) * HW;
  const int r = pose[3 * pair + 0], dy = pose[3 * pair + 1], dx = pose[3 * pair + 2];
  // a pose out of range: no coef entry and no key pixel is read (uniform over the workgroup)
  const bool valid = r >= 0 && r < n_rot && dy > -H && dy < H && dx > -W && dx < W;
  const float4 cf = valid ? coef[r] : make_float4(0.f, 0.f, 0.f, 0.f);
  unsigned char* O = overlay_out ? overlay_out + (size_t)pair * HW : nullptr;
  int nl = 0, nk = 0, np = 0, nb = 0;  // wave-uniform: sums of ballot popcounts
  for (int base = 0; base < HW; base += RR_T) {  // every lane of a wave makes every ballot
    const int pix = base + tid;
    const bool in = pix < HW;
    const int y = pix / W, x = pix - y * W;
    const bool lb = in && L[pix] >= 128;
    bool kr = false, pb = false;
    if (valid && in) {
      kr = rotated_bit(K, H, W, cf, x, y);
      const int ys = y - dy, xs = x - dx;
      if (ys >= 0 && ys < H && xs >= 0 && xs < W) pb = rotated_bit(K, H, W, cf, xs, ys);
    }
    if (O && in) O[pix] = (unsigned char)((lb ? 1 : 0) | (pb ? 2 : 0));
    nl += __popcll(__ballot(lb));
    nk += __popcll(__ballot(kr));
    np += __popcll(__ballot(pb));
    nb += __popcll(__ballot(lb && pb));
  }
  if (!stats_out) return;  // uniform
  if (lane == 0) {
    red[wave][0] = nl;
    red[wave][1] = nk;
    red[wave][2] = np;
    red[wave][3] = nb;
  }
  __syncthreads();
  if (tid < 4) {
    int s = 0;
    for (int w = 0; w < RR_WAVES; ++w) s += red[w][tid];
    stats_out[4 * pair + tid] = (valid || tid == 0) ? s : -1;
  }
}

inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

size_t rerank_work_bytes(long long N, int R, int n_rot) {
  const long long count = N * R;
  // [overlap partials | lock list | key list | areas | poses], each part 8-byte aligned
  return align8(overlap_work_bytes(count, n_rot)) + 3 * align8((size_t)count * 4) + align8((size_t)count * 12);
}

hipError_t launch_rerank(const unsigned char* locks, const unsigned char* keys, int H, int W, const int* lock_idx,
                         const int* cand, long long N, int R, const float* coef, int n_rot, int* key_out,
                         int* area_out, int* pose_out, int* from_out, void* work, hipStream_t st) {
  if (N < 1 || N > RERANK_MAX_LOCKS || R < 1 || R > 64) return hipErrorInvalidValue;
  const long long count = N * R;
  char* w = static_cast<char*>(work);
  const size_t list = align8((size_t)count * 4);
  int* li = reinterpret_cast<int*>(w + align8(overlap_work_bytes(count, n_rot)));
  int* ki = reinterpret_cast<int*>(reinterpret_cast<char*>(li) + list);
  int* area = reinterpret_cast<int*>(reinterpret_cast<char*>(ki) + list);
  int* pose = reinterpret_cast<int*>(reinterpret_cast<char*>(area) + list);
  const long long eb = (count + RR_T - 1) / RR_T;  // N <= 2^31 - 1 and R <= 64: below 2^31
  hipLaunchKernelGGL(rerank_expand, dim3((unsigned)eb), dim3(RR_T), 0, st, lock_idx, cand, count, R, li, ki);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_overlap_pairs(locks, keys, H, W, li, ki, count, coef, n_rot, area, pose, work, st);
  if (e != hipSuccess) return e;
  const long long ob = (N + RR_WAVES - 1) / RR_WAVES;
  hipLaunchKernelGGL(rerank_order, dim3((unsigned)ob), dim3(RR_T), 0, st, cand, area, pose, N, R, key_out, area_out,
                     pose_out, from_out);
  return hipGetLastError();
}

hipError_t launch_overlap_place(const unsigned char* locks, const unsigned char* keys, int H, int W,
                                const int* lock_idx, const int* key_idx, long long count, const float* coef,
                                int n_rot, const int* pose, unsigned char* overlay_out, int* stats_out,
                                hipStream_t st) {
  if (H < 1 || H > 256 || W < 1 || W > 256 || count < 1 || n_rot < 1 || n_rot > OVERLAP_MAX_ROT ||
      (!overlay_out && !stats_out))
    return hipErrorInvalidValue;
  const long long slice = 0x7fffffffll;  // pairs per launch: the grid's x is below 2^31
  for (long long p0 = 0; p0 < count; p0 += slice) {
    const long long np = std::min(slice, count - p0);
    hipLaunchKernelGGL(rerank_place, dim3((unsigned)np), dim3(RR_T), 0, st, locks, keys, H, W, lock_idx, key_idx, p0,
                       reinterpret_cast<const float4*>(coef), n_rot, pose, overlay_out, stats_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mvae
