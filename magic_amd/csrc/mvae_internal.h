// Internal declarations shared by the libmvae translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstddef>
#include <cstdint>
#include "gemm_plan.h"

namespace mvae {

enum EpiMode {
  EPI_STORE = 0,    // C = acc
  EPI_ACT = 1,      // C = act(acc)                     (forward layer, bias folded via ones column)
  EPI_DACT = 2,     // C = acc * act'(aux[remap(row)])  (dgrad through the producing activation)
  EPI_BCE = 3,      // sigmoid + reconstruction BCE row partials + dU = (y - x) * scale (+ optional y)
  EPI_SIGMOID = 4,  // C = sigmoid(acc)                 (generate / reconstruct)
  EPI_BCEB = 5,     // EPI_BCE whose target form the epilogue chooses at run time (kernel-
                    // internal: gemm_run makes one EPI_BCEB launch when the target has a bf16
                    // plane): its bits while *xnb == 0 (GemmEpi::xbits), its bf16 plane while
                    // *xdyn == 0, else the fp32 rows (bce_x16 in gemm_common.h)
  EPI_DACTB = 6,    // EPI_DACT reading aux from its bf16 plane auxp (kernel-internal: the wide
                    // bf16 kernels' instantiation when auxp is set, so the fp32-aux path and its
                    // registers are not compiled into it)
};

enum Act { ACT_TANH = 0, ACT_ELU = 1 };

// GEMM arithmetic: native fp32 MFMA; bf16 operands (fp32 accumulate); fp32-accurate
// 3-term exact bf16 split (see gemm_bf16.hip).
enum GemmPrec { GEMM_F32 = 0, GEMM_BF16 = 1, GEMM_F32X = 2 };

struct GemmEpi {
  int mode = EPI_STORE;
  int act = ACT_TANH;
  const float* aux = nullptr;   // DACT: activation output the gradient flows through
  int ld_aux = 0;
  // DACT: bf16 plane 0 of aux (same ld), read instead of aux when set (bf16 mode: the
  // activations are then stored as bf16 planes only)
  const unsigned short* auxp = nullptr;
  int remap_split = 1 << 30;    // aux row = row >= remap_split ? row - remap_shift : row
  int remap_shift = 0;
  const float* x = nullptr;     // BCE: target pixels (lock image), fp32
  int ldx = 0;
  // BCE: bf16 plane 0 of the target (same ld). Read instead of x when *xdyn == 0, i.e. every
  // pixel of the batch is exact in bf16; the fp32 rows are then never written.
  const unsigned short* xp = nullptr;
  const int* xdyn = nullptr;
  // BCE: *xnb == 0 when every target pixel is 0 or 1 (the de-interleave's second flag word, two
  // slots past xdyn's): the epilogue then takes the one-logarithm form without testing pixels
  const int* xnb = nullptr;
  // BCE: the target as one bit per pixel (byte c of row r: columns 8c .. 8c + 7, bit j = column
  // 8c + j nonzero), valid while *xnb == 0: read instead of the bf16 plane, 16x fewer bytes
  const unsigned char* xbits = nullptr;
  int ldbits = 0;
  float scale = 1.f;            // BCE: 1/global_batch
  float* y = nullptr;           // BCE: optional sigmoid output
  int ldy = 0;
  float* rowpart = nullptr;     // BCE: [M][nblk_n] per-row partial sums of the BCE terms
  int rp_ld = 0, rp_off = 0;    // ... its row stride (0: this GEMM's nblk_n) and first block (a
                                // launch over a column range of a wider head)
  // bf16 planes of the output (same layout/ld as C, plane stride pc): the operand image
  // of the next GEMM in the bf16 / f32x modes. ncp = 0 (none), 1 (RN) or 3 (exact split).
  unsigned short* cp = nullptr;
  long long pc = 0;
  int ncp = 0;
  int c32 = 1;                  // 0: no fp32 C store (every consumer reads the planes)
  // Row padding [N, round8(N)) of the output and of the DACT / BCE operand rows (all strides
  // multiples of 8) may be read and written as whole 8-column chunks, the padding written with
  // its constant value: 1.0 at column N when padw == 2 (an activation's ones column), else 0.
  // (Element-wise stores of a partial last chunk cost ~5 us per 256x256-tile epilogue.)
  int padw = 0;
};

// bf16 operand shadows (precision = bf16). When set, the GEMM reads A/B from these
// instead of the fp32 pointers (same logical layout/ld) and accumulates in fp32.
struct GemmDesc {
  int M = 0, N = 0, K = 0;
  const float* A = nullptr; int lda = 0; bool at = false;  // at: A stored [K][M]
  const float* B = nullptr; int ldb = 0; bool bt = false;  // bt: B stored [N][K]
  float* C = nullptr; int ldc = 0;
  int batch = 1; long long sA = 0, sB = 0, sC = 0;          // per-batch element strides
  // bf16 planes of A and B (bf16 / f32x modes): planes at Ap + i*pA, same layout and ld
  const unsigned short* Ap = nullptr; long long pA = 0; int nA = 1;
  const unsigned short* Bp = nullptr; long long pB = 0; int nB = 1;
  const int* dynA = nullptr;           // != 0 when A's residual planes may be nonzero
  int prec = GEMM_F32;                 // GemmPrec
  GemmForce force;                     // what the caller fixes of the kernel choice (gemm_plan.h); default: nothing
  int group = -1;                      // bf16 DMA kernels' tile order (Params::group); -1 planner
  // A as bits (bf16 / f32x modes, a 0/1 operand: the layer-0 pixels): the BitMat below, read by
  // the eight-phase kernel instead of A's planes while *anb == 0 (the de-interleave's not-binary
  // word); strips of abits_kts blocks, batch stride abits_sb words. The planes stay the operand of
  // every batch with a pixel other than 0 or 1.
  const unsigned* Abits = nullptr;
  int abits_kts = 0;
  long long abits_sb = 0;
  const int* anb = nullptr;
  int bits_reg = 0;                    // bits path: A words by loads to registers (gemm_bf16e.hip E8)
  int x3 = 0;                          // f32x ring plans at tile N 128 on the plane-stacked kernel (gemm_bf16.hip)
  GemmEpi epi;
};

// BitMat: a 0/1 GEMM operand A (logical [M][K], rows x k) at one bit per element, laid out for
// the eight-phase kernel's 256 x 256 x 64 tiles and its 16x16x32 MFMA A fragments. Blocks of 256
// rows x 64 k (2 KB = 512 words): block (mt, kt) at word 512 (mt kts + kt), kts >= ceil(K / 64)
// blocks per 256-row strip. In a block, word 2 ((2 s + wm) 64 + lane) + j holds the 64-row
// quarter (s, wm) of lane `lane`'s fragments: for row 128 s + 64 wm + 16 (2 j + h) + (lane & 15)
// and k = 32 kh + 8 (lane >> 4) + el (h, kh in {0,1}, el < 8), bit 8 h + 4 kh + (el >> 1) +
// 16 (el & 1) -- so the bf16 pair (el, el + 1) = (2 d, 2 d + 1) of fragment (2 j + h, kh) is
// ((w >> 8 h) & (0x10001 << p)) * (0x3F80 >> p), p = 4 kh + d: two VALU operations per dword.
// Rows >= M and k >= K are 0.
constexpr int BITMAT_BLOCK_WORDS = 512;
inline int bitmat_kts(int K) { return (K + 63) / 64; }
inline size_t bitmat_words(int M, int K) { return (size_t)((M + 255) / 256) * bitmat_kts(K) * BITMAT_BLOCK_WORDS; }
// (tests / diagnostics) a bf16 plane of 0/1 values -> BitMat: plane[row * ld + k], or
// plane[k * ld + row] when trans (A stored [K][M]); *nb (optional) set if a value is not 0 or 1
hipError_t launch_bits_from_plane(const unsigned short* plane, int ld, bool trans, int M, int K,
                                  unsigned* out, int kts, int* nb, hipStream_t st);

// Launch the plan gemm_plan(d, ws_elems) makes (gemm_plan.h; a split-K plan reduces its slabs in a
// fixed order). ws: device workspace of >= gemm_workspace_elems(d) floats.
hipError_t gemm_run(const GemmDesc& d, float* ws, size_t ws_elems, hipStream_t st);
// the launchers gemm_run dispatches to by GemmPlan::kernel: p carries the plan's grid, tile and split
namespace gemm { struct Params; }
hipError_t gemm_bf16_launch(const gemm::Params& p, const GemmDesc& d, const GemmPlan& pl, hipStream_t st);
hipError_t gemm_valu_launch(const gemm::Params& p, bool at, bool bt, int epi, hipStream_t st);
// Number of column blocks the BCE epilogue writes per row (rowpart's inner dim).
int gemm_bce_nblk(int N);

// ---- the encoder's hidden layers in one launch (enc_chain.hip, bf16 planes) ----
// layer: out = act(in W) on bf16 planes; W [K][ldw] (K incl. the bias row), N output columns,
// out [M][ldo] with the row padding of GemmEpi::padw = 2 (1.0 at column N, zeros to round8(N+1))
struct ChainLayer {
  const unsigned short* w = nullptr;
  int ldw = 0, K = 0, N = 0;
  unsigned short* out = nullptr;
  int ldo = 0;
};
struct ChainArgs {
  const unsigned short* x = nullptr;  // the first layer's input plane [M][ldx] (padded rows)
  int ldx = 0, M = 0, nl = 0, act = 0;
  int rows = 0;  // rows per workgroup forced (create option enc_chain_rows; 0: enc_chain_rows)
  ChainLayer l[4];
};
// rows per workgroup for M rows (a multiple of 16, <= 96; forced: a valid forced value wins)
int enc_chain_rows(int M, int forced = 0);
// K <= 512, N <= 511, 16-B aligned planes and strides multiple of 8, else hipErrorInvalidValue
hipError_t launch_enc_chain(const ChainArgs& a, hipStream_t st);

// bf16 plane image of an fp32 buffer (same layout): planes at p + t*stride, t < n
struct Planes {
  unsigned short* p = nullptr;
  long long stride = 0;
  int n = 0;
};
// ---- batch input (batch_input.hip): the plane de-interleave, the bits path, the producers ----
// The plane path. f32mask: bit c -> write fp32 rows of block c (0 rot, 1 lock, 2 key). Plane 0 always (when
// xp.p); *dyn (zero on entry) is set when a pixel is not a bf16 value, and only then are
// planes 1-2 (3-plane mode) and the fp32 rows of the blocks in f32dyn_mask written. The flag has
// two slots used in turn: each launch zeroes the other one (dyn_next, the next launch's dyn),
// whose last readers ran before it on the stream.
// xbits (optional): the lock block's pixels as bits (GemmEpi::xbits, ldbits bytes per row), written
// by the 8-pixel form only (D % 8 == 0; the other forms raise the not-binary word instead)
hipError_t launch_deinterleave(const float* x, float* xs, const Planes& xp, int* dyn, int* dyn_next,
                               int B, int D, int ldx, int f32mask, int f32dyn_mask, hipStream_t st,
                               unsigned char* xbits = nullptr, int ldbits = 0);
// Where the bits path writes the layer-0 operand of a [B][D] batch: the forward BitMat xbf (3B x
// (D + 1), kts_f = bitmat_kts(D + 1)), the weight-gradient BitMat xbw ((D + 1) x 3B, kts_w =
// bitmat_kts(3B)), the BCE target bits (GemmEpi::xbits, ldbits >= D / 8 bytes per row) and, for a
// batch with a pixel other than 0 / 1, what launch_deinterleave writes: the planes xp of the stacked
// rows [3B][ldx] and the fp32 rows xs of the blocks in f32dyn_mask. Both BitMats must be zero-filled
// once (their padding is never written). A context fills it once, at plan time (mvae_ctx::in_dst).
struct BitsDst {
  unsigned* xbf = nullptr; int kts_f = 0;
  unsigned* xbw = nullptr; int kts_w = 0;
  unsigned char* xbits = nullptr; int ldbits = 0;
  float* xs = nullptr; Planes xp; int ldx = 0;
  int f32dyn_mask = 0;
};
// The three forms of a batch. XBatch: fp32 X [B][3 D]. PairsBatch: row b is lock idx[b], its rotation
// by coef[b] and key kidx[b], an index into `keys` (NULL: idx, the own pair); H x W images. ImagesBatch
// (an embedding pass): 3B independent images, image t of the pass = row t of the stacked operand
// (block t / B, batch row t % B): table image idx[t] (t when idx is null) for t < nvalid, an all-zero
// image past that (idx not read).
struct XBatch { const float* x; int B, D; };
struct PairsBatch {
  const unsigned char* locks; const unsigned char* keys; int H, W;
  const int* idx; const int* kidx; const float* coef; float div; int B;
};
struct ImagesBatch { const unsigned char* table; int H, W; const int* idx; int nvalid; float div; int B; };
// The bits path, one launcher per form; all three write the same bits for the same batch. *dyn slot 2
// is raised when a pixel is not 0 / 1, and then (a gated second kernel) the planes, the fp32 rows and
// the inexact flag (*dyn) are written. dyn_next: the other flag slot, zeroed. no_xbw: the forward
// words only (launch_bits_transpose then writes xbw from xbf). Each returns hipErrorInvalidValue,
// before anything is launched, for a batch it does not serve: D % 8 == 0 and B % 64 == 0 for all; a
// 16-byte aligned x; 8-byte aligned tables and a 16-byte aligned coef (pairs_bits_fits,
// images_bits_fits).
hipError_t launch_deint_bits(const XBatch& src, const BitsDst& dst, int* dyn, int* dyn_next, bool no_xbw,
                             hipStream_t st);
bool pairs_bits_fits(const unsigned char* locks, const unsigned char* keys, const float* coef, int B, int D);
hipError_t launch_pairs_bits(const PairsBatch& src, const BitsDst& dst, int* dyn, int* dyn_next, bool no_xbw,
                             hipStream_t st);
bool images_bits_fits(const unsigned char* table, int B, int D);
hipError_t launch_images_bits(const ImagesBatch& src, const BitsDst& dst, int* dyn, int* dyn_next, bool no_xbw,
                              hipStream_t st);
// the weight gradient's BitMat xbw from the forward's xbf (both of a 3B-row batch; see
// bits_transpose_kernel)
hipError_t launch_bits_transpose(const unsigned* xbf, int kts_f, unsigned* xbw, int kts_w, int B, hipStream_t st);
// The producers: a pairs batch / an embedding pass as X [B][3 D] (any D, any alignment):
// x[b, 3 p + ch] = (lock, rotated lock, key)[ch] / div, for a pass image((1, 0, 2)[ch] B + b)[p] / div
hipError_t launch_make_batch(const unsigned char* locks, const unsigned char* keys, int H, int W,
                             const int* idx, const int* kidx, const float* coef, int B, float div, float* x,
                             hipStream_t st);  // kidx: the key of each row; NULL: idx
hipError_t launch_images_x(const ImagesBatch& src, float* x, hipStream_t st);
// ---- elementwise / reduction kernels (mvae_kernels.hip) ----
// N(0,1) into out[slots][B][L]: elements (s*Bg + off + b)*L + l of the counter's global stream
// (Bg rows per slot over all ranks, this rank's rows starting at off)
hipError_t launch_normal(float* out, int slots, int B, int L, int Bg, int off, uint64_t seed,
                         uint64_t counter, hipStream_t st);
// eps of the latent head: the [3][B][L] buffer `buf` (caller-given draws), or, when buf is
// NULL, the Philox stream (seed, counter) regenerated inside the kernels at this rank's rows
// (global batch Bg, first row off): the same values launch_normal would write.
struct LatentEps {
  const float* buf = nullptr;
  uint64_t seed = 0, counter = 0;
  int Bg = 0, off = 0;
};
// Fused latent forward (one wave per row): z = mu + sqrt(exp s) eps for the three passes,
// z written where read (zmask bit 1: fp32 lock rows, bit 2: fp32 key rows; zp: lock planes),
// rowfwd[b] = {sum KL term, sum (z_lock - z_rot)^2, sum (z_lock - z_key)^2, 0}.
hipError_t launch_latent_fwd(const float* ms, const LatentEps& eps, float* z, const Planes& zp,
                             int zmask, int B, int L, int ldz, float* rowfwd, hipStream_t st);
// out[j] for j in [0, ncols): mode 0 = colsq (z_lock^2 | z_key^2), mode 1 = coldot. cnt (zeroed
// ints, one per 64 columns; left zeroed): one launch, the last chunk's workgroup sums; else two.
hipError_t launch_colstats(int mode, const float* z, int B, int L, int ldz, const float* colsq,
                           const float* draw, float* part, int nchunk, float* out, hipStream_t st,
                           int* cnt = nullptr);
int colstats_nchunk(int B);
hipError_t launch_metric(const float* z, int ldz, const float* rowfwd, const float* rowpart, int nblk,
                         const float* areas, const float* colsq, int B, int L, int metric, int recip,
                         float w, float inv_bg, float* rowvals, float* dist, float* draw,
                         hipStream_t st);
hipError_t launch_loss_reduce(const float* rowvals, int B, float inv_bg, float* losses, hipStream_t st);
hipError_t launch_latent_bwd(const float* ms, const LatentEps& eps, const float* dzdec, const float* draw,
                             const float* colsq, const float* coldot, int B, int L, int metric, float w,
                             float inv_bg, float* dhead, int ldh, const Planes& hp, hipStream_t st);
struct AdamArgs {
  float* theta; const float* g1; const float* g2; float* m1; float* v1; float* m2; float* v2;
  size_t n_all, n_enc; float lr1, lr2, b1, b2, eps;
  Planes tp;  // bf16 plane image of theta refreshed in the same pass (bf16 / f32x modes)
  size_t i0 = 0, i1 = ~size_t(0);  // the index range [i0, min(i1, n_all)) this launch updates
  int nt = 0;  // moments and fp32 theta stored non-temporal (read again only by the next Adam)
};
hipError_t launch_adam(const AdamArgs& a, hipStream_t st);
hipError_t launch_split_planes(const float* src, size_t n, const Planes& dst, hipStream_t st);
// x[i] = x[i] > 0 ? 1 : 0 (diagnostics: binary BCE targets for the GEMM harness)
hipError_t launch_binarize(float* x, size_t n, hipStream_t st);
// ---- all-pairs distance with fused top-k (match.hip) ----
// match_plan: key rows per split (a multiple of 64) and the number of splits of M for N lock rows.
void match_plan(long long N, long long M, long long* split_len, int* splits);
// r[l] = 1 / sqrt(max(sum_rows z[row][l]^2, 1e-12)) in a fixed order; part: match_colnorm_chunks(n) L doubles
int match_colnorm_chunks(long long n);
hipError_t launch_colnorm(const float* z, long long n, int L, double* part, float* r, hipStream_t st);
// top_val / top_idx [N][k] (1 <= k <= min(M, 64)); dist null or [N][M]; ws_val / ws_idx [N][splits][k]
// (splits > 1); rl / rk: the cosine metric's reciprocal column norms (metric 0)
hipError_t launch_match(const float* zl, long long N, const float* zk, long long M, int L, int k, int order,
                        int metric, int recip, const float* rl, const float* rk, long long split_len, int splits,
                        float* dist, float* ws_val, int* ws_idx, float* top_val, int* top_idx, hipStream_t st);
// The same over one shard of a gallery (mvae_match_ex): the lists hold key_base + j (0 <= key_base,
// key_base + M < 2^31) and k may exceed M; dist has row stride dist_ld >= M; carry: top_val / top_idx
// hold the list of earlier shards and the merge starts from it. thr_val / thr_idx / ahead [N] (all or
// none): ahead[i] (carry: +=) the keys strictly before (thr_val[i], thr_idx[i]) in the order. The
// per-split lists (and counts, ws_cnt [N][splits]) go through the workspace whenever splits > 1 or carry.
hipError_t launch_match_ex(const float* zl, long long N, const float* zk, long long M, int L, int k, int order,
                           int metric, int recip, const float* rl, const float* rk, long long split_len, int splits,
                           float* dist, long long dist_ld, long long key_base, int carry, const float* thr_val,
                           const int* thr_idx, int* ahead, float* ws_val, int* ws_idx, int* ws_cnt,
                           float* top_val, int* top_idx, hipStream_t st);
// merge_kernel alone: vals / idx [N][parts][k] (carry: after the list top_val / top_idx already hold);
// cnt null or [N][parts]: ahead[i] = (add ? ahead[i] : 0) + the row's counts in order
hipError_t launch_match_merge(const float* vals, const int* idx, long long N, int parts, int k, int order,
                              int carry, const int* cnt, int add, float* top_val, int* top_idx, int* ahead,
                              hipStream_t st);
// colsq [L] doubles = (accumulate ? colsq : 0) + launch_colnorm's chunk sums in order; r = its last line
hipError_t launch_colsq(const float* z, long long n, int L, double* part, double* colsq, int accumulate,
                        hipStream_t st);
hipError_t launch_rnorm(const double* colsq, int L, float* r, hipStream_t st);
// out[i] = the score of lock row i and key row i, in match_kernel's operations
hipError_t launch_pair_scores(const float* zl, const float* zk, long long n, int L, int metric, int recip,
                              const float* rl, const float* rk, float* out, hipStream_t st);
// ---- maximum overlap of lock / key pairs over rotations and shifts (overlap.hip) ----
// area_out[i] = max over r < n_rot, dy, dx of |lock lock_idx[i] & shift(rotate(key key_idx[i], coef[r]),
// dy, dx)|, pose_out[i] (or null) its smallest (r, dy, dx); null index lists: i. H, W in 1 .. 256,
// n_rot in 1 .. OVERLAP_MAX_ROT, work of overlap_work_bytes bytes (hipErrorInvalidValue otherwise,
// before anything is launched).
constexpr int OVERLAP_MAX_ROT = 1 << 24;
size_t overlap_work_bytes(long long count, int n_rot);
hipError_t launch_overlap_pairs(const unsigned char* locks, const unsigned char* keys, int H, int W,
                                const int* lock_idx, const int* key_idx, long long count, const float* coef,
                                int n_rot, int* area_out, int* pose_out, void* work, hipStream_t st);
// ---- verified retrieval: a shortlist ordered by exact overlap, a key placed at its pose (rerank.hip) ----
// Pair (i, c), c < R <= 64: lock lock_idx[i] (null: i) and key cand[i][c] (negative: an empty entry,
// which indexes no table); area and pose as launch_overlap_pairs, each row then ordered by area
// (larger first, ties in column order, empties last with key -1, area -1, pose 0): key_out, area_out,
// pose_out (or null), from_out (or null: the column an entry came from), all [N][R]. work of
// rerank_work_bytes bytes, 8-byte aligned. N in 1 .. RERANK_MAX_LOCKS (hipErrorInvalidValue otherwise).
constexpr long long RERANK_MAX_LOCKS = 0x7fffffffll;
size_t rerank_work_bytes(long long N, int R, int n_rot);
hipError_t launch_rerank(const unsigned char* locks, const unsigned char* keys, int H, int W, const int* lock_idx,
                         const int* cand, long long N, int R, const float* coef, int n_rot, int* key_out,
                         int* area_out, int* pose_out, int* from_out, void* work, hipStream_t st);
// overlay_out[i] (or null) = lock bit | 2 * bit of the key rotated by coef[r] and shifted by (dy, dx),
// (r, dy, dx) = pose[i]; stats_out[i] (or null) = (|Lb|, |Kr_r|, |P|, |Lb & P|). A pose out of range
// reads no coef entry and no key pixel: the lock alone and (|Lb|, -1, -1, -1).
hipError_t launch_overlap_place(const unsigned char* locks, const unsigned char* keys, int H, int W,
                                const int* lock_idx, const int* key_idx, long long count, const float* coef,
                                int n_rot, const int* pose, unsigned char* overlay_out, int* stats_out,
                                hipStream_t st);
// ---- conv-encoder tower (conv_tower.hip, conv_mfma.hip) ----
// NHWC fp32 activations of the stacked batch (3B forward rows, 4B backward rows); S = image
// side, S1 = S/2 (after pool 1), S2 = S/4 (after pool 2).
struct ConvTower {
  int S = 0, S1 = 0, S2 = 0;
  float* p1 = nullptr;             // pool-1 output        [3B][S1*S1][64]
  unsigned char* arg1 = nullptr;   // its window argmax    [3B][S1*S1][64]
  float* n1 = nullptr;             // LRN-1 output = conv2 input (fp32 kernels only)
  unsigned short* n1b = nullptr;   // ... bf16 (MFMA mode)
  float* a2 = nullptr;             // conv2 + ReLU output  [3B][S1*S1][64]
  unsigned char* arg2 = nullptr;   // pool-2 window argmax [3B][S2*S2][64]
  float* da2 = nullptr;            // d conv2 pre-activation [4B][S1*S1][64] (fp32 kernels only)
  unsigned short* da2b = nullptr;  // ... bf16 (MFMA mode)
  float* dn1 = nullptr;            // d LRN-1 output (conv2 data gradient)
  unsigned short *w2f = nullptr, *w2d = nullptr;  // bf16 conv2 kernel images [25][64 n][64 k]
  float* slab = nullptr;           // weight-gradient partial sums (fixed-order reduction)
  int nchunk1 = 1, nchunk2 = 1, nchunk2m = 1;
  bool mfma = false;               // conv2 on bf16 MFMA (bf16 mode)
};
hipError_t launch_conv1_fwd(const ConvTower& T, const float* xs, int ldx, const float* w1, int nimg,
                            hipStream_t st);
// fwd: a2 = relu(conv(n1, W2) + b2) over nimg images; !fwd: dn1 = conv_dgrad(da2, W2)
hipError_t launch_conv2(const ConvTower& T, bool fwd, const float* in, const unsigned short* inb,
                        const float* w2, const unsigned short* w2b, float* out, int nimg, hipStream_t st);
hipError_t launch_lrn2_pool2_fwd(const ConvTower& T, int nimg, float* xf, int ldf, int f32,
                                 const Planes& xfp, hipStream_t st);
hipError_t launch_pool2_bwd(const ConvTower& T, const float* dxf, int ldf, int B, hipStream_t st);
hipError_t launch_conv1_wgrad(const ConvTower& T, const float* xs, int ldx, int B, float* g1, float* g2,
                              hipStream_t st);
hipError_t launch_conv2_wgrad(const ConvTower& T, int B, float* g1, float* g2, hipStream_t st);
hipError_t launch_conv2_wprep(const ConvTower& T, const float* w2, hipStream_t st);
hipError_t launch_conv2_mfma(const ConvTower& T, bool fwd, const unsigned short* inb,
                             const unsigned short* wimg, const float* w2, float* out, int nimg,
                             hipStream_t st);
hipError_t launch_conv2_wgrad_mfma(const ConvTower& T, int B, hipStream_t st);
int conv2_wgrad_rows(int S1);

// empty kernel of MARKER_GRID + region workgroups (64 threads): a region boundary that a
// rocprofv3 kernel trace shows (counter passes attribute the dispatches between two markers)
constexpr int MARKER_GRID = 4096;
hipError_t launch_marker(int region, hipStream_t st);
hipError_t launch_copy2d(const float* src, int lds, float* dst, int ldd, int rows, int cols,
                         hipStream_t st);

}  // namespace mvae
