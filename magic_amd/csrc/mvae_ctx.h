// libmvae host code, private: the context and the helpers its translation units share (mvae_api.cpp
// the ABI's bookkeeping, mvae_plan.cpp context creation, mvae_step.cpp the step, mvae_match.cpp
// retrieval, mvae_diag.cpp debug_* / bench_*). The helpers are static inline: no call per launch.
//
// HBM layout (all fp32, row-major, every row stride a multiple of 4 floats):
//   theta  = [enc blocks | head | dec blocks], each block the augmented [W; b] of one layer
//            ((fan_in+1) x fan_out; the head block is [W_mean W_logsigma; b_mean b_logsigma]).
//   grads  = [g1 (same layout as theta) | g2 (encoder slice)] — ONE all-reduce bucket.
//   adam   = [m1 | v1 | m2 | v2].
//   Activation buffers carry a constant ones column after the last feature so every GEMM
//   folds its bias (see gemm_f32.hip). Stacked encoder rows: [rot | lock | key] (3B),
//   backward rows [rot:g1 | lock:g1 | lock:g2 | key:g2] (4B).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mvae.h"
#include "mvae_internal.h"

using namespace mvae;  // (a private header: only the five host files include it)

struct Block {
  size_t off = 0;  // element offset in theta / g1
  int K = 0, N = 0;
  int ld = 0;      // row stride: N rounded up to 8 (16-B rows for the bf16 plane images)
};

static inline int round8(int v) { return (v + 7) & ~7; }
static inline size_t align64(size_t v) { return (v + 63) & ~size_t(63); }
// Philox call counters of inference draws carry this bit (a stream disjoint from training's)
constexpr uint64_t EVAL_STREAM = 1ull << 63;

struct mvae_ctx {
  mvae_cfg cfg{};
  int device = 0;
  // a batch given as (tables, idx, coefficients) (the *_pairs entry points) or an embedding pass
  // where the direct kernel does not apply: X materialised here, allocated on first need
  float* pairs_x = nullptr;
  // mvae_match's workspace, allocated at the first call that needs it and grown on demand: the
  // per-split top-k lists [N][splits][k] (values, indices) and, for the cosine metric, the column
  // norms' chunk sums and reciprocal norms of both galleries
  void* match_ws = nullptr;
  size_t match_ws_bytes = 0;
  int B = 0, D = 0, L = 0, nenc = 0, d0 = 0, d1 = 0;
  float inv_bg = 1.f;
  int ldx = 0, ldz = 0, ld_d1 = 0, ld_d2 = 0, ld_u = 0, lddz = 0, ld_dh = 0, nblk = 0, nchunk = 0;
  std::vector<int> ldh;
  // parameters
  std::vector<Block> enc;
  Block head, v1, v2, vo;
  // conv-encoder variant (cfg.conv): tower blocks [25*c_in; b] x 64 before the FC encoder
  bool conv = false;
  Block cv1, cv2;
  ConvTower tower;
  int F = 0, ldf = 0;        // tower features per image (FC layer-0 fan-in) and row stride
  float* xf = nullptr;       // [3B][ldf] tower features (+ ones column): FC layer-0 operand
  float* dxf = nullptr;      // [4B][ldf] their gradient
  int xf32 = 1;              // write the fp32 xf rows (some fp32 GEMM reads them)
  GemmDesc bwd_feat;         // dxf = dZ_0 W_0^T
  int bwd_feat_r = 0;
  size_t n_all = 0, n_enc = 0;
  float* theta = nullptr;
  float* grads = nullptr;
  float* adam = nullptr;
  float* dead = nullptr;
  // activations / workspaces
  float* xs = nullptr;
  std::vector<float*> H;
  float *ms = nullptr, *z = nullptr, *a1 = nullptr, *a2 = nullptr, *du = nullptr;
  float *rowpart = nullptr, *rowvals = nullptr, *dist = nullptr, *draw = nullptr, *losses = nullptr;
  float *colsq = nullptr, *coldot = nullptr, *cspart = nullptr, *eps = nullptr;
  int* cscnt = nullptr;  // create option cs_one: the column statistics' per-column-block counters
  float* rowfwd = nullptr;   // [B][4] latent forward row sums (KL, deformation, sq-diff distance)
  LatentEps le;              // eps of the last forward (buffer, or the Philox call regenerated)
  bool eps_lazy = false;     // le is a Philox call whose values the eps buffer does not hold yet
  int zmask = 6;             // fp32 z rows the latent forward writes (bit 1 lock, bit 2 key)
  float *dzd2 = nullptr, *dzd1 = nullptr, *dzdec = nullptr, *dhead = nullptr;
  std::vector<float*> dzl;  // dZ of every encoder layer [4B][lddz] (all live until its wgrad)
  int enc_part1 = 0;        // bwd_enc[0, enc_part1): dgrad chain + layer-0 wgrad
  // the layer-0 weight gradient in R row chunks (option "wgrad0_chunks", R = 2, 4, 8): chunk r
  // covers rows [w0m[R][r], w0m[R][r+1]) of the [W_0; b_0] block, one backward part each, so a
  // data-parallel host all-reduces each chunk while the next one computes (R = 1: one GEMM)
  int w0_chunks = 1;
  std::vector<GemmDesc> w0c[9];
  std::vector<int> w0m[9];
  int bpart = 0;            // next backward part expected (phase 4)
  float* zgen = nullptr;
  int dhead32 = 1;           // latent_bwd writes fp32 dhead rows (some fp32 GEMM reads them)
  float* ws = nullptr;       // split-K slabs of GEMMs on the caller's stream
  float* ws_side = nullptr;  // ... and of GEMMs on the side stream (concurrent)
  size_t ws_elems = 0;
  // side stream: the weight gradients run beside the dgrad chain (backward)
  hipStream_t side = nullptr;
  std::vector<hipEvent_t> sync_ev;  // fork/join events (timing disabled), reused round robin
  size_t sync_next = 0;
  bool use_side = true;      // option "side_stream"
  bool side_pending = false; // side stream holds work the caller's stream has not joined
  bool early_adam = false;   // option "early_adam": Adam of the parameters after the layer-0
                             // block runs on the side stream beside the layer-0 weight gradient
  bool early_fork = false;   // ... the side stream waits for the dgrad chain this step
  // ... and, with the layer-0 weight gradient in R > 1 chunks, Adam of chunk k's rows ran on the
  // side stream beside chunk k + 1's GEMM: mvae_adam's layer-0 launch starts here
  size_t adam0_from = 0;
  // the single-call backward with the early Adam runs the layer-0 weight gradient in this many
  // chunks when "wgrad0_chunks" is 1 (option "early_chunks"; 1: one GEMM, the default since the
  // chunks keep the one-GEMM plan: 1 vs 2 chunks C2 -2.5 %, C3 -2.4 %, C5 -1.0 %, r6l)
  int early_chunks = 1;
  int side_mask = 3;         // option "side_mask": weight gradients on the side stream -- bit 0
                             // the decoder's, bit 1 the encoder's (else in order on the caller's)
  bool valu = true;          // skinny GEMMs on the fp32 VALU kernel (env MVAE_NO_VALU=1: off)
  std::vector<void*> allocs;
  // bf16 plane images (bf16 / f32x modes): fp32 buffer -> planes of the same layout
  struct PlaneBuf { float* base; size_t n; Planes pl; };
  std::vector<PlaneBuf> planes;
  int np = 0;            // planes per buffer: 0 (fp32 mode), 1 (bf16), 3 (f32x)
  int* dyn = nullptr;    // bf16/f32x: some de-interleaved pixel not exact in bf16?
  int* dyn_cur = nullptr;  // ... its slot of the last de-interleave (two slots, used in turn)
  int x32mask = 7;       // fp32 row blocks of xs the step reads (bit c: 0 rot, 1 lock, 2 key)
  // Where the batch input stage writes (filled at plan time: plan_fp32_copies, plan_pixel_bits): xs,
  // its planes and ldx again; f32dyn_mask, the fp32 rows written only when *dyn != 0 (the BCE target,
  // else read as bf16); xbits / ldbits, the BCE target (lock block) as bits (GemmEpi::xbits); and,
  // with bits_on, the layer-0 pixel operand of a 0/1 batch as bits (create option bits, default on
  // where it applies): the BitMats of the forward (xbf, 3B x (D + 1)) and the weight gradient (xbw,
  // (D + 1) x 3B), written by the de-interleave instead of the bf16 plane, read by the eight-phase
  // kernel's bits path
  BitsDst in_dst;
  bool bits_on = false;
  int adam_nt = 0;  // create option adam_nt
  // create option xbw_split: the de-interleave writes the forward BitMat only and the weight
  // gradient's (xbw) is transposed from it on the side stream (launch_bits_transpose), joined by
  // xbw_ev before the layer-0 weight gradient
  int xbw_split = 0;
  hipEvent_t xbw_ev = nullptr;
  bool xbw_pending = false;
  // schedule (each GEMM tagged with its timing region)
  std::vector<GemmDesc> fwd_enc;  // encoder layers + head
  // the hidden layers fwd_enc[1 .. nenc-1] as one launch (enc_chain.hip; create option enc_chain)
  bool chain = false;
  ChainArgs chain_args;
  int chain_r = 0;
  GemmDesc f_d1, f_d2, f_out;
  // the decoder's hidden layers f_d1, f_d2 as one launch (the same kernel; option dec_chain)
  bool dchain = false;
  ChainArgs dchain_args;
  int dchain_r = 0;
  GemmDesc f_out_a, f_out_b;  // f_out as whole rounds of 256x256 tiles + the rest (f_split)
  bool f_split = false;
  bool use_split = true;      // option "bce_split" (default 1)
  std::vector<GemmDesc> bwd_dec;  // W_out, D_out, W_d2, D_d2, W_d1, D_d1
  std::vector<GemmDesc> bwd_enc;  // W_head, D_head, (W_i, D_i)..., W_0
  std::vector<int> fwd_enc_r, bwd_dec_r, bwd_enc_r;
  int f_d1_r = 0, f_d2_r = 0, f_out_r = 0;
  // HIP-event timing regions (diagnostics / bench roofline)
  std::vector<std::string> region_names;
  std::vector<double> region_ms;
  std::vector<int64_t> region_n;
  struct Pending { int region; hipEvent_t a, b; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> event_pool;
  bool timing = false;
  int timing_sel = -1;   // record only this region (-1: all)
  std::vector<char> marker;  // launch marker kernels around these regions (profiler runs)
  // optimizer state (TF beta1_power / beta2_power are fp32 variables)
  int64_t t1 = 0, t2 = 0;
  float b1p[2] = {0, 0}, b2p[2] = {0, 0};
  uint64_t rng_counter = 0;   // training draws (eps == NULL in mvae_forward / train_step)
  uint64_t rng_eval = 0;      // inference draws (predict / reconstruct): a separate stream, so
                              // evaluation never shifts the training noise sequence
  int row_off = 0;            // this rank's first row in the global batch (eps sampling)
  int phase = 0;  // 0 idle, 1 forward done, 2 metric done, 3 backward done
  std::string err;
};

// Plan-time kernel switches of one context (mvae_create_ex options; the library reads no
// environment outside its diagnostics entry points). Defaults are the measured best plans.
struct CreateOpts {
  int e8 = 1;           // 256-row bf16 GEMMs: 1 planner (eight-phase + ring kernels), 0 ring only,
                        // 2 the eight-phase kernel wherever a 256-row kernel runs
  int thin_ring = 2;    // f32x latent head: 2 ring kernel incl. its weight gradient, 1 weight
                        // gradient on the fp32 kernel, 0 the VALU kernel
  int valu = 1;         // skinny products on the fp32 VALU kernel
  int dact_planes = 1;  // bf16 mode: DACT epilogues read the activation's bf16 plane
  int bce_split = 1;    // the BCE head in whole rounds + 256x128 ring tiles
  int plan_log = 0;     // print the GEMM plans on stderr
  int enc_chain = 1;    // bf16 mode: the encoder's hidden layers in one launch (0: one GEMM each)
  int enc_chain_rows = 0;  // ... its rows per workgroup forced (16..96, multiple of 16; 0 auto)
  int dec_chain = 1;    // bf16 mode: the decoder's two hidden layers in one launch (0: one GEMM each)
  int bits = 1;         // plane modes: the layer-0 pixel operand of a 0/1 batch as bits (BitMat)
  int bits_reg = 1;     // ... the eight-phase bits path loading A's words to registers (E8 BITS 2;
                        // 0: through an LDS copy -- C3 1.784 vs 1.769 ms, C5 2.450 vs 2.432, r6t)
  int adam_nt = 1;      // Adam's moment / fp32 parameter stores non-temporal (C2 -0.6 %, C3 -0.3 %, r6za)
  int x3 = 2;           // f32x: ring plans on the plane-stacked kernels (gemm_bf16.hip): 1 the tile-N-128
                        // plans (C2 -2.1 / -2.9 % on two boxes, r6zi / r6zj), 2 also the 256x256 ones
                        // (C2's hidden weight gradients 68.5 -> 66.5 us, step -0.2 %, r6zp)
  int cs_one = 2;       // the column statistics in one launch (the last chunk's workgroup sums the
                        // partials in colstats_final_kernel's order: the same bits): 0 off, 1 on, 2
                        // where L <= 32 (one 64-column block: C2 -0.9 %; C3, L 200: +0.2 %, r6zh / r6zi)
  int xbw_split = 2;    // the weight gradient's BitMat transposed from the forward's (mvae_ctx):
                        // 0 off, 1 on, 2 where the layer-0 forward's workgroups leave >= 32 CUs
                        // (C3 -0.6 %, C5 -0.4 %; C2, 480 forward workgroups: +3.8 % on, r6zf)
  int conv2_nchunk = 0;
};

namespace mvae {
std::string& create_err();  // this thread's error of a call without a context (mvae_api.cpp)
// mvae_plan.cpp: the three steps of mvae_create_ex (errors through fail(nullptr, ...))
int validate(const mvae_cfg* cfg);
int parse_opts(const char* s, CreateOpts* o);
int plan_context(mvae_ctx* ctx, const CreateOpts& opt);
// the BCE head f as two launches: *a its columns [0, c0), *b the columns [c0, N) on the ring kernel
// at tile N 128 (c0 a multiple of 256; plan_bce_split and mvae_debug_epi)
void bce_split_descs(const GemmDesc& f, int c0, GemmDesc* a, GemmDesc* b);
}  // namespace mvae

static inline int fail(mvae_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg; else create_err() = msg;
  return code;
}

// a failed HIP call ends the calling function with fail(ctxp, the HIP error, what + HIP's text)
#define MV_TRY(ctxp, what, expr)                                                                    \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return fail(ctxp, (int)e_, std::string(what) + hipGetErrorString(e_));    \
  } while (0)
#define MV_CHECK(expr) MV_TRY(ctx, #expr ": ", expr)  // (a context `ctx` in scope)

static inline Planes planes_of(const mvae_ctx* c, const float* p) {
  for (const auto& b : c->planes)
    if (p >= b.base && p < b.base + b.n) {
      Planes r = b.pl;
      r.p += (p - b.base);
      return r;
    }
  return Planes{};
}

static inline GemmDesc gd(int M, int N, int K, const float* A, int lda, bool at, const float* Bm, int ldb,
                          bool bt, float* C, int ldc, int mode = EPI_STORE) {
  GemmDesc d;
  d.M = M; d.N = N; d.K = K; d.A = A; d.lda = lda; d.at = at; d.B = Bm; d.ldb = ldb; d.bt = bt;
  d.C = C; d.ldc = ldc; d.epi.mode = mode;
  return d;
}

static inline int region(mvae_ctx* c, const std::string& name) {
  for (size_t i = 0; i < c->region_names.size(); ++i)
    if (c->region_names[i] == name) return (int)i;
  c->region_names.push_back(name);
  c->region_ms.push_back(0.0);
  c->region_n.push_back(0);
  return (int)c->region_names.size() - 1;
}

static inline hipEvent_t take_event(mvae_ctx* c) {
  if (!c->event_pool.empty()) {
    hipEvent_t e = c->event_pool.back();
    c->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  // timing only: no system-scope fence (a cache writeback + invalidate per record otherwise)
  (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  return e;
}

// RAII: records a start/stop event pair around one region on the launch stream; in profiler
// runs (mvae_timing_marker) it also brackets the region with marker kernels whose grid size
// (MARKER_GRID + region) names the region in a kernel trace
struct TimeScope {
  mvae_ctx* c; int r; hipStream_t st; hipEvent_t a = nullptr; bool mk = false;
  TimeScope(mvae_ctx* c_, int r_, hipStream_t st_) : c(c_), r(r_), st(st_) {
    mk = r < (int)c->marker.size() && c->marker[r];
    if (mk) (void)launch_marker(r, st);
    if (c->timing && (c->timing_sel < 0 || c->timing_sel == r)) {
      a = take_event(c);
      (void)hipEventRecord(a, st);
    }
  }
  ~TimeScope() {
    if (a) {
      hipEvent_t b = take_event(c);
      (void)hipEventRecord(b, st);
      c->pending.push_back({r, a, b});
    }
    if (mk) (void)launch_marker(r, st);
  }
};
// a TimeScope of the named region over the rest of the block (ctx and st in scope)
#define MV_PASTE2(a, b) a##b
#define MV_PASTE(a, b) MV_PASTE2(a, b)
#define TIMED(name) TimeScope MV_PASTE(ts_, __LINE__)(ctx, region(ctx, name), st)
// ... over one checked launch alone
#define TIMED_CHECK(name, expr) do { TIMED(name); MV_CHECK(expr); } while (0)

static inline int run(mvae_ctx* ctx, const GemmDesc& d, hipStream_t st, int r = -1) {
  TimeScope ts(ctx, r < 0 ? region(ctx, "other_gemm") : r, st);
  const bool sd = st == ctx->side && ctx->side;
  float* ws = sd ? ctx->ws_side : ctx->ws;
  // descriptors name the pixel flag by its first slot; the last de-interleave raised dyn_cur
  if (ctx->dyn_cur && ctx->dyn_cur != ctx->dyn &&
      (d.dynA == ctx->dyn || d.epi.xdyn == ctx->dyn || d.anb == ctx->dyn + 2)) {
    GemmDesc dd = d;
    if (dd.dynA == ctx->dyn) dd.dynA = ctx->dyn_cur;
    if (dd.epi.xdyn == ctx->dyn) dd.epi.xdyn = ctx->dyn_cur;
    if (dd.epi.xnb == ctx->dyn + 2) dd.epi.xnb = ctx->dyn_cur + 2;
    if (dd.anb == ctx->dyn + 2) dd.anb = ctx->dyn_cur + 2;
    MV_CHECK(gemm_run(dd, ws, ctx->ws_elems, st));
    return MVAE_OK;
  }
  MV_CHECK(gemm_run(d, ws, ctx->ws_elems, st));
  return MVAE_OK;
}

// `to` waits for the work enqueued on `from` so far
static inline int stream_wait(mvae_ctx* ctx, hipStream_t from, hipStream_t to) {
  hipEvent_t ev = ctx->sync_ev[ctx->sync_next++ % ctx->sync_ev.size()];
  MV_CHECK(hipEventRecord(ev, from));
  MV_CHECK(hipStreamWaitEvent(to, ev, 0));
  return MVAE_OK;
}

// layer-0 weight-gradient chunks in use: the option's R, or fewer when the block has fewer rows
// than R chunks of 256 (chunk boundaries are tile multiples); the backward has that many + 2 parts
static inline int w0n(const mvae_ctx* c) { return c->w0_chunks == 1 ? 1 : (int)c->w0c[c->w0_chunks].size(); }
static inline int nparts(const mvae_ctx* c) { return w0n(c) + 2; }

// Adam's arguments for this step (TF ApplyAdam: lr_t = lr * sqrt(1 - beta2_power) /
// (1 - beta1_power), all fp32), the whole index range
static inline AdamArgs adam_args(const mvae_ctx* c) {
  AdamArgs a;
  a.theta = c->theta; a.g1 = c->grads; a.g2 = c->grads + c->n_all;
  a.m1 = c->adam; a.v1 = c->adam + c->n_all;
  a.m2 = c->adam + 2 * c->n_all; a.v2 = c->adam + 2 * c->n_all + c->n_enc;
  a.n_all = c->n_all; a.n_enc = c->n_enc;
  a.b1 = c->cfg.beta1; a.b2 = c->cfg.beta2; a.eps = c->cfg.epsilon;
  a.lr1 = (c->cfg.lr[0] * std::sqrt(1.f - c->b2p[0])) / (1.f - c->b1p[0]);
  a.lr2 = (c->cfg.lr[1] * std::sqrt(1.f - c->b2p[1])) / (1.f - c->b1p[1]);
  a.tp = planes_of(c, c->theta);
  a.nt = c->adam_nt;
  return a;
}
