// libmvae: retrieval (match*, pair_scores, match_merge) and the context-free batch and overlap
// helpers (make_batch*, overlap_*, rerank*).
#include "mvae_ctx.h"

// the match workspace holds at least `need` bytes (growing it waits for the whole device first)
static int match_ws_reserve(mvae_ctx* ctx, size_t need) {
  if (need <= ctx->match_ws_bytes) return MVAE_OK;
  if (ctx->match_ws) {  // (its last readers may still be queued, on this stream or another)
    MV_CHECK(hipDeviceSynchronize());
    MV_CHECK(hipFree(ctx->match_ws));
    ctx->match_ws = nullptr;
    ctx->match_ws_bytes = 0;
  }
  MV_CHECK(hipMalloc(&ctx->match_ws, need));
  ctx->match_ws_bytes = need;
  return MVAE_OK;
}

extern "C" int mvae_match(mvae_ctx* ctx, const float* zl, int64_t N, const float* zk, int64_t M, int k, int order,
                          float* dist_out, float* top_val, int* top_idx, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (!zl || !zk || !top_val || !top_idx) return fail(ctx, MVAE_EINVAL, "mvae_match: null zl, zk, top_val or top_idx");
  if (N < 1 || M < 1 || M > 0x7FFFFFFFll || N > (0x7FFFFFFFll << 6))
    return fail(ctx, MVAE_EINVAL, "mvae_match: N and M must be at least 1 (M below 2^31)");
  if (k < 1 || k > 64 || k > M) return fail(ctx, MVAE_EINVAL, "mvae_match: k must be in [1, min(M, 64)]");
  if (order != 1 && order != -1) return fail(ctx, MVAE_EINVAL, "mvae_match: order must be +1 or -1");
  hipStream_t st = (hipStream_t)stream;
  const int L = ctx->L;
  const bool cosine = ctx->cfg.metric == MVAE_METRIC_COSINE;
  long long split_len = 0;
  int splits = 1;
  match_plan(N, M, &split_len, &splits);
  // workspace: [per-split values | indices | chunk sums of zl, zk (doubles) | rl | rk]
  const size_t n_list = splits > 1 ? (size_t)N * splits * k : 0;
  const size_t pl = cosine ? (size_t)match_colnorm_chunks(N) * L : 0, pk = cosine ? (size_t)match_colnorm_chunks(M) * L : 0;
  const size_t o_idx = align64(n_list * 4), o_part = o_idx + align64(n_list * 4);
  const size_t o_r = o_part + align64((pl + pk) * 8), need = o_r + (cosine ? 2 * align64((size_t)L * 4) : 0);
  if (int rc = match_ws_reserve(ctx, need)) return rc;
  // (sqdiff in one split needs no workspace at all: ws may then be null and is not offset)
  char* ws = static_cast<char*>(ctx->match_ws);
  float* ws_val = n_list ? reinterpret_cast<float*>(ws) : nullptr;
  int* ws_idx = n_list ? reinterpret_cast<int*>(ws + o_idx) : nullptr;
  float* rl = nullptr;
  float* rk = nullptr;
  if (cosine) {
    TIMED("match_colnorm");
    double* part = reinterpret_cast<double*>(ws + o_part);
    rl = reinterpret_cast<float*>(ws + o_r);
    rk = reinterpret_cast<float*>(ws + o_r + align64((size_t)L * 4));
    MV_CHECK(launch_colnorm(zl, N, L, part, rl, st));
    MV_CHECK(launch_colnorm(zk, M, L, part + pl, rk, st));
  }
  TIMED_CHECK("match", launch_match(zl, N, zk, M, L, k, order, ctx->cfg.metric, ctx->cfg.reciprocal, rl, rk, split_len,
                                    splits, dist_out, ws_val, ws_idx, top_val, top_idx, st));
  return MVAE_OK;
}

extern "C" int mvae_match_colsq(mvae_ctx* ctx, const float* z, int64_t n, double* colsq, int accumulate,
                                void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (!z || !colsq) return fail(ctx, MVAE_EINVAL, "mvae_match_colsq: null z or colsq");
  if (n < 1 || n > (0xFFFFll << 8)) return fail(ctx, MVAE_EINVAL, "mvae_match_colsq: n must be in [1, 65535 * 256]");
  if (accumulate != 0 && accumulate != 1) return fail(ctx, MVAE_EINVAL, "mvae_match_colsq: accumulate must be 0 or 1");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = match_ws_reserve(ctx, (size_t)match_colnorm_chunks(n) * ctx->L * 8)) return rc;
  TIMED_CHECK("match_colnorm", launch_colsq(z, n, ctx->L, static_cast<double*>(ctx->match_ws), colsq, accumulate, st));
  return MVAE_OK;
}

extern "C" int mvae_match_rnorm(mvae_ctx* ctx, const double* colsq, float* rnorm, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (!colsq || !rnorm) return fail(ctx, MVAE_EINVAL, "mvae_match_rnorm: null colsq or rnorm");
  hipStream_t st = (hipStream_t)stream;
  TIMED_CHECK("match_colnorm", launch_rnorm(colsq, ctx->L, rnorm, st));
  return MVAE_OK;
}

extern "C" int mvae_match_ex(mvae_ctx* ctx, const float* zl, int64_t N, const float* zk, int64_t M, int k, int order,
                             const mvae_match_opts* opts, float* dist_out, float* top_val, int* top_idx,
                             void* stream) {
  if (!ctx) return MVAE_EINVAL;
  const mvae_match_opts none{};
  const mvae_match_opts& o = opts ? *opts : none;
  if (!zl || !zk || !top_val || !top_idx)
    return fail(ctx, MVAE_EINVAL, "mvae_match_ex: null zl, zk, top_val or top_idx");
  if (N < 1 || M < 1 || M > 0x7FFFFFFFll || N > (0x7FFFFFFFll << 6))
    return fail(ctx, MVAE_EINVAL, "mvae_match_ex: N and M must be at least 1 (M below 2^31)");
  if (k < 1 || k > 64) return fail(ctx, MVAE_EINVAL, "mvae_match_ex: k must be in [1, 64]");
  if (order != 1 && order != -1) return fail(ctx, MVAE_EINVAL, "mvae_match_ex: order must be +1 or -1");
  if (o.key_base < 0 || o.key_base > 0x7FFFFFFFll - M)
    return fail(ctx, MVAE_EINVAL, "mvae_match_ex: key_base must be >= 0 and key_base + M <= 2^31 - 1");
  if (o.carry != 0 && o.carry != 1) return fail(ctx, MVAE_EINVAL, "mvae_match_ex: carry must be 0 or 1");
  if (o.dist_ld < 0 || (o.dist_ld > 0 && o.dist_ld < M))
    return fail(ctx, MVAE_EINVAL, "mvae_match_ex: dist_ld must be 0 (= M) or at least M");
  const int nthr = (o.thr_val != nullptr) + (o.thr_idx != nullptr) + (o.ahead != nullptr);
  if (nthr != 0 && nthr != 3)
    return fail(ctx, MVAE_EINVAL, "mvae_match_ex: thr_val, thr_idx and ahead go together (all three or none)");
  hipStream_t st = (hipStream_t)stream;
  const int L = ctx->L;
  const bool cosine = ctx->cfg.metric == MVAE_METRIC_COSINE;
  const bool norm_l = cosine && !o.rl, norm_k = cosine && !o.rk;
  long long split_len = 0;
  int splits = 1;
  match_plan(N, M, &split_len, &splits);
  // workspace: [per-split values | indices | counts | chunk sums of zl, zk (doubles) | rl | rk]
  const bool merge = splits > 1 || o.carry;
  const size_t n_list = merge ? (size_t)N * splits * k : 0, n_cnt = merge && nthr ? (size_t)N * splits : 0;
  const size_t pl = norm_l ? (size_t)match_colnorm_chunks(N) * L : 0, pk = norm_k ? (size_t)match_colnorm_chunks(M) * L : 0;
  const size_t o_idx = align64(n_list * 4), o_cnt = o_idx + align64(n_list * 4), o_part = o_cnt + align64(n_cnt * 4);
  const size_t o_r = o_part + align64((pl + pk) * 8);
  const size_t need = o_r + (norm_l || norm_k ? 2 * align64((size_t)L * 4) : 0);
  if (int rc = match_ws_reserve(ctx, need)) return rc;
  char* ws = static_cast<char*>(ctx->match_ws);
  float* ws_val = n_list ? reinterpret_cast<float*>(ws) : nullptr;
  int* ws_idx = n_list ? reinterpret_cast<int*>(ws + o_idx) : nullptr;
  int* ws_cnt = n_cnt ? reinterpret_cast<int*>(ws + o_cnt) : nullptr;
  const float* rl = o.rl;
  const float* rk = o.rk;
  if (norm_l || norm_k) {
    TIMED("match_colnorm");
    double* part = reinterpret_cast<double*>(ws + o_part);
    if (norm_l) {
      float* r = reinterpret_cast<float*>(ws + o_r);
      MV_CHECK(launch_colnorm(zl, N, L, part, r, st));
      rl = r;
    }
    if (norm_k) {
      float* r = reinterpret_cast<float*>(ws + o_r + align64((size_t)L * 4));
      MV_CHECK(launch_colnorm(zk, M, L, part + pl, r, st));
      rk = r;
    }
  }
  TIMED_CHECK("match", launch_match_ex(zl, N, zk, M, L, k, order, ctx->cfg.metric, ctx->cfg.reciprocal, rl, rk, split_len,
                                       splits, dist_out, o.dist_ld ? o.dist_ld : M, o.key_base, o.carry, o.thr_val,
                                       o.thr_idx, o.ahead, ws_val, ws_idx, ws_cnt, top_val, top_idx, st));
  return MVAE_OK;
}

extern "C" int mvae_pair_scores(mvae_ctx* ctx, const float* zl, const float* zk, int64_t n, const float* rl,
                                const float* rk, float* out, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (!zl || !zk || !out) return fail(ctx, MVAE_EINVAL, "mvae_pair_scores: null zl, zk or out");
  if (n < 1 || n > (0xFFFFll << 8)) return fail(ctx, MVAE_EINVAL, "mvae_pair_scores: n must be in [1, 65535 * 256]");
  hipStream_t st = (hipStream_t)stream;
  const int L = ctx->L;
  const bool cosine = ctx->cfg.metric == MVAE_METRIC_COSINE;
  const bool norm_l = cosine && !rl, norm_k = cosine && !rk;
  if (norm_l || norm_k) {  // workspace: [chunk sums of zl, zk (doubles) | rl | rk]
    const size_t p = (size_t)match_colnorm_chunks(n) * L, o_r = align64(2 * p * 8);
    if (int rc = match_ws_reserve(ctx, o_r + 2 * align64((size_t)L * 4))) return rc;
    char* ws = static_cast<char*>(ctx->match_ws);
    double* part = reinterpret_cast<double*>(ws);
    TIMED("match_colnorm");
    if (norm_l) {
      float* r = reinterpret_cast<float*>(ws + o_r);
      MV_CHECK(launch_colnorm(zl, n, L, part, r, st));
      rl = r;
    }
    if (norm_k) {
      float* r = reinterpret_cast<float*>(ws + o_r + align64((size_t)L * 4));
      MV_CHECK(launch_colnorm(zk, n, L, part + p, r, st));
      rk = r;
    }
  }
  TIMED_CHECK("match_pair_scores", launch_pair_scores(zl, zk, n, L, ctx->cfg.metric, ctx->cfg.reciprocal, rl, rk, out, st));
  return MVAE_OK;
}

extern "C" int mvae_match_merge(mvae_ctx* ctx, const float* vals, const int* idx, int64_t N, int parts, int k,
                                int order, float* top_val, int* top_idx, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (!vals || !idx || !top_val || !top_idx)
    return fail(ctx, MVAE_EINVAL, "mvae_match_merge: null vals, idx, top_val or top_idx");
  if (N < 1 || N > (0x7FFFFFFFll << 2) || parts < 1)
    return fail(ctx, MVAE_EINVAL, "mvae_match_merge: N and parts must be at least 1");
  if (k < 1 || k > 64) return fail(ctx, MVAE_EINVAL, "mvae_match_merge: k must be in [1, 64]");
  if (order != 1 && order != -1) return fail(ctx, MVAE_EINVAL, "mvae_match_merge: order must be +1 or -1");
  hipStream_t st = (hipStream_t)stream;
  TIMED_CHECK("match", launch_match_merge(vals, idx, N, parts, k, order, 0, nullptr, 0, top_val, top_idx, nullptr, st));
  return MVAE_OK;
}

// ---- context-free helpers (errors through mvae_last_error(NULL))
extern "C" int mvae_make_batch(const unsigned char* locks, const unsigned char* keys, int height,
                               int width, const int* idx, const float* coef, int batch,
                               float divisor, float* x_out, void* stream) {
  if (!locks || !keys || !idx || !coef || !x_out || height <= 0 || width <= 0 || batch <= 0 ||
      !(divisor > 0.f))
    return fail(nullptr, MVAE_EINVAL, "mvae_make_batch: bad argument");
  if ((reinterpret_cast<uintptr_t>(coef) & 15) != 0)
    return fail(nullptr, MVAE_EINVAL, "mvae_make_batch: coef must be 16-byte aligned");
  MV_TRY(nullptr, "", launch_make_batch(locks, keys, height, width, idx, nullptr, coef, batch, divisor, x_out,
                                        (hipStream_t)stream));
  return MVAE_OK;
}

extern "C" int mvae_make_batch_x(const unsigned char* locks, const unsigned char* keys, int height, int width,
                                 const int* lock_idx, const int* key_idx, const float* coef, int batch,
                                 float divisor, float* x_out, void* stream) {
  if (!locks || !keys || !lock_idx || !coef || !x_out)
    return fail(nullptr, MVAE_EINVAL, "mvae_make_batch_x: null locks, keys, lock_idx, coef or x_out");
  if (height <= 0 || width <= 0 || batch <= 0)
    return fail(nullptr, MVAE_EINVAL, "mvae_make_batch_x: height, width and batch must be positive");
  if (!(divisor > 0.f)) return fail(nullptr, MVAE_EINVAL, "mvae_make_batch_x: divisor must be positive");
  if ((reinterpret_cast<uintptr_t>(coef) & 15) != 0)
    return fail(nullptr, MVAE_EINVAL, "mvae_make_batch_x: coef must be 16-byte aligned");
  MV_TRY(nullptr, "", launch_make_batch(locks, keys, height, width, lock_idx, key_idx, coef, batch, divisor, x_out,
                                        (hipStream_t)stream));
  return MVAE_OK;
}

extern "C" size_t mvae_overlap_work_bytes(int64_t count, int n_rot, int height, int width) {
  if (count < 1 || n_rot < 1 || n_rot > OVERLAP_MAX_ROT || height < 1 || height > 256 || width < 1 || width > 256)
    return 0;  // mvae_overlap_pairs refuses these arguments
  return overlap_work_bytes(count, n_rot);
}

extern "C" int mvae_overlap_pairs(const unsigned char* locks, const unsigned char* keys, int height, int width,
                                  const int* lock_idx, const int* key_idx, int64_t count, const float* coef,
                                  int n_rot, int* area_out, int* pose_out, void* work, void* stream) {
  if (!locks || !keys || !coef || !area_out)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_pairs: null locks, keys, coef or area_out");
  if (count < 1) return fail(nullptr, MVAE_EINVAL, "mvae_overlap_pairs: count must be at least 1");
  if (n_rot < 1 || n_rot > OVERLAP_MAX_ROT)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_pairs: n_rot must be in [1, 16777216]");
  if (height < 1 || height > 256 || width < 1 || width > 256)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_pairs: height and width must be in [1, 256]");
  if ((reinterpret_cast<uintptr_t>(coef) & 15) != 0)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_pairs: coef must be 16-byte aligned");
  if (!work && overlap_work_bytes(count, n_rot) != 0)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_pairs: work is null but mvae_overlap_work_bytes is not 0");
  if ((reinterpret_cast<uintptr_t>(work) & 7) != 0)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_pairs: work must be 8-byte aligned");
  MV_TRY(nullptr, "", launch_overlap_pairs(locks, keys, height, width, lock_idx, key_idx, count, coef, n_rot, area_out,
                                           pose_out, work, (hipStream_t)stream));
  return MVAE_OK;
}

extern "C" size_t mvae_rerank_work_bytes(int64_t N, int R, int n_rot, int height, int width) {
  if (N < 1 || N > RERANK_MAX_LOCKS || R < 1 || R > 64 || n_rot < 1 || n_rot > OVERLAP_MAX_ROT || height < 1 ||
      height > 256 || width < 1 || width > 256)
    return 0;  // mvae_rerank refuses these arguments
  return rerank_work_bytes(N, R, n_rot);
}

extern "C" int mvae_rerank(const unsigned char* locks, const unsigned char* keys, int height, int width,
                           const int* lock_idx, const int* cand, int64_t N, int R, const float* coef, int n_rot,
                           int* key_out, int* area_out, int* pose_out, int* from_out, void* work, void* stream) {
  if (!locks || !keys || !cand || !coef || !key_out || !area_out)
    return fail(nullptr, MVAE_EINVAL, "mvae_rerank: null locks, keys, cand, coef, key_out or area_out");
  if (N < 1 || N > RERANK_MAX_LOCKS) return fail(nullptr, MVAE_EINVAL, "mvae_rerank: N must be in [1, 2^31 - 1]");
  if (R < 1 || R > 64) return fail(nullptr, MVAE_EINVAL, "mvae_rerank: R must be in [1, 64]");
  if (n_rot < 1 || n_rot > OVERLAP_MAX_ROT)
    return fail(nullptr, MVAE_EINVAL, "mvae_rerank: n_rot must be in [1, 16777216]");
  if (height < 1 || height > 256 || width < 1 || width > 256)
    return fail(nullptr, MVAE_EINVAL, "mvae_rerank: height and width must be in [1, 256]");
  if ((reinterpret_cast<uintptr_t>(coef) & 15) != 0)
    return fail(nullptr, MVAE_EINVAL, "mvae_rerank: coef must be 16-byte aligned");
  if (!work) return fail(nullptr, MVAE_EINVAL, "mvae_rerank: work is null but mvae_rerank_work_bytes is not 0");
  if ((reinterpret_cast<uintptr_t>(work) & 7) != 0)
    return fail(nullptr, MVAE_EINVAL, "mvae_rerank: work must be 8-byte aligned");
  MV_TRY(nullptr, "", launch_rerank(locks, keys, height, width, lock_idx, cand, N, R, coef, n_rot, key_out, area_out,
                                    pose_out, from_out, work, (hipStream_t)stream));
  return MVAE_OK;
}

extern "C" int mvae_overlap_place(const unsigned char* locks, const unsigned char* keys, int height, int width,
                                  const int* lock_idx, const int* key_idx, int64_t count, const float* coef,
                                  int n_rot, const int* pose, unsigned char* overlay_out, int* stats_out,
                                  void* stream) {
  if (!locks || !keys || !coef || !pose)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_place: null locks, keys, coef or pose");
  if (!overlay_out && !stats_out)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_place: overlay_out and stats_out are both null");
  if (count < 1) return fail(nullptr, MVAE_EINVAL, "mvae_overlap_place: count must be at least 1");
  if (n_rot < 1 || n_rot > OVERLAP_MAX_ROT)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_place: n_rot must be in [1, 16777216]");
  if (height < 1 || height > 256 || width < 1 || width > 256)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_place: height and width must be in [1, 256]");
  if ((reinterpret_cast<uintptr_t>(coef) & 15) != 0)
    return fail(nullptr, MVAE_EINVAL, "mvae_overlap_place: coef must be 16-byte aligned");
  MV_TRY(nullptr, "", launch_overlap_place(locks, keys, height, width, lock_idx, key_idx, count, coef, n_rot, pose,
                                           overlay_out, stats_out, (hipStream_t)stream));
  return MVAE_OK;
}
