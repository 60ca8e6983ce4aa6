// libmvae C ABI: version / build id / last error, create and destroy, the views of the context's
// parameters and buffers, its counters and run-time options, gradient ranges and the timing API.
// The context itself: mvae_ctx.h; what creation plans: mvae_plan.cpp; the step: mvae_step.cpp.
#include <new>

#include "mvae_ctx.h"

std::string& mvae::create_err() {
  static thread_local std::string err;
  return err;
}

extern "C" {

int mvae_abi_version(void) { return MVAE_ABI_VERSION; }

#ifndef MVAE_BUILD_ID
#error "MVAE_BUILD_ID must be defined by the build (magic_amd/build.py source_hash)"
#endif
const char* mvae_build_id(void) { return MVAE_BUILD_ID; }

const char* mvae_last_error(mvae_ctx* ctx) { return ctx ? ctx->err.c_str() : create_err().c_str(); }

int mvae_destroy(mvae_ctx* ctx) {
  if (!ctx) return MVAE_EINVAL;
  int dev = 0;
  hipGetDevice(&dev);
  hipSetDevice(ctx->device);
  hipDeviceSynchronize();
  for (auto& pd : ctx->pending) { hipEventDestroy(pd.a); hipEventDestroy(pd.b); }
  for (auto e : ctx->event_pool) hipEventDestroy(e);
  for (auto e : ctx->sync_ev) hipEventDestroy(e);
  if (ctx->xbw_ev) hipEventDestroy(ctx->xbw_ev);
  if (ctx->side) hipStreamDestroy(ctx->side);
  for (void* p : ctx->allocs) hipFree(p);
  if (ctx->match_ws) hipFree(ctx->match_ws);
  hipSetDevice(dev);
  delete ctx;
  return MVAE_OK;
}

int mvae_create(const mvae_cfg* cfg, int device, mvae_ctx** out) { return mvae_create_ex(cfg, device, nullptr, out); }

int mvae_create_ex(const mvae_cfg* cfg, int device, const char* options, mvae_ctx** out) {
  if (!out) return fail(nullptr, MVAE_EINVAL, "out is NULL");
  *out = nullptr;
  int rc = validate(cfg);
  if (rc) return rc;
  CreateOpts opt;
  if ((rc = parse_opts(options, &opt))) return rc;
  mvae_ctx* ctx = new (std::nothrow) mvae_ctx();
  if (!ctx) return fail(nullptr, MVAE_EINVAL, "out of host memory");
  ctx->cfg = *cfg;
  ctx->device = device;
  if ((rc = plan_context(ctx, opt))) {  // the stage's error string stands; free what it left
    mvae_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return MVAE_OK;
}

int mvae_param_count(mvae_ctx* ctx) { return ctx ? 2 * ctx->nenc + 4 + 8 + (ctx->conv ? 4 : 0) : MVAE_EINVAL; }

int mvae_param_info(mvae_ctx* ctx, int kind, int index, mvae_tensor* out) {
  if (!ctx || !out) return MVAE_EINVAL;
  const int n = ctx->nenc;
  const int count = mvae_param_count(ctx);
  if (index < 0 || index >= count) return fail(ctx, MVAE_EINVAL, "param index out of range");
  std::memset(out, 0, sizeof(*out));
  const Block* cvb = nullptr;
  if (ctx->conv) {  // enc_conv1_W, enc_conv1_b, enc_conv2_W, enc_conv2_b come first
    if (index < 4) cvb = index < 2 ? &ctx->cv1 : &ctx->cv2;
    else index -= 4;
  }
  // resolve (name, block-relative pointer) in reference creation order (11a/vae.py:85-153)
  const Block* blk = nullptr;
  bool bias = false;
  int col0 = 0, cols = 0, ld = 0, enc_part = 0;
  std::string name;
  if (cvb) {
    blk = cvb;
    bias = index & 1;
    name = std::string(index < 2 ? "enc_conv1" : "enc_conv2") + (bias ? "_b" : "_W");
    cols = blk->N; ld = blk->ld; enc_part = 1;
  } else if (index < 2 * n) {
    const int i = index / 2;
    bias = index & 1;
    blk = &ctx->enc[i];
    name = "enc_h" + std::to_string(i) + (bias ? "_b" : "_W");
    cols = blk->N; ld = blk->ld; enc_part = 1;
  } else if (index < 2 * n + 4) {
    const int j = index - 2 * n;
    blk = &ctx->head;
    bias = j & 1;
    const bool logsig = j >= 2;
    name = std::string(logsig ? "enc_out_log_sigma" : "enc_out_mean") + (bias ? "_b" : "_W");
    col0 = logsig ? ctx->L : 0; cols = ctx->L; ld = blk->ld; enc_part = 1;
  } else if (index < 2 * n + 10) {
    const int j = index - 2 * n - 4;
    const Block* bl[3] = {&ctx->v1, &ctx->v2, &ctx->vo};
    const char* nm[3] = {"dec_h1", "dec_h2", "dec_out_mean"};
    blk = bl[j / 2];
    bias = j & 1;
    name = std::string(nm[j / 2]) + (bias ? "_b" : "_W");
    cols = blk->N; ld = blk->ld;
  } else {  // dead decoder log-sigma variables (11a/vae.py:147,153): allocated, never trained
    bias = (index - 2 * n - 10) == 1;
    std::strncpy(out->name, bias ? "dec_out_log_sigma_b" : "dec_out_log_sigma_W", sizeof(out->name) - 1);
    if (kind != MVAE_KIND_PARAM) return fail(ctx, MVAE_EINVAL, "dead variables have no optimizer state");
    out->data = ctx->dead + (bias ? (size_t)ctx->d1 * ctx->D : 0);
    out->rows = bias ? 1 : ctx->d1;
    out->cols = ctx->D;
    out->ld = ctx->D;
    out->trained_by = 0;
    return MVAE_OK;
  }
  std::strncpy(out->name, name.c_str(), sizeof(out->name) - 1);
  float* base = nullptr;
  switch (kind) {
    case MVAE_KIND_PARAM: base = ctx->theta; break;
    case MVAE_KIND_GRAD1: base = ctx->grads; break;
    case MVAE_KIND_GRAD2: base = enc_part ? ctx->grads + ctx->n_all : nullptr; break;
    case MVAE_KIND_M1: base = ctx->adam; break;
    case MVAE_KIND_V1: base = ctx->adam + ctx->n_all; break;
    case MVAE_KIND_M2: base = enc_part ? ctx->adam + 2 * ctx->n_all : nullptr; break;
    case MVAE_KIND_V2: base = enc_part ? ctx->adam + 2 * ctx->n_all + ctx->n_enc : nullptr; break;
    default: return fail(ctx, MVAE_EINVAL, "bad kind");
  }
  if (!base) return fail(ctx, MVAE_EINVAL, "decoder variables are not trained by the metric optimizer");
  out->data = base + blk->off + (bias ? (size_t)blk->K * ld : 0) + col0;
  out->rows = bias ? 1 : blk->K;
  out->cols = cols;
  out->ld = ld;
  out->trained_by = enc_part ? 3 : 1;
  return MVAE_OK;
}

int mvae_buffer(mvae_ctx* ctx, int which, float** ptr, size_t* count) {
  if (!ctx || !ptr || !count) return MVAE_EINVAL;
  switch (which) {
    case MVAE_BUF_PARAMS: *ptr = ctx->theta; *count = ctx->n_all; break;
    case MVAE_BUF_GRADS: *ptr = ctx->grads; *count = ctx->n_all + ctx->n_enc; break;
    case MVAE_BUF_ADAM: *ptr = ctx->adam; *count = 2 * ctx->n_all + 2 * ctx->n_enc; break;
    case MVAE_BUF_LOSSES: *ptr = ctx->losses; *count = 5; break;
    case MVAE_BUF_COLSQ: *ptr = ctx->colsq; *count = 2 * (size_t)ctx->L; break;
    case MVAE_BUF_COLDOT: *ptr = ctx->coldot; *count = ctx->L; break;
    case MVAE_BUF_DIST: *ptr = ctx->dist; *count = ctx->B; break;
    case MVAE_BUF_GRADS_DEC: *ptr = ctx->grads + ctx->n_enc; *count = ctx->n_all - ctx->n_enc; break;
    case MVAE_BUF_DEAD: *ptr = ctx->dead; *count = (size_t)ctx->d1 * ctx->D + ctx->D; break;
    case MVAE_BUF_EPS:
      if (ctx->eps_lazy) {  // the last forward's internal draw, written out on request
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess)
          e = launch_normal(ctx->eps, 3, ctx->B, ctx->L, ctx->le.Bg, ctx->le.off, ctx->le.seed,
                            ctx->le.counter, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return fail(ctx, (int)e, std::string("eps: ") + hipGetErrorString(e));
        ctx->eps_lazy = false;
      }
      *ptr = ctx->eps; *count = (size_t)3 * ctx->B * ctx->L; break;
    case MVAE_BUF_DYN:
      if (!ctx->dyn) return fail(ctx, MVAE_EINVAL, "no dyn flag in this precision mode");
      *ptr = reinterpret_cast<float*>(ctx->dyn_cur ? ctx->dyn_cur : ctx->dyn); *count = 1; break;
    default: return fail(ctx, MVAE_EINVAL, "bad buffer id");
  }
  return MVAE_OK;
}

int mvae_get_step(mvae_ctx* ctx, int64_t* t1, int64_t* t2) {
  if (!ctx || !t1 || !t2) return MVAE_EINVAL;
  *t1 = ctx->t1; *t2 = ctx->t2;
  return MVAE_OK;
}

int mvae_set_step(mvae_ctx* ctx, int64_t t1, int64_t t2) {
  if (!ctx || t1 < 0 || t2 < 0) return MVAE_EINVAL;
  ctx->t1 = t1; ctx->t2 = t2;
  // recompute the fp32 beta powers exactly as TF accumulates them (one fp32 multiply per step)
  for (int o = 0; o < 2; ++o) {
    const int64_t t = o == 0 ? t1 : t2;
    float b1p = ctx->cfg.beta1, b2p = ctx->cfg.beta2;
    for (int64_t s = 0; s < t; ++s) { b1p *= ctx->cfg.beta1; b2p *= ctx->cfg.beta2; }
    ctx->b1p[o] = b1p; ctx->b2p[o] = b2p;
  }
  return MVAE_OK;
}

int mvae_get_rng(mvae_ctx* ctx, uint64_t* train, uint64_t* eval) {
  if (!ctx || !train || !eval) return MVAE_EINVAL;
  *train = ctx->rng_counter; *eval = ctx->rng_eval;
  return MVAE_OK;
}

int mvae_set_rng(mvae_ctx* ctx, uint64_t train, uint64_t eval) {
  if (!ctx || (train | eval) & EVAL_STREAM) return MVAE_EINVAL;
  ctx->rng_counter = train; ctx->rng_eval = eval;
  return MVAE_OK;
}

int mvae_set_shard(mvae_ctx* ctx, int64_t row_offset) {
  if (!ctx) return MVAE_EINVAL;
  if (row_offset < 0 || row_offset + ctx->B > ctx->cfg.global_batch)
    return fail(ctx, MVAE_EINVAL, "row_offset outside [0, global_batch - batch]");
  ctx->row_off = (int)row_offset;
  return MVAE_OK;
}

int mvae_sync_params(mvae_ctx* ctx, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  MV_CHECK(launch_split_planes(ctx->theta, ctx->n_all, planes_of(ctx, ctx->theta), (hipStream_t)stream));
  return MVAE_OK;
}

}  // extern "C"

extern "C" int mvae_set_option(mvae_ctx* ctx, const char* name, int value) {
  if (!ctx || !name) return MVAE_EINVAL;
  const std::string k(name);
  if (k == "side_stream") {
    // not while forked weight gradients are still un-joined (mid-backward)
    if (ctx->side_pending)
      return fail(ctx, MVAE_ESTATE, "side_stream cannot change while side-stream work is pending");
    ctx->use_side = value != 0;
    return MVAE_OK;
  }
  if (k == "bce_split") {
    ctx->use_split = value != 0;
    return MVAE_OK;
  }
  if (k == "side_mask") {
    if (value < 0 || value > 3) return fail(ctx, MVAE_EINVAL, "side_mask must be in [0, 3]");
    if (ctx->phase == 4) return fail(ctx, MVAE_ESTATE, "side_mask cannot change mid-backward");
    ctx->side_mask = value;
    return MVAE_OK;
  }
  if (k == "early_adam") {
    // only for callers that do not touch the gradients between mvae_backward and mvae_adam (no
    // all-reduce): the side stream reads them as soon as the backward has written them. Taken by
    // mvae_backward only; the per-part API (mvae_backward_part, the all-reduce path) ignores it
    if (ctx->phase == 4) return fail(ctx, MVAE_ESTATE, "early_adam cannot change mid-backward");
    ctx->early_adam = value != 0;
    return MVAE_OK;
  }
  if (k == "early_chunks" || k == "wgrad0_chunks") {
    if (value != 1 && value != 2 && value != 4 && value != 8) return fail(ctx, MVAE_EINVAL, k + " must be 1, 2, 4 or 8");
    if (ctx->phase == 4) return fail(ctx, MVAE_ESTATE, k + " cannot change mid-backward");
    (k == "early_chunks" ? ctx->early_chunks : ctx->w0_chunks) = value;
    return MVAE_OK;
  }
  return fail(ctx, MVAE_EINVAL, "unknown option " + k);
}

// The ranges of grads [g1 (n_all) | g2 (n_enc)] that part `part` finishes: part 0 the decoder
// slice of g1; parts 1 .. R the layer-0 rows of chunk part-1 in g1 and in g2 (the last chunk up
// to the end of the layer-0 block, plus the conv-tower blocks in front of it); part R + 1 the
// rest of the encoder slice in g1 and g2. Together they cover grads exactly once.
extern "C" int mvae_grad_range(mvae_ctx* ctx, int part, int index, float** ptr, size_t* count) {
  if (!ctx || !ptr || !count) return MVAE_EINVAL;
  const int R = w0n(ctx);
  const Block& b0 = ctx->enc[0];
  const size_t l1 = ctx->nenc > 1 ? ctx->enc[1].off : ctx->head.off;  // end of the layer-0 block
  float* g1 = ctx->grads;
  float* g2 = ctx->grads + ctx->n_all;
  std::vector<std::pair<float*, size_t>> r;
  if (part == 0) {
    r.push_back({g1 + ctx->n_enc, ctx->n_all - ctx->n_enc});
  } else if (part >= 1 && part <= R) {
    const int m0 = R == 1 ? 0 : ctx->w0m[ctx->w0_chunks][part - 1];
    const int m1 = R == 1 ? b0.K + 1 : ctx->w0m[ctx->w0_chunks][part];
    const size_t a = b0.off + (size_t)m0 * b0.ld;
    const size_t e = part == R ? l1 : b0.off + (size_t)m1 * b0.ld;
    for (float* g : {g1, g2}) r.push_back({g + a, e - a});
    if (part == R && b0.off > 0)  // conv-tower blocks / leading alignment
      for (float* g : {g1, g2}) r.push_back({g, b0.off});
  } else if (part == R + 1) {
    for (float* g : {g1, g2}) r.push_back({g + l1, ctx->n_enc - l1});
  }
  if (index < 0 || index >= (int)r.size()) return MVAE_EINVAL;
  *ptr = r[index].first;
  *count = r[index].second;
  return MVAE_OK;
}

extern "C" int mvae_timing_enable(mvae_ctx* ctx, int on) {
  if (!ctx) return MVAE_EINVAL;
  ctx->timing = on != 0;
  return MVAE_OK;
}

extern "C" int mvae_timing_select(mvae_ctx* ctx, int region) {
  if (!ctx || region < -1 || region >= (int)ctx->region_names.size()) return MVAE_EINVAL;
  ctx->timing_sel = region;
  return MVAE_OK;
}

extern "C" int mvae_timing_marker(mvae_ctx* ctx, int region, int on) {
  if (!ctx || region < 0 || region >= (int)ctx->region_names.size()) return MVAE_EINVAL;
  if ((int)ctx->marker.size() < (int)ctx->region_names.size()) ctx->marker.resize(ctx->region_names.size(), 0);
  ctx->marker[region] = on != 0;
  return MVAE_OK;
}

extern "C" int mvae_timing_regions(mvae_ctx* ctx) {
  return ctx ? (int)ctx->region_names.size() : MVAE_EINVAL;
}

extern "C" const char* mvae_timing_name(mvae_ctx* ctx, int r) {
  if (!ctx || r < 0 || r >= (int)ctx->region_names.size()) return nullptr;
  return ctx->region_names[r].c_str();
}

static int collect(mvae_ctx* ctx) {
  for (auto& pd : ctx->pending) {
    MV_CHECK(hipEventSynchronize(pd.b));
    float ms = 0.f;
    MV_CHECK(hipEventElapsedTime(&ms, pd.a, pd.b));
    ctx->region_ms[pd.region] += ms;
    ctx->region_n[pd.region] += 1;
    ctx->event_pool.push_back(pd.a);
    ctx->event_pool.push_back(pd.b);
  }
  ctx->pending.clear();
  return MVAE_OK;
}

extern "C" int mvae_timing_read(mvae_ctx* ctx, int r, double* total_ms, int64_t* count) {
  if (!ctx || !total_ms || !count || r < 0 || r >= (int)ctx->region_names.size()) return MVAE_EINVAL;
  int rc = collect(ctx);
  if (rc) return rc;
  *total_ms = ctx->region_ms[r];
  *count = ctx->region_n[r];
  return MVAE_OK;
}

extern "C" int mvae_timing_reset(mvae_ctx* ctx) {
  if (!ctx) return MVAE_EINVAL;
  int rc = collect(ctx);
  if (rc) return rc;
  std::fill(ctx->region_ms.begin(), ctx->region_ms.end(), 0.0);
  std::fill(ctx->region_n.begin(), ctx->region_n.end(), 0);
  return MVAE_OK;
}

