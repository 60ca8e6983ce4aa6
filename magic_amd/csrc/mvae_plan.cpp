// libmvae: what mvae_create_ex plans -- configuration and option checks, then plan_context, which
// builds the context in named stages (parameter layout, buffers, the GEMM schedule and its wiring,
// the per-configuration kernel decisions, workspace, streams). Every stage reports through
// fail(nullptr, ...) and returns; mvae_create_ex owns the one cleanup exit. The order of the
// allocations and of the region() registrations is part of the plan: buffer placement affects
// channel / cache behaviour and region ids are visible through mvae_timing_name.
#include "mvae_ctx.h"

int mvae::validate(const mvae_cfg* cfg) {
  if (!cfg) return fail(nullptr, MVAE_EINVAL, "cfg is NULL");
  if (cfg->image_size <= 0 || cfg->batch <= 0 || cfg->latent <= 0)
    return fail(nullptr, MVAE_ECONFIG, "image_size, batch and latent must be positive");
  if (cfg->global_batch < cfg->batch) return fail(nullptr, MVAE_ECONFIG, "global_batch < batch");
  if (cfg->n_enc < 1 || cfg->n_enc > MVAE_MAX_ENC) return fail(nullptr, MVAE_ECONFIG, "n_enc out of range");
  for (int i = 0; i < cfg->n_enc; ++i)
    if (cfg->enc[i] <= 0) return fail(nullptr, MVAE_ECONFIG, "encoder width must be positive");
  if (cfg->dec[0] <= 0 || cfg->dec[1] <= 0) return fail(nullptr, MVAE_ECONFIG, "decoder widths must be positive");
  if (cfg->act != MVAE_ACT_TANH && cfg->act != MVAE_ACT_ELU) return fail(nullptr, MVAE_ECONFIG, "bad act");
  if (cfg->metric != MVAE_METRIC_COSINE && cfg->metric != MVAE_METRIC_SQDIFF)
    return fail(nullptr, MVAE_ECONFIG, "bad metric");
  if (cfg->precision != MVAE_PREC_F32 && cfg->precision != MVAE_PREC_BF16 &&
      cfg->precision != MVAE_PREC_F32X)
    return fail(nullptr, MVAE_ECONFIG, "bad precision");
  if (cfg->conv != 0 && cfg->conv != 1) return fail(nullptr, MVAE_ECONFIG, "conv must be 0 or 1");
  // conv tower: sizes up to BASELINE's 100 x 100 are the tested range (tests/test_gpu_conv.py);
  // larger images would need > 64 KB of dynamic LDS in the conv2 MFMA kernels, never run
  if (cfg->conv && (cfg->image_size % 4 != 0 || cfg->image_size > 100))
    return fail(nullptr, MVAE_ECONFIG, "conv encoder: image_size must be a multiple of 4 (<= 100)");
  const long long D = (long long)cfg->image_size * cfg->image_size;
  if (D * 3 * cfg->batch > (1LL << 31) - 1 || 3LL * cfg->batch * (D + 4) > (1LL << 31) * 8)
    return fail(nullptr, MVAE_ECONFIG, "batch too large for 32-bit row indexing");
  return MVAE_OK;
}

int mvae::parse_opts(const char* s, CreateOpts* o) {
  if (!s) return MVAE_OK;
  std::string all(s);
  size_t i = 0;
  while (i < all.size()) {
    size_t j = all.find(',', i);
    if (j == std::string::npos) j = all.size();
    const std::string kv = all.substr(i, j - i);
    i = j + 1;
    if (kv.empty()) continue;
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return fail(nullptr, MVAE_EINVAL, "option without '=': " + kv);
    const std::string k = kv.substr(0, eq);
    char* end = nullptr;
    const long v = std::strtol(kv.c_str() + eq + 1, &end, 10);
    if (end == kv.c_str() + eq + 1 || *end) return fail(nullptr, MVAE_EINVAL, "option value not an integer: " + kv);
    auto in = [&](long lo, long hi) { return v >= lo && v <= hi; };
    if (k == "e8" && in(0, 2)) o->e8 = (int)v;
    else if (k == "thin_ring" && in(0, 2)) o->thin_ring = (int)v;
    else if (k == "valu" && in(0, 1)) o->valu = (int)v;
    else if (k == "dact_planes" && in(0, 1)) o->dact_planes = (int)v;
    else if (k == "bce_split" && in(0, 1)) o->bce_split = (int)v;
    else if (k == "plan_log" && in(0, 1)) o->plan_log = (int)v;
    else if (k == "enc_chain" && in(0, 1)) o->enc_chain = (int)v;
    else if (k == "dec_chain" && in(0, 1)) o->dec_chain = (int)v;
    else if (k == "bits" && in(0, 1)) o->bits = (int)v;
    else if (k == "bits_reg" && in(0, 1)) o->bits_reg = (int)v;
    else if (k == "adam_nt" && in(0, 1)) o->adam_nt = (int)v;
    else if (k == "xbw_split" && in(0, 2)) o->xbw_split = (int)v;
    else if (k == "cs_one" && in(0, 2)) o->cs_one = (int)v;
    else if (k == "x3" && in(0, 2)) o->x3 = (int)v;
    else if (k == "enc_chain_rows" && (v == 0 || (in(16, 96) && v % 16 == 0))) o->enc_chain_rows = (int)v;
    else if (k == "conv2_nchunk" && in(0, 1 << 20)) o->conv2_nchunk = (int)v;
    else return fail(nullptr, MVAE_EINVAL, "unknown option or value out of range: " + kv);
  }
  return MVAE_OK;
}

namespace {

// `count` elements of T on the device, zero-filled, freed by mvae_destroy. The size is rounded up
// to whole 4-byte words (at least one), as every buffer of the context has always been sized.
template <class T>
hipError_t dalloc(mvae_ctx* ctx, T** p, size_t count) {
  const size_t bytes = std::max<size_t>((count * sizeof(T) + 3) / 4, 1) * 4;
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return e;
  ctx->allocs.push_back(q);
  *p = static_cast<T*>(q);
  return hipMemset(q, 0, bytes);
}

// stage-local checks: record the error of a failed allocation / HIP call and leave the stage
#define PLAN_ALLOC(p, n) MV_TRY(nullptr, "hipMalloc " #p ": ", dalloc(c, &(p), (n)))
#define PLAN_HIP(what, expr) MV_TRY(nullptr, what ": ", expr)

// Every GEMM of the schedule with its timing region, in the order the step runs them: the encoder
// forward and head, the decoder forward, the decoder and encoder backward, the conv tower's feature
// gradient. (f_out_a / f_out_b and the w0c chunks are copies made from these after the wiring.)
template <class F>
void for_each_gemm(mvae_ctx* c, F fn) {
  for (size_t i = 0; i < c->fwd_enc.size(); ++i) fn(c->fwd_enc[i], c->fwd_enc_r[i]);
  fn(c->f_d1, c->f_d1_r);
  fn(c->f_d2, c->f_d2_r);
  fn(c->f_out, c->f_out_r);
  for (size_t i = 0; i < c->bwd_dec.size(); ++i) fn(c->bwd_dec[i], c->bwd_dec_r[i]);
  for (size_t i = 0; i < c->bwd_enc.size(); ++i) fn(c->bwd_enc[i], c->bwd_enc_r[i]);
  if (c->conv) fn(c->bwd_feat, c->bwd_feat_r);
}

bool in_xs(const mvae_ctx* c, const float* p) { return p >= c->xs && p < c->xs + (size_t)3 * c->B * c->ldx; }
// a GEMM on the 256-row bf16-plane kernels
bool plane_kernel(const GemmDesc& d) { return gemm_wide_kernel(gemm_plan(d, ~size_t(0)).kernel); }

int layout_params(mvae_ctx* c, const CreateOpts&) {
  const mvae_cfg* cfg = &c->cfg;
  c->B = cfg->batch; c->D = cfg->image_size * cfg->image_size; c->L = cfg->latent;
  c->nenc = cfg->n_enc; c->d0 = cfg->dec[0]; c->d1 = cfg->dec[1];
  c->inv_bg = 1.f / (float)cfg->global_batch;
  c->b1p[0] = c->b1p[1] = cfg->beta1;
  c->b2p[0] = c->b2p[1] = cfg->beta2;
  // ---- parameter layout
  size_t off = 0;
  auto place = [&](Block& b, int K, int N) {  // the next [W; b] block: (K + 1) rows of round8(N)
    b.off = off; b.K = K; b.N = N; b.ld = round8(N);
    off = align64(off + (size_t)(K + 1) * b.ld);
  };
  int fan_in = c->D;
  c->conv = cfg->conv != 0;
  if (c->conv) {
    const int S = cfg->image_size;
    c->tower.S = S; c->tower.S1 = S / 2; c->tower.S2 = S / 4;
    place(c->cv1, 25, 64);
    place(c->cv2, 25 * 64, 64);
    c->F = c->tower.S2 * c->tower.S2 * 64;
    c->ldf = round8(c->F + 1);
    fan_in = c->F;
  }
  c->enc.resize(c->nenc);
  for (int i = 0; i < c->nenc; ++i) {
    place(c->enc[i], fan_in, cfg->enc[i]);
    fan_in = cfg->enc[i];
  }
  place(c->head, fan_in, 2 * c->L);
  c->n_enc = off;
  place(c->v1, c->L, c->d0);
  place(c->v2, c->d0, c->d1);
  place(c->vo, c->d1, c->D);
  c->n_all = off;
  // ---- strides
  c->ldx = round8(c->D + 1);
  c->ldz = round8(c->L + 1);
  c->ld_d1 = round8(c->d0 + 1);
  c->ld_d2 = round8(c->d1 + 1);
  c->ld_u = round8(c->D);
  c->ld_dh = round8(2 * c->L);
  int maxe = 0;
  for (int i = 0; i < c->nenc; ++i) {
    c->ldh.push_back(round8(cfg->enc[i] + 1));
    maxe = std::max(maxe, cfg->enc[i]);
  }
  c->lddz = round8(maxe);
  c->nblk = gemm_bce_nblk(c->D);
  c->nchunk = colstats_nchunk(c->B);
  return MVAE_OK;
}

int alloc_buffers(mvae_ctx* c, const CreateOpts& opt) {
  const size_t B = c->B, L = c->L;
  PLAN_ALLOC(c->theta, c->n_all);
  PLAN_ALLOC(c->grads, c->n_all + c->n_enc);
  PLAN_ALLOC(c->adam, 2 * c->n_all + 2 * c->n_enc);
  PLAN_ALLOC(c->dead, (size_t)c->d1 * c->D + c->D);
  PLAN_ALLOC(c->xs, 3 * B * c->ldx);
  c->H.resize(c->nenc);
  for (int i = 0; i < c->nenc; ++i) PLAN_ALLOC(c->H[i], 3 * B * c->ldh[i]);
  PLAN_ALLOC(c->ms, 3 * B * 2 * L);
  PLAN_ALLOC(c->z, 3 * B * c->ldz);
  PLAN_ALLOC(c->zgen, B * c->ldz);
  PLAN_ALLOC(c->a1, B * c->ld_d1);
  PLAN_ALLOC(c->a2, B * c->ld_d2);
  PLAN_ALLOC(c->du, B * c->ld_u);
  PLAN_ALLOC(c->rowpart, B * c->nblk);
  PLAN_ALLOC(c->rowvals, 4 * B);
  PLAN_ALLOC(c->dist, B);
  PLAN_ALLOC(c->draw, B);
  PLAN_ALLOC(c->losses, 8);
  PLAN_ALLOC(c->colsq, 2 * L);
  PLAN_ALLOC(c->coldot, L);
  PLAN_ALLOC(c->cspart, (size_t)c->nchunk * 2 * L);
  if (opt.cs_one == 1 || (opt.cs_one == 2 && L <= 32)) PLAN_ALLOC(c->cscnt, (2 * L + 63) / 64);
  PLAN_ALLOC(c->eps, 3 * B * L);
  PLAN_ALLOC(c->rowfwd, 4 * B);
  PLAN_ALLOC(c->dzd2, B * c->ld_d2);
  PLAN_ALLOC(c->dzd1, B * c->ld_d1);
  PLAN_ALLOC(c->dzdec, B * L);
  PLAN_ALLOC(c->dhead, 4 * B * c->ld_dh);
  c->dzl.resize(c->nenc);
  for (int i = 0; i < c->nenc; ++i) PLAN_ALLOC(c->dzl[i], 4 * B * c->lddz);
  return MVAE_OK;
}

int alloc_tower(mvae_ctx* c, const CreateOpts& opt) {
  if (!c->conv) return MVAE_OK;
  ConvTower& T = c->tower;
  const size_t B = c->B;
  const size_t a1 = (size_t)T.S1 * T.S1 * 64, a2n = (size_t)T.S2 * T.S2 * 64;
  T.mfma = c->cfg.precision == MVAE_PREC_BF16;
  PLAN_ALLOC(c->xf, 3 * B * c->ldf);
  PLAN_ALLOC(c->dxf, 4 * B * c->ldf);
  PLAN_ALLOC(T.p1, 3 * B * a1);
  if (!T.mfma) PLAN_ALLOC(T.n1, 3 * B * a1);   // the MFMA kernels read the bf16 images only
  PLAN_ALLOC(T.a2, 3 * B * a1);
  if (!T.mfma) PLAN_ALLOC(T.da2, 4 * B * a1);
  PLAN_ALLOC(T.dn1, 4 * B * a1);
  PLAN_ALLOC(T.arg1, 3 * B * a1);
  PLAN_ALLOC(T.arg2, 3 * B * a2n);
  if (T.mfma) {
    PLAN_ALLOC(T.n1b, 3 * B * a1);
    PLAN_ALLOC(T.da2b, 4 * B * a1);
    PLAN_ALLOC(T.w2f, 25 * 64 * 64);
    PLAN_ALLOC(T.w2d, 25 * 64 * 64);
  }
  const int B2 = 2 * (int)B;
  T.nchunk1 = std::min(B2, 1024);
  T.nchunk2 = std::min(B2, 32);
  // image chunks of the MFMA weight gradient: 64 -> 256 workgroups at C5CONV, one per CU
  // (same box: 1.085 ms vs 1.11 at 128 and 1.17 at 256, profiles/r2/conv2_wgrad_ab.txt)
  T.nchunk2m = std::min(B2, 64);
  if (opt.conv2_nchunk > 0) T.nchunk2m = std::min(B2, opt.conv2_nchunk);
  const size_t s1 = (size_t)2 * T.nchunk1 * 26 * 64;
  const size_t s2 = (size_t)2 * (T.mfma ? T.nchunk2m : T.nchunk2) * (25 * 64 + 1) * 64;
  PLAN_ALLOC(T.slab, std::max(s1, s2));
  return MVAE_OK;
}

// constant ones columns (bias folding)
int write_ones_columns(mvae_ctx* c, const CreateOpts&) {
  const int B = c->B;
  const std::vector<float> one(3 * B, 1.f);
  auto ones_column = [&](float* base, int ld, int col, int rows) {
    return hipMemcpy2D(base + col, (size_t)ld * sizeof(float), one.data(), sizeof(float), sizeof(float),
                       rows, hipMemcpyHostToDevice);
  };
  PLAN_HIP("ones column", ones_column(c->xs, c->ldx, c->D, 3 * B));
  if (c->conv) PLAN_HIP("ones column", ones_column(c->xf, c->ldf, c->F, 3 * B));
  for (int i = 0; i < c->nenc; ++i) PLAN_HIP("ones column", ones_column(c->H[i], c->ldh[i], c->cfg.enc[i], 3 * B));
  PLAN_HIP("ones column", ones_column(c->z, c->ldz, c->L, 3 * B));
  PLAN_HIP("ones column", ones_column(c->zgen, c->ldz, c->L, B));
  PLAN_HIP("ones column", ones_column(c->a1, c->ld_d1, c->d0, B));
  PLAN_HIP("ones column", ones_column(c->a2, c->ld_d2, c->d1, B));
  return MVAE_OK;
}

int build_schedule(mvae_ctx* c, const CreateOpts&) {
  const int B = c->B, L = c->L, n = c->nenc, act = c->cfg.act;
  float* th = c->theta;
  float* g1 = c->grads;
  const long long n_all = (long long)c->n_all;
  // ---- forward: encoder on the stacked 3B rows
  c->fwd_enc.clear();
  const float* X0 = c->conv ? c->xf : c->xs;   // layer-0 operand: pixels or tower features
  const int ld0 = c->conv ? c->ldf : c->ldx;
  for (int i = 0; i < n; ++i) {
    const float* A = i == 0 ? X0 : c->H[i - 1];
    const int lda = i == 0 ? ld0 : c->ldh[i - 1];
    GemmDesc d = gd(3 * B, c->enc[i].N, c->enc[i].K + 1, A, lda, false, th + c->enc[i].off,
                    c->enc[i].ld, false, c->H[i], c->ldh[i], EPI_ACT);
    d.epi.act = act;
    d.epi.padw = 2;  // H[i]: the ones column at N, zeros beyond
    c->fwd_enc.push_back(d);
    c->fwd_enc_r.push_back(region(c, "enc_fwd_" + std::to_string(i)));
  }
  c->fwd_enc.push_back(gd(3 * B, 2 * L, c->head.K + 1, c->H[n - 1], c->ldh[n - 1], false,
                          th + c->head.off, c->head.ld, false, c->ms, 2 * L));
  c->fwd_enc_r.push_back(region(c, "head_fwd"));
  c->f_d1_r = region(c, "dec_fwd_1");
  c->f_d2_r = region(c, "dec_fwd_2");
  c->f_out_r = region(c, "dec_fwd_out_bce");
  for (const char* nm : {"dec_bwd_w_out", "dec_bwd_d_out", "dec_bwd_w_2", "dec_bwd_d_2", "dec_bwd_w_1",
                         "dec_bwd_d_z"})
    c->bwd_dec_r.push_back(region(c, nm));
  // ---- decoder on the lock rows
  c->f_d1 = gd(B, c->d0, L + 1, c->z + (size_t)B * c->ldz, c->ldz, false, th + c->v1.off, c->v1.ld,
               false, c->a1, c->ld_d1, EPI_ACT);
  c->f_d1.epi.act = act;
  c->f_d1.epi.padw = 2;
  c->f_d2 = gd(B, c->d1, c->d0 + 1, c->a1, c->ld_d1, false, th + c->v2.off, c->v2.ld, false, c->a2,
               c->ld_d2, EPI_ACT);
  c->f_d2.epi.act = act;
  c->f_d2.epi.padw = 2;
  c->f_out = gd(B, c->D, c->d1 + 1, c->a2, c->ld_d2, false, th + c->vo.off, c->vo.ld, false, c->du,
                c->ld_u, EPI_BCE);
  c->f_out.epi.x = c->xs + (size_t)B * c->ldx;
  c->f_out.epi.ldx = c->ldx;
  c->f_out.epi.scale = c->inv_bg;
  c->f_out.epi.rowpart = c->rowpart;
  // ---- decoder backward (g1 only)
  c->bwd_dec.clear();
  c->bwd_dec.push_back(gd(c->d1 + 1, c->D, B, c->a2, c->ld_d2, true, c->du, c->ld_u, false,
                          g1 + c->vo.off, c->vo.ld));
  GemmDesc dout = gd(B, c->d1, c->D, c->du, c->ld_u, false, th + c->vo.off, c->vo.ld, true, c->dzd2,
                     c->ld_d2, EPI_DACT);
  dout.epi.act = act; dout.epi.aux = c->a2; dout.epi.ld_aux = c->ld_d2; dout.epi.padw = 1;
  c->bwd_dec.push_back(dout);
  c->bwd_dec.push_back(gd(c->d0 + 1, c->d1, B, c->a1, c->ld_d1, true, c->dzd2, c->ld_d2, false,
                          g1 + c->v2.off, c->v2.ld));
  GemmDesc dd2 = gd(B, c->d0, c->d1, c->dzd2, c->ld_d2, false, th + c->v2.off, c->v2.ld, true, c->dzd1,
                    c->ld_d1, EPI_DACT);
  dd2.epi.act = act; dd2.epi.aux = c->a1; dd2.epi.ld_aux = c->ld_d1; dd2.epi.padw = 1;
  c->bwd_dec.push_back(dd2);
  c->bwd_dec.push_back(gd(L + 1, c->d0, B, c->z + (size_t)B * c->ldz, c->ldz, true, c->dzd1,
                          c->ld_d1, false, g1 + c->v1.off, c->v1.ld));
  c->bwd_dec.push_back(gd(B, L, c->d0, c->dzd1, c->ld_d1, false, th + c->v1.off, c->v1.ld, true,
                          c->dzdec, L));
  // ---- encoder backward: g1 over rows [rot|lock], g2 over [lock|key] (batched GEMMs).
  // Part 1 runs the dgrad chain (head -> layer 1) and then the big layer-0 weight gradient;
  // part 2 the small weight gradients of the head and hidden layers. Each part ends with a
  // set of finished gradient ranges (the all-reduce buckets of mvae_grad_range), so a data-
  // parallel host overlaps the decoder and layer-0 all-reduces with the remaining work.
  c->bwd_enc.clear();
  c->bwd_enc_r.clear();
  auto dgrad = [&](int i) {  // dZ_{i-1} = (dZ_i W_i^T) * act'(H_{i-1}); i == n: the head
    const bool head = i == n;
    const Block& blk = head ? c->head : c->enc[i];
    const float* src = head ? c->dhead : c->dzl[i];
    const int lds = head ? c->ld_dh : c->lddz;
    GemmDesc d = gd(4 * B, blk.K, blk.N, src, lds, false, th + blk.off, blk.ld, true, c->dzl[i - 1],
                    c->lddz, EPI_DACT);
    d.epi.act = act; d.epi.aux = c->H[i - 1]; d.epi.ld_aux = c->ldh[i - 1];
    d.epi.remap_split = 2 * B; d.epi.remap_shift = B;
    d.epi.padw = 1;  // dZ rows: zero padding
    c->bwd_enc.push_back(d);
    c->bwd_enc_r.push_back(region(c, head ? std::string("head_bwd_d") : "enc_bwd_d_" + std::to_string(i)));
  };
  auto wgrad = [&](int i) {  // [W_i; b_i] gradients (g1 and g2 as one batch-2 GEMM); i == n: head
    const bool head = i == n;
    const Block& blk = head ? c->head : c->enc[i];
    const float* A = i == 0 ? X0 : c->H[i - 1];
    const int lda = i == 0 ? ld0 : c->ldh[i - 1];
    const float* src = head ? c->dhead : c->dzl[i];
    const int lds = head ? c->ld_dh : c->lddz;
    GemmDesc w = gd(blk.K + 1, blk.N, 2 * B, A, lda, true, src, lds, false, g1 + blk.off, blk.ld);
    w.batch = 2; w.sA = (long long)B * lda; w.sB = (long long)2 * B * lds; w.sC = n_all;
    c->bwd_enc.push_back(w);
    c->bwd_enc_r.push_back(region(c, head ? std::string("head_bwd_w") : "enc_bwd_w_" + std::to_string(i)));
  };
  for (int i = n; i >= 1; --i) dgrad(i);
  if (c->conv) {  // gradient of the tower features: dxf = dZ_0 W_0^T (no activation)
    c->bwd_feat = gd(4 * B, c->F, c->enc[0].N, c->dzl[0], c->lddz, false, th + c->enc[0].off,
                     c->enc[0].ld, true, c->dxf, c->ldf);
    c->bwd_feat_r = region(c, "enc_bwd_d_0");
  }
  wgrad(0);
  c->enc_part1 = (int)c->bwd_enc.size();
  wgrad(n);
  for (int i = n - 1; i >= 1; --i) wgrad(i);
  for (const char* nm : {"deinterleave", "eps_rng", "latent_fwd", "colsq", "metric_loss", "coldot",
                         "latent_bwd", "adam"})
    region(c, nm);
  if (c->conv)
    for (const char* nm : {"conv1_fwd", "conv2_fwd", "lrn2_pool2_fwd", "pool2_bwd", "conv2_wgrad",
                           "conv2_dgrad", "conv1_wgrad"})
      region(c, nm);
  return MVAE_OK;
}

// plane images of every GEMM operand buffer (filled from the fp32 buffer once here, then written
// by each producer: de-interleave, epilogues, latent kernels, Adam)
int make_plane_images(mvae_ctx* c, const CreateOpts&) {
  if (!c->np) return MVAE_OK;
  const size_t B = c->B;
  auto add = [&](float* base, size_t n) -> hipError_t {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (size_t)c->np * n * sizeof(unsigned short));
    if (e != hipSuccess) return e;
    c->allocs.push_back(q);
    mvae_ctx::PlaneBuf pb{base, n, Planes{static_cast<unsigned short*>(q), (long long)n, c->np}};
    c->planes.push_back(pb);
    return launch_split_planes(base, n, pb.pl, nullptr);
  };
  PLAN_HIP("plane images", add(c->theta, c->n_all));
  PLAN_HIP("plane images", add(c->xs, 3 * B * c->ldx));
  if (c->conv) PLAN_HIP("plane images", add(c->xf, 3 * B * c->ldf));
  for (int i = 0; i < c->nenc; ++i) PLAN_HIP("plane images", add(c->H[i], 3 * B * c->ldh[i]));
  PLAN_HIP("plane images", add(c->z, 3 * B * c->ldz));
  PLAN_HIP("plane images", add(c->zgen, B * c->ldz));
  PLAN_HIP("plane images", add(c->a1, B * c->ld_d1));
  PLAN_HIP("plane images", add(c->a2, B * c->ld_d2));
  PLAN_HIP("plane images", add(c->du, B * c->ld_u));
  PLAN_HIP("plane images", add(c->dzd2, B * c->ld_d2));
  PLAN_HIP("plane images", add(c->dzd1, B * c->ld_d1));
  PLAN_HIP("plane images", add(c->dhead, 4 * B * c->ld_dh));
  for (int i = 0; i < c->nenc; ++i) PLAN_HIP("plane images", add(c->dzl[i], 4 * B * c->lddz));
  PLAN_HIP("plane images", dalloc(c, &c->dyn, 4));
  PLAN_HIP("plane images", hipDeviceSynchronize());
  return MVAE_OK;
}

// arithmetic, kernel family and operand planes of one GEMM
void wire(mvae_ctx* c, const CreateOpts& opt, GemmDesc& d) {
  const int gp = c->np == 1 ? GEMM_BF16 : (c->np == 3 ? GEMM_F32X : GEMM_F32);
  const int e8_mode = opt.e8, thin_ring = opt.thin_ring;  // (see CreateOpts)
  d.prec = gp;
  d.x3 = opt.x3;
  // skinny products (an output dimension or K <= 64 and no 256x256 plane-kernel shape: the
  // latent head and the decoder's first layer at small L) run on the fp32 VALU kernel
  const long long t256 = (long long)((d.M + 255) / 256) * ((d.N + 255) / 256) * d.batch;
  const bool wide_shape = d.M >= 256 && d.N >= 256 && !(d.K <= 64 && t256 < 256);
  // ... except the f32x latent head at small L over the tall stacked rows (C2: forward
  // 12288 x 40 x 501, dgrad 16384 x 500 x 40): the ring kernel's plane products (on any
  // shape) beat the VALU kernel there (24.3 / 23.9 us vs 30.8 / 38.0 us in the step,
  // profiles/r4/r4g_plan_c2.txt and bench_default_r4p_regions.txt), and its weight gradient
  // (501 x 40 x 8192, two products: 35.6 vs 40.7 us on the fp32 kernel, r4ar_thin_gemms.txt)
  const int lo = d.M < d.N ? d.M : d.N;
  const bool tall = d.M >= 4096 || (thin_ring == 2 && d.K >= 4096);
  if (gp == GEMM_F32X && e8_mode == 1 && !wide_shape && tall && lo >= 32 && d.K >= 32 &&
      !d.force.names_kernel() && thin_ring) {
    d.force.kernel = K_RING;
    d.force.any_shape = true;
  }
  if (c->valu && gemm_valu_fits(d) && !(gp != GEMM_F32 && wide_shape)) {
    d.prec = GEMM_F32;
    d.force.kernel = K_VALU;
  }
  if (!c->np) return;
  const Planes a = planes_of(c, d.A), b = planes_of(c, d.B), o = planes_of(c, d.C);
  d.Ap = a.p; d.pA = a.stride; d.nA = c->np;
  d.Bp = b.p; d.pB = b.stride; d.nB = c->np;
  d.epi.cp = o.p; d.epi.pc = o.stride; d.epi.ncp = o.p ? c->np : 0;
  d.dynA = (c->np == 3 && in_xs(c, d.A)) ? c->dyn : nullptr;
  // exact split: GEMMs the 256x256 bf16 kernel does not serve (a dimension < 256: the
  // latent head, thin decoder layers) run faster as one native fp32 MFMA GEMM than as six
  // bf16 plane products on the 128x128 kernel; same accuracy class
  if (gp == GEMM_F32X && !plane_kernel(d)) d.prec = GEMM_F32;
  // create option e8: 0 never the eight-phase kernel, 2 wherever its offsets fit (A/B, tests)
  if (plane_kernel(d) && e8_mode == 0) {
    d.force.no_e8 = true;
  } else if (plane_kernel(d) && e8_mode != 1) {
    d.force.kernel = K_E8;
    d.force.any_shape = true;
  }
  // bf16 mode: a plane-kernel DACT epilogue reads the activation's bf16 plane (act' from the
  // bf16-rounded output, the operand precision of this mode), so the forward epilogues write
  // the activations as planes only (no fp32 copy); dact_planes=0: the fp32 activations (A/B)
  if (c->np == 1 && d.epi.mode == EPI_DACT && d.prec != GEMM_F32 && d.force.kernel != K_VALU && opt.dact_planes)
    d.epi.auxp = planes_of(c, d.epi.aux).p;
}

int wire_gemms(mvae_ctx* c, const CreateOpts& opt) {
  for_each_gemm(c, [&](GemmDesc& d, int) { wire(c, opt, d); });
  return MVAE_OK;
}

// which fp32 copies the step writes beside the plane images: x32mask / in_dst.f32dyn_mask (pixel rows), the
// BCE target's bits, c32 of every GEMM output, zmask, dhead32, xf32
int plan_fp32_copies(mvae_ctx* c, const CreateOpts&) {
  const size_t B = c->B;
  // fp32 xs rows: everything when a GEMM reads xs in fp32; otherwise only the BCE target
  // (lock block), and only for a batch whose pixels are not all bf16 values (the BCE epilogue
  // reads plane 0 while *dyn == 0)
  if (c->np) {
    c->x32mask = 0;
    c->in_dst.f32dyn_mask = 2;
    // (the encoder's forward and backward only: no other GEMM of the schedule has xs as its A
    // operand -- the BCE head reads it through its epilogue, handled below)
    for (auto* v : {&c->fwd_enc, &c->bwd_enc})
      for (auto& d : *v)
        if (d.prec == GEMM_F32 && in_xs(c, d.A)) c->x32mask = 7;
    if (c->f_out.prec != GEMM_F32) {
      const Planes xp = planes_of(c, c->xs);
      c->f_out.epi.xp = xp.p + (size_t)B * c->ldx;
      c->f_out.epi.xdyn = c->dyn;
      c->f_out.epi.xnb = c->dyn + 2;
      if (c->D % 8 == 0) {  // the 8-pixel de-interleave writes the target's bits beside its plane
        c->in_dst.ldbits = (c->D / 8 + 15) & ~15;
        PLAN_ALLOC(c->in_dst.xbits, B * c->in_dst.ldbits);
        c->f_out.epi.xbits = c->in_dst.xbits;
        c->f_out.epi.ldbits = c->in_dst.ldbits;
      }
    } else {
      c->x32mask |= 2;  // the native fp32 BCE GEMM reads the fp32 target rows
    }
    // fp32 copies only of the GEMM outputs something reads in fp32: an operand of a native
    // fp32 GEMM or the aux of a DACT epilogue (e.g. dU and the dgrads feeding plane GEMMs
    // only are written as planes alone). Outputs without a plane image keep their fp32 store.
    for_each_gemm(c, [&](GemmDesc& d, int) {
      const mvae_ctx::PlaneBuf* pb = nullptr;
      for (const auto& q : c->planes)
        if (d.C >= q.base && d.C < q.base + q.n) pb = &q;
      if (!pb || !d.epi.cp) return;
      auto in = [&](const float* x) { return x && x >= pb->base && x < pb->base + pb->n; };
      bool fp32_reader = false;
      for_each_gemm(c, [&](const GemmDesc& g, int) {
        if (g.prec == GEMM_F32 && (in(g.A) || in(g.B))) fp32_reader = true;
        if (g.epi.mode == EPI_DACT && in(g.epi.aux) && !g.epi.auxp) fp32_reader = true;
      });
      d.epi.c32 = fp32_reader ? 1 : 0;
    });
  }
  {  // fp32 z rows: lock for fp32 decoder GEMMs (layer-1 forward, its weight gradient) and the
     // cosine column statistics; key for the cosine statistics only
    const bool cos = c->cfg.metric == MVAE_METRIC_COSINE;
    const bool lock32 = !c->np || cos || c->f_d1.prec == GEMM_F32 || c->bwd_dec[4].prec == GEMM_F32;
    c->zmask = (lock32 ? 2 : 0) | (cos ? 4 : 0);
  }
  if (c->np) {  // fp32 dhead only for a native-fp32 head GEMM (else its planes alone)
    c->dhead32 = 0;
    for (auto& d : c->bwd_enc)
      if (d.prec == GEMM_F32 && (d.A == c->dhead || d.B == c->dhead)) c->dhead32 = 1;
  }
  if (c->conv) {
    // conv1 reads the fp32 pixels of all three row blocks (forward and weight gradient); the
    // fp32 feature rows are written only when an fp32 GEMM reads them
    c->x32mask = 7;
    c->xf32 = !c->np || c->fwd_enc[0].prec == GEMM_F32 || c->bwd_enc[c->nenc].prec == GEMM_F32;
  }
  // (the three vectors only, as this check always ran: f_d1 / f_d2 / f_out and bwd_feat read
  // buffers that all have plane images, see DESIGN.md "host code layout")
  for (auto* v : {&c->fwd_enc, &c->bwd_dec, &c->bwd_enc})
    for (auto& d : *v)
      if (c->np && (!d.Ap || !d.Bp)) return fail(nullptr, MVAE_EINVAL, "internal: GEMM operand without plane image");
  c->in_dst.xs = c->xs;
  c->in_dst.xp = planes_of(c, c->xs);
  c->in_dst.ldx = c->ldx;
  return MVAE_OK;
}

// the pixel operand as bits: both layer-0 GEMMs on the bf16-plane kernels, the target bits
// written (D % 8 == 0), whole 64-row blocks, no fp32 pixel rows read
int plan_pixel_bits(mvae_ctx* c, const CreateOpts& opt) {
  GemmDesc& f0 = c->fwd_enc[0];
  GemmDesc& w0 = c->bwd_enc[c->nenc];
  if (!(opt.bits && c->np && !c->conv && c->in_dst.xbits && c->B % 64 == 0 && c->x32mask == 0 && plane_kernel(f0) &&
        plane_kernel(w0) && f0.A == c->xs && w0.A == c->xs))
    return MVAE_OK;
  BitsDst& t = c->in_dst;
  t.kts_f = bitmat_kts(c->D + 1);
  t.kts_w = bitmat_kts(3 * c->B);
  PLAN_ALLOC(t.xbf, bitmat_words(3 * c->B, c->D + 1));
  PLAN_ALLOC(t.xbw, bitmat_words(c->D + 1, 3 * c->B));
  f0.Abits = t.xbf; f0.abits_kts = t.kts_f; f0.anb = c->dyn + 2;
  // the weight gradient's batch 2 (g2) reads stacked rows B .. 3B: k-tiles from B / 64
  w0.Abits = t.xbw; w0.abits_kts = t.kts_w; w0.anb = c->dyn + 2;
  w0.abits_sb = (long long)(c->B / 64) * BITMAT_BLOCK_WORDS;
  f0.bits_reg = w0.bits_reg = opt.bits_reg;
  c->bits_on = true;
  return MVAE_OK;
}

// layer-0 weight-gradient row chunks (see w0c): the wired GEMM re-pointed at row ranges, with the
// whole GEMM's split-K and kernel pinned, so each output row is summed exactly as the one-GEMM
// backward sums it (chunked and unchunked backwards are bitwise equal: the early Adam's chunks,
// the data-parallel parts)
int plan_w0_chunks(mvae_ctx* c, const CreateOpts&) {
  const GemmDesc& w = c->bwd_enc[c->nenc];
  const GemmPlan wp = gemm_plan(w, ~size_t(0));
  GemmForce pin = w.force;
  pin.split = wp.split;
  if (gemm_wide_kernel(wp.kernel) && !w.force.names_kernel()) {
    if (wp.kernel == K_E8) {
      pin.kernel = K_E8;
      pin.any_shape = true;
    } else {  // (tile M: 256 for an A^T operand)
      pin.kernel = K_RING;
      pin.tile_n = wp.tn;
    }
  }
  for (int R : {2, 4, 8}) {
    const int per = ((w.M + R - 1) / R + 255) / 256 * 256;
    for (int m0 = 0; m0 < w.M; m0 += per) {
      GemmDesc d = w;
      const int m1 = std::min(w.M, m0 + per);
      d.M = m1 - m0;
      d.A = w.A + m0;                  // A stored [K][M] (at): the chunk's columns
      if (d.Ap) d.Ap = w.Ap + m0;
      d.C = w.C + (size_t)m0 * w.ldc;  // output rows
      if (d.Abits) d.Abits = w.Abits + (size_t)(m0 / 256) * w.abits_kts * BITMAT_BLOCK_WORDS;
      d.force = pin;
      c->w0c[R].push_back(d);
      c->w0m[R].push_back(m0);
    }
    c->w0m[R].push_back(w.M);
  }
  return MVAE_OK;
}

// The BCE head in whole rounds: when its 256x256 tiles leave a partial last round on the 256 CUs
// (C2: 16 x 40 = 640 tiles = 2.5 rounds), the columns of the whole rounds run as one launch and
// the rest as 256x128 ring tiles (half the work per tile, so the last round takes about half as
// long); elementwise the same results and the same 128-column row partials.
// create option bce_split=0: never; set_option "bce_split" 0: one launch (A/B, tests)
int plan_bce_split(mvae_ctx* c, const CreateOpts& opt) {
  const GemmDesc& f = c->f_out;
  const long long tm = (f.M + 255) / 256, tn = (f.N + 255) / 256, tiles = tm * tn;
  const long long n1 = (tiles / 256) * 256 / tm;  // n-tiles of the whole rounds
  c->f_split = false;
  // (the rest at least 128 columns wide: a narrower one is no ring-kernel shape and would run on
  // the 128x128 plane kernel, which the split's same-results argument does not cover)
  if (!(opt.bce_split && plane_kernel(f) && tiles > 256 && tiles % 256 != 0 && tiles % 256 <= 128 && n1 >= 1 &&
        n1 < tn && f.N - 256 * n1 >= 128))
    return MVAE_OK;
  bce_split_descs(f, (int)(256 * n1), &c->f_out_a, &c->f_out_b);
  c->f_split = true;
  return MVAE_OK;
}

// xbw_split=2: on where the layer-0 forward's workgroups leave CUs free for the transpose
int plan_xbw_split(mvae_ctx* c, const CreateOpts& opt) {
  if (opt.xbw_split != 2 || !c->bits_on) return MVAE_OK;
  const GemmDesc& f0 = c->fwd_enc[0];
  // (bits_on: plan_pixel_bits found f0 on a 256-row kernel, so these are its 256- or 192-row tiles)
  const GemmPlan fp = gemm_plan(f0, ~size_t(0));
  c->xbw_split = (long long)fp.ntm * fp.ntn * f0.batch * fp.split <= 224 ? 1 : 0;
  return MVAE_OK;
}

// split-K slabs, one set per stream: the largest any GEMM of the schedule needs, and any layer-0
// chunk (f_out_a / f_out_b are not visited: a BCE-epilogue GEMM never splits K, so needs none)
int size_workspace(mvae_ctx* c, const CreateOpts&) {
  size_t ws = 0;
  for (int R : {2, 4, 8})
    for (auto& d : c->w0c[R]) ws = std::max(ws, gemm_workspace_elems(d));
  for_each_gemm(c, [&](const GemmDesc& d, int) { ws = std::max(ws, gemm_workspace_elems(d)); });
  c->ws_elems = ws;
  PLAN_ALLOC(c->ws, ws);
  PLAN_ALLOC(c->ws_side, ws);
  return MVAE_OK;
}

// hidden layers as one launch (enc_chain.hip): bf16 planes in and out, tanh / elu epilogues
// writing planes only, widths that fit the kernel's 512-column activation block; ds[i] reads
// ds[i - 1]'s output plane
bool chain_of(const std::vector<const GemmDesc*>& ds, int rows, ChainArgs& ca) {
  const GemmDesc& d0 = *ds[0];
  ca.x = d0.Ap;
  ca.ldx = d0.lda;
  ca.M = d0.M;
  ca.nl = (int)ds.size();
  ca.act = d0.epi.act;
  ca.rows = rows;
  bool ok = ca.nl >= 1 && ca.nl <= 4;
  for (int i = 0; i < ca.nl && i < 4; ++i) {
    const GemmDesc& d = *ds[i];
    ok = ok && d.prec == GEMM_BF16 && d.force.kernel != K_VALU && d.epi.mode == EPI_ACT && d.epi.c32 == 0 &&
         d.epi.cp && d.epi.ncp == 1 && d.epi.padw == 2 && d.Ap && d.Bp && d.batch == 1 && !d.at &&
         !d.bt && d.K <= 512 && d.N <= 511 && d.M == ca.M && d.epi.act == ca.act;
    ChainLayer& cl = ca.l[i];
    cl.w = d.Bp; cl.ldw = d.ldb; cl.K = d.K; cl.N = d.N; cl.out = d.epi.cp; cl.ldo = d.ldc;
    if (i) ok = ok && d.Ap == ds[i - 1]->epi.cp && d.lda == ds[i - 1]->ldc;
  }
  return ok;
}

int plan_chains(mvae_ctx* c, const CreateOpts& opt) {
  if (opt.enc_chain && c->np == 1 && c->nenc >= 3 && c->nenc <= 5) {  // layers 1 .. nenc-1
    std::vector<const GemmDesc*> ds;
    for (int i = 1; i < c->nenc; ++i) ds.push_back(&c->fwd_enc[i]);
    c->chain = chain_of(ds, opt.enc_chain_rows, c->chain_args);
  }
  if (c->chain) c->chain_r = region(c, "enc_fwd_chain");
  if (opt.dec_chain && c->np == 1) c->dchain = chain_of({&c->f_d1, &c->f_d2}, opt.enc_chain_rows, c->dchain_args);
  if (c->dchain) c->dchain_r = region(c, "dec_fwd_chain");
  return MVAE_OK;
}

// the GEMM plans of this context on stderr (diagnostics): shape, arithmetic, kernel, split-K
int log_plans(mvae_ctx* c, const CreateOpts& opt) {
  if (!opt.plan_log) return MVAE_OK;
  const size_t ws = c->ws_elems;
  for_each_gemm(c, [&](const GemmDesc& d, int r) {
    if (&d == &c->bwd_feat) return;  // (never listed; the log's text is kept as it is)
    const GemmPlan pl = gemm_plan(d, ws);
    // (the text as it always was: an eight-phase tile prints as 256x2)
    const bool valu = pl.kernel == K_VALU, wide = gemm_wide_kernel(pl.kernel);
    std::fprintf(stderr, "[mvae plan] %-16s M %6d N %6d K %6d batch %d prec %d valu %d wide %d tile %dx%d split %d\n",
                 r >= 0 ? c->region_names[r].c_str() : "?", d.M, d.N, d.K, d.batch, d.prec, (int)valu,
                 (int)wide, wide ? pl.tm : 0, wide ? (pl.kernel == K_E8 ? 2 : pl.tn) : 0, pl.split);
    if (&d == &c->fwd_enc.back() && c->chain)
      std::fprintf(stderr, "[mvae plan] enc_fwd_chain    layers 1..%d in one launch, %d rows per workgroup\n",
                   c->nenc - 1, enc_chain_rows(c->chain_args.M, c->chain_args.rows));
    if (&d == &c->f_out && c->dchain)
      std::fprintf(stderr, "[mvae plan] dec_fwd_chain    f_d1, f_d2 in one launch, %d rows per workgroup\n",
                   enc_chain_rows(c->dchain_args.M, c->dchain_args.rows));
  });
  return MVAE_OK;
}

// the side stream (lowest priority), the xbw event and the fork / join events
int make_streams(mvae_ctx* c, const CreateOpts&) {
  int lo = 0, hi = 0;
  PLAN_HIP("side stream", hipDeviceGetStreamPriorityRange(&lo, &hi));
  PLAN_HIP("side stream", hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, lo));
  PLAN_HIP("side stream", hipEventCreateWithFlags(&c->xbw_ev, hipEventDisableTiming));
  for (int i = 0; i < 16; ++i) {
    hipEvent_t ev = nullptr;
    // stream-to-stream ordering on this device only: no system-scope fence. The producer side
    // of every fork / join is a kernel, and a kernel's end-of-dispatch release is at least agent
    // scope -- the whole device, every XCD's L2 written back -- which is what a consumer kernel
    // on another queue of the same device needs; system scope adds only host / peer visibility,
    // which nothing here reads through these events (they order GPU work; the host waits on
    // stream / device synchronisation, which keeps its own fences). Measured: -0.009 ms per step
    // at C2 / C3 (profiles/r5/r5z_events_without_system_fence.txt); the bitwise tests of the
    // side-stream schedules (test_gpu_r2.py early Adam, side_mask) run with these events.
    PLAN_HIP("side stream", hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventDisableSystemFence));
    c->sync_ev.push_back(ev);
  }
  return MVAE_OK;
}

}  // namespace

// (B [K][ldb]: the head is never bt; rowpart keeps f's row stride and first block when it sets them)
void mvae::bce_split_descs(const GemmDesc& f, int c0, GemmDesc* pa, GemmDesc* pb) {
  GemmDesc a = f, b = f;
  const int rp_ld = f.epi.rp_ld ? f.epi.rp_ld : gemm_bce_nblk(f.N);
  a.N = c0;
  a.epi.rp_ld = rp_ld;
  b.N = f.N - c0;
  b.B = f.B + c0;
  if (b.Bp) b.Bp = f.Bp + c0;
  if (b.C) b.C = f.C + c0;
  if (b.epi.cp) b.epi.cp = f.epi.cp + c0;
  if (b.epi.x) b.epi.x = f.epi.x + c0;
  if (b.epi.xp) b.epi.xp = f.epi.xp + c0;
  if (b.epi.xbits) b.epi.xbits = f.epi.xbits + c0 / 8;  // (c0: a multiple of 256)
  if (b.epi.y) b.epi.y = f.epi.y + c0;
  b.epi.rp_ld = rp_ld;
  b.epi.rp_off = f.epi.rp_off + c0 / 128;
  b.force = GemmForce{};  // the ring kernel at 256x128 tiles, whatever f forces
  b.force.kernel = K_RING;
  b.force.tile_n = 128;
  *pa = a;
  *pb = b;
}

int mvae::plan_context(mvae_ctx* c, const CreateOpts& opt) {
  hipError_t he = hipSetDevice(c->device);
  if (he != hipSuccess) return fail(nullptr, (int)he, hipGetErrorString(he));
  c->adam_nt = opt.adam_nt;
  c->xbw_split = opt.xbw_split == 1 ? 1 : 0;  // (2: decided with the forward's plan, plan_xbw_split)
  if (!opt.valu) c->valu = false;
  c->np = c->cfg.precision == MVAE_PREC_BF16 ? 1 : (c->cfg.precision == MVAE_PREC_F32X ? 3 : 0);
  using Stage = int (*)(mvae_ctx*, const CreateOpts&);
  for (Stage stage : {layout_params, alloc_buffers, alloc_tower, write_ones_columns, build_schedule,
                      make_plane_images, wire_gemms, plan_fp32_copies, plan_pixel_bits, plan_w0_chunks,
                      plan_bce_split, plan_xbw_split, size_workspace, plan_chains, log_plans, make_streams})
    if (int rc = stage(c, opt)) return rc;
  return MVAE_OK;
}
