// libmvae: the training and inference step -- the encoder pass, forward / metric / backward / Adam
// and the entry points built from them (train_step*, predict*, transform*, reconstruct*, generate,
// embed_images). The schedule they launch is planned in mvae_plan.cpp.
#include "mvae_ctx.h"

// Encoder pass over the stacked [rot | lock | key] rows. draw: ENC_TRAIN samples eps from the
// training counter when eps == NULL, ENC_EVAL from the inference counter; ENC_MEAN computes the
// latent mean/log-sigma heads only (transform: no eps, no z, no column statistics).
enum { ENC_TRAIN = 0, ENC_EVAL = 1, ENC_MEAN = 2 };

// What a pass encodes: the caller's X, a pairs batch (the *_pairs and *_xpairs entry points), or one
// pass of mvae_embed_images -- the 3B images [first, first + 3B) of the call, image t of the pass
// being stacked row t.
struct BatchSrc {
  enum Kind { X, PAIRS, IMAGES } kind;
  const float* x;
  PairsBatch pairs;
  ImagesBatch images;
};
static BatchSrc batch_x(const float* x) {
  BatchSrc s{};
  s.kind = BatchSrc::X;
  s.x = x;
  return s;
}
// kidx (the *_xpairs entry points): the key of each row, NULL for the own pair (p->idx)
static BatchSrc batch_pairs(const mvae_ctx* c, const mvae_pairs* p, const int* kidx = nullptr) {
  BatchSrc s{};
  s.kind = BatchSrc::PAIRS;
  s.pairs = PairsBatch{p->locks, p->keys, p->height, p->width, p->idx, kidx, p->coef, p->divisor, c->B};
  return s;
}

// The input stage of a pass: the batch into the layer-0 operand (mvae_ctx::in_dst). A pairs batch or
// an embedding pass takes its direct kernel (launch_pairs_bits / launch_images_bits: the BitMats
// straight from the tables) exactly where an x batch would take the bits branch below and the
// launcher's shape / alignment conditions hold; in every other configuration X is materialised into
// the context's scratch and the x code runs on it. train: the pass feeds a backward (evaluation
// passes need no xbw).
static int batch_input(mvae_ctx* ctx, const BatchSrc& src, bool train, hipStream_t st) {
  auto c = ctx;
  const BitsDst& dst = c->in_dst;
  const PairsBatch& pb = src.pairs;
  const ImagesBatch& ib = src.images;
  const bool direct = c->bits_on && ((src.kind == BatchSrc::PAIRS && pairs_bits_fits(pb.locks, pb.keys, pb.coef, c->B, c->D)) ||
                                     (src.kind == BatchSrc::IMAGES && images_bits_fits(ib.table, c->B, c->D)));
  const float* x = src.x;
  if (src.kind != BatchSrc::X && !direct) {
    if (!c->pairs_x) {
      void* q = nullptr;
      MV_CHECK(hipMalloc(&q, (size_t)c->B * 3 * c->D * sizeof(float)));
      c->allocs.push_back(q);
      c->pairs_x = static_cast<float*>(q);
    }
    if (src.kind == BatchSrc::PAIRS)
      TIMED_CHECK("pairs_make_batch", launch_make_batch(pb.locks, pb.keys, pb.H, pb.W, pb.idx, pb.kidx, pb.coef, c->B,
                                                        pb.div, c->pairs_x, st));
    else
      TIMED_CHECK("images_make_x", launch_images_x(ib, c->pairs_x, st));
    x = c->pairs_x;
  }
  const char* name = !direct ? "deinterleave" : (src.kind == BatchSrc::IMAGES ? "images_bits" : "pairs_bits");
  TimeScope ts_deint(ctx, region(ctx, name), st);
  // the flag's slots alternate: this pass raises the one the previous pass zeroed and zeroes
  // the previous one (its readers are all behind on this stream), no memset launch per step
  int* prev = c->dyn_cur ? c->dyn_cur : c->dyn;
  int* cur = c->dyn ? (prev == c->dyn ? c->dyn + 1 : c->dyn) : nullptr;
  if (c->bits_on) {  // the BitMats and target bits; the planes only for a batch not all 0 / 1
    const bool split = c->xbw_split && train;
    if (direct && src.kind == BatchSrc::IMAGES)  // (an evaluation pass: the forward words only, no transpose)
      MV_CHECK(launch_images_bits(ib, dst, cur, prev, true, st));
    else if (direct)
      MV_CHECK(launch_pairs_bits(pb, dst, cur, prev, split, st));
    else
      MV_CHECK(launch_deint_bits(XBatch{x, c->B, c->D}, dst, cur, prev, split, st));
    if (split) {  // xbw from xbf on the side stream, beside the layer-0 forward
      const bool two = c->use_side && c->side;
      hipStream_t sd = two ? c->side : st;
      if (two)
        if (int rc = stream_wait(c, st, sd)) return rc;
      MV_CHECK(launch_bits_transpose(dst.xbf, dst.kts_f, dst.xbw, dst.kts_w, c->B, sd));
      MV_CHECK(hipEventRecord(c->xbw_ev, sd));
      c->xbw_pending = true;
    }
  } else {
    MV_CHECK(launch_deinterleave(x, dst.xs, dst.xp, cur, c->dyn ? prev : nullptr, c->B, c->D, dst.ldx, c->x32mask,
                                 dst.f32dyn_mask, st, dst.xbits, dst.ldbits));
  }
  c->dyn_cur = cur;
  return MVAE_OK;
}

static int encode(mvae_ctx* ctx, const BatchSrc& src, const float* eps, hipStream_t st, int draw = ENC_TRAIN) {
  auto c = ctx;
  if (c->side && c->side_pending) {  // an early-Adam backward whose mvae_adam never came
    c->side_pending = false;
    c->early_fork = false;
    if (int rc = stream_wait(c, c->side, st)) return rc;
  }
  if (c->xbw_pending) {  // the last transpose read the forward BitMat this pass rewrites
    c->xbw_pending = false;
    MV_CHECK(hipStreamWaitEvent(st, c->xbw_ev, 0));
  }
  if (int rc = batch_input(ctx, src, draw == ENC_TRAIN, st)) return rc;
  const size_t ne = (size_t)3 * c->B * c->L;
  if (draw != ENC_MEAN) {
    // eps of this forward: the caller's draws (copied: the backward needs them after the
    // caller's buffer may be gone), or the next call of the training / inference Philox
    // stream, regenerated inside the latent kernels (no eps buffer traffic)
    LatentEps le;
    le.seed = c->cfg.seed;
    le.Bg = c->cfg.global_batch;
    le.off = c->row_off;
    if (eps) {
      TIMED("eps_rng");
      MV_CHECK(hipMemcpyAsync(c->eps, eps, ne * sizeof(float), hipMemcpyDeviceToDevice, st));
      le.buf = c->eps;
    } else {
      le.counter = draw == ENC_TRAIN ? c->rng_counter++ : (EVAL_STREAM | c->rng_eval++);
    }
    c->eps_lazy = le.buf == nullptr;
    c->le = le;
  }
  if (c->conv) {  // the tower: xs pixels -> xf features (the FC layer-0 operand)
    const ConvTower& T = c->tower;
    const float* w2 = c->theta + c->cv2.off;
    const int nimg = 3 * c->B;
    TIMED_CHECK("conv1_fwd", launch_conv1_fwd(T, c->xs, c->ldx, c->theta + c->cv1.off, nimg, st));
    {
      TIMED("conv2_fwd");
      if (T.mfma) MV_CHECK(launch_conv2_wprep(T, w2, st));
      MV_CHECK(launch_conv2(T, true, T.n1, T.n1b, w2, T.w2f, T.a2, nimg, st));
    }
    TIMED_CHECK("lrn2_pool2_fwd", launch_lrn2_pool2_fwd(T, nimg, c->xf, c->ldf, c->xf32, planes_of(c, c->xf), st));
  }
  for (size_t i = 0; i < c->fwd_enc.size(); ++i) {
    if (c->chain && i == 1) {  // the hidden layers 1 .. nenc-1
      TimeScope ts(c, c->chain_r, st);
      MV_CHECK(launch_enc_chain(c->chain_args, st));
      i = c->nenc - 1;
      continue;
    }
    int rc = run(c, c->fwd_enc[i], st, c->fwd_enc_r[i]);
    if (rc) return rc;
  }
  if (draw == ENC_MEAN) return MVAE_OK;
  TIMED_CHECK("latent_fwd", launch_latent_fwd(c->ms, c->le, c->z, planes_of(c, c->z), c->zmask, c->B, c->L, c->ldz,
                                              c->rowfwd, st));
  if (c->cfg.metric == MVAE_METRIC_COSINE)
    TIMED_CHECK("colsq", launch_colstats(0, c->z, c->B, c->L, c->ldz, nullptr, nullptr, c->cspart, c->nchunk,
                                         c->colsq, st, c->cscnt));
  return MVAE_OK;
}

// the decoder's hidden layers: one chain launch or one GEMM each
static int decode_hidden(mvae_ctx* ctx, hipStream_t st) {
  if (ctx->dchain) {
    TimeScope ts(ctx, ctx->dchain_r, st);
    MV_CHECK(launch_enc_chain(ctx->dchain_args, st));
    return MVAE_OK;
  }
  int rc = run(ctx, ctx->f_d1, st, ctx->f_d1_r);
  return rc ? rc : run(ctx, ctx->f_d2, st, ctx->f_d2_r);
}

// a pairs descriptor's arguments (idx's range is the caller's precondition, as for mvae_make_batch)
static int check_pairs(mvae_ctx* ctx, const mvae_pairs* p, const char* who) {
  const std::string w(who);
  if (!p || !p->locks || !p->keys || !p->idx || !p->coef)
    return fail(ctx, MVAE_EINVAL, w + ": null pairs descriptor, table, idx or coef");
  if (p->height != ctx->cfg.image_size || p->width != ctx->cfg.image_size)
    return fail(ctx, MVAE_EINVAL, w + ": tables are " + std::to_string(p->height) + " x " + std::to_string(p->width) +
                                      ", the context's image_size is " + std::to_string(ctx->cfg.image_size));
  if ((reinterpret_cast<uintptr_t>(p->coef) & 15) != 0)
    return fail(ctx, MVAE_EINVAL, w + ": coef must be 16-byte aligned");
  if (!(p->divisor > 0.f)) return fail(ctx, MVAE_EINVAL, w + ": divisor must be positive");
  return MVAE_OK;
}

static int forward_any(mvae_ctx* ctx, const BatchSrc& src, const float* eps, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = encode(ctx, src, eps, st, ENC_TRAIN);
  if (rc) return rc;
  if ((rc = decode_hidden(ctx, st))) return rc;
  if (ctx->f_split && ctx->use_split) {
    if ((rc = run(ctx, ctx->f_out_a, st, ctx->f_out_r))) return rc;
    if ((rc = run(ctx, ctx->f_out_b, st, ctx->f_out_r))) return rc;
  } else if ((rc = run(ctx, ctx->f_out, st, ctx->f_out_r))) {
    return rc;
  }
  ctx->phase = 1;
  return MVAE_OK;
}

extern "C" int mvae_forward(mvae_ctx* ctx, const float* x, const float* eps, void* stream) {
  if (!ctx || !x) return MVAE_EINVAL;
  return forward_any(ctx, batch_x(x), eps, stream);
}

extern "C" int mvae_forward_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, const float* eps, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (int rc = check_pairs(ctx, pairs, "mvae_forward_pairs")) return rc;
  return forward_any(ctx, batch_pairs(ctx, pairs), eps, stream);
}

// the *_xpairs twins: the *_pairs code with the key of each row from key_idx
static int check_xpairs(mvae_ctx* ctx, const mvae_xpairs* xp, const char* who) {
  return check_pairs(ctx, xp ? &xp->p : nullptr, who);
}

extern "C" int mvae_forward_xpairs(mvae_ctx* ctx, const mvae_xpairs* xp, const float* eps, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (int rc = check_xpairs(ctx, xp, "mvae_forward_xpairs")) return rc;
  return forward_any(ctx, batch_pairs(ctx, &xp->p, xp->key_idx), eps, stream);
}

extern "C" int mvae_metric(mvae_ctx* ctx, const float* areas, void* stream) {
  if (!ctx || !areas) return MVAE_EINVAL;
  if (ctx->phase != 1) return fail(ctx, MVAE_ESTATE, "mvae_metric before mvae_forward");
  hipStream_t st = (hipStream_t)stream;
  auto c = ctx;
  {
    TIMED("metric_loss");
    MV_CHECK(launch_metric(c->z, c->ldz, c->rowfwd, c->rowpart, c->nblk, areas, c->colsq, c->B, c->L,
                           c->cfg.metric, c->cfg.reciprocal, c->cfg.deform_weight, c->inv_bg,
                           c->rowvals, c->dist, c->draw, st));
    MV_CHECK(launch_loss_reduce(c->rowvals, c->B, c->inv_bg, c->losses, st));
  }
  if (c->cfg.metric == MVAE_METRIC_COSINE)
    TIMED_CHECK("coldot", launch_colstats(1, c->z, c->B, c->L, c->ldz, c->colsq, c->draw, c->cspart, c->nchunk,
                                          c->coldot, st, c->cscnt));
  ctx->phase = 2;
  return MVAE_OK;
}

// back through the conv tower, after the last layer-0 chunk (its gradients final after it)
static int tower_backward(mvae_ctx* ctx, hipStream_t st) {
  auto c = ctx;
  const ConvTower& T = c->tower;
  float* g1 = c->grads;
  float* g2 = c->grads + c->n_all;
  if (int rc = run(c, c->bwd_feat, st, c->bwd_feat_r)) return rc;
  TIMED_CHECK("pool2_bwd", launch_pool2_bwd(T, c->dxf, c->ldf, c->B, st));
  TIMED_CHECK("conv2_wgrad", launch_conv2_wgrad(T, c->B, g1 + c->cv2.off, g2 + c->cv2.off, st));
  TIMED_CHECK("conv2_dgrad", launch_conv2(T, false, T.da2, T.da2b, c->theta + c->cv2.off, T.w2d, T.dn1, 4 * c->B, st));
  TIMED_CHECK("conv1_wgrad", launch_conv1_wgrad(T, c->xs, c->ldx, c->B, g1 + c->cv1.off, g2 + c->cv1.off, st));
  return MVAE_OK;
}

// Backward in R + 2 parts (R = the layer-0 weight-gradient chunks, option "wgrad0_chunks";
// phase 2 -> 4 ... -> 3); after part k the ranges mvae_grad_range(ctx, k, i, ...) hold final
// (rank-local) gradients on the caller's stream. Part 0: the decoder; part 1: the latent head
// backward, the encoder dgrad chain and layer-0 chunk 0; parts 2 .. R: layer-0 chunks 1 .. R-1
// (the conv tower's backward after the last chunk); part R + 1: joins the side stream.
// The dgrad chain (decoder output -> ... -> encoder layer 1) runs on the caller's stream; each
// weight gradient runs on the side stream as soon as its dZ exists, beside the chain (the
// chain's GEMMs leave CUs idle: few tiles, split-K reductions). Part 0 joins the decoder's
// weight gradients, the last part the encoder's (the layer-0 weight gradient runs on the
// caller's stream). join_dec = false (the single-call mvae_backward) leaves the decoder's
// weight gradients running beside the encoder chain too.
static int backward_part(mvae_ctx* ctx, int part, hipStream_t st, bool join_dec) {
  auto c = ctx;
  int rc;
  const int R = w0n(c);
  const bool two = c->use_side && c->side;
  hipStream_t sd = two ? c->side : st;
  auto fork = [&]() -> int { return two ? stream_wait(c, st, sd) : MVAE_OK; };
  // join whatever the side stream still holds, even if "side_stream" was switched off after
  // the fork (the pending weight gradients would otherwise race with Adam / the all-reduce)
  auto join = [&]() -> int {
    if (!c->side || !c->side_pending) return MVAE_OK;
    c->side_pending = false;
    return stream_wait(c, c->side, st);
  };
  const int n = c->nenc;
  auto w0chunk = [&](int r) -> int {  // layer-0 weight gradient, chunk r of R
    if (c->xbw_pending) {  // its BitMat, transposed on the side stream (xbw_split)
      c->xbw_pending = false;
      MV_CHECK(hipStreamWaitEvent(st, c->xbw_ev, 0));
    }
    const GemmDesc& d = R == 1 ? c->bwd_enc[n] : c->w0c[c->w0_chunks][r];
    return run(c, d, st, c->bwd_enc_r[n]);
  };
  // early Adam with R > 1 chunks: chunk k's rows (final in g1 and g2 after its GEMM) updated on the
  // side stream beside chunk k + 1's GEMM, which reads no weights (elementwise: the same values)
  auto chunk_adam = [&](int k) -> int {
    if (!c->early_fork || !c->side || R == 1 || k >= R - 1 || c->enc[0].off != 0) return MVAE_OK;
    AdamArgs a = adam_args(c);
    a.i0 = c->adam0_from;
    a.i1 = (size_t)c->w0m[c->w0_chunks][k + 1] * c->enc[0].ld;
    if (int rc2 = stream_wait(c, st, c->side)) return rc2;
    MV_CHECK(launch_adam(a, c->side));
    c->adam0_from = a.i1;
    return MVAE_OK;
  };
  auto tower = [&]() -> int { return c->conv ? tower_backward(c, st) : MVAE_OK; };
  if (part == 0) {
    // bwd_dec: W_out, D_out, W_d2, D_d2, W_d1, D_z
    if (!(c->side_mask & 1)) {  // option side_mask: the decoder's weight gradients in order here
      for (int i = 0; i < 6; ++i)
        if ((rc = run(c, c->bwd_dec[i], st, c->bwd_dec_r[i]))) return rc;
    } else {
      if ((rc = fork())) return rc;
      c->side_pending = two;
      if ((rc = run(c, c->bwd_dec[0], sd, c->bwd_dec_r[0]))) return rc;
      if ((rc = run(c, c->bwd_dec[1], st, c->bwd_dec_r[1]))) return rc;
      if ((rc = fork())) return rc;
      if ((rc = run(c, c->bwd_dec[2], sd, c->bwd_dec_r[2]))) return rc;
      if ((rc = run(c, c->bwd_dec[3], st, c->bwd_dec_r[3]))) return rc;
      if ((rc = fork())) return rc;
      if ((rc = run(c, c->bwd_dec[4], sd, c->bwd_dec_r[4]))) return rc;
      if ((rc = run(c, c->bwd_dec[5], st, c->bwd_dec_r[5]))) return rc;
    }
    if (join_dec && (rc = join())) return rc;
  } else if (part == 1) {
    TIMED_CHECK("latent_bwd", launch_latent_bwd(c->ms, c->le, c->dzdec, c->draw, c->colsq, c->coldot,
                                                c->B, c->L, c->cfg.metric, c->cfg.deform_weight, c->inv_bg,
                                                c->dhead32 ? c->dhead : nullptr,
                                                c->ld_dh, planes_of(c, c->dhead), st));
    // bwd_enc: [dgrad(n) .. dgrad(1), wgrad(0) | wgrad(n), wgrad(n-1) .. wgrad(1)]; dgrad(i)
    // produces dZ_{i-1}, wgrad(i) needs dZ_i (dgrad(n) = the head's: dZ of layer n-1)
    auto wg = [&](int i) -> const GemmDesc& { return c->bwd_enc[c->enc_part1 + (n - i)]; };
    auto wr = [&](int i) { return c->bwd_enc_r[c->enc_part1 + (n - i)]; };
    const bool es = (c->side_mask & 2) != 0;  // the encoder's weight gradients on the side stream
    hipStream_t se = es ? sd : st;
    if (es) {
      if ((rc = fork())) return rc;
      c->side_pending = two;
    }
    if ((rc = run(c, wg(n), se, wr(n)))) return rc;  // head weight gradient (dhead)
    for (int j = 0; j < n; ++j) {
      const int i = n - j;  // dgrad(i) -> dZ_{i-1}
      if ((rc = run(c, c->bwd_enc[j], st, c->bwd_enc_r[j]))) return rc;
      if (i - 1 >= 1) {
        if (es && (rc = fork())) return rc;
        if ((rc = run(c, wg(i - 1), se, wr(i - 1)))) return rc;
      }
    }
    // early Adam: the side stream's Adam of the blocks after layer 0 (mvae_adam) may start once
    // the dgrad chain -- the last reader of their weights -- is done, beside the layer-0
    // weight gradient. Only in the single-call mvae_backward (join_dec false): a caller of
    // mvae_backward_part all-reduces the gradients between the parts and mvae_adam, and the side
    // stream is not ordered after those collectives
    c->early_fork = false;
    c->adam0_from = 0;
    if (c->early_adam && two && !join_dec) {
      if ((rc = fork())) return rc;
      c->early_fork = true;
      c->side_pending = true;  // (if mvae_adam never comes, the next encode() joins the side stream)
    }
    if ((rc = w0chunk(0))) return rc;
    if ((rc = chunk_adam(0))) return rc;
    if (R == 1 && (rc = tower())) return rc;
  } else if (part <= R) {
    if ((rc = w0chunk(part - 1))) return rc;
    if ((rc = chunk_adam(part - 1))) return rc;
    if (part == R && (rc = tower())) return rc;
  } else if (!c->early_fork) {
    if ((rc = join())) return rc;
  }
  // (early Adam: mvae_adam joins the side stream after its last launch there -- one cross-stream
  // wait per step instead of two, each ~10 us of idle GPU at the end of the step, r5y)
  c->bpart = part + 1;
  ctx->phase = part == R + 1 ? 3 : 4;
  return MVAE_OK;
}

extern "C" int mvae_backward_nparts(mvae_ctx* ctx) { return ctx ? nparts(ctx) : MVAE_EINVAL; }

extern "C" int mvae_backward_part(mvae_ctx* ctx, int part, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (part < 0 || part >= nparts(ctx))
    return fail(ctx, MVAE_EINVAL, "backward part must be in [0, mvae_backward_nparts)");
  const bool ok = part == 0 ? ctx->phase == 2 : (ctx->phase == 4 && ctx->bpart == part);
  if (!ok) return fail(ctx, MVAE_ESTATE, "mvae_backward_part out of order");
  return backward_part(ctx, part, (hipStream_t)stream, true);
}

extern "C" int mvae_backward(mvae_ctx* ctx, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (ctx->phase != 2) return fail(ctx, MVAE_ESTATE, "mvae_backward before mvae_metric");
  // early Adam: the layer-0 weight gradient in early_chunks chunks (default 1), Adam of each chunk
  // but the last beside the next chunk's GEMM (r5zw: -0.003 to -0.034 ms at 2 chunks with the
  // chunks' own plans; with the one-GEMM plan pinned, 2 chunks cost +1-2.5 %, r6l)
  const int w0 = ctx->w0_chunks;
  if (ctx->early_adam && ctx->use_side && ctx->side && w0 == 1 && ctx->early_chunks > 1 && !ctx->conv &&
      ctx->enc[0].off == 0)
    ctx->w0_chunks = ctx->early_chunks;
  int rc = MVAE_OK;
  for (int part = 0; part < nparts(ctx) && !rc; ++part) rc = backward_part(ctx, part, (hipStream_t)stream, false);
  ctx->w0_chunks = w0;
  return rc;
}
extern "C" int mvae_adam(mvae_ctx* ctx, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (ctx->phase != 3) return fail(ctx, MVAE_ESTATE, "mvae_adam before mvae_backward");
  auto c = ctx;
  const AdamArgs a = adam_args(c);
  hipStream_t st = (hipStream_t)stream;
  if (c->early_fork && c->side) {
    // the blocks after layer 0 on the side stream (already past the dgrad chain), layer 0 and the
    // conv-tower blocks in front of it here; the caller's stream then waits for the side stream
    c->early_fork = false;
    const size_t l1 = c->nenc > 1 ? c->enc[1].off : c->head.off;
    AdamArgs a1 = a, a0 = a;
    a1.i0 = l1;
    a0.i0 = c->adam0_from;  // (the layer-0 chunks before the last: updated in the backward)
    a0.i1 = l1;
    c->adam0_from = 0;
    MV_CHECK(launch_adam(a1, c->side));
    TIMED_CHECK("adam", launch_adam(a0, st));
    if (int rc = stream_wait(c, c->side, st)) return rc;
    c->side_pending = false;
  } else {
    TIMED_CHECK("adam", launch_adam(a, st));
  }
  for (int o = 0; o < 2; ++o) { c->b1p[o] *= c->cfg.beta1; c->b2p[o] *= c->cfg.beta2; }
  c->t1++; c->t2++;
  ctx->phase = 0;
  return MVAE_OK;
}

static int train_step_any(mvae_ctx* ctx, const BatchSrc& src, const float* areas, const float* eps,
                          float* losses_out, float* dist_out, void* stream) {
  int rc;
  if ((rc = forward_any(ctx, src, eps, stream))) return rc;
  if ((rc = mvae_metric(ctx, areas, stream))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (losses_out) MV_CHECK(hipMemcpyAsync(losses_out, ctx->losses, 5 * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (dist_out) MV_CHECK(hipMemcpyAsync(dist_out, ctx->dist, ctx->B * sizeof(float), hipMemcpyDeviceToDevice, st));
  // nothing touches the gradients between the two: Adam of the blocks after layer 0 may run
  // beside the layer-0 weight gradient (option "early_adam"; f32x since profiles/r4/
  // r4ae_early_adam.txt, bf16 since the round-5 kernels: C3 1.837 vs 1.844 ms, r5m / r5n)
  const bool ea = ctx->early_adam;
  ctx->early_adam = ea || ctx->np != 0;
  rc = mvae_backward(ctx, stream);
  ctx->early_adam = ea;
  if (rc) return rc;
  return mvae_adam(ctx, stream);
}

extern "C" int mvae_train_step(mvae_ctx* ctx, const float* x, const float* areas, const float* eps,
                               float* losses_out, float* dist_out, void* stream) {
  if (!ctx || !x || !areas) return MVAE_EINVAL;
  return train_step_any(ctx, batch_x(x), areas, eps, losses_out, dist_out, stream);
}

extern "C" int mvae_train_step_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, const float* areas, const float* eps,
                                     float* losses_out, float* dist_out, void* stream) {
  if (!ctx || !areas) return MVAE_EINVAL;
  if (int rc = check_pairs(ctx, pairs, "mvae_train_step_pairs")) return rc;
  return train_step_any(ctx, batch_pairs(ctx, pairs), areas, eps, losses_out, dist_out, stream);
}

extern "C" int mvae_train_step_xpairs(mvae_ctx* ctx, const mvae_xpairs* xp, const float* areas, const float* eps,
                                      float* losses_out, float* dist_out, void* stream) {
  if (!ctx || !areas) return MVAE_EINVAL;
  if (int rc = check_xpairs(ctx, xp, "mvae_train_step_xpairs")) return rc;
  return train_step_any(ctx, batch_pairs(ctx, &xp->p, xp->key_idx), areas, eps, losses_out, dist_out, stream);
}

// get_predictions in two phases (a data-parallel host all-reduces MVAE_BUF_COLSQ between them:
// the cosine distance normalises over the GLOBAL batch, 8c/vae.py:449-450)
static int predict_encode_any(mvae_ctx* ctx, const BatchSrc& src, const float* eps, void* stream) {
  int rc = encode(ctx, src, eps, (hipStream_t)stream, ENC_EVAL);
  if (rc) return rc;
  ctx->phase = 6;
  return MVAE_OK;
}

extern "C" int mvae_predict_encode(mvae_ctx* ctx, const float* x, const float* eps, void* stream) {
  if (!ctx || !x) return MVAE_EINVAL;
  return predict_encode_any(ctx, batch_x(x), eps, stream);
}

extern "C" int mvae_predict_encode_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, const float* eps, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (int rc = check_pairs(ctx, pairs, "mvae_predict_encode_pairs")) return rc;
  return predict_encode_any(ctx, batch_pairs(ctx, pairs), eps, stream);
}

extern "C" int mvae_predict_encode_xpairs(mvae_ctx* ctx, const mvae_xpairs* xp, const float* eps, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (int rc = check_xpairs(ctx, xp, "mvae_predict_encode_xpairs")) return rc;
  return predict_encode_any(ctx, batch_pairs(ctx, &xp->p, xp->key_idx), eps, stream);
}

extern "C" int mvae_predict_finish(mvae_ctx* ctx, float* dist_out, void* stream) {
  if (!ctx || !dist_out) return MVAE_EINVAL;
  if (ctx->phase != 6) return fail(ctx, MVAE_ESTATE, "mvae_predict_finish before mvae_predict_encode");
  hipStream_t st = (hipStream_t)stream;
  auto c = ctx;
  MV_CHECK(launch_metric(c->z, c->ldz, c->rowfwd, c->rowpart, c->nblk, nullptr, c->colsq, c->B, c->L,
                         c->cfg.metric, c->cfg.reciprocal, c->cfg.deform_weight, c->inv_bg,
                         c->rowvals, dist_out, c->draw, st));
  ctx->phase = 0;
  return MVAE_OK;
}

extern "C" int mvae_predict(mvae_ctx* ctx, const float* x, const float* eps, float* dist_out, void* stream) {
  if (!ctx || !x || !dist_out) return MVAE_EINVAL;
  int rc = mvae_predict_encode(ctx, x, eps, stream);
  return rc ? rc : mvae_predict_finish(ctx, dist_out, stream);
}

extern "C" int mvae_predict_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, const float* eps, float* dist_out,
                                  void* stream) {
  if (!ctx || !dist_out) return MVAE_EINVAL;
  int rc = mvae_predict_encode_pairs(ctx, pairs, eps, stream);
  return rc ? rc : mvae_predict_finish(ctx, dist_out, stream);
}

extern "C" int mvae_predict_xpairs(mvae_ctx* ctx, const mvae_xpairs* xp, const float* eps, float* dist_out,
                                   void* stream) {
  if (!ctx || !dist_out) return MVAE_EINVAL;
  if (int rc = check_xpairs(ctx, xp, "mvae_predict_xpairs")) return rc;
  int rc = predict_encode_any(ctx, batch_pairs(ctx, &xp->p, xp->key_idx), eps, stream);
  return rc ? rc : mvae_predict_finish(ctx, dist_out, stream);
}

static int transform_any(mvae_ctx* ctx, const BatchSrc& src, float* zmean_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = encode(ctx, src, nullptr, st, ENC_MEAN);
  if (rc) return rc;
  MV_CHECK(launch_copy2d(ctx->ms + (size_t)ctx->B * 2 * ctx->L, 2 * ctx->L, zmean_out, ctx->L,
                         ctx->B, ctx->L, st));
  ctx->phase = 0;
  return MVAE_OK;
}

extern "C" int mvae_transform(mvae_ctx* ctx, const float* x, float* zmean_out, void* stream) {
  if (!ctx || !x || !zmean_out) return MVAE_EINVAL;
  return transform_any(ctx, batch_x(x), zmean_out, stream);
}

extern "C" int mvae_transform_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, float* zmean_out, void* stream) {
  if (!ctx || !zmean_out) return MVAE_EINVAL;
  if (int rc = check_pairs(ctx, pairs, "mvae_transform_pairs")) return rc;
  return transform_any(ctx, batch_pairs(ctx, pairs), zmean_out, stream);
}

extern "C" int mvae_transform_xpairs(mvae_ctx* ctx, const mvae_xpairs* xp, float* zmean_out, void* stream) {
  if (!ctx || !zmean_out) return MVAE_EINVAL;
  if (int rc = check_xpairs(ctx, xp, "mvae_transform_xpairs")) return rc;
  return transform_any(ctx, batch_pairs(ctx, &xp->p, xp->key_idx), zmean_out, stream);
}

// ceil(count / 3B) encoder passes, every stacked row a wanted image; the means (and log-sigmas) of
// a pass's rows leave ms with one strided copy per output, clipped to count
extern "C" int mvae_embed_images(mvae_ctx* ctx, const mvae_images* im, int64_t count, float* zmean_out,
                                 float* zlogsig_out, void* stream) {
  if (!ctx) return MVAE_EINVAL;
  if (!im || !im->table || !zmean_out)
    return fail(ctx, MVAE_EINVAL, "mvae_embed_images: null images descriptor, table or zmean_out");
  if (count < 1) return fail(ctx, MVAE_EINVAL, "mvae_embed_images: count must be at least 1");
  if (im->height != ctx->cfg.image_size || im->width != ctx->cfg.image_size)
    return fail(ctx, MVAE_EINVAL, "mvae_embed_images: table is " + std::to_string(im->height) + " x " +
                                      std::to_string(im->width) + ", the context's image_size is " +
                                      std::to_string(ctx->cfg.image_size));
  if (!(im->divisor > 0.f)) return fail(ctx, MVAE_EINVAL, "mvae_embed_images: divisor must be positive");
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = 3 * (int64_t)ctx->B;
  const int L = ctx->L;
  for (int64_t first = 0; first < count; first += rows) {
    BatchSrc pass{};
    pass.kind = BatchSrc::IMAGES;
    const int nvalid = (int)std::min<int64_t>(rows, count - first);
    // (idx given: the whole table and this pass's indices; else the table from image `first` on)
    pass.images = ImagesBatch{im->idx ? im->table : im->table + (size_t)first * ctx->D, im->height, im->width,
                              im->idx ? im->idx + first : nullptr, nvalid, im->divisor, ctx->B};
    int rc = encode(ctx, pass, nullptr, st, ENC_MEAN);
    if (rc) return rc;
    TIMED("embed_copy_out");
    MV_CHECK(launch_copy2d(ctx->ms, 2 * L, zmean_out + (size_t)first * L, L, nvalid, L, st));
    if (zlogsig_out) MV_CHECK(launch_copy2d(ctx->ms + L, 2 * L, zlogsig_out + (size_t)first * L, L, nvalid, L, st));
  }
  ctx->phase = 0;
  return MVAE_OK;
}
static int reconstruct_any(mvae_ctx* ctx, const BatchSrc& src, const float* eps, float* y_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = encode(ctx, src, eps, st, ENC_EVAL);
  if (rc) return rc;
  if ((rc = decode_hidden(ctx, st))) return rc;
  GemmDesc d = ctx->f_out;
  d.epi.y = y_out;
  d.epi.ldy = ctx->D;
  if ((rc = run(ctx, d, st))) return rc;
  ctx->phase = 0;
  return MVAE_OK;
}

extern "C" int mvae_reconstruct(mvae_ctx* ctx, const float* x, const float* eps, float* y_out, void* stream) {
  if (!ctx || !x || !y_out) return MVAE_EINVAL;
  return reconstruct_any(ctx, batch_x(x), eps, y_out, stream);
}

extern "C" int mvae_reconstruct_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, const float* eps, float* y_out,
                                      void* stream) {
  if (!ctx || !y_out) return MVAE_EINVAL;
  if (int rc = check_pairs(ctx, pairs, "mvae_reconstruct_pairs")) return rc;
  return reconstruct_any(ctx, batch_pairs(ctx, pairs), eps, y_out, stream);
}

extern "C" int mvae_reconstruct_xpairs(mvae_ctx* ctx, const mvae_xpairs* xp, const float* eps, float* y_out,
                                       void* stream) {
  if (!ctx || !y_out) return MVAE_EINVAL;
  if (int rc = check_xpairs(ctx, xp, "mvae_reconstruct_xpairs")) return rc;
  return reconstruct_any(ctx, batch_pairs(ctx, &xp->p, xp->key_idx), eps, y_out, stream);
}

extern "C" int mvae_generate(mvae_ctx* ctx, const float* zin, int n, float* y_out, void* stream) {
  if (!ctx || !zin || !y_out || n <= 0 || n > ctx->B) return MVAE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  auto c = ctx;
  MV_CHECK(launch_copy2d(zin, c->L, c->zgen, c->ldz, n, c->L, st));
  MV_CHECK(launch_split_planes(c->zgen, (size_t)n * c->ldz, planes_of(c, c->zgen), st));
  // the decoder's first GEMM re-pointed at zgen: fp32 rows and (plane modes) zgen's own plane
  // images, whose plane stride is B*ldz (z's is 3*B*ldz)
  GemmDesc d1 = c->f_d1; d1.M = n; d1.A = c->zgen; d1.dynA = nullptr;
  { const Planes zp = planes_of(c, c->zgen); d1.Ap = zp.p; d1.pA = zp.stride; }
  GemmDesc d2 = c->f_d2; d2.M = n;
  GemmDesc d3 = c->f_out;
  d3.M = n; d3.C = y_out; d3.ldc = c->D; d3.epi = GemmEpi(); d3.epi.mode = EPI_SIGMOID;
  int rc;
  if ((rc = run(c, d1, st))) return rc;
  if ((rc = run(c, d2, st))) return rc;
  if ((rc = run(c, d3, st))) return rc;
  ctx->phase = 0;
  return MVAE_OK;
}
