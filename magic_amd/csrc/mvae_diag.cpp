// libmvae: the diagnostics entry points (debug_* for the tests, bench_* for kernel timing). They
// run the step's own launchers on caller data or on operands made here, need no context, and
// report through mvae_last_error(NULL). Device memory and events of one call live in an Arena.
#include "mvae_ctx.h"

namespace {

// device buffers and events of one diagnostics call, released when it returns
struct Arena {
  hipStream_t st;
  hipError_t err = hipSuccess;  // the first failure; later requests then return null at once
  std::vector<void*> ptrs;
  std::vector<hipEvent_t> events;
  explicit Arena(hipStream_t s) : st(s) {}
  ~Arena() {
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (void* p : ptrs) (void)hipFree(p);
  }
  // count elements of T; zero: cleared on the stream. Check err (DIAG(ar.err)) before use
  template <class T>
  T* alloc(size_t count, bool zero = false) {
    const size_t bytes = std::max<size_t>(count * sizeof(T), 4);
    void* q = nullptr;
    if (err == hipSuccess && (err = hipMalloc(&q, bytes)) == hipSuccess) ptrs.push_back(q);
    if (q && zero) err = hipMemsetAsync(q, 0, bytes, st);
    return static_cast<T*>(q);
  }
  hipEvent_t event() {
    hipEvent_t ev = nullptr;
    if (err == hipSuccess && (err = hipEventCreate(&ev)) == hipSuccess) events.push_back(ev);
    return ev;
  }
};

// early return with the error string stored (`who`: the caller's prefix, in scope)
#define DIAG(expr) MV_TRY(nullptr, who, expr)
bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// The kernel numbers of the ABI (mvae_debug_gemm, mvae_bench_gemm, mvae_debug_epi, mvae_debug_plan;
// include/mvae.h has the table) as forces: the only place that knows the numbers. False: no such number.
bool force_from_abi(int v, GemmForce* f) {
  *f = GemmForce{};
  switch (v) {
    case 0: return true;
    case 1: case 2: f->kernel = K_PLANE; f->staging = v; return true;
    case 3: f->kernel = K_RING; f->any_shape = true; return true;
    case 4: f->kernel = K_PLANE; return true;
    case 5: case 7: case 8: f->kernel = K_RING; f->late_256 = true; return true;
    case 6: f->kernel = K_E8; f->any_shape = true; f->ring_from_128 = true; return true;
    case 9: f->kernel = K_VALU; return true;
    case 10: f->kernel = K_RING; f->cd_epilogue = true; return true;
    case 11: f->kernel = K_RING; f->tile_n = 128; return true;
    case 12: f->kernel = K_RING; f->tile_n = 256; return true;
    case 13: case 14: f->kernel = K_E8; f->any_shape = true; return true;
    case 15: f->no_e8 = true; return true;
    default: return false;
  }
}
// ... into d; the VALU kernel is fp32 arithmetic
bool force_desc(int v, GemmDesc* d) {
  if (!force_from_abi(v, &d->force)) return false;
  if (d->force.kernel == K_VALU) d->prec = GEMM_F32;
  return true;
}

// mvae_bench_gemm's epilogue (variant >> 8): the step's fused epilogues with their operand reads
// and the output planes the next GEMM would read (np planes of nc elements)
int bench_epilogue(Arena& ar, GemmDesc& d, int epi, int np, size_t nc) {
  const char* who = "";
  hipStream_t st = ar.st;
  const int M = d.M, N = d.N, ldc = d.ldc;
  if (epi > EPI_SIGMOID) DIAG(hipErrorInvalidValue);
  d.epi.mode = epi;
  d.epi.act = ACT_TANH;
  float* aux = ar.alloc<float>((size_t)M * ldc);
  DIAG(ar.err);
  DIAG(launch_normal(aux, 1, 1, M * ldc, 1, 0, 3, 0, st));
  float* rowpart = epi == EPI_BCE ? ar.alloc<float>((size_t)M * gemm_bce_nblk(N)) : nullptr;
  d.epi.aux = aux; d.epi.ld_aux = ldc;
  d.epi.x = aux; d.epi.ldx = ldc;
  d.epi.rowpart = rowpart;
  d.epi.scale = 1.f / M;
  if (epi == EPI_ACT || epi == EPI_DACT) d.epi.padw = 1;  // as the step's padded rows
  if (!np) return MVAE_OK;
  d.epi.cp = ar.alloc<unsigned short>((size_t)np * nc); d.epi.pc = (long long)nc; d.epi.ncp = np;
  // MVAE_BENCH_PLANES_ONLY=1: the output as planes only, as the step's producers write it;
  // the BCE head as in the step: binary targets read from their bf16 plane (EPI_BCEB)
  if (const char* po = std::getenv("MVAE_BENCH_PLANES_ONLY"); po && *po == '1') {
    d.epi.c32 = 0;
    if (epi == EPI_BCE) {
      const size_t nx = (size_t)M * ldc;
      DIAG(launch_binarize(aux, nx, st));
      auto* xpl = ar.alloc<unsigned short>(nx + 8);  // (+ 16 B: the zeroed flag words behind the plane)
      DIAG(ar.err);
      DIAG(launch_split_planes(aux, nx, Planes{xpl, 0, 1}, st));
      DIAG(hipMemsetAsync(xpl + nx, 0, 16, st));
      d.epi.xp = xpl;
      d.epi.xdyn = reinterpret_cast<const int*>(xpl + nx);
      d.epi.xnb = d.epi.xdyn + 2;  // (the zeroed 16 B: binarized targets)
    }
  }
  return MVAE_OK;
}

}  // namespace

extern "C" int mvae_debug_gemm(int M, int N, int K, const float* A, int lda, int at, const float* Bm,
                               int ldb, int bt, float* Cm, int ldc, int epi, int act, const float* aux,
                               int ld_aux, void* stream) {
  if ((epi & 15) == EPI_BCE || epi < 0 || (epi & 15) > EPI_SIGMOID || ((epi >> 4) & 15) > 2)
    return fail(nullptr, MVAE_EINVAL, "bad epilogue");
  const char* who = "";
  hipStream_t st = (hipStream_t)stream;
  Arena ar(st);
  GemmDesc d = gd(M, N, K, A, lda, at != 0, Bm, ldb, bt != 0, Cm, ldc, epi & 15);
  d.prec = (epi >> 4) & 15;  // 0 fp32, 1 bf16, 2 fp32-accurate bf16 split
  if (!force_desc((epi >> 8) & 15, &d)) return fail(nullptr, MVAE_EINVAL, "no such kernel number");
  if ((epi >> 13) & 1) d.force.tile_m = 192;  // epi bit 13: the ring kernel's 192-row tiles where eligible
  d.x3 = (epi >> 16) & 3;           // epi bits 16-17: f32x ring plans on the plane-stacked kernels (x3 option)
  d.epi.act = act;
  d.epi.aux = aux;
  d.epi.ld_aux = ld_aux;
  const int np = d.prec == GEMM_BF16 ? 1 : 3;  // (plane modes)
  if (d.prec != GEMM_F32) {  // plane images of the operands (the step's producers write these)
    const size_t na = (size_t)(at ? K : M) * lda, nb = (size_t)(bt ? N : K) * ldb;
    Planes A_{ar.alloc<unsigned short>(np * na), (long long)na, np};
    Planes B_{ar.alloc<unsigned short>(np * nb), (long long)nb, np};
    DIAG(ar.err);
    DIAG(launch_split_planes(A, na, A_, st));
    DIAG(launch_split_planes(Bm, nb, B_, st));
    d.Ap = A_.p; d.pA = A_.stride; d.nA = np;
    d.Bp = B_.p; d.pB = B_.stride; d.nB = np;
  }
  // epi bit 14 (plane modes, A of 0/1 values): A also as a BitMat, the eight-phase kernel's bits path
  if (((epi >> 14) & 1) && d.prec != GEMM_F32) {
    const int kts = bitmat_kts(K);
    auto* pbits = ar.alloc<unsigned>(bitmat_words(M, K));
    auto* pnb = ar.alloc<int>(4, true);
    DIAG(ar.err);
    DIAG(launch_bits_from_plane(d.Ap, lda, at != 0, M, K, pbits, kts, pnb, st));
    d.Abits = pbits; d.abits_kts = kts; d.anb = pnb;
    d.bits_reg = (epi >> 15) & 1;  // epi bit 15: its words loaded to registers (E8 BITS 2)
  }
  // epi bit 12 (plane modes): the output as bf16 planes only (no fp32 store), as the step's
  // producers write their operand images; C then receives the planes' sum (host side)
  const bool planes_out = ((epi >> 12) & 1) && d.prec != GEMM_F32;
  const size_t nc = (size_t)M * ldc;
  unsigned short* cpl = planes_out ? ar.alloc<unsigned short>(np * nc, true) : nullptr;
  if (planes_out) { d.epi.cp = cpl; d.epi.pc = (long long)nc; d.epi.ncp = np; d.epi.c32 = 0; }
  const size_t ws_n = gemm_workspace_elems(d);
  float* ws = ws_n ? ar.alloc<float>(ws_n) : nullptr;
  DIAG(ar.err);
  DIAG(gemm_run(d, ws, ws_n, st));
  DIAG(hipStreamSynchronize(st));
  if (planes_out) {
    std::vector<unsigned short> h(np * nc);
    std::vector<float> c(nc);
    DIAG(hipMemcpy(h.data(), cpl, h.size() * 2, hipMemcpyDeviceToHost));
    DIAG(hipMemcpy(c.data(), Cm, nc * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < M; ++r)
      for (int j = 0; j < N; ++j) {
        const size_t o = (size_t)r * ldc + j;
        float v = 0.f;
        for (int t = np - 1; t >= 0; --t) {
          uint32_t u = (uint32_t)h[t * nc + o] << 16;
          float f;
          std::memcpy(&f, &u, 4);
          v += f;
        }
        c[o] = v;
      }
    DIAG(hipMemcpy(Cm, c.data(), nc * 4, hipMemcpyHostToDevice));
  }
  return MVAE_OK;
}

// (diagnostics) the de-interleave of a [B][3D] batch of random 0/1 pixels (half of them 1), iters
// launches on the stream: variant 0 the step's bits form (launch_deint_bits), 7 the same without
// the weight-gradient words (no_xbw), 100 the bf16-plane pass; any other variant is MVAE_EINVAL
extern "C" int mvae_bench_deint(int B, int D, int variant, int iters, void* stream, float* avg_ms) {
  if (B <= 0 || D <= 0 || B % 64 || D % 8 || iters <= 0 || !avg_ms || variant < 0) return MVAE_EINVAL;
  {
    const int form = variant % 2000 % 1000;  // (the modifiers below taken off)
    if (form != 0 && form != 7 && form != 100) return MVAE_EINVAL;
  }
  const char* who = "";
  hipStream_t st = (hipStream_t)stream;
  Arena ar(st);
  const int ldx = (D + 1 + 7) / 8 * 8, ldbits = (D / 8 + 15) & ~15;
  const int kf = bitmat_kts(D + 1), kw = bitmat_kts(3 * B);
  // variant + 1000: four X images in turn (none of the next launch's X left in the 256 MB
  // last-level cache, as in the step, where the rest of the step's traffic evicts it)
  // variant + 2000 / + 4000: before every timed launch (each timed alone by its own events) a
  // heater -- a bf16 8192^3 GEMM (~1 ms of MFMA load, as the step's layer-0 weight gradient
  // precedes the next step's pass) / a 1 GB device memset (dirty lines)
  const int heat = variant >= 4000 ? 2 : (variant >= 2000 ? 1 : 0);
  variant %= 2000;
  const int nx = variant >= 1000 ? 4 : 1;
  variant %= 1000;
  float* xr[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < nx; ++i) xr[i] = ar.alloc<float>((size_t)B * 3 * D, true);
  float* x = xr[0];
  auto* xs = ar.alloc<float>((size_t)3 * B * ldx, true);
  auto* xp = ar.alloc<unsigned short>((size_t)3 * B * ldx, true);
  auto* xbf = ar.alloc<unsigned>(bitmat_words(3 * B, D + 1), true);
  auto* xbw = ar.alloc<unsigned>(bitmat_words(D + 1, 3 * B), true);
  auto* xb = ar.alloc<unsigned char>((size_t)B * ldbits, true);
  auto* dyn = ar.alloc<int>(16, true);
  DIAG(ar.err);
  for (int i = 0; i < nx; ++i) {
    DIAG(launch_normal(xr[i], 1, 1, B * 3 * D, 1, 0, 5 + i, 0, st));
    DIAG(launch_binarize(xr[i], (size_t)B * 3 * D, st));  // x > 0: half the pixels 1
  }
  int it = 0;
  const Planes pl{xp, (long long)3 * B * ldx, 1};
  BitsDst dst;
  dst.xbf = xbf; dst.kts_f = kf; dst.xbw = xbw; dst.kts_w = kw; dst.xbits = xb; dst.ldbits = ldbits;
  dst.xs = xs; dst.xp = pl; dst.ldx = ldx; dst.f32dyn_mask = 2;
  auto one = [&]() -> hipError_t {
    x = xr[it++ % nx];
    if (variant == 100) return launch_deinterleave(x, xs, pl, dyn, dyn + 4, B, D, ldx, 0, 2, st, xb, ldbits);
    return launch_deint_bits(XBatch{x, B, D}, dst, dyn, dyn + 4, variant == 7, st);
  };
  hipEvent_t t0 = ar.event(), t1 = ar.event();
  DIAG(ar.err);
  for (int i = 0; i < 3; ++i) DIAG(one());
  float ms = 0.f;
  if (heat) {
    const int G = 8192;
    auto* ga = ar.alloc<unsigned short>((size_t)G * G, true);
    auto* gb = ar.alloc<unsigned short>((size_t)G * G, true);
    auto* gc = ar.alloc<float>((size_t)G * G, true);
    char* junk = heat == 2 ? ar.alloc<char>((size_t)1 << 30, true) : nullptr;
    DIAG(ar.err);
    // random operands (a GEMM on zeros draws less power and holds a higher clock)
    DIAG(launch_normal(gc, 1, 1, G * G, 1, 0, 11, 0, st));
    DIAG(launch_split_planes(gc, (size_t)G * G, Planes{ga, (long long)G * G, 1}, st));
    DIAG(launch_normal(gc, 1, 1, G * G, 1, 0, 12, 0, st));
    DIAG(launch_split_planes(gc, (size_t)G * G, Planes{gb, (long long)G * G, 1}, st));
    GemmDesc d = gd(G, G, G, nullptr, G, false, nullptr, G, false, gc, G);
    d.prec = GEMM_BF16; d.Ap = ga; d.pA = (long long)G * G; d.nA = 1; d.Bp = gb; d.pB = (long long)G * G; d.nB = 1;
    for (int i = 0; i < iters; ++i) {
      DIAG(heat == 1 ? gemm_run(d, nullptr, 0, st) : hipMemsetAsync(junk, i & 0xff, (size_t)1 << 30, st));
      DIAG(hipEventRecord(t0, st));
      DIAG(one());
      DIAG(hipEventRecord(t1, st));
      DIAG(hipEventSynchronize(t1));
      float m1 = 0.f;
      DIAG(hipEventElapsedTime(&m1, t0, t1));
      ms += m1;
    }
  } else {
    DIAG(hipEventRecord(t0, st));
    for (int i = 0; i < iters; ++i) DIAG(one());
    DIAG(hipEventRecord(t1, st));
    DIAG(hipEventSynchronize(t1));
    DIAG(hipEventElapsedTime(&ms, t0, t1));
  }
  *avg_ms = ms / iters;
  return MVAE_OK;
}

// Time one GEMM shape of the step's kernel family (diagnostics): operands are allocated
// and filled with uniform [-1,1) values inside, `iters` launches are timed with HIP events
// on `stream` after 3 warm-ups. variant & 15: a kernel number (force_from_abi); include/mvae.h
// has the other bits.
extern "C" int mvae_bench_gemm(int M, int N, int K, int at, int bt, int batch, int variant, int iters,
                               void* stream, float* avg_ms) {
  if (M <= 0 || N <= 0 || K <= 0 || iters <= 0 || !avg_ms || batch <= 0) return MVAE_EINVAL;
  if ((variant >> 12) & 255)  // the removed kernel timing diagnostics
    return fail(nullptr, MVAE_EINVAL, "mvae_bench_gemm: variant bits 12-19 are not supported");
  const char* who = "";
  hipStream_t st = (hipStream_t)stream;
  Arena ar(st);
  // operand rows padded to 8 elements (16 B), as the step's buffers are
  // MVAE_BENCH_LDPAD (diagnostics): row strides rounded to this many elements (default 8)
  int pad = 8;
  if (const char* lp = std::getenv("MVAE_BENCH_LDPAD"); lp && std::atoi(lp) >= 8) pad = std::atoi(lp) & ~7;
  auto rnd = [&](int v) { return (v + pad - 1) / pad * pad; };
  const int lda = rnd(at ? M : K), ldb = rnd(bt ? K : N);
  const size_t sa = (size_t)(at ? K : M) * lda, sb = (size_t)(bt ? N : K) * ldb;
  const int ldc = rnd(N);  // output rows padded to 16 B as well (the 16-B epilogue stores)
  const size_t na = sa * batch, nb = sb * batch, nc = (size_t)M * ldc * batch;
  GemmDesc d = gd(M, N, K, nullptr, lda, at != 0, nullptr, ldb, bt != 0, nullptr, ldc);
  d.batch = batch; d.sA = (long long)sa; d.sB = (long long)sb; d.sC = (long long)M * ldc;
  d.prec = (variant >> 4) & 15;  // 0 fp32, 1 bf16, 2 fp32-accurate bf16 split
  if (!force_desc(variant & 15, &d)) return fail(nullptr, MVAE_EINVAL, "mvae_bench_gemm: no such kernel number");
  // MVAE_BENCH_SPLIT (diagnostics): split-K forced (0 / unset: the planner's)
  if (const char* sp = std::getenv("MVAE_BENCH_SPLIT"); sp && std::atoi(sp) > 0) d.force.split = std::atoi(sp);
  // MVAE_BENCH_TILE_GROUP (diagnostics): the bf16 DMA kernels' tile order (m-tiles per band)
  if (const char* tg = std::getenv("MVAE_BENCH_TILE_GROUP"); tg && std::atoi(tg) >= 0) d.group = std::atoi(tg);
  const int np = d.prec == GEMM_F32 ? 0 : (d.prec == GEMM_BF16 ? 1 : 3);
  float *A = ar.alloc<float>(na), *Bm = ar.alloc<float>(nb), *Cm = ar.alloc<float>(nc);
  DIAG(ar.err);
  DIAG(launch_normal(A, 1, 1, (int)na, 1, 0, 1, 0, st));
  DIAG(launch_normal(Bm, 1, 1, (int)nb, 1, 0, 2, 0, st));
  d.A = A; d.B = Bm; d.C = Cm;
  // variant bit 20: A of 0/1 values (the layer-0 pixels; in f32x its residual planes then zero);
  // bit 21: ... and also as a BitMat per batch (the eight-phase kernel's bits path)
  const bool bin = (variant >> 20) & 1, use_bits = bin && ((variant >> 21) & 1);
  if (bin) DIAG(launch_binarize(A, na, st));
  if (np) {
    auto* planes = ar.alloc<unsigned short>((size_t)np * (na + nb));
    DIAG(ar.err);
    Planes A_{planes, (long long)na, np}, B_{planes + np * na, (long long)nb, np};
    DIAG(launch_split_planes(A, na, A_, st));
    DIAG(launch_split_planes(Bm, nb, B_, st));
    d.Ap = A_.p; d.pA = A_.stride; d.nA = np;
    d.Bp = B_.p; d.pB = B_.stride; d.nB = np;
    // a zero flag: the step's pixel operand with its residual planes zero
    int* bnb = (bin && np == 3) || use_bits ? ar.alloc<int>(4, true) : nullptr;
    if (bin && np == 3) d.dynA = bnb;
    if (use_bits) {
      const int kts = bitmat_kts(K);
      const size_t bw = bitmat_words(M, K);
      auto* bits = ar.alloc<unsigned>(bw * batch);
      DIAG(ar.err);
      for (int b = 0; b < batch; ++b)
        DIAG(launch_bits_from_plane(A_.p + (size_t)b * sa, lda, at != 0, M, K, bits + b * bw, kts, bnb + 2, st));
      d.Abits = bits; d.abits_kts = kts; d.abits_sb = (long long)bw; d.anb = bnb + 2;
    }
  }
  if (const int epi = (variant >> 8) & 15; epi != EPI_STORE)
    if (int rc = bench_epilogue(ar, d, epi, np, nc)) return rc;
  const size_t ws_n = gemm_workspace_elems(d);
  float* ws = ws_n ? ar.alloc<float>(ws_n) : nullptr;
  hipEvent_t t0 = ar.event(), t1 = ar.event();
  DIAG(ar.err);
  for (int i = 0; i < 3; ++i) DIAG(gemm_run(d, ws, ws_n, st));
  DIAG(hipEventRecord(t0, st));
  for (int i = 0; i < iters; ++i) DIAG(gemm_run(d, ws, ws_n, st));
  DIAG(hipEventRecord(t1, st));
  DIAG(hipEventSynchronize(t1));
  float ms = 0.f;
  DIAG(hipEventElapsedTime(&ms, t0, t1));
  *avg_ms = ms / iters;
  return MVAE_OK;
}

// One conv2 kernel of the conv tower on caller data (tests only; synchronous): S1 x S1 x 64
// images, B = batch (3B forward images, 4B backward images). mode 0: out = relu(conv(x, W) + b)
// over 3B images (y = W2 block [1601][64]); mode 1: out = data gradient conv(x, W rotated) over
// 4B images (y = W2); mode 2: out[2][1601][64] = the two weight gradients of x = n1 (3B) and
// y = d a2 (4B). mfma: the bf16 MFMA kernels (operands rounded to bf16) instead of fp32 VALU.
extern "C" int mvae_debug_conv2(int S1, int B, int mode, int mfma, const float* x, const float* y,
                                float* out, void* stream) {
  if (S1 <= 0 || S1 > 50 || B <= 0 || mode < 0 || mode > 2 || !x || !y || !out)
    return fail(nullptr, MVAE_EINVAL, "mvae_debug_conv2: bad argument");
  if (mfma & 0x7e)
    return fail(nullptr, MVAE_EINVAL, "mvae_debug_conv2: mfma bits 1-6 (the removed kernel forms) must be 0");
  const char* who = "";
  hipStream_t st = (hipStream_t)stream;
  Arena ar(st);
  ConvTower T;
  T.S1 = S1; T.S = 2 * S1; T.S2 = S1 / 2;
  // mfma bit 0: the MFMA kernels; bits 8-19 the weight gradient's chunk count
  T.mfma = (mfma & 1) != 0;
  const size_t img = (size_t)S1 * S1 * 64;
  const int B2 = 2 * B;
  T.nchunk2 = std::min(B2, 32);
  T.nchunk2m = std::min(B2, 64);
  // bits 8-19: the weight gradient's chunk count (0: the step's defaults above)
  const int nchunk = (mfma >> 8) & 0xfff;
  if (nchunk) T.nchunk2 = T.nchunk2m = std::min(B2, nchunk);
  auto bf16_of = [&](const float* src, size_t n) -> unsigned short* {
    auto* p = ar.alloc<unsigned short>(n);
    if (p) ar.err = launch_split_planes(src, n, Planes{p, (long long)n, 1}, st);
    return p;
  };
  if (mode == 2) {
    T.n1 = const_cast<float*>(x);
    T.da2 = const_cast<float*>(y);
    const size_t ns = (size_t)2 * (T.mfma ? T.nchunk2m : T.nchunk2) * (25 * 64 + 1) * 64;
    T.slab = ar.alloc<float>(ns);
    DIAG(ar.err);
    // every chunk writes its whole slab, the empty ones zeros: a slab left unwritten sums to NaN
    DIAG(hipMemsetAsync(T.slab, 0xff, ns * 4, st));
    if (T.mfma) { T.n1b = bf16_of(x, 3 * B * img); T.da2b = bf16_of(y, 4 * B * img); }
    DIAG(ar.err);
    DIAG(launch_conv2_wgrad(T, B, out, out + (size_t)(25 * 64 + 1) * 64, st));
  } else {
    const int nimg = mode == 0 ? 3 * B : 4 * B;
    const unsigned short* xb = nullptr;
    if (T.mfma) {
      xb = bf16_of(x, nimg * img);
      T.w2f = ar.alloc<unsigned short>(25 * 64 * 64);
      T.w2d = ar.alloc<unsigned short>(25 * 64 * 64);
      DIAG(ar.err);
      DIAG(launch_conv2_wprep(T, y, st));
    }
    DIAG(launch_conv2(T, mode == 0, x, xb, y, mode == 0 ? T.w2f : T.w2d, out, nimg, st));
  }
  DIAG(hipStreamSynchronize(st));
  return MVAE_OK;
}

// One per-pixel kernel of the conv tower on caller buffers (tests only; synchronous): the step's
// own launcher of conv1_fwd (mode 0), lrn2_pool2_fwd (1), pool2_bwd (2) or conv1_wgrad (3), on a
// ConvTower whose pointers are the caller's. S: image size; include/mvae.h lists what each mode
// reads and writes. Only mode 3 allocates (its slab, prefilled with NaN bits).
extern "C" int mvae_debug_tower(int mode, int S, int n, int ld, int opt, const float* in0, const float* in1,
                                const float* xs, const unsigned char* arg_in, float* out0, float* out1,
                                unsigned short* outb, unsigned char* arg_out, void* stream) {
  const char* who = "mvae_debug_tower: ";
  auto bad = [&](const std::string& m) { return fail(nullptr, MVAE_EINVAL, who + m); };
  if (mode < 0 || mode > 3) return bad("mode must be in [0, 3]");
  if (S < 4 || S > 100 || S % 4) return bad("S must be a multiple of 4 in [4, 100]");
  if (n < 1 || n > 16384) return bad("n must be in [1, 16384]");
  ConvTower T;
  T.S = S; T.S1 = S / 2; T.S2 = S / 4;
  const bool pixels = mode == 0 || mode == 3;   // ld strides pixel rows, else feature rows
  if (ld < (pixels ? S * S : T.S2 * T.S2 * 64)) return bad("ld is smaller than a row");
  hipStream_t st = (hipStream_t)stream;
  Arena ar(st);
  if (mode == 0) {
    if (opt) return bad("opt must be 0 in mode 0");
    if (!in0 || !in1 || !out0 || !arg_out || (!out1 && !outb)) return bad("null buffer");
    T.p1 = out0; T.arg1 = arg_out; T.n1 = out1; T.n1b = outb;
    DIAG(launch_conv1_fwd(T, in0, ld, in1, n, st));
  } else if (mode == 1) {
    const int f32 = opt & 1, np = opt >> 1;
    if (opt < 0 || (np != 0 && np != 1 && np != 3) || (!f32 && !np)) return bad("opt must be f32 | planes << 1, planes 0, 1 or 3");
    if (!in0 || !arg_out || (f32 && !out0) || (np && !outb)) return bad("null buffer");
    T.a2 = const_cast<float*>(in0); T.arg2 = arg_out;
    DIAG(launch_lrn2_pool2_fwd(T, n, out0, ld, f32, Planes{np ? outb : nullptr, (long long)n * ld, np}, st));
  } else if (mode == 2) {
    if (opt) return bad("opt must be 0 in mode 2");
    if (!in0 || !in1 || !arg_in || (!out0 && !outb)) return bad("null buffer");
    T.a2 = const_cast<float*>(in1); T.arg2 = const_cast<unsigned char*>(arg_in);
    T.da2 = out0; T.da2b = outb;
    DIAG(launch_pool2_bwd(T, in0, ld, n, st));
  } else {
    if (opt < 0 || opt > (1 << 20)) return bad("opt (the chunk count) must be in [0, 2^20]");
    if (!in0 || !in1 || !xs || !arg_in || !out0 || !out1) return bad("null buffer");
    T.dn1 = const_cast<float*>(in0); T.p1 = const_cast<float*>(in1);
    T.arg1 = const_cast<unsigned char*>(arg_in);
    T.nchunk1 = std::min(2 * n, opt ? opt : 1024);
    const size_t ns = (size_t)2 * T.nchunk1 * 26 * 64;
    T.slab = ar.alloc<float>(ns);
    DIAG(ar.err);
    DIAG(hipMemsetAsync(T.slab, 0xff, ns * sizeof(float), st));
    DIAG(launch_conv1_wgrad(T, xs, ld, n, out0, out1, st));
  }
  DIAG(hipStreamSynchronize(st));
  return MVAE_OK;
}

// The batch's bit operands on caller buffers (tests only; synchronous; allocates nothing): mode 0
// launch_make_batch into x then launch_deint_bits (no_xbw: its forward words only), mode 1
// launch_pairs_bits; mode 2 launch_images_bits (the embedding pass's kernel): `locks` is the one
// table, idx holds 3B entries (the images of stacked rows 0 .. 3B - 1: three index arrays of B),
// keys and coef are not read; mode 3 the step's de-interleave alone on the caller's x (the
// reference of mode 2: x built by the host). S x S images, B rows. Caller buffers, zero-filled (padding is never written):
// xbf bitmat_words(3B, D + 1) words, xbw bitmat_words(D + 1, 3B) words, xbits [B][ldbits] bytes,
// dyn 4 ints, plane [3B][ldx] bf16 (plane 0, written when the not-binary word rises), x [B][3D]
// floats (mode 0 only).
static int debug_bits(const char* caller, const unsigned char* locks, const unsigned char* keys, const int* idx,
                      const int* kidx, const float* coef, int B, int S, float divisor, int mode, int no_xbw,
                      float* x, unsigned* xbf, unsigned* xbw, unsigned char* xbits, int ldbits, int* dyn,
                      unsigned short* plane, int ldx, void* stream) {
  const std::string w(caller);
  const char* who = "";
  const bool pairs_mode = mode == 0 || mode == 1;
  if ((mode != 3 && (!locks || !idx)) || (pairs_mode && (!keys || !coef)) || B <= 0 || S <= 0 || S > 4096 ||
      !(divisor > 0.f) || mode < 0 || mode > 3 || ((mode == 0 || mode == 3) && !x) || !xbf || !xbw || !xbits || !dyn || !plane || ldx < S * S || ldbits < (S * S + 7) / 8)
    return fail(nullptr, MVAE_EINVAL, w + ": bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int D = S * S;
  BitsDst dst;  // (no fp32 rows: xs null, f32dyn_mask 0)
  dst.xbf = xbf; dst.kts_f = bitmat_kts(D + 1); dst.xbw = xbw; dst.kts_w = bitmat_kts(3 * B);
  dst.xbits = xbits; dst.ldbits = ldbits; dst.xp = Planes{plane, (long long)3 * B * ldx, 1}; dst.ldx = ldx;
  int* dyn_next = dyn + 1;
  const bool now = no_xbw != 0;
  hipError_t e;
  if (mode == 0 || mode == 3) {  // x from the tables / the caller's x, then the step's de-interleave
    const bool served = !((D % 8) || (B % 64) || (ldx % 8));
    e = mode == 0 ? launch_make_batch(locks, keys, S, S, idx, kidx, coef, B, divisor, x, st)
                  : (served ? hipSuccess : hipErrorInvalidValue);
    if (e == hipSuccess) e = launch_deint_bits(XBatch{x, B, D}, dst, dyn, dyn_next, now, st);
  } else if (mode == 1) {
    e = launch_pairs_bits(PairsBatch{locks, keys, S, S, idx, kidx, coef, divisor, B}, dst, dyn, dyn_next, now, st);
  } else {
    e = launch_images_bits(ImagesBatch{locks, S, S, idx, 3 * B, divisor, B}, dst, dyn, dyn_next, now, st);
  }
  if (e == hipErrorInvalidValue)
    return fail(nullptr, MVAE_EINVAL, w + ": shape or alignment the kernels do not serve");
  DIAG(e);
  DIAG(hipStreamSynchronize(st));
  return MVAE_OK;
}

extern "C" int mvae_debug_pairs_bits(const unsigned char* locks, const unsigned char* keys, const int* idx,
                                     const float* coef, int B, int S, float divisor, int mode, int no_xbw,
                                     float* x, unsigned* xbf, unsigned* xbw, unsigned char* xbits, int ldbits,
                                     int* dyn, unsigned short* plane, int ldx, void* stream) {
  return debug_bits("mvae_debug_pairs_bits", locks, keys, idx, nullptr, coef, B, S, divisor, mode, no_xbw, x, xbf,
                    xbw, xbits, ldbits, dyn, plane, ldx, stream);
}

// modes 0 and 1 with the key of each row from key_idx (NULL: idx)
extern "C" int mvae_debug_xpairs_bits(const unsigned char* locks, const unsigned char* keys, const int* idx,
                                      const int* key_idx, const float* coef, int B, int S, float divisor, int mode,
                                      int no_xbw, float* x, unsigned* xbf, unsigned* xbw, unsigned char* xbits,
                                      int ldbits, int* dyn, unsigned short* plane, int ldx, void* stream) {
  if (mode != 0 && mode != 1) return fail(nullptr, MVAE_EINVAL, "mvae_debug_xpairs_bits: mode must be 0 or 1");
  return debug_bits("mvae_debug_xpairs_bits", locks, keys, idx, key_idx, coef, B, S, divisor, mode, no_xbw, x, xbf,
                    xbw, xbits, ldbits, dyn, plane, ldx, stream);
}

// The plane side of batch input on caller buffers (tests only; synchronous; allocates nothing): fills
// a Planes / BitsDst with every field the step sets -- the fp32 rows and their two masks, one or three
// planes, the flag slot in use -- and launches one route: the plane path's de-interleave (its form
// chosen by the caller's x, D and ldx) or a bits launcher, whose grey pass writes the planes.
// Everything the kernels' addressing relies on is checked here, before any HIP call; include/mvae.h
// lists the fields.
extern "C" int mvae_debug_input_planes(const mvae_input_args* args, void* stream) {
  const char* who = "mvae_debug_input_planes: ";
  auto bad = [&](const std::string& m) { return fail(nullptr, MVAE_EINVAL, who + m); };
  if (!args) return bad("args is NULL");
  const mvae_input_args& a = *args;
  if (a.route < 0 || a.route > 3) return bad("route must be in [0, 3]");
  if (a.np != 0 && a.np != 1 && a.np != 3) return bad("np must be 0, 1 or 3");
  if (a.slot != 0 && a.slot != 1) return bad("slot must be 0 or 1");
  if ((a.f32mask & ~7) || (a.f32dyn_mask & ~7)) return bad("f32mask and f32dyn_mask must be in [0, 7]");
  if (a.B < 1 || a.H < 1 || a.W < 1) return bad("B, H and W must be at least 1");
  if (a.B > 65535 || (long long)a.H * a.W > (1 << 24)) return bad("B or H W too large");  // (B: a grid dimension)
  const bool bits = a.route != 0;
  if (bits && a.np == 0) return bad("np 0 is the plane path's (route 0)");
  if (bits && a.f32mask) return bad("f32mask is the plane path's (route 0)");
  const int B = a.B, D = a.H * a.W;
  if (a.ldx < D) return bad("ldx is smaller than a row");
  if (!a.dyn) return bad("dyn is NULL");
  const long long rows = 3LL * B * a.ldx;
  if (a.route <= 1) {
    if (!a.x) return bad("x is NULL");
    if (a.x_elems < 3LL * B * D) return bad("x_elems is smaller than the batch");
  }
  if (a.route == 2 && (!a.locks || !a.keys || !a.idx || !a.coef)) return bad("locks, keys, idx or coef is NULL");
  if (a.route == 3 && (!a.locks || !a.idx)) return bad("locks (the table) or idx is NULL");
  if (a.route >= 2 && !(a.divisor > 0.f)) return bad("divisor must be positive");
  if (a.np) {
    if (!a.planes) return bad("planes is NULL");
    if (a.np == 3 && a.plane_stride < rows) return bad("plane_stride is smaller than a plane");
    if (a.planes_elems < (a.np - 1) * a.plane_stride + rows) return bad("planes_elems is smaller than the planes");
    if (misaligned(a.planes)) return bad("planes is not 16-byte aligned");
  }
  if (a.f32mask | a.f32dyn_mask) {
    if (!a.xs) return bad("xs is NULL");
    if (a.xs_elems < rows) return bad("xs_elems is smaller than the stacked rows");
    if (misaligned(a.xs)) return bad("xs is not 16-byte aligned");
  }
  if (bits && !a.xbits) return bad("xbits is NULL");
  if (a.xbits) {
    if (a.ldbits < D / 8) return bad("ldbits is smaller than a row");
    if (a.xbits_elems < (long long)B * a.ldbits) return bad("xbits_elems is smaller than the rows");
  }
  if (bits && (!a.xbf || (!a.no_xbw && !a.xbw))) return bad("xbf or xbw is NULL");
  if (bits) {  // the launchers' own conditions
    bool serves = (D % 8) == 0 && (B % 64) == 0 && (a.ldx % 8) == 0;
    if (a.route == 1) serves = serves && !misaligned(a.x);
    if (a.route == 2) serves = serves && pairs_bits_fits(a.locks, a.keys, a.coef, B, D);
    if (a.route == 3) serves = serves && images_bits_fits(a.locks, B, D);
    if (!serves) return bad("shape or alignment the route does not serve");
  }
  hipStream_t st = (hipStream_t)stream;
  const Planes xp{a.np ? a.planes : nullptr, a.plane_stride, a.np};
  int* flag = a.dyn + a.slot;
  int* next = a.dyn + 1 - a.slot;
  hipError_t e;
  if (!bits) {
    e = launch_deinterleave(a.x, a.xs, xp, flag, next, B, D, a.ldx, a.f32mask, a.f32dyn_mask, st, a.xbits, a.ldbits);
  } else {
    BitsDst dst;
    dst.xbf = a.xbf; dst.kts_f = bitmat_kts(D + 1); dst.xbw = a.xbw; dst.kts_w = bitmat_kts(3 * B);
    dst.xbits = a.xbits; dst.ldbits = a.ldbits; dst.xs = a.xs; dst.xp = xp; dst.ldx = a.ldx;
    dst.f32dyn_mask = a.f32dyn_mask;
    const bool now = a.no_xbw != 0;
    if (a.route == 1)
      e = launch_deint_bits(XBatch{a.x, B, D}, dst, flag, next, now, st);
    else if (a.route == 2)
      e = launch_pairs_bits(PairsBatch{a.locks, a.keys, a.H, a.W, a.idx, a.key_idx, a.coef, a.divisor, B}, dst, flag,
                            next, now, st);
    else
      e = launch_images_bits(ImagesBatch{a.locks, a.H, a.W, a.idx, 3 * B, a.divisor, B}, dst, flag, next, now, st);
  }
  if (e == hipErrorInvalidValue) return bad("shape or alignment the route does not serve");
  DIAG(e);
  DIAG(hipStreamSynchronize(st));
  return MVAE_OK;
}

// The fused hidden-layer chain on caller buffers (tests only; synchronous; allocates nothing): fills a
// ChainArgs as mvae_plan.cpp's chain_of does and launches the step's kernel. Everything the kernel's
// addressing relies on is checked here, before any HIP call: it reads 16-B chunks of x up to
// min(ldx, 512) columns, of W_l up to round8(N_l) columns of its K_l rows, and writes
// round8(N_l + 1) columns of out_l's first M rows.
extern "C" int mvae_debug_chain(int M, int nl, const int* K, const int* N, int act, int rows,
                                const unsigned short* x, int ldx, const unsigned short* const* w,
                                const int* ldw, unsigned short* const* out, const int* ldo, void* stream) {
  const char* who = "mvae_debug_chain: ";
  auto bad = [&](const std::string& m) { return fail(nullptr, MVAE_EINVAL, who + m); };
  if (nl < 1 || nl > 4) return bad("nl must be in [1, 4]");
  if (M < 1) return bad("M must be at least 1");
  if (act != 0 && act != 1) return bad("act must be 0 (tanh) or 1 (elu)");
  if (rows != 0 && (rows < 16 || rows > 96 || rows % 16))
    return bad("rows must be 0 or a multiple of 16 in [16, 96]");
  if (!K || !N || !w || !ldw || !out || !ldo) return bad("null K, N, w, ldw, out or ldo array");
  if (!x || misaligned(x)) return bad("x is null or not 16-byte aligned");
  if (ldx < 8 || (ldx & 7)) return bad("ldx must be a positive multiple of 8");
  ChainArgs ca;
  ca.x = x; ca.ldx = ldx; ca.M = M; ca.nl = nl; ca.act = act; ca.rows = rows;
  for (int l = 0; l < nl; ++l) {
    const std::string at = " (layer " + std::to_string(l) + ")";
    if (K[l] < 1 || K[l] > 512) return bad("K must be in [1, 512]" + at);
    if (N[l] < 1 || N[l] > 511) return bad("N must be in [1, 511]" + at);
    if (l == 0 && K[0] > ldx) return bad("K[0] exceeds ldx");
    if ((ldw[l] & 7) || ldw[l] < ((N[l] + 7) & ~7))
      return bad("ldw must be a multiple of 8, at least round8(N)" + at);
    if ((ldo[l] & 7) || ldo[l] < ((N[l] + 8) & ~7))
      return bad("ldo must be a multiple of 8, at least round8(N + 1)" + at);
    if (!w[l] || misaligned(w[l])) return bad("w is null or not 16-byte aligned" + at);
    if (!out[l] || misaligned(out[l])) return bad("out is null or not 16-byte aligned" + at);
    ChainLayer& cl = ca.l[l];
    cl.w = w[l]; cl.ldw = ldw[l]; cl.K = K[l]; cl.N = N[l]; cl.out = out[l]; cl.ldo = ldo[l];
  }
  hipStream_t st = (hipStream_t)stream;
  DIAG(launch_enc_chain(ca, st));
  DIAG(hipStreamSynchronize(st));
  return MVAE_OK;
}

// One kernel of the latent head on caller buffers (tests only; synchronous; allocates nothing): the
// step's own launcher of latent_fwd, colstats, metric, loss_reduce or latent_bwd, with the plane
// strides the step uses (the whole fp32 buffer: 3B ldz resp. 4B ldh elements). Everything the
// kernels' addressing relies on is checked here, before any HIP call; include/mvae.h lists what
// each mode reads and writes.
extern "C" int mvae_debug_head(const mvae_head_args* args, void* stream) {
  const char* who = "mvae_debug_head: ";
  auto bad = [&](const std::string& m) { return fail(nullptr, MVAE_EINVAL, who + m); };
  if (!args) return bad("args is NULL");
  const mvae_head_args& a = *args;
  if (a.mode < MVAE_HEAD_FWD || a.mode > MVAE_HEAD_BWD) return bad("mode must be in [0, 4]");
  if (a.B < 1 || a.L < 1) return bad("B and L must be at least 1");
  if (a.B > (1 << 24) || a.L > (1 << 20)) return bad("B or L too large");
  if (a.Bg < a.B) return bad("Bg must be at least B");
  const int B = a.B, L = a.L;
  const float inv_bg = 1.f / (float)a.Bg;
  const bool uses_z = a.mode == MVAE_HEAD_FWD || a.mode == MVAE_HEAD_COLSTATS || a.mode == MVAE_HEAD_METRIC;
  if (uses_z && a.ldz < L) return bad("ldz is smaller than a row");
  if (a.mode == MVAE_HEAD_BWD && a.ldh < 2 * L) return bad("ldh is smaller than a row");
  LatentEps le;
  if (a.mode == MVAE_HEAD_FWD || a.mode == MVAE_HEAD_BWD) {
    if (!a.ms) return bad("ms is NULL");
    le.buf = a.eps; le.seed = a.seed; le.counter = a.counter; le.Bg = a.Bg; le.off = a.off;
    if (!a.eps && (a.off < 0 || a.off > a.Bg - B)) return bad("off outside [0, Bg - B]");
  }
  hipStream_t st = (hipStream_t)stream;
  if (a.mode == MVAE_HEAD_FWD) {
    const int np = a.z_planes;
    if (a.zmask & ~6) return bad("zmask must be 0, 2, 4 or 6");
    if (np != 0 && np != 1 && np != 3) return bad("z_planes must be 0, 1 or 3");
    if (!a.rowfwd || (a.zmask && !a.z) || (np && !a.zp)) return bad("null buffer");
    if (misaligned(a.rowfwd)) return bad("rowfwd is not 16-byte aligned");
    if (L % 4 == 0 && a.ldz % 4 == 0 &&
        (misaligned(a.ms) || misaligned(a.eps) || (a.zmask && misaligned(a.z)) || (np && misaligned(a.zp))))
      return bad("ms, eps, z or zp is not 16-byte aligned");
    DIAG(launch_latent_fwd(a.ms, le, a.z, Planes{np ? a.zp : nullptr, (long long)3 * B * a.ldz, np}, a.zmask, B, L,
                           a.ldz, a.rowfwd, st));
  } else if (a.mode == MVAE_HEAD_COLSTATS) {
    if (a.cs_mode != 0 && a.cs_mode != 1) return bad("cs_mode must be 0 or 1");
    if (!a.z || !a.part || !a.out || (a.cs_mode == 1 && (!a.colsq || !a.draw))) return bad("null buffer");
    DIAG(launch_colstats(a.cs_mode, a.z, B, L, a.ldz, a.colsq, a.draw, a.part, colstats_nchunk(B), a.out, st, a.cnt));
  } else if (a.mode == MVAE_HEAD_METRIC) {
    if (a.metric != 0 && a.metric != 1) return bad("metric must be 0 (cosine) or 1 (sqdiff)");
    if (a.nblk < 0) return bad("nblk must not be negative");
    if (!a.z || !a.rowfwd || (a.nblk && !a.rowpart) || (a.metric == 0 && !a.colsq) || !a.rowvals || !a.dist ||
        !a.draw)
      return bad("null buffer");
    if (misaligned(a.rowfwd)) return bad("rowfwd is not 16-byte aligned");
    if (a.metric == 0 && L % 4 == 0 && L >= 64 && a.ldz % 4 == 0 && misaligned(a.z))
      return bad("z is not 16-byte aligned");
    DIAG(launch_metric(a.z, a.ldz, a.rowfwd, a.rowpart, a.nblk, a.areas, a.colsq, B, L, a.metric, a.recip != 0, a.w,
                       inv_bg, a.rowvals, a.dist, a.draw, st));
  } else if (a.mode == MVAE_HEAD_LOSS) {
    if (!a.rowvals || !a.losses) return bad("null buffer");
    if (misaligned(a.rowvals)) return bad("rowvals is not 16-byte aligned");
    DIAG(launch_loss_reduce(a.rowvals, B, inv_bg, a.losses, st));
  } else {
    const int np = a.h_planes;
    if (a.metric != 0 && a.metric != 1) return bad("metric must be 0 (cosine) or 1 (sqdiff)");
    if (np != 0 && np != 1 && np != 3) return bad("h_planes must be 0, 1 or 3");
    if (!a.dhead && !np) return bad("neither dhead nor planes to write");
    if (!a.dzdec || !a.draw || (a.metric == 0 && (!a.colsq || !a.coldot)) || (np && !a.hp)) return bad("null buffer");
    if (L % 4 == 0 && a.ldh % 4 == 0 &&
        (misaligned(a.ms) || misaligned(a.eps) || misaligned(a.dzdec) || misaligned(a.dhead) || (np && misaligned(a.hp))))
      return bad("ms, eps, dzdec, dhead or hp is not 16-byte aligned");
    DIAG(launch_latent_bwd(a.ms, le, a.dzdec, a.draw, a.colsq, a.coldot, B, L, a.metric, a.w, inv_bg, a.dhead, a.ldh,
                           Planes{np ? a.hp : nullptr, (long long)4 * B * a.ldh, np}, st));
  }
  DIAG(hipStreamSynchronize(st));
  return MVAE_OK;
}

// One GEMM with a fused epilogue of the step on caller buffers (tests only; synchronous): builds the
// GemmDesc the step's wiring would and calls gemm_run, as mvae_debug_gemm does, with every GemmEpi
// field the step sets -- the BCE head (all target and output forms, rowpart's stride and first
// block, the two launches of plan_bce_split through bce_split_descs), the dgrad's row remap and bf16
// aux, the padded rows' whole-chunk stores. Allocates the operands' planes and a split-K workspace;
// everything the epilogue reads or writes is the caller's. Everything the kernels' addressing relies
// on is checked here, before any HIP call; include/mvae.h lists the fields.
extern "C" int mvae_debug_epi(const mvae_epi_args* args, void* stream) {
  const char* who = "mvae_debug_epi: ";
  auto bad = [&](const std::string& m) { return fail(nullptr, MVAE_EINVAL, who + m); };
  if (!args) return bad("args is NULL");
  const mvae_epi_args& a = *args;
  if (a.epi != MVAE_EPI_ACT && a.epi != MVAE_EPI_DACT && a.epi != MVAE_EPI_BCE) return bad("epi must be 1 (ACT), 2 (DACT) or 3 (BCE)");
  if (a.M < 1 || a.N < 1 || a.K < 1) return bad("M, N and K must be at least 1");
  if (a.M > (1 << 24) || a.N > (1 << 24) || a.K > (1 << 24)) return bad("M, N or K too large");
  if (a.prec < GEMM_F32 || a.prec > GEMM_F32X) return bad("prec must be 0, 1 or 2");
  {  // (argument validation: the subset of the kernel numbers this entry has always accepted)
    const int v = a.variant;
    if (v != 0 && v != 3 && v != 4 && !(v >= 10 && v <= 13)) return bad("variant must be 0, 3, 4, 10, 11, 12 or 13");
  }
  if (a.x3 < 0 || a.x3 > 2) return bad("x3 must be in [0, 2]");
  if (a.act != ACT_TANH && a.act != ACT_ELU) return bad("act must be 0 (tanh) or 1 (elu)");
  if (a.bt != 0 && a.bt != 1) return bad("bt must be 0 or 1");
  if (!a.A || !a.B) return bad("A or B is NULL");
  if (a.lda < a.K) return bad("lda is smaller than a row");
  if (a.ldb < (a.bt ? a.K : a.N)) return bad("ldb is smaller than a row");
  if (a.ncp != 0 && a.ncp != 1 && a.ncp != 3) return bad("ncp must be 0, 1 or 3");
  if (!a.du && !a.ncp) return bad("neither du nor planes to write");
  if (a.ncp && !a.cp) return bad("cp is NULL");
  if (a.ldc < a.N) return bad("ldc is smaller than a row");
  if (a.ncp && a.pc < (long long)a.M * a.ldc) return bad("pc is smaller than a plane");
  const int n8 = (a.N + 7) & ~7, nblk = gemm_bce_nblk(a.N);
  const bool bce = a.epi == MVAE_EPI_BCE;
  if (a.padw < 0 || a.padw > 2 || (bce && a.padw)) return bad("padw must be 0, 1 or 2 (0 with BCE)");
  if (a.padw && ((a.ldc & 7) || a.ldc < n8)) return bad("padw: ldc must be a multiple of 8, at least round8(N)");
  if (a.split_c0 && !bce) return bad("split_c0 is the BCE head's");
  if (a.epi == MVAE_EPI_DACT) {
    if (!a.aux && !a.auxp) return bad("aux and auxp are NULL");
    if (a.ld_aux < a.N) return bad("ld_aux is smaller than a row");
    if (a.padw && ((a.ld_aux & 7) || a.ld_aux < n8)) return bad("padw: ld_aux must be a multiple of 8, at least round8(N)");
    if (a.remap_split < 0 || a.remap_shift < 0 || a.remap_shift > a.remap_split)
      return bad("remap must satisfy 0 <= remap_shift <= remap_split");
  }
  if (bce) {
    if (!a.x) return bad("x is NULL");
    if (a.ldx < a.N) return bad("ldx is smaller than a row");
    if (!a.rowpart) return bad("rowpart is NULL");
    if (a.rp_off < 0 || (a.rp_ld ? a.rp_ld < a.rp_off + nblk : a.rp_off != 0))
      return bad("rp_ld is smaller than rp_off plus the launch's blocks");
    if (a.y && a.ldy < a.N) return bad("ldy is smaller than a row");
    if ((a.xp || a.xbits) && !a.dyn) return bad("xp or xbits without dyn");
    if (a.xbits && !a.xp) return bad("xbits without xp");
    if (a.xbits && a.ldbits < (a.N + 7) / 8) return bad("ldbits is smaller than a row");
    if (a.split_c0 < 0 || a.split_c0 % 256 || (a.split_c0 && a.N - a.split_c0 < 128))
      return bad("split_c0 must be a multiple of 256 that leaves at least 128 columns");
    if (a.split_c0 && (a.prec == GEMM_F32 || a.bt || a.M < 128))
      return bad("split_c0 needs a plane mode, bt = 0 and M >= 128");
  }
  hipStream_t st = (hipStream_t)stream;
  Arena ar(st);
  GemmDesc d = gd(a.M, a.N, a.K, a.A, a.lda, false, a.B, a.ldb, a.bt != 0, a.du, a.ldc, a.epi);
  d.prec = a.prec;
  if (!force_from_abi(a.variant, &d.force)) return bad("no such kernel number");
  d.x3 = a.x3;
  GemmEpi& e = d.epi;
  e.act = a.act;
  e.c32 = a.du ? 1 : 0;
  if (a.ncp) { e.cp = a.cp; e.pc = a.pc; e.ncp = a.ncp; }
  e.padw = a.padw;
  if (a.epi == MVAE_EPI_DACT) {
    e.aux = a.aux; e.auxp = a.auxp; e.ld_aux = a.ld_aux;
    e.remap_split = a.remap_split; e.remap_shift = a.remap_shift;
  }
  if (bce) {
    e.x = a.x; e.ldx = a.ldx; e.scale = a.scale;
    if (a.xp) { e.xp = a.xp; e.xdyn = a.dyn; e.xnb = a.dyn + 2; }  // the step's layout of the flag words
    if (a.xbits) { e.xbits = a.xbits; e.ldbits = a.ldbits; }
    e.y = a.y; e.ldy = a.ldy;
    e.rowpart = a.rowpart; e.rp_ld = a.rp_ld; e.rp_off = a.rp_off;
  }
  if (d.prec != GEMM_F32) {  // plane images of the operands (the step's producers write these)
    const int np = d.prec == GEMM_BF16 ? 1 : 3;
    const size_t na = (size_t)a.M * a.lda, nb = (size_t)(a.bt ? a.N : a.K) * a.ldb;
    Planes A_{ar.alloc<unsigned short>(np * na), (long long)na, np};
    Planes B_{ar.alloc<unsigned short>(np * nb), (long long)nb, np};
    DIAG(ar.err);
    DIAG(launch_split_planes(a.A, na, A_, st));
    DIAG(launch_split_planes(a.B, nb, B_, st));
    d.Ap = A_.p; d.pA = A_.stride; d.nA = np;
    d.Bp = B_.p; d.pB = B_.stride; d.nB = np;
  }
  if (a.split_c0) {  // a BCE-epilogue GEMM never splits K: no workspace
    GemmDesc da, db;
    bce_split_descs(d, a.split_c0, &da, &db);
    DIAG(gemm_run(da, nullptr, 0, st));
    DIAG(gemm_run(db, nullptr, 0, st));
  } else {
    const size_t ws_n = gemm_workspace_elems(d);
    float* ws = ws_n ? ar.alloc<float>(ws_n) : nullptr;
    DIAG(ar.err);
    DIAG(gemm_run(d, ws, ws_n, st));
  }
  DIAG(hipStreamSynchronize(st));
  return MVAE_OK;
}

// The plan gemm_run would launch for these arguments (include/mvae.h): host arithmetic only, no HIP
// call, no pointer followed. The descriptor is built as mvae_debug_gemm / mvae_debug_epi build theirs.
extern "C" int mvae_debug_plan(const mvae_plan_args* args, mvae_plan_out* out) {
  const char* who = "mvae_debug_plan: ";
  auto bad = [&](const std::string& m) { return fail(nullptr, MVAE_EINVAL, who + m); };
  if (!args || !out) return bad("args or out is NULL");
  const mvae_plan_args& a = *args;
  if (a.M < 1 || a.N < 1 || a.K < 1 || a.batch < 1) return bad("M, N, K and batch must be at least 1");
  if (a.prec < GEMM_F32 || a.prec > GEMM_F32X) return bad("prec must be 0, 1 or 2");
  if (a.epi < EPI_STORE || a.epi > EPI_SIGMOID) return bad("epi must be in [0, 4]");
  if (a.tm != 0 && a.tm != 192 && a.tm != 256) return bad("tm must be 0, 192 or 256");
  if (a.x3 < 0 || a.x3 > 2) return bad("x3 must be in [0, 2]");
  if (a.nA < 1 || a.nA > 3 || a.nB < 1 || a.nB > 3) return bad("nA and nB must be in [1, 3]");
  if (a.split < 0) return bad("split must not be negative");
  static const int flag = 0;  // (a set flag pointer: never read)
  GemmDesc d = gd(a.M, a.N, a.K, nullptr, a.lda, a.at != 0, nullptr, a.ldb, a.bt != 0, (float*)a.C, a.ldc, a.epi);
  d.batch = a.batch; d.sA = a.sA; d.sB = a.sB; d.sC = a.sC;
  d.prec = a.prec;
  d.Ap = (const unsigned short*)a.Ap; d.pA = a.pA; d.nA = a.nA;
  d.Bp = (const unsigned short*)a.Bp; d.pB = a.pB; d.nB = a.nB;
  if (a.dynA) d.dynA = &flag;
  if (a.abits) d.Abits = reinterpret_cast<const unsigned*>(&flag);
  d.x3 = a.x3;
  GemmEpi& e = d.epi;
  e.c32 = a.c32; e.padw = a.padw;
  e.cp = (unsigned short*)a.cp; e.pc = a.pc; e.ncp = a.cp ? a.nA : 0;
  e.aux = (const float*)a.aux; e.auxp = (const unsigned short*)a.auxp; e.ld_aux = a.ld_aux;
  e.x = (const float*)a.x; e.xp = (const unsigned short*)a.xp; e.ldx = a.ldx;
  if (a.xdyn) e.xdyn = &flag;
  e.y = (float*)a.y; e.ldy = a.ldy;
  if (!force_desc(a.variant, &d)) return bad("no such kernel number");
  const bool valu_fits = gemm_valu_fits(d);  // (asked of the number alone, as the step's wiring asks)
  if (a.valu) d.force.kernel = K_VALU;
  d.force.tile_m = a.tm;
  d.force.split = a.split;
  const bool ws = a.ws && a.max_ws;
  const GemmPlan pl = gemm_plan(d, ws ? (size_t)a.max_ws : 0, !misaligned(a.ws));
  *out = mvae_plan_out{pl.kernel, pl.staging, pl.tm, pl.tn, pl.ntm, pl.ntn, pl.group, pl.split, pl.kchunk,
                       (int)pl.lds_epilogue, (int)pl.vec_epilogue, pl.epi_launched, (int)valu_fits,
                       (int)gemm_plan_refused(pl, ws, (size_t)a.max_ws), pl.ws_elems};
  return MVAE_OK;
}

// One batched GEMM on caller buffers (tests only; synchronous): the GemmDesc mvae_debug_gemm builds,
// with what that entry fixes at one value -- the batch and its strides, a forced split, the tile
// order, the plane images' alignment, the BitMat's two batch forms, A's run-time flag. Everything the
// kernels' addressing relies on is checked here, before any HIP call; include/mvae.h lists the fields.
extern "C" int mvae_debug_gemm_ex(const mvae_gemm_args* args, mvae_plan_out* plan, void* stream) {
  const char* who = "mvae_debug_gemm_ex: ";
  auto bad = [&](const std::string& m) { return fail(nullptr, MVAE_EINVAL, who + m); };
  if (!args) return bad("args is NULL");
  const mvae_gemm_args& a = *args;
  if (!a.A || !a.B || !a.C) return bad("A, B or C is NULL");
  if (a.M < 1 || a.N < 1 || a.K < 1 || a.batch < 1) return bad("M, N, K and batch must be at least 1");
  if (a.M > (1 << 24) || a.N > (1 << 24) || a.K > (1 << 24) || a.batch > (1 << 16)) return bad("M, N, K or batch too large");
  if ((a.at != 0 && a.at != 1) || (a.bt != 0 && a.bt != 1)) return bad("at and bt must be 0 or 1");
  if (a.prec < GEMM_F32 || a.prec > GEMM_F32X) return bad("prec must be 0, 1 or 2");
  if (a.variant < 0 || a.variant > 15) return bad("variant must be in [0, 15]");
  if (a.x3 < 0 || a.x3 > 2) return bad("x3 must be in [0, 2]");
  if (a.tm != 0 && a.tm != 192 && a.tm != 256) return bad("tm must be 0, 192 or 256");
  if (a.split < 0 || a.split > 64) return bad("split must be in [0, 64]");
  if (a.group < -1 || a.group > (1 << 16)) return bad("group must be -1, 0 or a band height");
  if (a.epi != EPI_STORE && a.epi != EPI_ACT) return bad("epi must be 0 (store) or 1 (act)");
  if (a.act != ACT_TANH && a.act != ACT_ELU) return bad("act must be 0 (tanh) or 1 (elu)");
  if (a.bits < 0 || a.bits > 2) return bad("bits must be 0, 1 or 2");
  if (a.a_off < 0 || a.a_off > 7 || a.b_off < 0 || a.b_off > 7) return bad("a_off and b_off must be in [0, 7]");
  const int arows = a.at ? a.K : a.M, acols = a.at ? a.M : a.K;
  const int brows = a.bt ? a.N : a.K, bcols = a.bt ? a.K : a.N;
  if (a.lda < acols) return bad("lda is smaller than a row");
  if (a.ldb < bcols) return bad("ldb is smaller than a row");
  if (a.ldc < a.N) return bad("ldc is smaller than a row");
  if (a.sA < 0 || a.sB < 0 || a.sC < 0) return bad("a batch stride is negative");
  if (a.sA > (1LL << 40) || a.sB > (1LL << 40) || a.sC > (1LL << 40)) return bad("a batch stride is too large");
  const long long nb1 = a.batch - 1;
  if (a.a_elems < nb1 * a.sA + (long long)arows * a.lda) return bad("a_elems is smaller than the batch's A windows");
  if (a.b_elems < nb1 * a.sB + (long long)brows * a.ldb) return bad("b_elems is smaller than the batch's B windows");
  if (a.c_elems < nb1 * a.sC + (long long)a.M * a.ldc) return bad("c_elems is smaller than the batch's C windows");
  if (a.batch > 1 && a.sC < (long long)(a.M - 1) * a.ldc + a.N) return bad("the output windows overlap");
  const bool fp32 = a.prec == GEMM_F32 || a.variant == 9;  // (9: the VALU kernel, fp32 arithmetic)
  if (a.bits && fp32) return bad("bits needs a plane mode");
  if (a.bits_shared != 0 && a.bits_shared != 1) return bad("bits_shared must be 0 or 1");
  if (a.bits_shared && (!a.bits || !a.at || a.sA % (64LL * a.lda)))
    return bad("bits_shared needs bits, at = 1 and sA a multiple of 64 lda");
  if (a.a_dyn < 0 || a.a_dyn > 2) return bad("a_dyn must be 0, 1 or 2");
  if (a.a_dyn && (a.prec != GEMM_F32X || fp32)) return bad("a_dyn needs prec 2");
  hipStream_t st = (hipStream_t)stream;
  Arena ar(st);
  GemmDesc d = gd(a.M, a.N, a.K, a.A, a.lda, a.at != 0, a.B, a.ldb, a.bt != 0, a.C, a.ldc, a.epi);
  d.batch = a.batch; d.sA = a.sA; d.sB = a.sB; d.sC = a.sC;
  d.prec = a.prec;
  if (!force_desc(a.variant, &d)) return bad("no such kernel number");
  d.force.tile_m = a.tm;
  d.force.split = a.split;
  d.group = a.group == 0 ? -1 : (a.group < 0 ? 0 : a.group);  // (GemmDesc: -1 the planner's, 0 row by row)
  d.x3 = a.x3;
  d.epi.act = a.act;
  if (d.prec != GEMM_F32) {  // plane images of the whole buffers, a_off / b_off past a 16-byte boundary
    const int np = d.prec == GEMM_BF16 ? 1 : 3;
    const size_t na = (size_t)a.a_elems, nb = (size_t)a.b_elems;
    const size_t pa = (na + 7) & ~(size_t)7, pb = (nb + 7) & ~(size_t)7;  // plane strides: multiples of 8
    auto* ap = ar.alloc<unsigned short>(np * pa + 8);
    auto* bp = ar.alloc<unsigned short>(np * pb + 8);
    DIAG(ar.err);
    Planes A_{ap + a.a_off, (long long)pa, np}, B_{bp + a.b_off, (long long)pb, np};
    DIAG(launch_split_planes(a.A, na, A_, st));
    DIAG(launch_split_planes(a.B, nb, B_, st));
    d.Ap = A_.p; d.pA = A_.stride; d.nA = np;
    d.Bp = B_.p; d.pB = B_.stride; d.nB = np;
  }
  if (a.bits) {  // A (0/1 values) also as a BitMat: one per batch element, or one of the whole stored A
    auto* pnb = ar.alloc<int>(4, true);
    if (a.bits_shared) {
      const long long rs = a.sA / a.lda;  // stored rows (k) between two batch elements
      const int kall = (int)(nb1 * rs) + a.K, kts = bitmat_kts(kall);
      auto* pbits = ar.alloc<unsigned>(bitmat_words(a.M, kall));
      DIAG(ar.err);
      DIAG(launch_bits_from_plane(d.Ap, a.lda, true, a.M, kall, pbits, kts, pnb, st));
      d.Abits = pbits; d.abits_kts = kts; d.abits_sb = rs / 64 * BITMAT_BLOCK_WORDS;
    } else {
      const int kts = bitmat_kts(a.K);
      const size_t bw = bitmat_words(a.M, a.K);
      auto* pbits = ar.alloc<unsigned>(bw * a.batch);
      DIAG(ar.err);
      for (int b = 0; b < a.batch; ++b)
        DIAG(launch_bits_from_plane(d.Ap + (size_t)b * a.sA, a.lda, a.at != 0, a.M, a.K, pbits + b * bw, kts, pnb, st));
      d.Abits = pbits; d.abits_kts = kts; d.abits_sb = (long long)bw;
    }
    d.anb = pnb;
    d.bits_reg = a.bits == 2;
  }
  if (a.a_dyn) {  // A's run-time flag: a word of 0 (only the pairs with A's plane 0 run) or of 1
    static const int one = 1;
    auto* pdyn = ar.alloc<int>(4, true);
    DIAG(ar.err);
    if (a.a_dyn == 2) DIAG(hipMemcpyAsync(pdyn, &one, sizeof one, hipMemcpyHostToDevice, st));
    d.dynA = pdyn;
  }
  const size_t ws_n = gemm_workspace_elems(d);
  float* ws = ws_n ? ar.alloc<float>(ws_n) : nullptr;
  DIAG(ar.err);
  // every slice writes its whole slab, an empty one zeros: a slab left unwritten sums to NaN
  if (ws) DIAG(hipMemsetAsync(ws, 0xff, ws_n * sizeof(float), st));
  DIAG(gemm_run(d, ws, ws_n, st));
  DIAG(hipStreamSynchronize(st));
  if (plan) {
    const GemmPlan pl = gemm_plan(d, ws ? ws_n : 0, !misaligned(ws));  // (gemm_run's own call)
    *plan = mvae_plan_out{pl.kernel, pl.staging, pl.tm, pl.tn, pl.ntm, pl.ntn, pl.group, pl.split, pl.kchunk,
                          (int)pl.lds_epilogue, (int)pl.vec_epilogue, pl.epi_launched, (int)gemm_valu_fits(d),
                          (int)gemm_plan_refused(pl, ws != nullptr, ws_n), pl.ws_elems};
  }
  return MVAE_OK;
}
