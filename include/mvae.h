/*
 * mvae.h — C ABI of libmvae, the MI355X (gfx950) training step of the "magic"
 * asymmetric metric-VAE (reference: ag8/magic, class TangoEncoder).
 *
 * The reference has no FFI: its "operator API" is the Python class
 * TangoEncoder(sess) driven through tf.Session.run (11a/vae.py:13,22) and fed by
 * overlap_input.inputs() (11a/overlap_input.py:76). Each entry point below replaces
 * one of those graph evaluations; the Python mirror of the reference interface
 * (magic_amd/vae.py) binds them through ctypes. Plain pointers and sizes only:
 * every float* argument is a DEVICE pointer owned by the caller unless stated.
 *
 *   reference call (file:line)                      -> entry point(s)
 *   TangoEncoder.__init__  11a/vae.py:22-332         -> mvae_create (+ mvae_param_* for init)
 *   partial_fit            11a/vae.py:385-411        -> mvae_train_step
 *                                                      = mvae_forward, mvae_metric,
 *                                                        mvae_backward, mvae_adam
 *                                                      (split so a data-parallel host can
 *                                                       all-reduce between the phases)
 *   get_predictions        11a/vae.py:413-414        -> mvae_predict
 *   transform              11a/vae.py:416-420        -> mvae_transform
 *   generate               11a/vae.py:422-434        -> mvae_generate
 *   reconstruct            11a/vae.py:436-440        -> mvae_reconstruct
 *
 * Errors: 0 = ok; <0 = invalid argument / configuration (MVAE_E*); >0 = hipError_t.
 * No exception crosses the ABI; mvae_last_error() returns a message.
 * Threading: one context per device per process; a context is not thread-safe;
 * all work is enqueued on the caller's stream (hipStream_t passed as void*).
 */
#ifndef MVAE_H_
#define MVAE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVAE_ABI_VERSION 7
#define MVAE_MAX_ENC 8

enum { MVAE_OK = 0, MVAE_EINVAL = -1, MVAE_ECONFIG = -2, MVAE_ESTATE = -3 };
enum { MVAE_ACT_TANH = 0, MVAE_ACT_ELU = 1 };                    /* 8c family : 11a */
enum { MVAE_METRIC_COSINE = 0, MVAE_METRIC_SQDIFF = 1 };        /* 11a/constants.py:5-7 */
/* GEMM arithmetic: F32 = native fp32 MFMA; BF16 = bf16 operands, fp32 accumulate;
 * F32X = fp32-accurate: every fp32 operand split exactly into 3 bf16 terms, products
 * a_i*b_j with i+j<3 on bf16 MFMA, fp32 accumulate (exact-bf16 tiles take 1 term). */
enum { MVAE_PREC_F32 = 0, MVAE_PREC_BF16 = 1, MVAE_PREC_F32X = 2 };

/* Hyper-parameters the reference hard-codes in TangoEncoder.__init__ (11a/vae.py:30-65)
 * and FLAGS (11a/constants.py:32,49,52,60). */
typedef struct mvae_cfg {
  int image_size;        /* H = W; D = H*W pixels per image                    */
  int batch;             /* rows per call on this rank (FLAGS.BATCH_SIZE)      */
  int global_batch;      /* rows over all ranks; losses/grads scale by 1/global */
  int n_enc;             /* encoder depth (1..MVAE_MAX_ENC)                    */
  int enc[MVAE_MAX_ENC]; /* encoder widths, 11a/vae.py:30                      */
  int dec[2];            /* decoder widths, fixed [500,500] (11a/vae.py:36)    */
  int latent;            /* L, 11a/vae.py:49                                   */
  int act;               /* MVAE_ACT_*                                          */
  int metric;            /* MVAE_METRIC_*                                       */
  int reciprocal;        /* distance = 1/raw (11a/vae.py:307,309)              */
  float deform_weight;   /* 10 (8c/vae.py:287) or 100 (11a/vae.py:293)         */
  float lr[2];           /* [cost optimizer, metric optimizer]                 */
  float beta1, beta2, epsilon; /* TF AdamOptimizer defaults .9/.999/1e-8       */
  int precision;         /* MVAE_PREC_*                                         */
  uint64_t seed;         /* counter-based N(0,1) stream for eps when not given */
  int conv;              /* 1: conv-encoder variant (BASELINE config 5): the CifarNet
                            tower of 6b/net.py:50-60 (conv5x5x64, pool, LRN, conv5x5x64,
                            LRN, pool; weights shared by the three encoder passes) in front
                            of the FC encoder, whose first layer then reads the (S/4)^2*64
                            tower features. Variables enc_conv{1,2}_{W,b} come first in
                            mvae_param_info order (W as [25*c_in, 64], TF HWIO flattened).
                            Needs image_size % 4 == 0. bf16 precision runs the 64->64 conv
                            on MFMA; f32 / f32x run the tower in fp32. 0: FC encoder.  */
} mvae_cfg;

typedef struct mvae_ctx mvae_ctx;

/* Named views into context-owned device memory. */
enum {
  MVAE_KIND_PARAM = 0, MVAE_KIND_GRAD1 = 1, MVAE_KIND_GRAD2 = 2,
  MVAE_KIND_M1 = 3, MVAE_KIND_V1 = 4, MVAE_KIND_M2 = 5, MVAE_KIND_V2 = 6
};
typedef struct mvae_tensor {
  char name[48];    /* reference variable meaning, e.g. "enc_h0_W", "dec_out_mean_b" */
  float* data;      /* device pointer of element [0][0]                               */
  int rows, cols;   /* logical shape (a bias is rows=1)                                */
  int ld;           /* row stride in elements                                          */
  int trained_by;   /* bit0: cost optimizer, bit1: metric optimizer, 0: dead variable  */
} mvae_tensor;

/* Flat buffers (for checkpoints and the data-parallel gradient all-reduce). */
enum {
  MVAE_BUF_PARAMS = 0,   /* all trained parameters (augmented [W;b] blocks)            */
  MVAE_BUF_GRADS = 1,    /* [g1 (all trained) | g2 (encoder)] — the all-reduce bucket  */
  MVAE_BUF_ADAM = 2,     /* [m1 | v1 | m2 | v2]                                        */
  MVAE_BUF_LOSSES = 3,   /* float[8]: cost, training_loss, r_l, l_l, d_l (rank-local
                            partial sums scaled by 1/global_batch; global after a sum)  */
  MVAE_BUF_COLSQ = 4,    /* float[2L]: sum_b z_lock^2, sum_b z_key^2 (cosine metric)    */
  MVAE_BUF_COLDOT = 5,   /* float[L]:  sum_b draw_b n_lock n_key     (cosine metric)    */
  MVAE_BUF_DIST = 6,     /* float[B]: distance of the last forward                      */
  MVAE_BUF_GRADS_DEC = 7,/* decoder slice of g1 (ready first in mvae_backward)         */
  MVAE_BUF_DEAD = 8,     /* the never-trained decoder log-sigma variables               */
  MVAE_BUF_EPS = 9,      /* float[3,B,L]: eps of the last forward (given or generated).  */
                         /* A generated draw is regenerated inside the latent kernels and */
                         /* written to this buffer only when it is requested: the call    */
                         /* synchronises the device (hipDeviceSynchronize) and the pointer */
                         /* holds the draw of the forward BEFORE the call -- re-fetch it  */
                         /* after every forward whose eps you read.                        */
  MVAE_BUF_DYN = 10      /* int32[1] (count 1): nonzero when the last batch's pixels are
                            not all exact in bf16 (f32x: the layer-0 GEMMs then run all 6
                            plane pairs instead of 3; bf16/f32x: the BCE target is read in
                            fp32 instead of bf16); absent in f32 mode. The flag alternates
                            between two slots batch by batch: re-fetch the pointer after
                            each forward                                                    */
};

int mvae_abi_version(void);
/* Build id: the first 16 hex digits of the SHA-256 of the library's sources (magic_amd/csrc/*
 * and this header) at compile time (magic_amd/build.py source_hash). The Python loader refuses
 * a library whose id differs from the sources on disk, so a stale libmvae.so fails loudly. */
const char* mvae_build_id(void);
int mvae_create(const mvae_cfg* cfg, int device, mvae_ctx** out);
/* mvae_create with plan-time kernel switches (A/B and tests; NULL or "" = the defaults, which are
 * the measured best plans): "name=value[,name=value...]" with e8 (256-row bf16 GEMMs: 1 planner,
 * 0 ring kernels only, 2 the eight-phase kernel wherever a 256-row kernel runs), thin_ring (0-2),
 * valu (0/1), dact_planes (0/1), bce_split (0/1), plan_log (0/1: GEMM plans on stderr),
 * conv2_nchunk (> 0), enc_chain (0/1: bf16 mode, the encoder's hidden layers in one launch,
 * default 1), enc_chain_rows (its rows per workgroup, 16..96; 0 auto; both chains), dec_chain
 * (0/1: bf16 mode, the decoder's two hidden layers in one launch, default 1), bits (0/1: bf16 and
 * f32x modes, the layer-0 pixel operand of a 0/1 batch as one bit per pixel -- the de-interleave
 * writes BitMats instead of the bf16 plane and the eight-phase kernel expands the A fragments in
 * registers; a batch with another pixel value takes the planes; default 1), bits_reg (0/1: each
 * wave loads its A words straight to registers, else through an LDS copy of the block; default
 * 1), xbw_split (0/1/2: the weight gradient's BitMat transposed from the forward's on the side
 * stream instead of written by the de-interleave; 2 = where the layer-0 forward leaves CUs idle,
 * default), adam_nt (0/1: Adam's moments and fp32 parameters stored non-temporal, default 1), cs_one
 * (0-2: the cosine metric's column statistics in one launch, the last row chunk's workgroup
 * summing the partials in the two-launch order -- the same bits; 2, the default: where L <= 32),
 * x3 (0-2: f32x ring-kernel plans on the plane-stacked kernels, every operand plane of a k-tile in
 * LDS at once -- 1 the tile-N-128 plans, 2 also the 256x256 ones; the same products summed in
 * another order; default 2). Every option computes valid results.
 * An unknown name or a value out of range is MVAE_EINVAL; so are the names of removed kernel forms
 * (conv2_half, conv2_nw, conv2_tpb, conv2_fpw, conv2_wg: DESIGN.md 5w). The library reads no environment
 * variables (the diagnostics entry point mvae_bench_gemm aside). */
int mvae_create_ex(const mvae_cfg* cfg, int device, const char* options, mvae_ctx** out);
int mvae_destroy(mvae_ctx* ctx);
const char* mvae_last_error(mvae_ctx* ctx);   /* ctx may be NULL (creation errors) */

int mvae_param_count(mvae_ctx* ctx);
int mvae_param_info(mvae_ctx* ctx, int kind, int index, mvae_tensor* out);
int mvae_buffer(mvae_ctx* ctx, int which, float** ptr, size_t* count);
/* Optimizer step counters (TF beta1_power/beta2_power, kept on the host in fp32). */
int mvae_get_step(mvae_ctx* ctx, int64_t* t1, int64_t* t2);
int mvae_set_step(mvae_ctx* ctx, int64_t t1, int64_t t2);
/* Philox call counters of the internal N(0,1) sampler (eps == NULL): training draws
 * (mvae_forward / mvae_train_step) and inference draws (mvae_predict / mvae_reconstruct)
 * are separate streams, so evaluation never shifts the training noise; save both with a
 * checkpoint to resume the exact sequence. Counters must be < 2^63. */
/* Data parallelism: this rank's rows start at row_offset of the global batch (default 0).
 * The internal sampler then draws exactly this rank's slice of the eps a single process
 * would draw for the whole global batch. 0 <= row_offset <= global_batch - batch. */
int mvae_set_shard(mvae_ctx* ctx, int64_t row_offset);
int mvae_get_rng(mvae_ctx* ctx, uint64_t* train, uint64_t* eval);
int mvae_set_rng(mvae_ctx* ctx, uint64_t train, uint64_t eval);
/* Re-derive the bf16 plane images of the parameters from the fp32 masters: call after
 * writing parameters through mvae_param_info views (bf16 / f32x modes; no-op for f32). */
int mvae_sync_params(mvae_ctx* ctx, void* stream);

/* ---- training step, phase by phase --------------------------------------------- */
/* x: [B, 3*D] f32 HWC-interleaved (lock, rotated lock, key), 11a/overlap_input.py:117-119.
 * eps: [3, B, L] f32 in the reference's draw order (lock, rotated, key), or NULL to draw
 * from the context's counter-based generator (seed, call counter).                   */
int mvae_forward(mvae_ctx* ctx, const float* x, const float* eps, void* stream);
/* areas: [B] f32. Needs MVAE_BUF_COLSQ summed over ranks (cosine) before the call.    */
int mvae_metric(mvae_ctx* ctx, const float* areas, void* stream);
/* Needs MVAE_BUF_COLDOT summed over ranks (cosine). Writes MVAE_BUF_GRADS.           */
int mvae_backward(mvae_ctx* ctx, void* stream);
/* The same backward in mvae_backward_nparts(ctx) = R + 2 parts, R = option "wgrad0_chunks"
 * (0: decoder; 1: latent head, encoder dgrad chain and layer-0 weight-gradient chunk 0;
 * 2 .. R: layer-0 chunks 1 .. R-1; R + 1: the remaining encoder weight gradients). After
 * part k the ranges mvae_grad_range(ctx, k, i = 0, 1, ...) are final: a data-parallel host
 * all-reduces them while the later parts run (returns MVAE_EINVAL past the last range). Over
 * all parts the ranges cover MVAE_BUF_GRADS exactly once. */
int mvae_backward_nparts(mvae_ctx* ctx);
int mvae_backward_part(mvae_ctx* ctx, int part, void* stream);
int mvae_grad_range(mvae_ctx* ctx, int part, int index, float** ptr, size_t* count);
/* Schedule switches: "side_stream" (default 1) runs the weight gradients on a context-owned
 * side stream beside the dgrad chain, joined before the gradients they write are reported
 * final (mvae_backward / the end of each mvae_backward_part); "wgrad0_chunks" (1, 2, 4, 8;
 * default 1) splits the layer-0 weight gradient (40 MB of the 69 MB bucket at C4) into row
 * chunks that finish -- and can be all-reduced -- one after another; "early_adam" (default 0)
 * lets mvae_adam update the blocks after the layer-0 block on the side stream as soon as the
 * backward has written their gradients (beside the layer-0 weight gradient): only for callers
 * that neither read nor modify MVAE_BUF_GRADS between mvae_backward and mvae_adam (no
 * all-reduce): the caller's stream then joins the side stream in mvae_adam;
 * mvae_train_step uses it in the bf16 and f32x modes; "early_chunks" (1, 2, 4, 8; default 1):
 * with the early Adam and "wgrad0_chunks" 1, mvae_backward runs the layer-0 weight gradient in
 * that many row chunks and updates each chunk's parameter rows but the last's on the side stream
 * beside the next chunk's GEMM, i.e. already inside mvae_backward (so with early_adam the
 * parameters, their Adam state and MVAE_BUF_GRADS are not to be read between mvae_backward and
 * mvae_adam; 1: one GEMM, everything in mvae_adam); "bce_split" (default 1) runs a BCE head whose
 * 256x256 tiles leave a partial last round as the whole rounds plus 256x128 tiles for the rest
 * (bitwise the same results in bf16; in f32x equal to fp32 rounding: the two kernels sum the plane
 * pairs in different orders); "side_mask" (0-3, default 3): which weight gradients run on the side
 * stream -- bit 0 the decoder's, bit 1 the encoder's (a cleared bit: in order on the caller's
 * stream; the same results). */
int mvae_set_option(mvae_ctx* ctx, const char* name, int value);
/* Both TF ApplyAdam updates from MVAE_BUF_GRADS (theta -= d1(g1) + d2(g2)).           */
int mvae_adam(mvae_ctx* ctx, void* stream);
/* Single-GPU partial_fit: all four phases. losses_out: device float[5] or NULL;
 * dist_out: device float[B] or NULL.                                                  */
int mvae_train_step(mvae_ctx* ctx, const float* x, const float* areas, const float* eps,
                    float* losses_out, float* dist_out, void* stream);

/* ---- inference surface ------------------------------------------------------------ */
int mvae_predict(mvae_ctx* ctx, const float* x, const float* eps, float* dist_out, void* stream);
/* The same in two phases: a data-parallel host all-reduces MVAE_BUF_COLSQ (cosine metric)
 * between them, so every rank's distances use the global batch's column norms as the
 * single-process call on the whole batch does (8c/vae.py:449-450).                        */
int mvae_predict_encode(mvae_ctx* ctx, const float* x, const float* eps, void* stream);
int mvae_predict_finish(mvae_ctx* ctx, float* dist_out, void* stream);
/* transform: the lock image's latent mean only (no eps draw). */
int mvae_transform(mvae_ctx* ctx, const float* x, float* zmean_out, void* stream);
int mvae_reconstruct(mvae_ctx* ctx, const float* x, const float* eps, float* y_out, void* stream);
/* z: [n, L] (n <= B) -> y: [n, D] */
int mvae_generate(mvae_ctx* ctx, const float* z, int n, float* y_out, void* stream);

/* ---- batch producer (11a/overlap_input.py:127-261) -------------------------------- */
/* locks, keys: uint8 [n][H][W] (decoded PNGs, 0..255) on the device; idx: int [B] example
 * of each row; coef: float [B][4] = (cos, sin, x_off, y_off) of each row's rotation
 * (tf.contrib.image.rotate, computed on the host in fp32, 16-byte aligned).
 * Writes x_out [B, H*W*3] float32: per pixel (lock, rotated lock, key) / divisor
 * (255: inputs(normalize=True), 11a/overlap_input.py:113-115; 1: raw 0..255 pixels).       */
int mvae_make_batch(const unsigned char* locks, const unsigned char* keys, int height, int width,
                    const int* idx, const float* coef, int batch, float divisor, float* x_out,
                    void* stream);

/* ---- a batch described by its sources: no X ---------------------------------------- */
/* The batch mvae_make_batch would write, described instead of materialised: the uint8 tables
 * that already live in HBM, the example of each row and its rotation. Every entry point that takes
 * x has a *_pairs twin taking this descriptor; its results are bitwise those of mvae_make_batch
 * into an x followed by the x call, in every configuration.
 *
 * Direct path: where the context de-interleaves a 0/1 batch to bits in a launch of its own (bf16 /
 * f32x precision with the default "bits" and "e8" plans, FC encoder, batch % 64 == 0,
 * image_size^2 % 8 == 0) and both tables are 8-byte aligned,
 * one kernel writes the layer-0 bit operands straight from the tables (timing region
 * "pairs_bits"): 2 table bytes read per pixel triple instead of 12 bytes of X written and read
 * back. In every other configuration the twin materialises X into a context-owned [B, 3 D] fp32
 * scratch (allocated at the first such call, never at create) and runs the x code on it.
 *
 * Preconditions as for mvae_make_batch: every idx[b] in [0, n) (not checked: the kernels index the
 * tables with it), coef 16-byte aligned. height / width other than cfg.image_size, a null pointer,
 * a misaligned coef or a divisor <= 0 is MVAE_EINVAL with a message. The tables, idx and coef are
 * read by the kernels the call enqueues: keep them unchanged until those have run.             */
typedef struct mvae_pairs {
  const unsigned char *locks, *keys;  /* device, uint8 [n][H][W]                      */
  int height, width;                  /* must equal cfg.image_size                    */
  const int* idx;                     /* device int32 [B], each in [0, n)             */
  const float* coef;                  /* device float [B][4], 16-byte aligned         */
  float divisor;                      /* 255 (normalize) or 1                         */
} mvae_pairs;
int mvae_forward_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, const float* eps, void* stream);
int mvae_train_step_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, const float* areas, const float* eps,
                          float* losses_out, float* dist_out, void* stream);
int mvae_predict_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, const float* eps, float* dist_out,
                       void* stream);
/* (followed by mvae_predict_finish, as mvae_predict_encode) */
int mvae_predict_encode_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, const float* eps, void* stream);
int mvae_transform_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, float* zmean_out, void* stream);
int mvae_reconstruct_pairs(mvae_ctx* ctx, const mvae_pairs* pairs, const float* eps, float* y_out,
                           void* stream);

/* ---- any lock with any key: a key index of its own ----------------------------------- */
/* Additive to ABI 7 (the loader's build id rejects a stale library). Row b of a cross-pair batch is
 * lock p.idx[b], the rotation of that lock, and key key_idx[b]: the label of such a row is the
 * maximum overlap of that pair (mvae_overlap_pairs). The two tables may hold different numbers of
 * images, n locks and m keys of one height and width; the descriptor carries neither count and the
 * index ranges are the caller's precondition, as for mvae_make_batch (not checked: the kernels
 * index the tables with them). */
typedef struct mvae_xpairs {
  mvae_pairs p;        /* p.idx[b]: the lock (and rotated lock) of row b, in [0, n)            */
  const int* key_idx;  /* device int32 [B]: the key of row b, in [0, m); NULL: p.idx           */
} mvae_xpairs;         /* LP64: 56 bytes, key_idx at offset 48 */
/* mvae_make_batch with the key of row b taken from keys[key_idx[b]]; key_idx NULL or equal to
 * lock_idx gives the bits of mvae_make_batch. MVAE_EINVAL with a message beginning
 * "mvae_make_batch_x" for a null table, lock_idx, coef or x_out, a height, width or batch < 1, a
 * divisor <= 0 or a coef that is not 16-byte aligned. */
int mvae_make_batch_x(const unsigned char* locks, const unsigned char* keys, int height, int width,
                      const int* lock_idx, const int* key_idx, const float* coef, int batch,
                      float divisor, float* x_out, void* stream);
/* The twins of the *_pairs entry points, under their contract: results are bitwise those of
 * mvae_make_batch_x into an x followed by the x call, in every configuration. The direct kernel is
 * taken exactly where *_pairs takes it (the same conditions, timing region "pairs_bits": the same
 * kernels, which read the key's index from key_idx); everything else materialises into the
 * context's lazy [B, 3 D] scratch (region "pairs_make_batch"). Validation is that of *_pairs on
 * xpairs->p, the messages beginning with the entry point's name. */
int mvae_forward_xpairs(mvae_ctx* ctx, const mvae_xpairs* xpairs, const float* eps, void* stream);
int mvae_train_step_xpairs(mvae_ctx* ctx, const mvae_xpairs* xpairs, const float* areas, const float* eps,
                           float* losses_out, float* dist_out, void* stream);
int mvae_predict_xpairs(mvae_ctx* ctx, const mvae_xpairs* xpairs, const float* eps, float* dist_out,
                        void* stream);
int mvae_predict_encode_xpairs(mvae_ctx* ctx, const mvae_xpairs* xpairs, const float* eps, void* stream);
int mvae_transform_xpairs(mvae_ctx* ctx, const mvae_xpairs* xpairs, float* zmean_out, void* stream);
int mvae_reconstruct_xpairs(mvae_ctx* ctx, const mvae_xpairs* xpairs, const float* eps, float* y_out,
                            void* stream);

/* ---- retrieval: embed a gallery, score every lock against every key ------------------ */
/* Any number of single images from one uint8 table, encoded to their latent mean (and log-sigma):
 * what a trained metric model is used for. The call runs ceil(count / 3B) encoder passes; image t
 * of a pass (0 <= t < 3B) is row t of the context's stacked layer-0 operand, so every row of the
 * 3B-row encoder GEMMs carries a wanted image (mvae_transform carries one in three) and the rows
 * of the block mvae_transform copies from, [B, 2B), are bitwise what mvae_transform_pairs returns
 * for the same images as locks. Rows of the last pass at or past count are all-zero images: idx is
 * not read for them and nothing is written to the outputs past row count - 1.
 *
 * Direct path: exactly where the *_pairs twins take theirs (bf16 / f32x precision with the default
 * "bits" and "e8" plans, FC encoder, batch % 64 == 0, image_size^2 % 8 == 0) and the table is
 * 8-byte aligned, one kernel writes the layer-0 bit operand from
 * the table with three 8-byte loads per pixel octet (timing region "images_bits"). Every other
 * configuration materialises the pass as X -- x[b, 3 p + ch] = image((1, 0, 2)[ch] B + b)[p] /
 * divisor, the channel of stacked block 0, 1, 2 being the rotated lock's, the lock's, the key's --
 * into the context's lazily allocated [B, 3 D] scratch and runs the x code. Both routes give the
 * same bits where both exist.
 *
 * No eps is drawn and no RNG counter moves; the call leaves the context idle (as mvae_transform)
 * and may stand between two training steps without changing them. Preconditions as for
 * mvae_make_batch: every idx[i] in [0, n) (not checked: the kernels index the table with it); the
 * table and idx are read by the kernels the call enqueues. A null descriptor, table or zmean_out,
 * count < 1, a height / width other than cfg.image_size or a divisor <= 0 is MVAE_EINVAL with a
 * message. */
typedef struct mvae_images {
  const unsigned char* table;  /* device uint8 [n][H][W]                                        */
  int height, width;           /* must equal cfg.image_size                                     */
  const int* idx;              /* device int32 [count], each in [0, n); NULL: images 0..count-1 */
  float divisor;               /* 255 or 1, as mvae_pairs                                       */
} mvae_images;
/* zmean_out [count, L]; zlogsig_out [count, L] or NULL. */
int mvae_embed_images(mvae_ctx* ctx, const mvae_images* images, int64_t count, float* zmean_out,
                      float* zlogsig_out, void* stream);
/* zl [N, L], zk [M, L] fp32 device, row stride L. score(i, j) = the context's distance (cfg.metric,
 * cfg.reciprocal; 11a/vae.py:306-311, 444-458 taken to all pairs) between lock embedding i and key
 * embedding j: sqdiff raw = sum_l (zl[i,l] - zk[j,l])^2, summed in fp32 in that difference form;
 * cosine raw = sum_l (zl[i,l] rl[l]) (zk[j,l] rk[l]) with rl[l] = rsqrt(max(sum_i zl[i,l]^2, 1e-12))
 * over the N lock rows and rk the same over the M key rows (the galleries are the batch the
 * axis-0 l2_normalize ranges over; the column sums are taken in a fixed order; a NaN column sum is
 * clamped by the max to 1e-12 like a zero one, as in the step's metric kernel, so a NaN embedding
 * row leaves the norms numbers and makes only its own scores NaN); reciprocal: 1 / raw.
 * top_val / top_idx [N, k], 1 <= k <= min(M, 64): the k best keys of each lock in a total order --
 * by score (order +1: largest first, -1: smallest first), then by smaller j; NaN last for either
 * order. dist_out: NULL, or [N, M] to also store every score; top_val[i, r] is bit for bit
 * dist_out[i, top_idx[i, r]], and top_val / top_idx do not depend on whether dist_out is given nor
 * on how the call splits M over workgroups. With dist_out NULL no N x M buffer exists: the
 * workspace, O(N k splits) (+ O((N + M) L / 256) for the cosine norms), is allocated at the first
 * call that needs it and reused (growing it waits for the whole device first: an earlier call on
 * any stream may still read the old one). N, M >= 1, M < 2^31; else MVAE_EINVAL with a message. */
int mvae_match(mvae_ctx* ctx, const float* zl, int64_t N, const float* zk, int64_t M, int k, int order,
               float* dist_out, float* top_val, int* top_idx, void* stream);

/* ---- retrieval at gallery scale: a gallery in shards, fixed norms, key ranks --------------
 * Additive to ABI 7 (the loader's build id rejects a stale library). mvae_match is unchanged. All
 * five use the context's match workspace under mvae_match's growth rule; every invalid argument
 * is MVAE_EINVAL with a message starting with the entry point's name, before any launch or
 * allocation.
 *
 * Column sums of squares of a gallery in fp64, shard by shard: colsq [L] device doubles.
 * accumulate 0: colsq = this call's sum; 1: colsq += it. The n rows are summed as mvae_match sums
 * them (256-row chunks from row 0, four row quarters per column in turn, then the chunks in order
 * onto the running value). A gallery fed in shards whose row counts are multiples of 256 (the
 * last one free) therefore gives the bits of one call over all of it; other shard sizes agree to
 * fp64 rounding. n >= 1. */
int mvae_match_colsq(mvae_ctx* ctx, const float* z, int64_t n, double* colsq, int accumulate, void* stream);
/* rnorm[l] = (float)(1 / sqrt((double)max((float)colsq[l], 1e-12f))), l < L: the reciprocal column
 * norms mvae_match derives, bit for bit, when colsq came from mvae_match_colsq over the same rows. */
int mvae_match_rnorm(mvae_ctx* ctx, const double* colsq, float* rnorm, void* stream);

typedef struct mvae_match_opts {
  const float *rl, *rk;   /* cosine: reciprocal column norms [L] (device) of the lock / key side; NULL:
                             from the rows passed, as mvae_match. Each side on its own. Ignored for sqdiff. */
  int64_t key_base;       /* global index of zk row 0: top_idx holds key_base + j; ties break on the
                             global index; 0 <= key_base, key_base + M <= 2^31 - 1 */
  int carry;              /* 1: top_val / top_idx (and ahead) hold the result of earlier calls on
                             disjoint key ranges; the outputs are those of the union. 0: overwritten */
  int64_t dist_ld;        /* row stride of dist_out in floats; 0 = M; else >= M */
  const float* thr_val;   /* [N] \  all three or none: ahead[i] (+)= the number of keys of this call  */
  const int* thr_idx;     /* [N]  > strictly before (thr_val[i], thr_idx[i]) in the total order of    */
  int* ahead;             /* [N] /  `order` (score, then smaller global index; NaN last either way)   */
} mvae_match_opts;        /* LP64: 64 bytes; offsets 0, 8, 16, 24, 32, 40, 48, 56 */
/* mvae_match over one shard of the keys. opts NULL (or all zero) is mvae_match, except that k only
 * needs 1 <= k <= 64: a shard may hold fewer than k keys, and unfilled entries are the empty entry
 * (value bits 0x7FC00000, index -1), always at the end of a list. With carry the call merges its k
 * best into the list the outputs already hold (entries of index -1 never enter), so a sweep over
 * shards -- carry 0 on the first, 1 after -- leaves bit for bit what one mvae_match over the whole
 * gallery returns, in any shard order, provided the shards' key ranges [key_base, key_base + M)
 * are disjoint: that is the caller's precondition and is NOT checked (a key seen twice appears
 * twice). For cosine presets the scores equal the one-shot call's only under the same norms: pass
 * rl / rk computed over the whole galleries (mvae_match_colsq + mvae_match_rnorm); with fixed
 * norms a score no longer depends on which other rows are in the call. dist_out, if given, holds
 * this call's [N, M] block at row stride dist_ld (point it at column key_base of a wider matrix).
 * thr_*: the count of keys before a threshold entry, fused into the scoring pass (no matrix);
 * with (thr_val[i], thr_idx[i]) = (the score of lock i and its own key t, t) the accumulated
 * ahead[i] is the 0-based rank of key t for lock i. carry 0 overwrites ahead, 1 adds to it.
 * EINVAL: a null zl / zk / top_val / top_idx, N or M < 1, k outside [1, 64], order not +-1,
 * key_base < 0, key_base + M > 2^31 - 1, carry not 0 / 1, 0 < dist_ld < M (or < 0), one or two of
 * the thr_* trio. */
int mvae_match_ex(mvae_ctx* ctx, const float* zl, int64_t N, const float* zk, int64_t M, int k, int order,
                  const mvae_match_opts* opts, float* dist_out, float* top_val, int* top_idx, void* stream);
/* Row-aligned: out[i] = the score mvae_match(_ex) gives lock row i and a key row equal to zk[i], under
 * the same rl / rk -- the same bits, not merely close (one thread sums a row over l = 0 .. L - 1 in
 * order with the operations of the all-pairs kernel). NULL rl / rk (each on its own): norms over the
 * n rows passed. n >= 1. */
int mvae_pair_scores(mvae_ctx* ctx, const float* zl, const float* zk, int64_t n, const float* rl,
                     const float* rk, float* out, void* stream);
/* vals / idx [N][parts][k] (empty entries: idx -1) -> the k best of each row, top_val / top_idx
 * [N][k]: the merge step of mvae_match, for lists computed apart (other calls, other devices). The
 * indices must be distinct within a row. N, parts >= 1, 1 <= k <= 64, order +-1. */
int mvae_match_merge(mvae_ctx* ctx, const float* vals, const int* idx, int64_t N, int parts, int k, int order,
                     float* top_val, int* top_idx, void* stream);

/* ---- maximum overlap of a lock and a key: the label the distance is trained on -------------
 * Additive to ABI 7 (the loader's build id rejects a stale library).
 *   foreground   a table byte >= 128: Lb of the lock, Kb of the key
 *   Kr_r         Kb rotated by coef[r] = (cos, sin, x_off, y_off) exactly as mvae_make_batch rotates
 *                the lock (output (x, y) samples ((c x - s y) + x_off, (s x + c y) + y_off) in
 *                unfused fp32, roundf, zero fill)
 *   ov(r, dy, dx) = sum_{y,x} Lb[y, x] Kr_r[y - dy, x - dx],  |dy| <= H - 1, |dx| <= W - 1
 *   area = max ov;  pose = the lexicographically smallest (r, dy, dx) reaching it; (0, 0, 0) when
 *   the area is 0. Integer work: the result is exact.
 * Maximum overlap of lock lock_idx[i] and key key_idx[i], i < count.
 * locks, keys: device uint8 [n][H][W]; lock_idx / key_idx: device int32 [count] (NULL: i), not
 * checked, as for mvae_make_batch; coef: device float [n_rot][4], 16-byte aligned, shared by all
 * pairs; area_out: device int32 [count]; pose_out: device int32 [count][3] or NULL;
 * work: device buffer of mvae_overlap_work_bytes(...) bytes, 8-byte aligned (NULL allowed if that
 * is 0), one 8-byte partial per pair and chunk of angles: its contents need not survive the call.
 * Context-free, allocates nothing, enqueues on `stream`, like mvae_make_batch.
 * MVAE_EINVAL with a message (mvae_last_error(NULL)) beginning "mvae_overlap_pairs", before any
 * launch: a null table, coef or area_out, count < 1, n_rot outside 1 .. 2^24, height or width
 * outside 1 .. 256, a misaligned coef or work, work null while bytes are needed.
 * mvae_overlap_work_bytes returns 0 for arguments mvae_overlap_pairs refuses. */
size_t mvae_overlap_work_bytes(int64_t count, int n_rot, int height, int width);
int mvae_overlap_pairs(const unsigned char* locks, const unsigned char* keys, int height, int width,
                       const int* lock_idx, const int* key_idx, int64_t count,
                       const float* coef, int n_rot, int* area_out, int* pose_out,
                       void* work, void* stream);

/* ---- verified retrieval: a shortlist ordered by exact overlap, a key shown at its pose ---------
 * Additive to ABI 7. Context-free, allocate nothing, enqueue on `stream`, like mvae_overlap_pairs;
 * Lb, Kr_r, area and pose are those of the definition above, bit for bit.
 *
 * mvae_rerank: lock i of the call is lock lock_idx[i] (device int32 [N], NULL: i); cand: device int32
 * [N][R], the key index of each entry of its shortlist, a negative value being an empty entry, as
 * mvae_match_ex leaves them (it indexes no table and costs next to nothing). Pair (i, c) is that lock
 * with key cand[i][c]. Each row is then ordered by exact area: entry e gets rank = the number of
 * entries e' of the row with area' > area, or area' == area and column e' < e -- larger area first,
 * ties in cand's column order (the model's), empties (area -1) last in their column order; a key
 * listed twice in a row stays twice. Outputs, device int32, every slot written:
 *   key_out  [N][R]     the key at each rank, -1 for empties
 *   area_out [N][R]     its area, -1 for empties
 *   pose_out [N][R][3]  or NULL: its pose (r, dy, dx); 0, 0, 0 for empties
 *   from_out [N][R]     or NULL: the column of cand the entry came from
 * work: device buffer of mvae_rerank_work_bytes(...) bytes, 8-byte aligned (the overlap partials of
 * the N R pairs, the two expanded index lists, the unordered areas and poses): its contents need not
 * survive the call. The ranges of lock_idx and of the non-negative entries of cand are the caller's
 * precondition, not checked, as for mvae_overlap_pairs.
 * MVAE_EINVAL with a message (mvae_last_error(NULL)) beginning "mvae_rerank", before any launch: a null
 * table, cand, coef, key_out or area_out, N outside 1 .. 2^31 - 1, R outside 1 .. 64, n_rot outside
 * 1 .. 2^24, height or width outside 1 .. 256, a misaligned coef or work, a null work.
 * mvae_rerank_work_bytes returns 0 for arguments mvae_rerank refuses.
 *
 * mvae_overlap_place: for pair i < count of lock lock_idx[i] and key key_idx[i] (NULL: i, as for
 * mvae_overlap_pairs; not checked) and pose[i] = (r, dy, dx), device int32 [count][3]:
 *   P[y, x]     = Kr_r[y - dy, x - dx] inside the image, 0 outside
 *   overlay_out   device uint8 [count][H][W] or NULL: byte = (Lb ? 1 : 0) | (P ? 2 : 0)
 *   stats_out     device int32 [count][4] or NULL: (|Lb|, |Kr_r|, |P|, |Lb & P|); for a pose of
 *                 mvae_overlap_pairs or mvae_rerank the last is that call's area
 * A pose out of range (r outside [0, n_rot), |dy| >= H or |dx| >= W) is defined: no coef entry and
 * no key pixel is read, the overlay is the lock alone and the stats are (|Lb|, -1, -1, -1).
 * MVAE_EINVAL with a message beginning "mvae_overlap_place", before any launch: a null table, coef or
 * pose, both outputs null, count < 1, n_rot outside 1 .. 2^24, height or width outside 1 .. 256, a
 * misaligned coef. */
size_t mvae_rerank_work_bytes(int64_t N, int R, int n_rot, int height, int width);
int mvae_rerank(const unsigned char* locks, const unsigned char* keys, int height, int width,
                const int* lock_idx, const int* cand, int64_t N, int R,
                const float* coef, int n_rot,
                int* key_out, int* area_out, int* pose_out, int* from_out,
                void* work, void* stream);
int mvae_overlap_place(const unsigned char* locks, const unsigned char* keys, int height, int width,
                       const int* lock_idx, const int* key_idx, int64_t count,
                       const float* coef, int n_rot, const int* pose,
                       unsigned char* overlay_out, int* stats_out, void* stream);

/* ---- diagnostics ------------------------------------------------------------------ */
/* HIP-event timing of named regions (one GEMM incl. its split-K reduction, or one
 * bandwidth kernel group), recorded on the launch stream while enabled.               */
int mvae_timing_enable(mvae_ctx* ctx, int on);
/* Restrict recording to one region (-1: all regions, the default): a timed loop can carry the
   events of the one kernel it reports without the event pairs of every other region. */
int mvae_timing_select(mvae_ctx* ctx, int region);
/* Profiler runs: bracket every launch of `region` with an empty marker kernel of
 * 4096 + region workgroups, so a rocprofv3 kernel trace can attribute dispatches (and their
 * counters) to the region. Off by default. */
int mvae_timing_marker(mvae_ctx* ctx, int region, int on);
int mvae_timing_regions(mvae_ctx* ctx);
const char* mvae_timing_name(mvae_ctx* ctx, int region);
int mvae_timing_read(mvae_ctx* ctx, int region, double* total_ms, int64_t* count);
int mvae_timing_reset(mvae_ctx* ctx);
/* One GEMM of the step's kernel family: C[M,N] = epi(A[M,K] B[K,N]); A stored [M][K]
 * (at=0) or [K][M] (at=1), B stored [K][N] (bt=0) or [N][K] (bt=1). epi: 0 store,
 * 1 act (act: 0 tanh, 1 elu), 2 C = acc * act'(aux), 4 sigmoid; epi | (prec << 4) |
 * (variant << 8) selects the arithmetic (MVAE_PREC_*) and the kernel (the table of kernel numbers
 * at mvae_debug_plan below; 0 the planner's choice). Workspace is allocated and freed inside
 * (synchronous; tests only).
 * mvae_bench_gemm times `iters` launches of one shape on operands it makes itself (average ms in
 * *avg_ms). Its variant:
 *    bits 0-3    the kernel number (the same table)
 *    bits 4-7    prec (MVAE_PREC_*)
 *    bits 8-11   epi, with the operands the step's epilogue reads (0 store, 1 act, 2 dact, 3 BCE,
 *                4 sigmoid)
 *    bits 12-19  refused: MVAE_EINVAL with a message, before anything is allocated (they selected
 *                kernel timing diagnostics that were removed)
 *    bit 20      A of 0/1 values (in f32x its residual planes then zero)
 *    bit 21      with bit 20: A also as a BitMat, the eight-phase kernel's bits path
 * Of the environment it reads MVAE_BENCH_LDPAD, MVAE_BENCH_SPLIT, MVAE_BENCH_TILE_GROUP and
 * MVAE_BENCH_PLANES_ONLY. */
int mvae_bench_gemm(int M, int N, int K, int at, int bt, int batch, int variant, int iters,
                    void* stream, float* avg_ms);
/* Diagnostics: the step's de-interleave of a [B][3D] batch of random 0/1 pixels, iters launches
 * (B % 64 == 0, D % 8 == 0): variant 0 the step's bits form (the pixel operand as BitMats), 7 the
 * same without the weight-gradient words (the xbw_split form), 100 the bf16-plane pass; + 1000 four
 * X images in turn, + 2000 / + 4000 a GEMM / memset heater before each launch. Any other variant is
 * MVAE_EINVAL. Average ms per launch in *avg_ms.                                              */
int mvae_bench_deint(int B, int D, int variant, int iters, void* stream, float* avg_ms);
/* One 5x5x64x64 conv kernel of the conv tower on caller data (tests; synchronous): S1 x S1 x 64
 * NHWC images, B rows (3B forward images, 4B backward). mode 0: relu(conv(x, W2) + b2), 3B
 * images, y = W2 block [1601][64]; mode 1: data gradient of x (4B images), y = W2; mode 2:
 * out[2][1601][64] = the cost / metric weight gradients of x = conv2 input (3B), y = d pre-
 * activation (4B). mfma bit 0: bf16 MFMA kernels (operands rounded to bf16), else fp32 VALU.
 * Bits 1-6 are refused: MVAE_EINVAL with a message, before anything is allocated (they selected
 * kernel forms that were removed). Bits 8-19: the weight gradient's
 * chunk count (mode 2): 0 the step's defaults min(2B, 32) VALU / min(2B, 64) MFMA, else
 * min(2B, value) for both; the slab is sized from it and prefilled with NaN bits.          */
int mvae_debug_conv2(int S1, int B, int mode, int mfma, const float* x, const float* y, float* out,
                     void* stream);
/* The bit operands of a batch of S x S images on caller buffers (tests; synchronous; allocates
 * nothing). mode 0: mvae_make_batch into x [B][3 S S], then the step's de-interleave to bits;
 * mode 1: the direct kernel of the *_pairs entry points; mode 2: the direct kernel of
 * mvae_embed_images -- locks is the one table, idx holds 3B entries (the images of stacked rows
 * 0 .. 3B - 1), keys and coef are not read; mode 3: the step's de-interleave alone on the caller's
 * x (mode 2's reference). no_xbw: the forward words only (the
 * xbw_split schedule). Outputs, zero-filled by the caller (padding is never written): xbf
 * ceil(3B/256) ceil((D+1)/64) 512 words, xbw ceil((D+1)/256) ceil(3B/64) 512 words, xbits
 * [B][ldbits] bytes, dyn 4 ints (slot 0: words 0 inexact, 2 not-binary), and -- written only when
 * the not-binary word rises -- plane 0 of the bf16 image plane [3B][ldx]. B % 64 == 0,
 * S S % 8 == 0, ldx % 8 == 0, tables 8-byte and coef 16-byte aligned, else MVAE_EINVAL.        */
int mvae_debug_pairs_bits(const unsigned char* locks, const unsigned char* keys, const int* idx,
                          const float* coef, int B, int S, float divisor, int mode, int no_xbw, float* x,
                          unsigned* xbf, unsigned* xbw, unsigned char* xbits, int ldbits, int* dyn,
                          unsigned short* plane, int ldx, void* stream);
/* mvae_debug_pairs_bits, modes 0 and 1 only, with the key of each row from key_idx (NULL: idx);
 * keys may hold another number of images than locks. */
int mvae_debug_xpairs_bits(const unsigned char* locks, const unsigned char* keys, const int* idx,
                           const int* key_idx, const float* coef, int B, int S, float divisor, int mode,
                           int no_xbw, float* x, unsigned* xbf, unsigned* xbw, unsigned char* xbits,
                           int ldbits, int* dyn, unsigned short* plane, int ldx, void* stream);
int mvae_debug_gemm(int M, int N, int K, const float* A, int lda, int at, const float* B, int ldb,
                    int bt, float* C, int ldc, int epi, int act, const float* aux, int ld_aux,
                    void* stream);
/* One per-pixel kernel of the conv tower (conv_tower.hip) on caller data, through the step's own
 * launcher (tests; synchronous; only mode 3 allocates: its slab, prefilled with NaN bits). S: image
 * size (a multiple of 4 in 4..100), S1 = S/2, S2 = S/4; images are NHWC with 64 channels; n <= 16384.
 *  mode 0, conv1 + ReLU + pool 1 + LRN 1 of n images: in0 = pixels [n][ld] (ld >= S S), in1 = the
 *    conv1 block [26][64] -> out0 = p1 [n][S1 S1 64], arg_out = arg1 (same shape, bytes 0..3),
 *    out1 = n1 fp32 and / or outb = its bf16 image (either may be NULL, not both). opt = 0.
 *  mode 1, LRN 2 + pool 2 of n images: in0 = a2 [n][S1 S1 64] -> arg_out = arg2 [n][S2 S2 64] and
 *    feature rows [n][ld] (ld >= S2 S2 64; columns from S2 S2 64 on are never written): out0 fp32
 *    when opt & 1, outb = opt >> 1 (0, 1 or 3) bf16 planes [planes][n][ld].
 *  mode 2, pool 2 + LRN 2 + ReLU backward, batch n: in0 = dxf [4n][ld], in1 = a2 [3n][S1 S1 64],
 *    arg_in = arg2 [3n][S2 S2 64] -> out0 = da2 [4n][S1 S1 64] fp32 and / or outb = its bf16 image
 *    (backward image j reads forward image j < 2n ? j : j - n). opt = 0.
 *  mode 3, conv1 weight gradient, batch n: in0 = dn1 [4n][S1 S1 64], in1 = p1 [3n][S1 S1 64],
 *    arg_in = arg1 (p1's shape), xs = pixels [3n][ld] -> out0, out1 = the cost / metric gradient
 *    blocks [26][64]. opt: the chunk count, 0 = the step's min(2n, 1024), else min(2n, opt).
 * Buffers a mode does not name are not touched. MVAE_EINVAL with a message, before any HIP call:
 * another mode, S, n, ld or opt, or a NULL among the buffers the mode names.                    */
int mvae_debug_tower(int mode, int S, int n, int ld, int opt, const float* in0, const float* in1,
                     const float* xs, const unsigned char* arg_in, float* out0, float* out1,
                     unsigned short* outb, unsigned char* arg_out, void* stream);
/* The fused hidden-layer chain (enc_chain.hip) on caller data (tests; synchronous; allocates nothing).
 * x [M][ldx] bf16, layer l: w[l] [K[l]][ldw[l]] bf16 -> out[l] [M][ldo[l]] bf16. K, N, ldw, ldo, w, out are
 * HOST arrays of nl entries holding device pointers / sizes. rows: 0 auto, or 16..96 (multiple of 16).
 * out[l] = act(in_l w[l]) with in_0 = x and in_l = out[l-1] (so K[l] = N[l-1] + 1 in the step); column
 * N[l] of out[l] is 1.0 (the next layer's bias input), columns up to round8(N[l] + 1) are 0, nothing
 * else is written. Columns K[0] .. ldx - 1 of x must be zero. act: 0 tanh, 1 elu. MVAE_EINVAL with a
 * message, before any HIP call: nl outside 1..4, M < 1, K[l] outside 1..512 (K[0] <= ldx), N[l]
 * outside 1..511, a stride that is not a multiple of 8, ldw[l] < round8(N[l]),
 * ldo[l] < round8(N[l] + 1), a null or not 16-byte aligned pointer, another act, a bad rows. */
int mvae_debug_chain(int M, int nl, const int* K, const int* N, int act, int rows,
                     const unsigned short* x, int ldx, const unsigned short* const* w, const int* ldw,
                     unsigned short* const* out, const int* ldo, void* stream);
/* One kernel of the latent head (mvae_kernels.hip) on caller data, through the step's own launcher
 * (tests; synchronous; allocates nothing). Every pointer is a device pointer; a buffer the mode does
 * not name is not read (it may be NULL). B rows of this rank, L latent columns, global batch Bg
 * (inv_bg = 1 / Bg as the step forms it). Stacked rows are [rot | lock | key].
 *  eps source (modes FWD and BWD): eps [3][B][L] in the reference's slot order (lock, rot, key), or
 *    NULL: the Philox stream (seed, counter) at this rank's rows off .. off + B - 1 of Bg.
 *  MVAE_HEAD_FWD: ms [3B][2L] -> rowfwd [B][4]; z [3B][ldz] fp32 lock rows when zmask & 2, key rows
 *    when zmask & 4 (zmask in {0, 2, 4, 6}); z_planes (0, 1 or 3) bf16 planes of the lock rows into
 *    zp [z_planes][3B][ldz]. Rot rows, pad columns and unselected rows are never written.
 *  MVAE_HEAD_COLSTATS: cs_mode 0, out [2L] = column sums of squares of z's lock | key rows; cs_mode 1,
 *    out [L] = coldot from z, colsq [2L] and draw [B]. part: colstats_nchunk(B) = ceil(B / 128) rows
 *    of 2L (cs_mode 0) or L floats. cnt: NULL (two launches), or ceil(ncols / 64) zeroed ints (one
 *    launch; left zeroed).
 *  MVAE_HEAD_METRIC: z, rowfwd, rowpart [B][nblk], areas [B] or NULL (zeros), colsq (cosine only);
 *    metric 0 cosine / 1 sqdiff, recip, w -> rowvals [B][4], dist [B], draw [B].
 *  MVAE_HEAD_LOSS: rowvals [B][4] -> losses[0..4].
 *  MVAE_HEAD_BWD: ms, eps source, dzdec [B][L], draw [B], and for the cosine colsq [2L], coldot [L];
 *    metric, w -> dhead [4B][ldh] fp32 (or NULL) and h_planes (0, 1 or 3) bf16 planes
 *    hp [h_planes][4B][ldh]; columns from 2L on are never written.
 * MVAE_EINVAL with a message, before any HIP call: args NULL, another mode, B < 1, L < 1, Bg < B, a
 * stride smaller than the row (ldz < L, ldh < 2L), a bad zmask / plane count / cs_mode / metric /
 * nblk, off outside [0, Bg - B] with regenerated eps, a NULL among the buffers the mode names,
 * neither dhead nor planes in MVAE_HEAD_BWD, or a pointer that is not 16-byte aligned where the
 * kernel's 16-byte form is chosen (L % 4 == 0 with ldz % 4 == 0, resp. ldh % 4 == 0; rowfwd and
 * rowvals always).                                                                              */
enum { MVAE_HEAD_FWD = 0, MVAE_HEAD_COLSTATS = 1, MVAE_HEAD_METRIC = 2, MVAE_HEAD_LOSS = 3, MVAE_HEAD_BWD = 4 };
typedef struct mvae_head_args {
  int mode, B, L, Bg, ldz, ldh;
  int off;                          /* regenerated eps: this rank's first row */
  int zmask, z_planes, h_planes;
  int cs_mode, nblk, metric, recip;
  float w;                          /* deformation weight */
  unsigned long long seed, counter; /* regenerated eps */
  const float* ms;
  const float* eps;
  const float* areas;
  const float* rowpart;
  const float* dzdec;
  float* z;
  unsigned short* zp;
  float* rowfwd;
  float* colsq;
  float* coldot;
  float* draw;
  float* part;
  int* cnt;
  float* out;
  float* rowvals;
  float* dist;
  float* losses;
  float* dhead;
  unsigned short* hp;
} mvae_head_args;
int mvae_debug_head(const mvae_head_args* args, void* stream);
/* One GEMM with a fused epilogue of the step on caller data, through gemm_run (tests; synchronous;
 * allocates the operands' bf16 planes and a split-K workspace, nothing the epilogue touches). Every
 * pointer is a device pointer; a zeroed field is a NULL / 0 argument. v = A B with A [M][lda] and
 * B [K][ldb], or [N][ldb] with bt, in fp32; prec 0 fp32, 1 bf16, 2 f32x (the operands' planes are
 * split here); variant: a kernel number (mvae_debug_plan's table: 0, 3, 4, 10, 11, 12 or 13); x3: the
 * plane-stacked kernel where it serves. The output goes to du [M][ldc] fp32 (or NULL) and to ncp
 * (0, 1 or 3) bf16 planes cp [ncp][pc], same ld.
 *  MVAE_EPI_ACT: out = act(v). MVAE_EPI_DACT: out = v act'(aux[r']) with aux [.][ld_aux] fp32, or its
 *    bf16 image auxp (same ld) when set; r' = r < remap_split ? r : r - remap_shift (zeroed: r' = r),
 *    so aux holds max(min(M, remap_split), M - remap_shift) rows. padw 1 / 2 (both modes): the
 *    padding columns [N, round8(N)) may be read (aux) and written as whole 8-column chunks, 1.0 at
 *    column N with padw 2, else 0: every ld then a multiple of 8, at least round8(N).
 *  MVAE_EPI_BCE: y = sigmoid(v); rowpart[r][rp_off + b] = -sum over the columns of 128-column block
 *    b of x log y + (1 - x) log(1 - y) (each product 0 where its factor is 0; no epsilon), rowpart
 *    [M][rp_ld] (rp_ld 0: ceil(N / 128), rp_off then 0); out = (y - x) scale; y [M][ldy] or NULL.
 *    The target: x [M][ldx] fp32, always given; in the plane modes also xp, its bf16 plane (same
 *    ld), read instead while dyn[0] == 0, and xbits [M][ldbits] (byte c of a row = columns 8c .. 8c
 *    + 7, bit j = column 8c + j nonzero), read instead while dyn[2] == 0; dyn: 4 ints, the
 *    de-interleave's flag words (mvae_debug_pairs_bits). split_c0 > 0 (plane modes): two launches
 *    as the step's split head makes them, columns [0, c0) on the requested variant and [c0, N) on
 *    the ring kernel at tile N 128.
 * MVAE_EINVAL with a message, before any HIP call: args NULL, another mode / act / prec / variant /
 * x3, a size < 1, a stride smaller than its row, ncp not 0, 1 or 3, neither du nor planes, pc <
 * M ldc, a bad remap or padw, BCE with rowpart NULL, rp_ld < rp_off + ceil(N / 128) (rp_ld 0: rp_off
 * != 0), split_c0 not a multiple of 256, leaving fewer than 128 columns or in fp32 precision, xp or
 * xbits without dyn, xbits without xp, ldbits < ceil(N / 8), a NULL among the buffers a mode names. */
enum { MVAE_EPI_ACT = 1, MVAE_EPI_DACT = 2, MVAE_EPI_BCE = 3 };
typedef struct mvae_epi_args {
  int M, N, K;
  int lda, ldb, bt;
  int prec, variant, x3;
  int epi, act;
  int ldc, ncp;
  int ldx, ldbits, ldy;             /* BCE */
  int rp_ld, rp_off, split_c0;
  int ld_aux, remap_split, remap_shift; /* DACT */
  int padw;                         /* ACT / DACT */
  float scale;                      /* BCE */
  long long pc;                     /* plane stride of cp, elements */
  const float* A;
  const float* B;
  float* du;
  unsigned short* cp;
  const float* x;
  const unsigned short* xp;
  const int* dyn;
  const unsigned char* xbits;
  float* y;
  float* rowpart;
  const float* aux;
  const unsigned short* auxp;
} mvae_epi_args;
int mvae_debug_epi(const mvae_epi_args* args, void* stream);
/* Which kernel a GEMM would run on, and how: the plan gemm_run would launch for these arguments,
 * computed on the host alone (no HIP call, no GPU needed; a pointer is never followed, only its
 * low four bits are read). Tests pin the planner with it (tests/test_gemm_plan.py).
 * In: the shape, layouts and strides (elements); prec as mvae_debug_gemm's, nA / nB operand planes,
 * dynA != 0: A's residual planes flagged at run time; epi 0 store, 1 act, 2 dact, 3 BCE, 4 sigmoid
 * with the GemmEpi fields the choice reads (cp / auxp / xp non-NULL: set; c32, xdyn, padw); abits:
 * A also given as bits; x3 as mvae_debug_epi's; tm 0 / 192 / 256 and split > 0 forced; valu != 0
 * the fp32 VALU kernel forced; variant: the table below; max_ws: the workspace in floats (0: none),
 * at ws.
 * Out: kernel (MVAE_KERNEL_*), staging (the 128x128 kernels' diagnostic forms 1 / 2), the tile tm x
 * tn, the grid's ntm x ntn tiles and tile order group, split and kchunk (k per slice), lds_epilogue
 * (the row-major epilogue through LDS, else the accumulator layout's), vec_epilogue (its 16-byte
 * accesses), epi_launched (the kernel instantiation: 0-4, 5 BCE choosing its target form at run
 * time, 6 dact reading the bf16 aux), ws_elems (floats of split-K slabs), valu_fits (the step's
 * wiring would move this GEMM to the VALU kernel), refused (gemm_run returns an error: the slabs
 * exceed max_ws).
 * MVAE_EINVAL with a message: NULL arguments, sizes < 1, prec / epi / variant / tm / x3 out of range.
 *
 * The kernel numbers ("variant") of mvae_debug_gemm, mvae_bench_gemm, mvae_debug_epi and this call;
 * 9 is not in mvae_debug_epi; a number above 15 does not exist. Inside the library they are named forces:
 *    0      the planner decides
 *    1, 2   the 128x128 kernels (fp32 or bf16-plane by prec) in their diagnostic staging forms
 *           (store epilogue only; another epilogue runs the default form)
 *    3      the ring kernels on any shape, never the eight-phase kernel
 *    4      the 128x128 kernels
 *    5, 7, 8 (once timing forms; tests pass them) the ring kernel at 256x256 tiles where the default
 *           shape rules but the one-k-tile exclusion admit a 256-row kernel, with the split the
 *           planner chose for its own tile
 *    6      the eight-phase kernel on any shape where its 32-bit offsets fit (else: 13 on output
 *           dimensions >= 128, the unsplit 256x256 ring tile below)
 *    9      the fp32 VALU kernel (prec then 0); not in mvae_debug_epi
 *    10     default shape rules, ring kernels only, accumulator-layout epilogue
 *    11, 12 default shape rules, ring kernels only at tile N 128 / 256
 *    13, 14 the eight-phase kernel on any shape where its 32-bit offsets fit, else the ring kernels
 *    15     default shape rules, ring kernels only
 * Any number but 0 keeps the step's
 * wiring from choosing the VALU kernel, and only 0 lets A-as-bits prefer the eight-phase kernel. */
enum { MVAE_KERNEL_F32 = 1, MVAE_KERNEL_VALU = 2, MVAE_KERNEL_PLANE = 3, MVAE_KERNEL_RING = 4,
       MVAE_KERNEL_X3 = 5, MVAE_KERNEL_E8 = 6 };
typedef struct mvae_plan_args {
  int M, N, K, batch, at, bt;
  int lda, ldb, ldc;
  int prec, nA, nB, dynA;
  int epi, c32, xdyn, padw;
  int ld_aux, ldx, ldy;
  int abits, x3;
  int tm, split, valu, variant;
  long long pA, pB, sA, sB, sC, pc;  /* plane and batch strides */
  unsigned long long max_ws;
  const void* Ap;
  const void* Bp;
  const void* C;
  const void* cp;
  const void* aux;
  const void* auxp;
  const void* x;
  const void* xp;
  const void* y;
  const void* ws;
} mvae_plan_args;
typedef struct mvae_plan_out {
  int kernel, staging, tm, tn, ntm, ntn, group, split, kchunk;
  int lds_epilogue, vec_epilogue, epi_launched, valu_fits, refused;
  unsigned long long ws_elems;
} mvae_plan_out;
int mvae_debug_plan(const mvae_plan_args* args, mvae_plan_out* out);
/* One batched GEMM on caller data, through gemm_run (tests; synchronous; additive to ABI 7): what
 * mvae_debug_gemm does, with the dimensions it fixes -- the batch and its strides, a forced split-K,
 * the tile order, the operand images' alignment. A, B, C are fp32 device buffers of a_elems, b_elems,
 * c_elems elements; element b of the batch reads A + b sA ([M][lda], or [K][lda] with at), B + b sB
 * ([K][ldb], or [N][ldb] with bt) and writes C + b sC ([M][ldc]). The bf16 planes of the plane modes
 * are split here over the whole A and B buffers (so the batch windows of A and of B may overlap) and
 * start a_off / b_off elements (0..7) past a 16-byte boundary; the split-K workspace is allocated
 * here and filled with NaN bits before the launch. A zeroed field is its default.
 *  prec 0 fp32, 1 bf16, 2 f32x; variant: a kernel number (mvae_debug_plan's table); x3: the
 *  plane-stacked kernel where it serves; tm 0 / 192 / 256: the ring tile's rows; split 0: the planner's.
 *  group: the tile order of the 256-row kernels -- 0 the planner's, g > 0 bands of g m-tiles, -1 row by row.
 *  epi 0 store, 1 act (act 0 tanh, 1 elu).
 *  bits 1 / 2 (plane modes, A of 0/1 values): A also as a BitMat, read by the eight-phase kernel through
 *  LDS / into registers. bits_shared 0: one BitMat of M x K per batch element. bits_shared 1 (at = 1, sA
 *  a multiple of 64 lda): one BitMat of the whole stored A, element b at k-tile b sA / (64 lda) of every
 *  strip -- the form of the step's layer-0 weight gradient.
 *  a_dyn (prec 2 only): A's run-time flag, the de-interleave's inexact word (GemmDesc::dynA) -- 0 none
 *  (every plane pair runs), 1 a device word holding 0 (the kernels run only the leading pairs with A's
 *  plane 0, as the step does for a batch of bf16 values), 2 a word holding 1.
 * *plan (or NULL) receives the plan gemm_run launched.
 * MVAE_EINVAL with a message, before any HIP call: args or a buffer NULL, a size < 1, a stride smaller
 * than its row, a negative batch stride, an extent smaller than (batch - 1) s + rows ld, output
 * windows that overlap (batch > 1 and sC < (M - 1) ldc + N), prec / variant / x3 / tm / epi / act /
 * bits / group / an offset out of range, split < 0, bits in fp32 (prec 0 or variant 9), bits_shared
 * without bits, at = 1 and sA a multiple of 64 lda, a_dyn outside 0..2 or with prec != 2. */
typedef struct mvae_gemm_args {
  int M, N, K, batch, at, bt;
  int lda, ldb, ldc;
  int prec, variant, x3, tm, split, group;
  int epi, act;
  int bits, bits_shared;
  int a_off, b_off;
  long long sA, sB, sC;             /* batch strides, elements */
  long long a_elems, b_elems, c_elems;
  const float* A;
  const float* B;
  float* C;
  int a_dyn;                        /* f32x: A's run-time flag (GemmDesc::dynA); 0 none, 1 a word of 0, 2 of 1 */
} mvae_gemm_args;
int mvae_debug_gemm_ex(const mvae_gemm_args* args, mvae_plan_out* plan, void* stream);
/* The plane side of batch input on caller data, through one of the step's launchers (tests;
 * synchronous; allocates nothing; additive to ABI 7). Every pointer is a device pointer; a buffer the
 * route does not name is not read (it may be NULL). A batch of B rows of H x W images, D = H W; the
 * stacked rows are [rot | lock | key], 3B rows of ldx elements.
 *  route 0  launch_deinterleave (the plane path) on x [B][3D] fp32: the alignment of x, D and ldx choose
 *           the 8-pixel, 4-pixel or scalar form; any D >= 1
 *  route 1  launch_deint_bits on x
 *  route 2  launch_pairs_bits on the uint8 tables locks, keys with idx [B], key_idx [B] (NULL: idx),
 *           coef [B][4] and divisor
 *  route 3  launch_images_bits on the one table in locks with idx [3B] and divisor
 * np (0, 1 or 3): the bf16 planes written into planes [np][plane_stride]; 0 (route 0 only): no plane
 * image, the fp32 precision's form. xs [3B][ldx]: the fp32 rows of the blocks in f32mask (route 0
 * only; bit c: block c) and, once the inexact flag has risen, of those in f32dyn_mask; required only
 * when a mask names a block. xbits [B][ldbits]: the lock block as bits (optional on route 0). xbf, xbw
 * (routes 1-3; xbw may be NULL with no_xbw): the BitMats of mvae_debug_pairs_bits, zero-filled by the
 * caller. dyn: the 4 flag ints; the launch gets dyn + slot as its flags (the inexact word dyn[slot],
 * the not-binary word dyn[2 + slot], both zero on entry) and zeroes the other slot (dyn[1 - slot],
 * dyn[3 - slot]). x_elems, xs_elems, planes_elems, xbits_elems: the extents of those buffers.
 * MVAE_EINVAL with a message, before any HIP call: args or a required buffer NULL, route / np / slot /
 * a mask out of range, np 0 or f32mask != 0 on routes 1-3, a size < 1, ldx < D, ldbits < D / 8 where
 * bits are written, an extent smaller than B rows of 3D (x), 3B rows of ldx (xs; times np planes at
 * plane_stride: planes) or B rows of ldbits, xs or planes not 16-byte aligned, or a shape or alignment
 * the bits route does not serve (B % 64, D % 8, ldx % 8, x 16-byte, tables 8-byte, coef 16-byte). */
typedef struct mvae_input_args {
  int route, B, H, W;
  int ldx, np, f32mask, f32dyn_mask;
  int ldbits, no_xbw, slot;
  float divisor;
  long long plane_stride;           /* elements between two planes */
  long long x_elems, xs_elems, planes_elems, xbits_elems;
  const float* x;
  const unsigned char* locks;
  const unsigned char* keys;
  const int* idx;
  const int* key_idx;
  const float* coef;
  float* xs;
  unsigned short* planes;
  unsigned char* xbits;
  unsigned* xbf;
  unsigned* xbw;
  int* dyn;
} mvae_input_args;
int mvae_debug_input_planes(const mvae_input_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVAE_H_ */
