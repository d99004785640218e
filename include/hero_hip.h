/* hero_hip.h — C ABI of libhero_hip.so: hand-written HIP (gfx950 / MI355X) kernels for the
 * HERO hierarchical-encoder hot path (linjieli222/HERO: model/layers.py, model/encoder.py,
 * model/embed.py, model/model.py, optim/adamw.py).
 *
 * Conventions
 *   - plain pointers + sizes, no framework types; every pointer is DEVICE memory unless noted;
 *   - every entry point returns 0 on success or a negative HERO_ERR_* code; the message is
 *     available from hero_last_error() (thread-local, valid until the next failing call);
 *   - nothing allocates, nothing synchronises: work is enqueued on `stream` (a hipStream_t);
 *     scratch memory is passed in by the caller (see the *_workspace_bytes queries);
 *   - `dtype` is the ACTIVATION element type: HERO_F32 (exact-f32 MFMA path used for the parity
 *     gate) or HERO_BF16 (bf16 storage + bf16 MFMA, fp32 accumulation). Parameters that are
 *     small (bias, LayerNorm affine, embedding tables) are always fp32; GEMM weight operands are
 *     in the activation dtype; parameter gradients are always fp32;
 *   - row-major everywhere, leading dimensions in ELEMENTS.
 *
 * Each declaration cites the reference code (file:line in linjieli222/HERO) it replaces.
 */
#ifndef HERO_HIP_H_
#define HERO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hero_stream_t; /* hipStream_t */

enum { HERO_F32 = 0, HERO_BF16 = 1 };
enum { HERO_OK = 0, HERO_ERR_ARG = -1, HERO_ERR_LAUNCH = -2, HERO_ERR_UNSUPPORTED = -3 };

const char* hero_last_error(void);
/* ABI version of the structs and entry points below; a binding compiled against another version must refuse to run
 * (hero_amd/_lib.py does).  History: 1 = rounds 1-3.  2 = INCOMPATIBLE struct changes of round 4 - HeroQueryPool.dw is
 * [B, D] and OVERWRITTEN (was [D], accumulated), HeroStEd gained the required zero-initialised `ws`, HeroColsum gained
 * row_cols / dst_rows.  3 = the round-5 struct changes that went out under "2" by mistake - HeroTensorDesc 48 -> 64 bytes
 * (shadow, shadow_dtype; it is passed as an ARRAY, so the stride changed), HeroGemmEpilogue + 16 bytes (colsum_partial,
 * split_stride), HeroScoreMax + 8 bytes (gc_scale, gq_scale), HeroStEd.pad_ became g_scale - plus round 6: the three
 * scales are plain multipliers (the "0 means 1" sentinel is gone: pass 1.0f for "no weight"), hero_abi_struct_bytes().
 * Still 3: the retrieval entry points hero_topk_rows, hero_st_ed_probs and hero_moment_topk were ADDED later (plain pointer /
 * scalar arguments, no struct) - a backward-compatible addition, no struct moved, so the version stays.
 * Still 3: hero_moment_nms and hero_first_hit (what follows a search: NMS and recall ranks) were ADDED the same way.
 * Still 3: hero_first_hit_multi (recall ranks against several annotators' timestamps: DiDeMo) was ADDED the same way.
 * Still 3: hero_qa_pool_fwd and hero_qa_pool_bwd (the video-QA head) were ADDED the same way.
 * Still 3: hero_frame_pool_fwd/bwd and hero_bce_head_fwd/bwd (the VIOLIN head) were ADDED the same way.
 * Still 3: hero_dec_attention_fwd/bwd/in_envelope and hero_smooth_ce_fwd/bwd, the captioning decoder's kernels, were ADDED the
 * same way (a POINTER to the existing HeroDropout is an argument; the struct itself is unchanged).
 * Still 3: hero_gemm_route (host-only query of hero_gemm's kernel choice) was ADDED the same way (a pointer to the unchanged
 * HeroGemmEpilogue).
 * Still 3: hero_dec_attention_row, hero_dec_attention_step and hero_dec_attention_row_in_envelope (one query row per caption
 * against the encoder keys / a growing key-value cache: incremental captioning decode) were ADDED the same way.
 * Still 3: hero_beam_select and hero_beam_in_envelope (the selection step of beam-search captioning), and
 * hero_dec_attention_row_grouped and hero_dec_attention_step_beam (the one-row attentions of a beam: shared encoder keys, a
 * cache read through an ancestry table) were ADDED the same way.
 * Still 3: hero_sample_select and hero_sample_in_envelope (the sampling step of the captioning decode: temperature, top-k,
 * top-p, a Gumbel-max draw) were ADDED the same way.
 * Still 3: hero_caption_score and hero_caption_in_envelope (BLEU statistics, ROUGE-L and CIDEr-D of decoded id rows against
 * packed reference tables) were ADDED the same way.
 * Still 3: hero_ce_eval and hero_feat_eval (the validation counters of the pre-training heads) were ADDED the same way.
 * INTEGRATION.md section 2 lists the breaks per version. */
#define HERO_ABI_VERSION 3
int hero_abi_version(void);
/* sizeof() of every struct of this header as the LIBRARY was compiled, by HERO_STRUCT_* id (-1 for an unknown id): a
 * binding asserts its own layout against these at load time (hero_amd/_lib.py), so a struct that changes size without a
 * version bump is caught structurally and not by a crash.  hero_abi_struct_count() = number of ids. */
enum { HERO_STRUCT_DROPOUT = 0, HERO_STRUCT_GEMM_EPILOGUE, HERO_STRUCT_WGRAD_PROBLEM, HERO_STRUCT_LN_FWD, HERO_STRUCT_LN_BWD,
       HERO_STRUCT_COLSUM, HERO_STRUCT_ATTN, HERO_STRUCT_ADAMW, HERO_STRUCT_TENSOR_DESC, HERO_STRUCT_ADAMW_GROUP,
       HERO_STRUCT_ADAMW_MULTI, HERO_STRUCT_COPY_DESC, HERO_STRUCT_QUERY_POOL, HERO_STRUCT_ROW_NORM, HERO_STRUCT_SCORE_MAX,
       HERO_STRUCT_RANK_LOSS, HERO_STRUCT_ST_ED, HERO_STRUCT_CROSS_ENTROPY, HERO_STRUCT_DERIVE, HERO_STRUCT_COMM_BUCKET,
       HERO_STRUCT_COUNT_ };
int hero_abi_struct_count(void);
int hero_abi_struct_bytes(int which);

/* Counter-based dropout. keep(element) is a pure function of (*seed_ptr, site, element index), so
 * the backward kernels regenerate the forward mask instead of loading one. threshold16 = round(p *
 * 65536) (0 disables), scale = 1/(1-p). seed_ptr points to ONE device uint64 that the host
 * advances per step (it stays valid under hipGraph replay); site distinguishes call sites.
 * Replaces torch.nn.Dropout at model/layers.py:149,177,252,80-84 and model/embed.py:57,116,160. */
typedef struct HeroDropout {
  const uint64_t* seed_ptr;
  uint64_t site;
  uint32_t threshold16;
  float scale;
} HeroDropout;

/* ------------------------------------------------------------------------------------------ */
/* GEMM with fused epilogue — nn.Linear forward / dgrad / wgrad                                 */
/*   model/layers.py:125-127 (Q,K,V), :176 (attention out), :237 (FFN1), :251 (FFN2), :90       */
/*   (LinearLayer), model/embed.py:110 (img_linear) and their autograd transposes.              */
/* ------------------------------------------------------------------------------------------ */
enum { HERO_LAYOUT_K = 0, /* operand is [outer, reduction], reduction contiguous          */
       HERO_LAYOUT_O = 1  /* operand is [reduction, outer], outer (M or N) contiguous     */ };
enum { HERO_ACT_NONE = 0,
       HERO_ACT_GELU = 1,     /* fwd: aux <- acc+bias (pre-activation), out <- gelu_erf(.)     */
       HERO_ACT_RELU = 2,     /* fwd: out <- relu(acc+bias); aux <- that value (pre-residual) */
       HERO_ACT_GELU_BWD = 3, /* bwd: out <- acc * gelu_erf'(aux)                              */
       HERO_ACT_RELU_BWD = 4, /* bwd: out <- acc * (aux > 0)                                   */
       HERO_ACT_GELU_DG = 5,  /* fwd: out <- gelu_erf(acc+bias); aux <- gelu_erf'(acc+bias): the   */
                              /*      derivative is saved instead of the pre-activation (BertIntermediate, */
                              /*      model/layers.py:236-239: nothing else reads it), so that ...  */
       HERO_ACT_MUL_AUX = 6   /* bwd: out <- acc * aux   ... the backward epilogue is one multiply  */ };

typedef struct HeroGemmEpilogue {
  const float* bias;    /* [N] fp32 or NULL                                                  */
  const void* residual; /* [M, ldc] activation dtype or NULL; added last                     */
  void* aux;            /* [M, ldc] activation dtype; meaning depends on `act`               */
  int act;              /* HERO_ACT_*                                                        */
  int out_f32;          /* 1: C is fp32 regardless of dtype (wgrad)                          */
  float beta;           /* out_f32 only: C <- result + beta * C                              */
  int split_k;          /* >1: reduction split over blocks, fp32 atomics into C (needs       */
                        /*     out_f32, act NONE, no bias/residual/dropout; C pre-scaled)    */
  HeroDropout dropout;  /* applied after bias/act, before residual; index = m*N + n          */
  float* colsum;        /* optional [N] fp32, ACCUMULATED: colsum[n] += sum_m out[m, n] (the values  */
                        /* written to C, before rounding).  K,K operands, no split_k.  Gives the     */
                        /* bias gradient of the layer whose output gradient this GEMM produces        */
                        /* (dH = (dY W2) * gelu'(u) -> db1) without another pass over dH.             */
  int colsum_partial;   /* 0: `colsum` is [N], accumulated with fp32 atomics (order-dependent).  1: `colsum` is a   */
                        /* [ceil(M / 64), N] fp32 table that is OVERWRITTEN - every output tile writes its column     */
                        /* sums to row (first tile row / 64) and zeros to the rows of its other 64-row blocks; the     */
                        /* table's column sums (hero_colsum / hero_colsum_multi, fixed order) are the result:          */
                        /* bit-reproducible, no atomics.  Needs tile heights that are multiples of 64 (all kernels).    */
  int pad_;
  long long split_stride; /* split_k > 1 only.  0: the splits merge with fp32 atomics into C (order-dependent).      */
                        /* != 0 (elements, >= (M-1) ldc + N): split s WRITES its partial sum to the fp32 slab        */
                        /* C + s * split_stride (no pre-scale, beta ignored); the number of slabs written is the      */
                        /* return value of hero_gemm_splits(); hero_fold_slabs adds them in slab order (deterministic) */
} HeroGemmEpilogue;

/* C[M,N] = op(A)[M,K] * op(B)[K,N] (+ epilogue).
 *   a_layout K: A is [M, lda] ; O: A is [K, lda] (wgrad: dY^T)
 *   b_layout K: B is [N, ldb] (nn.Linear weight, x @ W^T) ; O: B is [K, ldb] (dgrad / wgrad)
 * Constraints: bf16: K-layout operands need K % 8 == 0, O-layout operands need their outer dim % 8
 * == 0; f32: % 4. N % 4 == 0. All base pointers 16-byte aligned, lda/ldb/ldc multiples of that
 * vector width. */
int hero_gemm(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
              int a_layout, int b_layout, int dtype, const HeroGemmEpilogue* epi, hero_stream_t stream);
/* The number of k-ranges hero_gemm actually cuts a reduction of length K into when asked for `split_k` (whole k-tiles
 * of 64 (bf16) / 32 (f32) per range, no empty range): the slab count of a split_stride launch. */
int hero_gemm_splits(int K, int split_k, int dtype);
/* out[i] = sum_{s < n_slabs} slabs[s * stride + i], s ascending (fixed order), i < n (n % 4 == 0); out_dtype F32 / BF16. */
int hero_fold_slabs(const float* slabs, int n_slabs, size_t stride, void* out, size_t n, int out_dtype, hero_stream_t stream);

/* The route hero_gemm takes for a problem RIGHT NOW (the hero_gemm_force_config state, the current device's compute units;
 * 256 where there is no device) - host only, no device work, pointers of `epi` are read as null / non-null only.  Same
 * shape checks and error codes as hero_gemm (no pointer-alignment checks).  Writes HERO_GEMM_ROUTE_WORDS int32 words and
 * returns that number:
 *   0 family     0 nothing to launch, 1 skinny fp32, 2 wave-specialised K,K, 3 wave-specialised O,O,
 *                4 4-wave direct-to-LDS K,K, 5 4-wave direct-to-LDS O,O, 6 4-wave register-staged
 *   1, 2 tile rows, tile columns        3 compile-time epilogue kind (0x100 generic; 1 bias, 2 GELU, 4 residual, 8 dropout, 16 gelu')
 *   4 workgroups   5 threads per workgroup   6 dynamic LDS bytes   7 reduction splits   8 reduction length per split
 *   9 M-tiles per L2 locality group   10 1: C is pre-scaled by beta in a launch of its own first   11 hero_prof_read slot
 * Plain arguments and an existing struct: a backward-compatible addition, HERO_ABI_VERSION stays. */
#define HERO_GEMM_ROUTE_WORDS 12
int hero_gemm_route(int M, int N, int K, int lda, int ldb, int ldc, int a_layout, int b_layout, int dtype,
                    const HeroGemmEpilogue* epi, int32_t* out, int capacity_words);

/* Per-launch timing of hero_gemm with HIP events recorded on the launch stream (bench.py's
 * roofline leg; off by default, never enable inside graph capture).  Slots (word 11 of hero_gemm_route):
 *   0-7  (dtype == HERO_BF16 ? 4 : 0) + a_layout * 2 + b_layout: the 4-wave kernels (3 also holds the skinny fp32 kernel)
 *   8    wave-specialised 192x192 K,K        9  wave-specialised O,O (hero_gemm, hero_wgrad_group, hero_wgrad_batch)
 *   10   wave-specialised 128x192 / 64x128 / 64x192 K,K (gemm_ws.hip)
 * hero_prof_read synchronises. */
/* Grouped weight gradient: dw_p[M_p, N_p] (fp32) += dy_p[K, :M_p]^T x_p[K, :N_p] for 1..4 problems that reduce over
 * the same K rows - the four nn.Linear weights of a BertLayer (model/layers.py:125-127, 176, 237, 251) - in ONE
 * launch (stream-K over the (tile, k) space of the whole group, fp32 atomics into dw).  Small / unaligned / fp32
 * groups run as one hero_gemm per problem (split_hint = its split_k). */
typedef struct HeroWgradProblem {
  const void* dy;   /* [K, ld_dy] dtype, the M columns starting at this pointer */
  const void* x;    /* [K, ld_x] dtype                                          */
  float* dw;        /* [M, ld_dw] fp32, accumulated                            */
  int M, N, ld_dy, ld_x, ld_dw;
  int split_hint;
  float* dbias;     /* optional [M] fp32 (hero_wgrad_batch only; must be NULL for hero_wgrad_group): += column sums of */
                    /* dy = the bias gradient of the same nn.Linear, taken from the dY panels the kernel streams anyway */
} HeroWgradProblem;
int hero_wgrad_group(const HeroWgradProblem* probs, int n, int K, int dtype, hero_stream_t stream);
/* Batched weight gradients, whole tiles: up to HERO_WGRAD_BATCH_MAX problems over the same K rows - the weight
 * gradients of ALL BertLayers of an encoder, queued during the backward pass (model/layers.py:112-114, 173, 231, 245 x
 * num_hidden_layers) - in ONE launch.  Whole 192 x 192 output tiles per workgroup in full rounds of the chip (plain
 * fp32 read-add-write, no atomics), the remaining tiles cut into k-slices whose atomics are applied in slice order:
 * dw is bit-reproducible for a fixed problem list.  Two steps:
 *   hero_wgrad_batch_plan  (host, no device work): writes the schedule for (shapes of probs, K) into `plan`
 *                          (int32 words, host memory); returns the number of words, 0 if the group is too small
 *                          for this kernel (fewer tiles than workgroups: use hero_wgrad_group), < 0 on error /
 *                          insufficient capacity.  Depends only on M, N of the problems and K: cache it.
 *   hero_wgrad_batch       launches with the plan copied to device memory by the caller (plan_dev, plan_words).
 * bf16 only; M, N multiples of 8; pointers 16-byte aligned; one launch at a time per device (the slice-order flags
 * are library state). */
#define HERO_WGRAD_BATCH_MAX 32
int hero_wgrad_batch_plan(const HeroWgradProblem* probs, int n, int K, int32_t* plan, int capacity_words);
int hero_wgrad_batch(const HeroWgradProblem* probs, int n, int K, int dtype, const int32_t* plan_dev, int plan_words,
                     hero_stream_t stream);
/* Tuning hook: which kernels hero_gemm may choose.
 *   -1        heuristic (only then fp32 GEMMs with M <= 32 run the skinny VALU kernel)
 *   0..7      4-wave kernels only; bits 0-1 tile geometry: 0 128x128, 1 192x128, 2 256x256, 3 64x64 (1 and 3: direct-to-LDS
 *             path only); bit 2: register staging
 *   8         4-wave kernels only, geometry by shape
 *   9 / 10    wave-specialised kernels always, 192x192 / 128x192 tiles (where the shape is legal)
 *   13 / 14   wave-specialised 64x128 (six-deep ring) / 64x192 (four-deep) tiles - what small-M GEMMs (the Temporal
 *             Transformer's 1920 rows into N = 768, the 480 query rows) take by default
 *   11, 12, 15 and up: read as bits like 0..7 (11 / 12 were round 4's deferred-epilogue lab variant: now plain 4-wave);
 *             bits 8+: M-tiles per L2 locality group */
int hero_gemm_force_config(int cfg);
int hero_prof_enable(int on);
int hero_prof_read(int slot, double* total_ms, double* total_flops, long long* launches);

/* Box probes (bench.py: `roofline.peak_measured`, `.hbm_peak_measured`, `.clock_ghz`): what this box's matrix pipes and HBM
 * deliver right now.  These two entries TIME themselves with HIP events and synchronise `stream` (like hero_prof_read);
 * never call them under stream capture.
 * hero_probe_mfma: ~0.2 s of back-to-back v_mfma_f32_32x32x16_bf16 on every CU (8 waves per CU, 9 accumulators per wave,
 *   no memory traffic; the first ~70 ms after idle run at ramping clocks and are not timed): dense bf16 TFLOP/s and the
 *   sustained matrix clock (from the MFMA occupancy: 32 pipe cycles per 32x32x16 bf16 MFMA).  scratch: device memory, >= CUs * 2048 + 16 bytes.
 * hero_probe_hbm: a streaming copy src -> dst and a streaming read of src over `bytes` (>= 256 MiB each, beyond the
 *   Infinity Cache): copy_gbps = (bytes read + bytes written) / time, read_gbps = bytes / time.  dst[0..3] may be written
 *   by the read pass. */
int hero_probe_mfma(void* scratch, size_t scratch_bytes, double* tflops, double* ghz, hero_stream_t stream);
int hero_probe_hbm(const void* src, void* dst, size_t bytes, double* copy_gbps, double* read_gbps, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* LayerNorm (apex FusedLayerNorm call sites: model/layers.py:52,79,171,246,338,               */
/* model/embed.py:25,93,99,143,171) fused with the embedding sums in front of it               */
/* (model/embed.py:28-58 SubEmbeddings, :102-117 ImageEmbeddings, :146-161 FrameEmbeddings)     */
/* and the dropout behind it.                                                                   */
/* ------------------------------------------------------------------------------------------ */
typedef struct HeroLnFwd {
  const void* x;        /* [rows, cols] x_dtype, or NULL                                       */
  const float* tab[3];  /* fp32 tables [*, cols] gathered and added to x (NULL = unused)        */
  const int32_t* idx[3];/* per-row table row; NULL = row 0 for every row                       */
  const float* gamma;   /* [cols] */
  const float* beta;    /* [cols] */
  void* y;              /* [rows, cols] y_dtype                                                */
  void* pre;            /* optional [rows, cols] y_dtype: the summed LN input (for backward)   */
  float* mean;          /* optional [rows] */
  float* rstd;          /* optional [rows] */
  int rows, cols;
  float eps;
  int x_dtype, y_dtype;
  HeroDropout dropout;  /* on y; index = row*cols + col                                         */
} HeroLnFwd;
int hero_layernorm_fwd(const HeroLnFwd* a, hero_stream_t stream);

typedef struct HeroLnBwd {
  const void* x;        /* [rows, cols] x_dtype: the LN input (or `pre` saved by forward)       */
  const void* dy;       /* [rows, cols] dtype                                                   */
  const float* gamma;
  const float* mean;
  const float* rstd;
  void* dx;             /* optional [rows, cols] dtype                                          */
  void* dx_dropped;     /* optional [rows, cols] dtype: dx * mask(dropout_in) — the gradient    */
                        /* of the pre-dropout branch feeding this LN's residual sum             */
  float* dgamma;        /* optional [cols]: dgamma <- grad_beta*dgamma + sum                    */
  float* dbeta;         /* optional [cols]                                                      */
  float grad_beta;      /* 0 overwrite, 1 accumulate                                            */
  void* workspace;      /* hero_layernorm_bwd_workspace_bytes(rows, cols) bytes                 */
  int rows, cols;
  int x_dtype, dtype;
  HeroDropout dropout_out; /* the forward's output dropout (applied to dy first)                */
  HeroDropout dropout_in;  /* dropout of the GEMM epilogue that produced x (for dx_dropped)     */
  float* dbias_in;         /* optional [cols] (cols <= 1024): += sum_rows dx*mask(dropout_in) =     */
                           /* bias gradient of the linear layer feeding this LN, same pass         */
  int defer_fold;          /* 1 (fused path only: cols <= 1024 and dx wanted): leave the per-block   */
                           /* partial sums in `workspace` as fp32 [hero_layernorm_bwd_blocks(rows)]  */
                           /* [3][cols] (dgamma | dbeta | dbias_in) and do not touch the outputs -   */
                           /* the caller folds them later, e.g. many at once with hero_colsum_multi  */
} HeroLnBwd;
size_t hero_layernorm_bwd_workspace_bytes(int rows, int cols);
int hero_layernorm_bwd_blocks(int rows);   /* rows of the partial-sum matrix the fused backward writes */
int hero_layernorm_bwd(const HeroLnBwd* a, hero_stream_t stream);

/* Column sum: out[c] <- beta*out[c] + sum_r x[r, c]  (bias gradients of every nn.Linear).      */
size_t hero_colsum_workspace_bytes(int rows, int cols);
int hero_colsum(const void* x, float* out, int rows, int cols, int ld, int dtype, float beta,
                void* workspace, hero_stream_t stream);
/* Many column sums in TWO launches (row-chunk partials, then a fixed-order fold: deterministic, no atomics): the   */
/* bias gradients of all nn.Linear layers of a backward pass (model/layers.py:125-127, 175-179, 236-239, 250-254)   */
/* and the deferred LayerNorm partial folds, queued and flushed together.  dst[c] <- beta*dst[c] + sum_r src[r,c]. */
#define HERO_COLSUM_MULTI_MAX 64
typedef struct HeroColsum {
  const void* src;   /* [rows, ld] dtype, the `cols` columns starting at this pointer (16-byte aligned) */
  float* dst;        /* [cols]                                                                         */
  int rows, cols, ld, dtype;   /* cols, ld multiples of 4                                              */
  float beta;
  int row_cols;      /* with dst_rows: width of a destination row (cols = n_rows * row_cols)           */
  const int32_t* dst_rows;     /* optional (hero_colsum_multi only; beta must be 1): the sum of columns  */
                     /* [j * row_cols, (j + 1) * row_cols) is ADDED to dst + dst_rows[j] * row_cols - the fold   */
                     /* of a periodic position-id gradient ([S, L * D] view of [S * L, D]) goes straight into  */
                     /* the embedding table's rows (model/embed.py:28-58, 146-161); rows < 0 are dropped      */
} HeroColsum;
size_t hero_colsum_multi_workspace_bytes(const HeroColsum* p, int n);
int hero_colsum_multi(const HeroColsum* p, int n, void* workspace, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Masked multi-head self-attention, head size 64 — model/layers.py:129-160                     */
/*   scores = Q K^T * scale + mask[s, key]; P = softmax(scores); ctx = dropout(P) V             */
/* qkv is the fused projection output [S*L, 3*H*64] (Q | K | V, head h at columns h*64).        */
/* ------------------------------------------------------------------------------------------ */
typedef struct HeroAttn {
  const void* qkv;    /* [S*L, 3*H*64] dtype                                                   */
  const float* mask;  /* [S, L] additive fp32 ((1-m)*-10000, model/layers.py:299-302) or NULL   */
  void* ctx;          /* fwd out [S*L, H*64] dtype; bwd in (optional): with it the bf16 backward of    */
                      /* 64 < L <= 256 runs on the matrix cores (delta_i = dO_i . ctx_i)               */
  float* probs;       /* [S, H, L, L] fp32 softmax output (pre-dropout); fwd out (may be NULL   */
                      /* for inference), bwd in                                                 */
  const void* dctx;   /* bwd in  [S*L, H*64] dtype                                              */
  void* dqkv;         /* bwd out [S*L, 3*H*64] dtype                                            */
  int S, L, H;
  float scale;        /* 1/sqrt(64)                                                             */
  int dtype;
  HeroDropout dropout; /* on P; index = ((s*H+h)*L + q)*round_up(L,4) + k                       */
  const int32_t* seq_off; /* optional [S+1] row offsets of a PACKED batch (L <= 64; bf16: 256): sequence s is */
                       /* rows [seq_off[s], seq_off[s+1]) of qkv/ctx/dctx/dqkv, at most L long;   */
                       /* probs keeps its [S, H, L, L] layout, dropout indices use L; mask NULL   */
  float* stats;        /* optional [S, H, L, 2] fp32 (row maximum, 1 / row sum) of the softmax: fwd out, bwd in.  Where */
                       /* hero_attention_stats_ok() says so, the backward takes stats INSTEAD of probs (probs NULL; it  */
                       /* needs `mask` again) and recomputes the probabilities bit-identically from q, k: 24x less      */
                       /* saved state at L = 24 (model/layers.py:129-160 keeps attention_probs for autograd)            */
} HeroAttn;
int hero_attention_fwd(const HeroAttn* a, hero_stream_t stream);
int hero_attention_bwd(const HeroAttn* a, hero_stream_t stream);
int hero_attention_max_len(int dtype, int backward);
/* longest sequence of a PACKED (seq_off) batch the kernels take for this dtype: 256 on the bf16 matrix-core */
/* kernels, 64 otherwise (fp32, or HERO_ATTN_MFMA=0) - callers fall back to the padded layout beyond it      */
int hero_attention_max_packed_len(int dtype);
int hero_attention_force_ppw(int ppw); /* tuning hook: (sequence, head) pairs per wave of the L <= 32 bf16 kernels, 1..3; 0 = heuristic */
/* 1 when forward + backward of this dtype / length run from `stats` without saved probabilities (bf16 matrix-core */
/* kernels, L <= 64)                                                                                               */
int hero_attention_stats_ok(int dtype, int L);

/* ------------------------------------------------------------------------------------------ */
/* Decoder attention, head size 64 - model/tvc.py:67-104 and the decoder's causal self-attention */
/*   scores = Q K^T * scale + key_mask_add[n, key] + (causal and key > query ? -10000 : 0)      */
/*   P = softmax(scores) in fp32; ctx = dropout(P) V                                            */
/* Query and key/value sequences are separate operands: q rows [N*Lq] with leading dimension   */
/* ldq, k and v rows [N*Lk] with leading dimension ldkv, head h at columns h*64 of each.  The    */
/* self-attention call passes the three column blocks of a fused [N*L, 3*H*64] projection        */
/* (ldq = ldkv = 3*H*64), the decoder-encoder call a [N*Lq, H*64] query and the halves of a      */
/* [N*Lk, 2*H*64] key/value projection.  dq / dk / dv follow q / k / v; ctx and dctx are         */
/* [N*Lq, H*64].  key_mask_add is [N, Lk] fp32 or NULL.  The masks are ADDITIVE, as in the        */
/* reference: a caption whose keys are all masked attends uniformly to its Lk keys.             */
/* Dropout on P (NULL: none): element index ((n*H + h)*Lq + i) * round_up(Lk, 4) + j; the         */
/* backward regenerates the mask.  fwd writes stats [N, H, Lq, 2] fp32 = (row maximum, 1 / row    */
/* sum); bwd recomputes P from q, k, the mask and stats and writes EVERY element of dq, dk, dv    */
/* of the H head blocks (no zero-fill by the caller, no atomics: two runs give the same bits).   */
/* Envelope: fp32 / bf16, 1 <= Lq <= 64, 1 <= Lk <= 128, H >= 1, N >= 0 (0: no launch); ldq, ldkv */
/* multiples of 8 and >= H*64; pointers 16-byte aligned.  Outside it HERO_ERR_ARG, no launch.    */
/* Plain arguments: a backward-compatible addition, HERO_ABI_VERSION stays.                     */
/* ------------------------------------------------------------------------------------------ */
int hero_dec_attention_in_envelope(int dtype, int Lq, int Lk);
int hero_dec_attention_fwd(const void* q, const void* k, const void* v, const float* key_mask_add, void* ctx, float* stats,
                           int N, int Lq, int Lk, int H, int ldq, int ldkv, int causal, float scale, int dtype,
                           const HeroDropout* dropout, hero_stream_t stream);
int hero_dec_attention_bwd(const void* q, const void* k, const void* v, const float* key_mask_add, const float* stats,
                           const void* dctx, void* dq, void* dk, void* dv, int N, int Lq, int Lk, int H, int ldq, int ldkv,
                           int causal, float scale, int dtype, const HeroDropout* dropout, hero_stream_t stream);

/* Incremental decoding (inference only: no dropout, no stats, no backward): ONE query row per  */
/* caption, the same arithmetic - scores = <q, k_j> * scale + key_mask_add[n, j], softmax in fp32, */
/* ctx = sum_j p_j v_j in a fixed order, no atomics - and ctx [N, H*64] written in full.          */
/*   hero_dec_attention_row    decoder-encoder attention of one decoder position: q [N, ldq], k / v */
/*       rows n*Lk + j with leading dimension ldkv (the packed K|V projection of the encoder rows, */
/*       computed once per decode), key_mask_add [N, Lk] fp32 or NULL.                            */
/*   hero_dec_attention_step   causal self-attention of position t against a cache: qkv [N, 3*H*64] */
/*       is this step's packed Q|K|V projection; kv_cache [N, Tcap, 2*H*64] holds K|V of the        */
/*       positions 0 .. t-1 on entry, and the kernel ALSO copies this step's K|V bits into its row t */
/*       (it reads position t from qkv, never from the row it writes).  Rows behind t are neither  */
/*       read nor written; no causal term is needed, the later keys are not there.                */
/*       t = pos_dev ? *pos_dev : pos - a device int32, so that one captured launch serves every   */
/*       step.  A device t outside [0, Tcap) cannot be refused on the host: the kernel then leaves */
/*       the cache alone and writes zeros to ctx.                                                 */
/* Envelope: fp32 / bf16, 1 <= Lk <= 128, 1 <= Tcap <= 128, H >= 1, N >= 1, a host pos in         */
/* [0, Tcap); ldq, ldkv multiples of 8 and >= H*64; pointers 16-byte aligned.  Outside it           */
/* HERO_ERR_ARG, no launch.  Plain arguments: a backward-compatible addition, HERO_ABI_VERSION stays. */
int hero_dec_attention_row_in_envelope(int dtype, int Lk);
int hero_dec_attention_row(const void* q, const void* k, const void* v, const float* key_mask_add, void* ctx,
                           int N, int Lk, int H, int ldq, int ldkv, float scale, int dtype, hero_stream_t stream);
int hero_dec_attention_step(const void* qkv, void* kv_cache, void* ctx, const int* pos_dev, int pos,
                            int N, int Tcap, int H, float scale, int dtype, hero_stream_t stream);

/* The same two kernels for the rows of a beam search, R = N captions x B beams, without a copy of */
/* any key or value:                                                                              */
/*   hero_dec_attention_row_grouped   as hero_dec_attention_row over N rows, but row r reads the    */
/*       keys, values and key mask of block r / group: k / v hold N / group blocks of Lk rows and    */
/*       key_mask_add is [N / group, Lk].  group = 1 is hero_dec_attention_row, bit for bit.         */
/*   hero_dec_attention_step_beam     as hero_dec_attention_step over N rows, with anc [N, Tcap]     */
/*       int32: key and value j < t of row r are read from cache row anc[r*Tcap + j] at position j,  */
/*       key t is this step's own row, and the row's K|V bits go to cache position t of row r as     */
/*       before.  An entry outside [0, N) is clamped into it; entries at j >= t are not read.  With  */
/*       anc[r, j] == r everywhere the result is hero_dec_attention_step's, bit for bit.             */
/* Envelope as above, group >= 1, anc not NULL.  Plain arguments: HERO_ABI_VERSION stays.           */
int hero_dec_attention_row_grouped(const void* q, const void* k, const void* v, const float* key_mask_add, void* ctx,
                                   int N, int group, int Lk, int H, int ldq, int ldkv, float scale, int dtype,
                                   hero_stream_t stream);
int hero_dec_attention_step_beam(const void* qkv, void* kv_cache, const int32_t* anc, void* ctx, const int* pos_dev, int pos,
                                 int N, int Tcap, int H, float scale, int dtype, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Beam-search selection (captioning decode; inference only)                                   */
/* ------------------------------------------------------------------------------------------ */
/* One call per decode step takes the beam tables of N captions x B beams (row r = n*B + b) to  */
/* the next step.  logits [R, ld] are the step's prediction scores (fp32 / bf16; arithmetic in   */
/* fp32).  A live beam b offers the candidates (b, v) with score cum[b] + logit[b, v] - lse_b,     */
/* lse_b = max + log(sum exp(x - max)) over its V scores; a finished beam (fin[b] != 0) offers     */
/* only (b, eos) with score cum[b].  The B best candidates of a caption - score descending, among  */
/* equal scores the lower flat index b*V + v - become its new beams in that order; with parent p   */
/* and token v of new beam i, and t the position of this step:                                    */
/*   cum[i] = score   fin[i] = fin[p] | (v == eos)   len[i] = len[p] + (fin[p] ? 0 : 1)             */
/*   ids[i, :t] = ids[p, :t], ids[i, t] = v   anc[i, :t] = anc[p, :t], anc[i, t] = n*B + p          */
/*   last[i] = v                                                                                  */
/* cum [R] fp32; fin, len, last [R] and ids, anc [R, Tcap] int32, all updated IN PLACE: every read  */
/* of a caption's old tables precedes every write.  Columns behind t are left alone.  anc is what   */
/* hero_dec_attention_step_beam reads at the next step.  The caller starts a caption with          */
/* cum = {0, -1e30, ...}, fin = len = 0, so that step 0 needs no special case.                      */
/* t = pos_dev ? *pos_dev + pos : pos - with a device counter `pos` is an OFFSET to it (-1 when the */
/* counter has already advanced past the step); a device t outside [0, Tcap) changes nothing.      */
/* workspace: N*B*B*8 bytes, 8-byte aligned, owned by the caller; nothing is allocated, nothing is  */
/* read on the host, no atomics: two runs give the same bits.                                      */
/* Envelope: fp32 / bf16, 1 <= B <= 8, B <= V <= 65536, 1 <= Tcap <= 128, ld >= V, 0 <= eos < V,    */
/* N >= 1, a host position in [0, Tcap).  Outside it HERO_ERR_ARG, no launch.                       */
/* Plain arguments: a backward-compatible addition, HERO_ABI_VERSION stays.                        */
int hero_beam_in_envelope(int dtype, int V, int B, int Tcap);
int hero_beam_select(const void* logits, float* cum, int32_t* fin, int32_t* len, int32_t* ids, int32_t* anc, int32_t* last,
                     void* workspace, const int* pos_dev, int pos, int N, int B, int V, int ld, int Tcap, int eos, int dtype,
                     hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Sampled decoding (captioning decode; inference only)                                         */
/* ------------------------------------------------------------------------------------------ */
/* One call per decode step draws the next token of R = N captions x S samples (row r = n*S + s) */
/* and updates the rows' tables - the buffers of the beam search, without anc: a row never changes */
/* its parent.  logits [R, ld] fp32 / bf16; all arithmetic in fp32.  With t the step's position:   */
/*   finished row (fin[r] != 0)  token = eos; cum, len unchanged; ids[r, t] = last[r] = eos;        */
/*       kept[r] = 0.                                                                              */
/*   live row                                                                                      */
/*     order   z_v = float(logit_v) * inv_temperature, one rounding.  Candidates are ordered by    */
/*             (order_bits(z_v) << 32) | ~v: larger z first, among equal z the lower token.          */
/*     top-k   keep the first min(top_k, V) candidates in that order; 0 = off.                      */
/*     top-p   masses exp(z_v - max z) over the survivors of top-k; keep the shortest prefix, in     */
/*             the same order, whose mass is >= top_p times the mass of all survivors, at least one   */
/*             candidate; top_p >= 1 = off.                                                          */
/*     draw    Gumbel-max: the kept v that maximises z_v + g_v, ties by the same composite on the     */
/*             perturbed score, where                                                                */
/*               base = splitmix64(seed ^ (site * 0xD6E8FEB86659FD93)), site = (uint64)t * R + r      */
/*               h = mix32((uint32)v ^ (uint32)base) >> 9,  u = (2h + 1) * 2^-24,                      */
/*               g = -logf(-log1pf(-u))                                                              */
/*     update  cum[r] += logit_v - lse_r, lse_r the log-sum-exp of the RAW row (temperature 1, no     */
/*             filter: the model's likelihood of the token); len[r] += 1; fin[r] = (v == eos);        */
/*             ids[r, t] = last[r] = v; kept[r] = the size of the kept set.                           */
/* cum [R] fp32; fin, len, last [R] and ids [R, Tcap] int32, updated IN PLACE; kept [R] int32 may be  */
/* NULL; columns other than t of ids are left alone.  seed_dev is ONE device uint64, read by the      */
/* kernel (a captured launch serves every seed).  t = pos_dev ? *pos_dev + pos : pos, as in           */
/* hero_beam_select; a device t outside [0, Tcap) changes nothing.                                   */
/* The masses of top-p are added as 64-bit integers in units of 2^-40 (LDS integer atomics): a sum    */
/* does not depend on the order of its terms, there are no floating-point atomics, two runs give the  */
/* same bits.  One launch; nothing is allocated or read on the host.                                 */
/* Envelope: fp32 / bf16, N, S >= 1, 1 <= V <= 65536, top_k >= 0, top_p > 0, inv_temperature finite   */
/* and > 0, 1 <= Tcap <= 128, ld >= V, 0 <= eos < V, a host position in [0, Tcap).  Outside it        */
/* HERO_ERR_ARG, no launch.  Plain arguments: a backward-compatible addition, HERO_ABI_VERSION stays. */
int hero_sample_in_envelope(int dtype, int V, int Tcap);
int hero_sample_select(const void* logits, float* cum, int32_t* fin, int32_t* len, int32_t* ids, int32_t* last, int32_t* kept,
                       const unsigned long long* seed_dev, const int* pos_dev, int pos, int N, int S, int V, int ld, int Tcap,
                       int eos, float inv_temperature, int top_k, float top_p, int dtype, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Caption metrics (BLEU statistics, ROUGE-L, CIDEr-D of decoded id rows; inference / rewards)  */
/* ------------------------------------------------------------------------------------------ */
/* One launch scores M caption rows against the references of their clips, as the reference's     */
/* eval/pycocoevalcap does on words (BleuScorer n = 4 "closest", Rouge, CiderScorer n = 4,         */
/* sigma = 6), restated on integer tokens.  ids [M, ld] int32 (ids_int64 = 0) or int64 rows as the  */
/* decoders leave them; the caption h of a row is what stands before its first `eos` within Tcap -  */
/* what follows is junk and reaches no count.  clip [M] int32 is the row's clip in the reference    */
/* tables `refs`, ONE packed device buffer built once by hero_amd.caption.CaptionRefs (layout: the  */
/* head of hero_amd/csrc/caption_metrics.hip); a clip outside the tables gives zeros.  With the     */
/* references r_1..r_R of the clip:                                                               */
/*   stats [M, ld_stats] int32, columns 0..9:  correct[n] = sum over the distinct n-grams g of h of  */
/*       min(count_h(g), max_r count_r(g));  guess[n] = max(0, |h| - n + 1), n = 1..4;  testlen =    */
/*       |h|;  reflen = the |r| with the smallest (||r| - |h||, |r|).  Columns >= 10 are left alone. */
/*   rouge [M] fp32:  p = max_r LCS(h, r) / max(|h|, 1), q = max_r LCS(h, r) / |r|,                   */
/*       2.44 p q / (q + 1.44 p), or 0 when p or q is 0.  lcs [M] int32 (may be NULL): max_r LCS.    */
/*   cider [M] fp32:  weights w(g) = count(g) * idf_n(g), idf_n(g) = log C - log max(1, df_n(g));     */
/*       per reference and order  sum_g min(w_h(g), w_r(g)) w_r(g), divided by |w_h| |w_r| when both  */
/*       are non-zero, times exp(-delta^2 / 72), delta = max(|h| - 1, 0) - max(|r| - 1, 0); the mean   */
/*       over the four orders, summed over the references, / R, * 10.  Sums and norms in float64.     */
/* n-grams are exact 64-bit keys of four 16-bit tokens: ids in [0, 65536) is a PRECONDITION (the      */
/* decoders guarantee it).  No atomics, nothing allocated, nothing read on the host: two runs give    */
/* the same bits and the launch can be captured.                                                    */
/* Envelope: 1 <= V <= 65536, 1 <= Tcap <= 128, ld >= Tcap, ld_stats >= 10, 0 <= eos < V, M >= 1;     */
/* refs 8-byte aligned.  Outside it HERO_ERR_ARG, no launch.                                         */
/* Plain arguments: a backward-compatible addition, HERO_ABI_VERSION stays.                          */
int hero_caption_in_envelope(int V, int Tcap);
int hero_caption_score(const void* ids, int ids_int64, const int32_t* clip, const void* refs, int32_t* stats, float* rouge,
                       float* cider, int32_t* lcs, int M, int ld, int ld_stats, int Tcap, int eos, int V, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Row gathers / scatters                                                                      */
/* ------------------------------------------------------------------------------------------ */
/* out[r] = idx[r] >= 0 ? a[idx[r]] : (idx[r] == -1 ? 0 : b[-idx[r]-2]).                         */
/* Replaces torch.gather(cat([img_emb, txt_emb]), gather_index) (model/encoder.py:271-279) and  */
/* serves as the backward of hero_csr_gather_sum.                                               */
int hero_gather_rows(const void* a, const void* b, const int32_t* idx, void* out, int rows, int cols,
                     int dtype, hero_stream_t stream);
/* out[r] = sum_{e in [offsets[r], offsets[r+1])} src[entries[e]].                               */
/* Replaces HierarchicalVlModel.collect_frame_outputs (model/model.py:156-187).                 */
/* inv[r] (r < na: rows of a) / inv[na + r] (rows of b) = the FIRST output row of a hero_gather_rows index that reads that
 * source row, -1 if none (na + nb <= 38400: one workgroup, LDS-resident, deterministic).  With it the backward of a gather
 * whose repeated references are known to carry no gradient (HERO's f_gather_index: a source row is re-referenced only from
 * padded positions behind its valid one, data/data.py:504-512, whose gradients are exactly zero) is ONE gather - no zero
 * fills, no scatter. */
int hero_inverse_first(const int32_t* idx, int n, int32_t* inv, int na, int nb, hero_stream_t stream);
int hero_csr_gather_sum(const void* src, const int32_t* offsets, const int32_t* entries, void* out,
                        int rows, int cols, int dtype, hero_stream_t stream);
/* dst[idx[r]] += src[r] (rows with idx[r] < 0 or == skip_idx are dropped).                      */
/* dst_dtype HERO_F32: embedding-table gradients (nn.Embedding backward, padding_idx = skip).   */
/* Two destinations as in hero_gather_rows when b != NULL.                                      */
int hero_scatter_add_rows(const void* src, const int32_t* idx, void* dst_a, void* dst_b, int rows,
                          int cols, int src_dtype, int dst_dtype, int skip_idx, hero_stream_t stream);
/* The same sum WITHOUT atomics, bit-reproducible (nn.Embedding backward into the fp32 gradient of word_embeddings,    */
/* model/embed.py:15-18, 28-58: destinations that receive three or more rows make the atomic version order-dependent): */
/*   hero_segment_sort        order[rows] = the row numbers sorted by (idx[row], row), rows with idx < 0 or == skip_idx */
/*                            last; one workgroup, stable radix sort; n_dst = rows of the table (bounds the key width); */
/*                            workspace of hero_segment_sort_workspace_bytes(rows) bytes.  Depends on idx only: cache it. */
/*   hero_scatter_add_sorted  blocks of 16 sorted rows, one wave each: a run of equal destinations inside a block is   */
/*                            added to dst[idx] by that wave (row order, fp32; the row has no other writer); a run that */
/*                            crosses blocks (a token at the head of every subtitle) leaves one partial sum per block   */
/*                            and the wave of its first block folds them in block order.  dst is fp32; cols % 4 == 0;   */
/*                            workspace of hero_scatter_add_sorted_workspace_bytes(rows, cols) bytes.                    */
size_t hero_segment_sort_workspace_bytes(int rows);
size_t hero_scatter_add_sorted_workspace_bytes(int rows, int cols);
int hero_segment_sort(const int32_t* idx, int rows, int n_dst, int skip_idx, int32_t* order, void* workspace,
                      hero_stream_t stream);
int hero_scatter_add_sorted(const void* src, const int32_t* idx, const int32_t* order, float* dst, int rows, int cols,
                            int src_dtype, int skip_idx, void* workspace, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Elementwise                                                                                  */
/* ------------------------------------------------------------------------------------------ */
/* dst <- (dst_dtype) src, n elements (fp32 master weights -> compute copies, outputs -> fp32). */
int hero_cast(const void* src, void* dst, size_t n, int src_dtype, int dst_dtype, hero_stream_t stream);
/* dst[c * ldd + r] <- (dst_dtype) src[r * cols + c]: transposed compute copies of the fp32 master
 * weights, so that dgrad (dY W) also runs with both operands reduction-contiguous. */
int hero_transpose_cast(const float* src, void* dst, int rows, int cols, int ldd, int dst_dtype, hero_stream_t stream);
/* dx <- dy * (y > 0) — F.relu backward (model/layers.py:92).                                   */
int hero_relu_bwd(const void* dy, const void* y, void* dx, size_t n, int dtype, hero_stream_t stream);
/* dx <- dy * gelu_erf'(u) — backward of model/layers.py:16-25 outside the fused FFN block.     */
int hero_gelu_bwd(const void* dy, const void* u, void* dx, size_t n, int dtype, hero_stream_t stream);
/* y <- a + b (gradient fan-in where two consumers read one activation).                        */
int hero_add(const void* a, const void* b, void* y, size_t n, int dtype, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Optimiser — optim/adamw.py:43-106 + clip_grad_norm_ (train_vcmr.py:257-260) over flat fp32   */
/* parameter / gradient arenas.                                                                 */
/* ------------------------------------------------------------------------------------------ */
/* sumsq[0] += sum g^2 (fp32 device scalar; caller zeroes it).  Deterministic (fixed summation  */
/* order): data-parallel replicas must derive the SAME clipping factor from the same gradients.  */
/* workspace: >= 2048 floats of device scratch.  `g` must be 16-byte aligned (it is read as      */
/* float4 with no scalar fallback); anything else is rejected with HERO_ERR_ARG before a launch. */
int hero_sumsq(const float* g, size_t n, float* sumsq, float* workspace, hero_stream_t stream);
typedef struct HeroAdamW {
  float* p;
  const float* g;
  float* m;
  float* v;
  size_t n;
  float lr, beta1, beta2, eps, weight_decay;
  int step;                /* 1-based, for bias correction                                     */
  const float* grad_sumsq; /* optional device scalar: global sum g^2 for clipping               */
  float max_grad_norm;     /* used when grad_sumsq != NULL: g *= min(1, max/(norm+1e-6))        */
  float grad_scale;        /* extra multiplier on g (e.g. 1/world_size); 1 = none               */
  void* shadow;            /* optional bf16 copy of p refreshed in the same pass               */
} HeroAdamW;
/* p, g, m, v must be 16-byte aligned and shadow 8-byte aligned (float4 / packed-bf16 accesses    */
/* with no scalar fallback); anything else is rejected with HERO_ERR_ARG before a launch.  The    */
/* multi-tensor form below tests its pointers itself and falls back to scalar accesses.          */
int hero_adamw(const HeroAdamW* a, hero_stream_t stream);

/* Multi-tensor form: ONE launch updates every tensor in a device-resident descriptor table (one
 * workgroup per hero_adamw_multi_chunk()-element chunk). `chunk_tensor[c]` is the descriptor a chunk
 * belongs to, `chunk_index[c]` its index within that tensor. A tensor's own step count is
 * step - step_lag (parameters that received no gradient in some steps lag behind, as with the
 * reference's per-parameter state['step']). */
typedef struct HeroTensorDesc {
  float* p;
  const float* g;
  float* m;
  float* v;
  uint64_t n;
  int32_t group;
  int32_t step_lag;
} HeroTensorDesc;
typedef struct HeroAdamWGroup {
  float lr, beta1, beta2, eps, weight_decay;
} HeroAdamWGroup;
typedef struct HeroAdamWMulti {
  const HeroTensorDesc* descs; /* device */
  const int32_t* chunk_tensor; /* device [n_chunks] */
  const int32_t* chunk_index;  /* device [n_chunks] */
  int n_chunks;
  HeroAdamWGroup groups[8];
  int step;
  const float* grad_sumsq;
  float max_grad_norm;
  float grad_scale;
  const int32_t* step_ptr; /* optional device scalar overriding `step` (hipGraph replays)      */
  const float* lr_ptr;     /* optional device array [8] overriding groups[].lr                 */
  int32_t* tensor_steps;   /* optional device array of PER-TENSOR step counts (round 3): a tensor's count lives  */
                           /* in slot descs[i].step_lag, is incremented by this call (a pre-pass over the        */
                           /* n_tensors descriptors) and is the step of its bias correction - the reference's    */
                           /* state['step'], which only advances when the parameter is updated                   */
                           /* (optim/adamw.py:71-72), kept on the device so that captured graphs of different    */
                           /* tasks do not advance the counters of parameters they skip                          */
  int n_tensors;           /* number of descriptors (needed with tensor_steps)                                   */
} HeroAdamWMulti;
int hero_adamw_multi(const HeroAdamWMulti* a, hero_stream_t stream);
int hero_adamw_multi_chunk(void);
/* hero_adamw_multi with a per-tensor DEVICE gate: `tensor_gate` is an int32 array in device memory, */
/* one entry per descriptor (n_tensors of them), read by the kernels when they run; NULL =           */
/* hero_adamw_multi.  A tensor whose entry is 0 is skipped completely - every chunk workgroup of it  */
/* returns before it reads or writes p, g, m or v, and its slot in tensor_steps does not advance:    */
/* the reference's `if p.grad is None: continue` (optim/adamw.py) decided on the device, so that a   */
/* captured optimiser step can leave out parameters whose loss term was gated off for the whole      */
/* accumulation window.  Tensors with a non-zero entry get hero_adamw_multi's arithmetic and bits.   */
/* A gate table needs tensor_steps and n_tensors (a skipped tensor's step count has to fall behind;  */
/* a host-side `step` cannot), else HERO_ERR_ARG and no launch.  Plain extra argument: a             */
/* backward-compatible addition, HERO_ABI_VERSION stays.                                             */
int hero_adamw_multi_gated(const HeroAdamWMulti* a, const int32_t* tensor_gate, hero_stream_t stream);

/* Multi-tensor refresh of the compute copies of the fp32 master weights (after an optimiser     */
/* step): ONE launch casts / transposes every tensor of a device-resident descriptor table.     */
/*   transpose == 0: dst[r * ldd + c]        = (dst_dtype) src[r * cols + c]                      */
/*   transpose == 1: dst[c * ldd + r]        = (dst_dtype) src[r * cols + c]                      */
/* (dst already points at the tensor's slot inside a packed [sum N, K] / [K, sum N] buffer.)     */
/* Work is cut into tiles of 64 x 64 elements: tile_desc[t] = descriptor, tile_index[t] = tile   */
/* number inside it (row-major over ceil(rows/64) x ceil(cols/64)).                              */
typedef struct HeroCopyDesc {
  const float* src;
  void* dst;
  int32_t rows, cols, ldd;
  int32_t transpose;
  int32_t dst_dtype;
  int32_t pad_;
} HeroCopyDesc;
int hero_copy_multi(const HeroCopyDesc* descs, const int32_t* tile_desc, const int32_t* tile_index,
                    int n_tiles, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* VSM / VCMR task head - model/pretrain.py:62-116,128-201,203-292,  */
/* model/encoder.py:460-471.  The few hundred tiny fp32 tensor ops between the encoders and the  */
/* three loss scalars as a dozen kernels.  Every op has its forward and backward here; the two   */
/* dense contractions in between (video_query_linear, normalised query x context scores) are    */
/* hero_gemm calls.  All row-major, fp32 unless a dtype is given.                                */
/* ------------------------------------------------------------------------------------------ */
/* Query pooling (QueryFeatEncoder.get_modularized_queries, model/encoder.py:460-471):           */
/*   sc[b,l] = <q[b,l,:], w>; att = softmax_l(sc*mask + (1-mask)*-1e4); pooled = sum_l att*q.    */
typedef struct HeroQueryPool {
  const void* q;          /* [B, L, D] dtype                                                    */
  const float* mask;      /* [B, L] 0/1                                                         */
  const float* w;         /* [D] modular_vector_mapping.weight                                  */
  float* pooled;          /* fwd out [B, D]                                                     */
  float* att;             /* fwd out / bwd in [B, L]                                            */
  const float* dpooled;   /* bwd in [B, D]                                                      */
  void* dq;               /* bwd out [B, L, D] dtype                                            */
  float* dw;              /* bwd out [B, D]: per-query shares of dw, OVERWRITTEN; the caller sums the  */
                          /* rows (hero_colsum): a fixed-order sum instead of B-way fp32 atomics       */
  int B, L, D, dtype;
} HeroQueryPool;
int hero_query_pool_fwd(const HeroQueryPool* a, hero_stream_t stream);
int hero_query_pool_bwd(const HeroQueryPool* a, hero_stream_t stream);

/* Video-QA head (HeroForVideoQA.get_modularized_video, model/videoQA.py:36-59): two attention pools over the frame   */
/* rows of the A answer copies of each video, from ONE read of the rows for both score vectors.                     */
/*   x [Nv * A, Lt, D] dtype: the encoder output, read in place - rows l < L of every sequence are frames, the QA  */
/*   token rows behind them are not touched.  mask [Nv * A, L] 0/1 fp32.  w_qa, w_se [D] fp32.                     */
/*   s_qa = <x, w_qa>, s_se = <x, w_se>, both through mask_logits (s * m + (1 - m) * -1e4);                        */
/*   att_qa = softmax over l -> qa_pooled [Nv, A, D];  att_se = softmax over a -> se_pooled [Nv, L, D]; both        */
/*   attention tables are [Nv, A, L] fp32 and are what the backward reads.  A masked frame has att_se = 1 / A.     */
/* Backward: dx [Nv * A, Lt, D] dtype is written WHOLE (rows >= L as zeros: no memset by the caller); dw_qa, dw_se  */
/* are [Nv, D] per-video shares, OVERWRITTEN - the caller sums the rows in a fixed order (no fp atomics).          */
/* Envelope: 1 <= A <= 8, 1 <= L <= 256, L <= Lt <= 512, D % 4 == 0, D <= 1024; outside it HERO_ERR_ARG.           */
/* Plain arguments, no struct: a backward-compatible addition, HERO_ABI_VERSION stays.                              */
int hero_qa_pool_fwd(const void* x, const float* mask, const float* w_qa, const float* w_se, float* qa_pooled, float* se_pooled,
                     float* att_qa, float* att_se, int Nv, int A, int L, int Lt, int D, int dtype, hero_stream_t stream);
int hero_qa_pool_bwd(const void* x, const float* mask, const float* w_qa, const float* w_se, const float* att_qa, const float* att_se,
                     const float* dqa, const float* dse, void* dx, float* dw_qa, float* dw_se,
                     int Nv, int A, int L, int Lt, int D, int dtype, hero_stream_t stream);

/* VIOLIN head (HeroForViolin, model/violin.py:30-47 and 73-81).  Plain arguments, no struct: a backward-compatible  */
/* addition, HERO_ABI_VERSION stays.                                                                                */
/* Frame pool: x [S, Lt, D] dtype is the encoder output, read in place - rows l < L of every sequence are frames,  */
/*   the statement tokens behind them are not touched.  mask [S, L] 0/1 fp32, w [D] fp32.                          */
/*   att[s, l] = softmax_l(<x[s, l], w> * m + (1 - m) * -1e4)  [S, L] fp32;  pooled[s] = sum_l att x  [S, D] fp32. */
/*   Backward: dx [S, Lt, D] dtype is written WHOLE (rows >= L as zeros: no memset by the caller); dw_part is      */
/*   [S, D] per-sequence shares, OVERWRITTEN - the caller sums the rows in a fixed order (no fp atomics).          */
/*   Envelope: S >= 0 (0: no launch), 1 <= L <= 256, L <= Lt <= 512, D % 4 == 0, 4 <= D <= 1024; else HERO_ERR_ARG.*/
int hero_frame_pool_fwd(const void* x, const float* mask, const float* w, float* pooled, float* att,
                        int S, int L, int Lt, int D, int dtype, hero_stream_t stream);
int hero_frame_pool_bwd(const void* x, const float* mask, const float* w, const float* att, const float* dpooled,
                        void* dx, float* dw_part, int S, int L, int Lt, int D, int dtype, hero_stream_t stream);
/* Classifier tail: h [S, K] dtype (the MLP's LayerNorm output), w [K] fp32, b [1] fp32, targets [S] int64 0/1.    */
/*   logits[s] = z = <h[s], w> + b;  term_s = min(softplus(t ? -z : z), 100), softplus(z) = max(z, 0) +            */
/*   log1p(exp(-|z|));  loss[0] = mean_s term_s.  acc (may be NULL) is float[3] and is ACCUMULATED:                */
/*   acc[0] += sum_s term_s, acc[1] += #{s: (z > 0) == (t == 1)} (z == 0 predicts 0), acc[2] += S.                 */
/*   Backward: dloss is a DEVICE float[1]; dz_s = dloss * (sigmoid(z_s) - t_s) / S (also past the clamp, where the */
/*   reference's gradient is 0); dh[s] = dz_s w [S, K] dtype, dw = sum_s dz_s h[s] [K] fp32, db = sum_s dz_s [1],  */
/*   all OVERWRITTEN.  Sums over s run in a fixed order.  Envelope: S >= 1, K % 4 == 0, 4 <= K <= 2048.            */
int hero_bce_head_fwd(const void* h, const float* w, const float* b, const long long* targets, float* logits, float* loss,
                      float* acc, int S, int K, int dtype, hero_stream_t stream);
int hero_bce_head_bwd(const void* h, const float* w, const float* logits, const long long* targets, const float* dloss,
                      void* dh, float* dw, float* db, int S, int K, int dtype, hero_stream_t stream);

/* F.normalize(x, dim=-1, eps) (model/pretrain.py:370-371): y = x / max(||x||_2, eps).           */
/* rnorm[r] = 1/max(||x_r||, eps), negated when the clamp was active (backward then skips the   */
/* projection term).                                                                            */
typedef struct HeroRowNorm {
  const void* x;          /* [rows, cols] x_dtype                                               */
  float* y;               /* fwd out [rows, cols] fp32                                          */
  float* rnorm;           /* fwd out / bwd in [rows]                                            */
  const float* dy;        /* bwd in [rows, cols] fp32                                           */
  void* dx;               /* bwd out [rows, cols] x_dtype                                       */
  int rows, cols, x_dtype;
  float eps;
} HeroRowNorm;
int hero_rownorm_fwd(const HeroRowNorm* a, hero_stream_t stream);
int hero_rownorm_bwd(const HeroRowNorm* a, hero_stream_t stream);

/* Video-level scores (model/pretrain.py:364-382): s[m, n*L + l] = <qn[m], cn[n, l]> comes from  */
/* hero_gemm; this is mask_logits + max over l:  out[m,n] = max_l (s*mask[n,l] + (1-mask)*-1e4). */
/* Backward: g[m,n] = gc[0]*ds_ctx[m,n] + gq[0]*ds_q[m,n] (the ranking loss' two gradient        */
/* matrices and the upstream gradients of its two scalars) flows to the arg-max entry only:     */
/*   dqn[m,:]  = sum_n g*mask[n,arg]*cn[n,arg,:];   dcn[n,arg,:] += g*mask*qn[m,:]  for          */
/* n in [n0, n0+n_own) (a data-parallel rank only needs its own videos' rows; dcn is            */
/* [n_own*L, D] and is fully written).                                                          */
/* Tie rule: arg[m,n] is the FIRST frame l that attains the maximum (numpy.argmax; a fully       */
/* masked video has every frame at exactly -1e4, so arg = 0 and mask[n,0] = 0 stops the          */
/* gradient).  The backward sends the whole gradient of a pair to that one frame.                */
typedef struct HeroScoreMax {
  const float* s;         /* [M, N*L], row stride ld_s >= N*L                                   */
  const float* mask;      /* [N, L] 0/1                                                         */
  float* out;             /* fwd out [M, N]                                                     */
  int32_t* arg;           /* fwd out / bwd in [M, N]                                            */
  const float* ds_ctx;    /* bwd in [M, N]                                                      */
  const float* ds_q;      /* bwd in [M, N]                                                      */
  const float* gc;        /* bwd in: device scalar                                              */
  const float* gq;        /* bwd in: device scalar                                              */
  const float* qn;        /* bwd in [M, D]                                                      */
  const float* cn;        /* bwd in [N*L, D]                                                    */
  float* dqn;             /* bwd out [M, D]                                                     */
  float* dcn;             /* bwd out [n_own*L, D]                                               */
  int M, N, L, D, n0, n_own, ld_s;
  float gc_scale, gq_scale; /* bwd: *gc and *gq are multiplied by these (the loss weights, folded in; 1.0f = none) */
} HeroScoreMax;
/* out[s] = scales[s] * sum(src[s * seg_len .. (s + 1) * seg_len)), 1..4 segments, fixed summation order: the final
 * reductions of the loss head (sum of the start / end rows, means of the ranking-loss rows) with the loss weights
 * (model/pretrain.py:283-290) folded in - one launch instead of sum / mean / mul per loss.  `scales` is a HOST array. */
int hero_sums_scaled(const float* src, int n_segs, int seg_len, const float* scales, float* out, hero_stream_t stream);
int hero_score_max_fwd(const HeroScoreMax* a, hero_stream_t stream);
int hero_score_max_bwd(const HeroScoreMax* a, hero_stream_t stream);

/* In-batch ranking loss over ALL negatives (get_video_level_loss, use_all_neg=True,            */
/* model/pretrain.py:203-264): query m belongs to video m / (nq/nv).  loss_ctx_rows[m] = mean    */
/* over the other videos n of w*rl(s[m,own], s[m,n]); loss_q_rows[m] = mean over the queries m2  */
/* of other videos of w*rl(s[m,own], s[m2,own]); rl = hinge(margin) or log1p(exp(neg-pos));      */
/* w = 1, or with hard negatives hard_w for the `pool` largest negatives of that row and easy_w  */
/* for the rest.  ds_ctx / ds_q = gradients of mean(loss_ctx_rows) / mean(loss_q_rows) w.r.t. s  */
/* (both fully written).                                                                        */
/* Tie rule of the hard-negative ranking: descending by value, equal values in index order (a    */
/* stable descending sort): rank(c) = #{c2 : s[c2] > s[c] or (s[c2] == s[c] and c2 < c)} over    */
/* the negatives of the row (index = video) / column (index = query); rank < pool is "hard".     */
typedef struct HeroRankLoss {
  const float* s;         /* [nq, nv]                                                           */
  float* loss_ctx_rows;   /* [nq]                                                               */
  float* loss_q_rows;     /* [nq]                                                               */
  float* ds_ctx;          /* [nq, nv]                                                           */
  float* ds_q;            /* [nq, nv]                                                           */
  int nq, nv;
  float margin;
  int lse;                /* 0 hinge, 1 lse                                                     */
  int hard;               /* use_hard_negative                                                  */
  int pool;               /* hard_pool_size                                                     */
  float hard_w, easy_w;   /* hard_neg_weight, 0.1                                               */
} HeroRankLoss;
int hero_rank_loss(const HeroRankLoss* a, hero_stream_t stream);

/* Start / end localisation (model/pretrain.py:128-166, 96-110): sim[b,l] = <q2[b], ctx[b,l]>,    */
/* st/ed = Conv1d(1,1,K,pad=K/2,no bias)(sim), mask_logits, cross-entropy against targets[b,0/1] */
/* (ignore_index -1, mean over the valid rows of each).  loss_rows[b] = ce_st[b]/n_st +           */
/* ce_ed[b]/n_ed (sum over b = the reference's loss_st_ed).                                      */
/* Every entry of `targets` must be -1 or in [0, L): the kernels index the logits with it        */
/* UNCHECKED (a masked frame is allowed as a target, a frame outside the video is not).  A       */
/* column whose targets are all -1 divides by zero, as the reference's mean does.                */
typedef struct HeroStEd {
  const float* q2;        /* [B, D] video_query_linear(modularized query)                       */
  const void* ctx;        /* [B, L, D] dtype: frame embeddings                                  */
  const float* mask;      /* [B, L] 0/1                                                         */
  const float* w_st;      /* [K]                                                                */
  const float* w_ed;      /* [K]                                                                */
  const int64_t* targets; /* [B, 2]                                                             */
  float* loss_rows;       /* fwd out [B]                                                        */
  float* p_st;            /* fwd out / bwd in [B, L] softmax                                    */
  float* p_ed;            /* fwd out / bwd in [B, L]                                            */
  float* sim;             /* fwd out / bwd in [B, L]                                            */
  const float* g;         /* bwd in: device scalar, upstream gradient of sum(loss_rows)         */
  float* dq2;             /* bwd out [B, D]                                                     */
  void* dctx;             /* bwd out [B, L, D] dtype                                            */
  float* dw_st;           /* bwd out [K], ACCUMULATED (+=)                                      */
  float* dw_ed;           /* bwd out [K], ACCUMULATED (+=)                                      */
  int B, L, D, K, dtype;
  float g_scale;          /* bwd: *g is multiplied by this (the loss weight, folded in; 1.0f = none)    */
  float* ws;              /* bwd scratch, hero_st_ed_bwd_workspace_bytes(B) bytes, ZERO before the first */
                          /* use (the kernel leaves its arrival counter at zero): per-pair shares of     */
                          /* dw_st / dw_ed, folded in pair order by the last workgroup to arrive - the   */
                          /* same sum every run (round 3: B-way fp32 atomics)                            */
} HeroStEd;
size_t hero_st_ed_bwd_workspace_bytes(int B);
int hero_st_ed_fwd(const HeroStEd* a, hero_stream_t stream);
int hero_st_ed_bwd(const HeroStEd* a, hero_stream_t stream);
/* The same two kernels behind a DEVICE gate word (the reference drops this term on a per-step   */
/* draw, model/pretrain.py:74-75; a captured launch cannot branch on the host).  `gate` points   */
/* to one int32 in device memory, read by the kernel when it runs - never by the host - so one   */
/* captured launch serves both values; NULL = the entry points above, which are this case.       */
/*   *gate != 0: exactly hero_st_ed_fwd / hero_st_ed_bwd.                                        */
/*   *gate == 0, fwd: loss_rows[b] = +0.0f for every pair; p_st, p_ed and sim keep their bytes.  */
/*   *gate == 0, bwd: exact +0 to all of dq2 and dctx (in dctx's dtype); nothing is added to     */
/*     dw_st / dw_ed; `ws` - shares and arrival counter - is not touched (the counter is still   */
/*     zero for the next gated-on launch); p_st, p_ed, sim, ctx and g are NOT READ: a NaN in     */
/*     them reaches no output.  A branch at the top of the kernel, uniform over the grid.        */
/* Plain extra argument: a backward-compatible addition, HERO_ABI_VERSION stays.                 */
int hero_st_ed_fwd_gated(const HeroStEd* a, const int32_t* gate, hero_stream_t stream);
int hero_st_ed_bwd_gated(const HeroStEd* a, const int32_t* gate, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Full-corpus moment retrieval (eval_vcmr.py:232-323, 327-338; utils/tvr_eval_utils.py:95-129, */
/* 237-260): plain pointer / scalar arguments only, no struct.  Both selections are exact (the  */
/* same multiset of scores as a full sort), bit-reproducible, and break ties by the lower index. */
/* ------------------------------------------------------------------------------------------ */
/* The k largest of every row of scores [M, N] (row stride ld), best first: val [M, k] fp32, idx [M, k] int32.  alpha != 0:
 * val = exp(alpha * score), selected on the score (eval_vcmr.py:266-269: exp(q2c_alpha * s), torch.topk); alpha == 0: val is
 * the score.  Equal scores: lower index first.  k > N: the remaining slots are val 0, idx -1.  N <= 65536, k <= 128. */
int hero_topk_rows(const float* scores, int M, int N, int ld, int k, float alpha, float* val, int* idx, hero_stream_t stream);
/* Start / end probabilities of selected (query, video) pairs (eval_vcmr.py:232-238, model/pretrain.py:96-110 cross branch).
 * sim [Nq, >= Nv * L] fp32 (row stride ld_sim): sim[q, v * L + l] = <video_query_linear(q), ctx[v, l]>, a GEMM output;
 * mask [Nv, L] 0/1 fp32; sel [Nq, K] int32 video indices.  For each (q, j): the L similarities of video sel[q, j], both
 * convolutions (odd, stride 1, `taps` <= 15, zero padding taps / 2) over the WHOLE row - positions beyond the video's
 * length included, as the reference's convolution sees them - then mask_logits and a softmax over L.  st_prob, ed_prob:
 * [Nq, K, L] fp32.  sel[q, j] outside [0, Nv) gives a row of zeros.  L <= 1024. */
int hero_st_ed_probs(const float* sim, long long ld_sim, const float* mask, const int* sel, const float* w_st, const float* w_ed, int Nq,
                     int Nv, int K, int L, int taps, float* st_prob, float* ed_prob, hero_stream_t stream);
/* The top_n moments of every query (eval_vcmr.py:284-323).  st_prob, ed_prob [Nq, K, L], w [Nq, K] fp32, all >= 0.  Candidates:
 * every (j, m, n) with min_l <= n - m < max_l and n < L - the ones of generate_min_max_length_mask; score = st[q, j, m] *
 * w[q, j] * ed[q, j, n].  score [Nq, top_n] fp32 best first, flat [Nq, top_n] int32 = (j * L + m) * L + n.  Equal scores: lower
 * flat index first.  Fewer than top_n candidates: score 0, flat -1 in the remaining slots.  The [Nq, K, L, L] products are never
 * stored.  K = 1 with w = 1 is the single-video case (SVMR).  L <= 256, K <= 128, top_n <= 1024. */
int hero_moment_topk(const float* st_prob, const float* ed_prob, const float* w, int Nq, int K, int L, int min_l, int max_l, int top_n,
                     float* score, int* flat, hero_stream_t stream);
/* Greedy temporal NMS of sorted candidate rows (utils/tvr_eval_utils.py:35-92 temporal_non_maximum_suppression, :132-175
 * filter_vcmr_by_nms, :214-234 post_processing_svmr_nms).  video, st, ed int32 [Nq, N]: FRAME indices, ed inclusive, rows in
 * descending score order (hero_moment_topk's order; scores are not read); video < 0 or st < 0 marks a vacant slot, which is
 * never kept and suppresses nothing.  Candidates of one video form a group (single-video rows: any one value >= 0).  The row is
 * walked in order: a candidate that is still alive and whose group has kept fewer than per_video_cap is kept and kills
 * every later candidate of its group whose IoU with it is STRICTLY greater than thd; the walk stops after max_after
 * survivors - the first max_after survivors in row order are the reference's sorted(...)[:max_after_nms].
 * per_video_cap is the reference's quirk, kept: it never hands its max_after_nms to the inner function, whose default of
 * 100 therefore always applies PER VIDEO (:35-36, 159-160, 229-230); pass 100 to reproduce it.
 * IoU is the reference's on the half-open frame spans [st, ed + 1): inter = max(0, min(ed) + 1 - max(st)), "union" =
 * max(ed) + 1 - min(st) (the hull), inter / union as a float64 division compared with thd as a double.  The reference divides
 * seconds = frames * vfeat_interval; where those products are exact (1.5, 2: every interval of its configs) both quotients
 * are the same rational correctly rounded, so no interval is needed and exact ties agree (3/5 at thd 0.6 survives).
 * keep int32 [Nq, max_after]: positions in the input row of the survivors, ascending, -1 in unused slots; count int32 [Nq].
 * One launch, no workspace, no atomics, bit-reproducible.  1 <= N <= 1024, 1 <= max_after <= N. */
int hero_moment_nms(const int* video, const int* st, const int* ed, int Nq, int N, double thd, int per_video_cap, int max_after, int* keep,
                    int* count, hero_stream_t stream);
/* Rank of the first correct prediction of every query (utils/tvr_standalone_eval.py:86-257 eval_by_task_type, without its
 * per-query matrices).  video, st, ed int32 [Nq, P] with row stride ld (st and ed may both be NULL: video retrieval, then T
 * must be 0); gt_video int32 [Nq]; gt_ts fp32 [Nq, 2] seconds; thds fp32 [T] on the device, 0 <= T <= 8.
 * first int32 [Nq, T + 1]: column 0 = first position whose video == gt_video; column 1 + t = first position with a video
 * match AND IoU >= thds[t]; P where there is none.  Vacant slots (video < 0 or st < 0) never match.  IoU in fp32 as
 * compute_temporal_iou_batch: prediction seconds float(st) * interval and float(ed + 1) * interval, "union" = max(end) -
 * min(start), 0 where that is 0, compared iou >= thd in fp32.  Single-timestamp ground truth only (TVR, How2R). */
int hero_first_hit(const int* video, const int* st, const int* ed, int Nq, int P, int ld, const int* gt_video, const float* gt_ts, float interval,
                   const float* thds, int T, int* first, hero_stream_t stream);
/* hero_first_hit for ground truth with several annotators (DiDeMo; utils/tvr_standalone_eval.py:157-170).  gt_ts fp32
 * [Nq, G, 2] seconds, padded; gt_n int32 [Nq], 1 <= gt_n[q] <= G (values outside are clamped), 1 <= G <= 16; slots at index
 * >= gt_n[q] are never read.  Column 1 + t = first position with a video match at which at least `need` of the gt_n[q]
 * timestamps have IoU >= thds[t]; need = 2 when gt_n[q] >= 4 (the reference's least_n_overlap), else 1.  Column 0, vacancy,
 * the fp32 IoU and every other argument are hero_first_hit's: the same row scan, of which hero_first_hit is the G = 1
 * instance.  T > 0 needs st, ed, gt_ts and gt_n. */
int hero_first_hit_multi(const int* video, const int* st, const int* ed, int Nq, int P, int ld, const int* gt_video, const float* gt_ts,
                         const int* gt_n, int G, float interval, const float* thds, int T, int* first, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Softmax cross-entropy over wide logit rows (pre-training heads, BASELINE configs[3]):        */
/*   MLM  model/encoder.py:355-389, model/layers.py:330-354 (vocabulary GEMM output; `cols`     */
/*        excludes the vocabulary padding of model/encoder.py:232-233, ld includes it)          */
/*   MFM-NCE model/model.py:271-291 (logits / nce_temp)   FOM model/model.py:293-336            */
/* x = logits * inv_temp;  loss[r] = lse(x[r, :cols]) - x[r, labels[r]]  (0 when labels[r] ==   */
/* ignore_index);  dlogits[r, c] = (softmax(x[r])[c] - [c == labels[r]]) * dloss[r] * inv_temp, */
/* zero rows for ignored labels, zero in columns >= cols.  dlogits may alias logits.            */
/* ------------------------------------------------------------------------------------------ */
typedef struct HeroCrossEntropy {
  const void* logits;    /* [rows, ld] dtype                                                    */
  const int64_t* labels; /* [rows]                                                              */
  float* loss;           /* fwd out [rows]                                                      */
  float* lse;            /* fwd out / bwd in [rows]: log-sum-exp of x[r, :cols]                 */
  const float* dloss;    /* bwd in [rows]                                                       */
  void* dlogits;         /* bwd out [rows, ld] dtype                                            */
  int rows, cols, ld, dtype;
  float inv_temp;
  int64_t ignore_index;
} HeroCrossEntropy;
int hero_cross_entropy_fwd(const HeroCrossEntropy* a, hero_stream_t stream);
int hero_cross_entropy_bwd(const HeroCrossEntropy* a, hero_stream_t stream);

/* The same loss with the live row count ON THE DEVICE - the loss heads of the fixed-capacity pre-training batches, whose    */
/* masks change under a replayed hipGraph.  count: one device word, NULL = rows.  Row r is live when r < min(*count, rows)     */
/* and labels[r] is not ignore_index and lies in [0, cols).                                                                   */
/* fwd: a row below the count gets loss[r] / lse[r] bit for bit as hero_cross_entropy_fwd writes them (one row body); a row at */
/*   or behind the count gets loss = lse = 0 and its logits are NOT read.  Then one workgroup folds the live rows' losses in   */
/*   float64 in a fixed order: mean_cnt[0] = (float)(sum / max(n_live, 1)), mean_cnt[1] = (float)n_live; no live row (or       */
/*   rows == 0) gives (0, 0).                                                                                                 */
/* bwd: g = dloss[0] / max(mean_cnt[1], 1), both read on the device; live rows get (softmax - onehot) * g * inv_temp with the  */
/*   columns [cols, ld) zero; every other row gets +0 over all ld columns, and no logits are read for it.  dlogits may alias    */
/*   logits.  No atomics, nothing read on the host: both calls can be captured.  logits / dlogits 16-byte aligned,            */
/* inv_temp > 0.  Plain arguments: a backward-compatible addition, HERO_ABI_VERSION stays.                                    */
int hero_ce_counted_fwd(const void* logits, const long long* labels, const int32_t* count, float* loss, float* lse, float* mean_cnt,
                        int rows, int cols, int ld, int dtype, float inv_temp, long long ignore_index, hero_stream_t stream);
int hero_ce_counted_bwd(const void* logits, const long long* labels, const int32_t* count, const float* lse, const float* dloss,
                        const float* mean_cnt, void* dlogits, int rows, int cols, int ld, int dtype, float inv_temp,
                        long long ignore_index, hero_stream_t stream);

/* Label-smoothed loss of the captioning decoder (model/tvc.py:19-64): the KL divergence of softmax(x) to the smoothed one-hot */
/* of label t, over the first `cols` columns of [rows, ld] logits, in closed form - no [rows, cols] target matrix:            */
/*   C = cols, s = eps / (C - 1), conf = 1 - eps, H0 = conf ln conf + (C - 1) s ln s with 0 ln 0 = 0 (eps = 1 is allowed)       */
/*   loss = H0 - (conf - s) (x_t - lse) - s (sum_c x_c - C lse),   dx_c = (softmax(x)_c - s - (conf - s) [c == t]) * g           */
/* Rows whose label equals ignore_index (or lies outside [0, cols)) give loss 0 and a zero gradient row; columns >= cols get   */
/* a zero gradient.  fwd: loss [rows], lse [rows], and sum_cnt [2] = (sum of the row losses, number of valid rows), folded by   */
/* one workgroup in a fixed order (rows == 0 gives (0, 0)).  bwd: g = dloss[0] (device scalar) * dloss_rows[r] (optional) /      */
/* max(mean_cnt[1], 1) (optional: pass the forward's sum_cnt for the gradient of the MEAN over the valid rows; the count is     */
/* read on the device, nothing synchronises, both calls can be captured into a hipGraph).  dlogits may alias logits.            */
/* 0 < eps <= 1, cols >= 2, logits / dlogits 16-byte aligned; plain arguments, HERO_ABI_VERSION stays.                         */
int hero_smooth_ce_fwd(const void* logits, const long long* labels, float* loss, float* lse, float* sum_cnt, int rows, int cols,
                       int ld, int dtype, double eps, long long ignore_index, hero_stream_t stream);
int hero_smooth_ce_bwd(const void* logits, const long long* labels, const float* lse, const float* dloss, const float* dloss_rows,
                       const float* mean_cnt, void* dlogits, int rows, int cols, int ld, int dtype, double eps,
                       long long ignore_index, hero_stream_t stream);

/* Validation counters of the pre-training heads (pretrain.py:462-608: validate_mlm / _mffr / _mfm_nce / _fom), one pass over  */
/* the raw head outputs, counters kept on the device.                                                                          */
/* hero_ce_eval: logits [rows, ld] (fp32 / bf16, 16-byte aligned), the first `cols` columns count, x = logits * inv_temp        */
/* (inv_temp > 0).  A row is valid when its label is not ignore_index and lies in [0, cols).  Per valid row: loss = lse(x[:cols]) */
/* - x[label] in fp32, the arithmetic of hero_cross_entropy_fwd; prediction = the lowest column among those whose STORED value  */
/* (converted to fp32, unscaled; -0 equals +0) is the row maximum - a column in [cols, ld) never wins; the row is correct when   */
/* the prediction equals the label.  acc[0..2] += (sum of the valid rows' losses, rows correct, rows valid) in float64: the two */
/* counts are exact integers.  pred (optional, int32 [rows]) is written for every row, valid or not.  NaN logits are not        */
/* ordered: a row that holds one has an unspecified prediction.                                                                */
/* hero_feat_eval: per row of pred [rows, ld_p] / target [rows, ld_t] (one dtype, 16-byte aligned) over `cols` columns, sums in */
/* fp32: l2 = sqrt(sum (p - t)^2), cos = p.t / (max(|p|, 1e-8) * max(|t|, 1e-8)) (F.cosine_similarity; a zero row gives 0).      */
/* acc[0..2] += (sum l2, sum cos, rows) in float64.                                                                            */
/* Both: a 256-thread workgroup per row writes the row results to `workspace` (at least 12 * rows bytes for hero_ce_eval,       */
/* 8 * rows bytes for hero_feat_eval, 4-byte aligned; contents unspecified afterwards), then ONE workgroup adds them to acc in  */
/* a fixed order - no atomics, two runs give the same bits.  rows == 0: no launch, acc untouched.  Nothing is read on the host; */
/* both launches can be captured into a hipGraph.  Plain arguments: a backward-compatible addition, HERO_ABI_VERSION stays.     */
int hero_ce_eval(const void* logits, const long long* labels, int rows, int cols, int ld, int dtype, float inv_temp,
                 long long ignore_index, double* acc, int32_t* pred, void* workspace, hero_stream_t stream);
int hero_feat_eval(const void* pred, const void* target, int rows, int cols, int ld_p, int ld_t, int dtype, double* acc,
                   void* workspace, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Collate on the device: the index tensors of a batch from per-subtitle / per-video length      */
/* arrays (data/data.py:406-512 video_collate + get_gather_index; the python walk of             */
/* sub_idx2frame_idx in model/model.py:156-187).  All arrays int32 on the device.                */
/* ------------------------------------------------------------------------------------------ */
/* gather_index / attn_mask [T, out_size] int64 (data/data.py:504-512, 380-382); out_size is the reference's  */
/* f_attn_masks width = max over rows of (frame slots + tokens) (data/data.py:433-436), <= max_vl + max_sl   */
int hero_collate_subs(const int32_t* sub_nfrm, const int32_t* sub_ntok, int64_t* gather_index, int64_t* attn_mask, int T,
                      int max_vl, int out_size, hero_stream_t stream);
/* f_v_feats [T, max_vl, D] fp32 <- c_v_feats [B, NF, D]: the per-subtitle frame feature copies of            */
/* VideoFeatSubTokDataset.__getitem__ (data/data.py:371-379: frames outside [0, vid_nfrm) dropped, zero rows   */
/* after the kept ones) made on the device; row_vid [T] is scratch (video of each subtitle row).  D % 4 == 0.  */
int hero_collate_gather_feats(const float* c_v_feats, float* f_v_feats, const int32_t* vid_sub_off, const int32_t* vid_nfrm,
                              const int32_t* sub_frm_off, const int32_t* sub_frm, int32_t* row_vid, int T, int max_vl, int B, int NF,
                              int D, hero_stream_t stream);
/* attn_mask [B, NF] int64 = f < vid_nfrm[b] */
int hero_collate_clip_mask(const int32_t* vid_nfrm, int64_t* attn_mask, int B, int NF, hero_stream_t stream);
/* Frame map of collect_frame_outputs, two passes around an exclusive scan done by the caller:       */
/* fill = 0: counts[b * NF + f] = number of (subtitle, slot) pairs matched to frame f of video b;     */
/* fill = 1: entries[offsets[bf] ...] = flat source rows (subtitle row * Lf + slot) in subtitle /     */
/* slot order, inverse[source row] = bf (inverse must be pre-filled with -1).                         */
int hero_collate_frame_map(const int32_t* vid_sub_off, const int32_t* sub_frm_off, const int32_t* sub_frm, const int32_t* offsets,
                           int32_t* counts, int32_t* entries, int32_t* inverse, int B, int NF, int Lf, int fill,
                           hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* The random draws of the pre-training batches on the device (data/mlm.py:21-58 random_word,    */
/* data/mfm.py:19-25 _get_img_mask, data/fom.py:96-115 random_reorder): one clean video batch ->   */
/* the MLM, MFM and FOM batch.  Inputs are DeviceCollate's length slots (int32, device), the clean */
/* f_sub_input_ids [T, max_sl] int64 and c_v_feats [B, NF, D] fp32; the clean tensors are only     */
/* read.  seed_dev is one device word, site a per-task constant, threshold = floor(p * 2^32)       */
/* (<= 2^32: p = 1 selects everything).  The draw is counter-based:                                */
/*   base = splitmix64(*seed_dev ^ site * 0xD6E8FEB86659FD93), k0 / k1 = its low / high half,      */
/*   element e of the padded layout: h = mix32(e ^ k0) (selected iff h < threshold), h2 =           */
/*   mix32(e ^ k1); a bounded integer is lo + ((uint64)x * n >> 32).                                */
/* hero_mlm_mask: e = r * max_sl + c, 1 <= c < sub_ntok[r].  A selected token becomes mask_id when */
/*   h < threshold * 4 / 5, v_lo + (h2 * (v_hi - v_lo) >> 32) when h < threshold * 9 / 10, else    */
/*   stays; a row with sub_ntok >= 2 and no selection selects column 1 (mask_id); column 0 of      */
/*   every row becomes first_token.  ids_out [T, max_sl] int64; txt_mask_tgt [T, out_size] bytes   */
/*   0 / 1 at column max(sub_nfrm[r], 1) + c; txt_labels [T * (max_sl - 1)] int64 = the original   */
/*   ids of the selected tokens in row-major order, -1 behind the count; txt_mask_rows             */
/*   [T * (max_sl - 1)] int32 = their flat indices into [T * out_size], -1 behind the count;       */
/*   count [1] int32.  T <= 4096.                                                                  */
/* hero_mfm_mask: e = b * NF + f, f < vid_nfrm[b]; a video with frames and no selection selects     */
/*   frame (mix32(~b ^ k1) * vid_nfrm[b]) >> 32.  c_v_masks [B, NF], f_v_masks [T, max_vl] bytes   */
/*   0 / 1 (slot k of a row = the k-th frame of its list inside the video, the walk of              */
/*   hero_collate_gather_feats; empty slots 0); feat_targets [B * NF, D] = the selected rows of     */
/*   c_v_feats in (b, f) order, zero rows behind the count; count [1] int32; c_v_feats_out          */
/*   [B, NF, D] and f_v_feats_out [T, max_vl, D] = masked copies (selected rows zero).  row_src     */
/*   [2 * B * NF + T * max_vl] int32 is scratch.  D % 4 == 0, B <= 4096, 16-byte aligned features.  */
/* hero_fom_shuffle: e = b * NF + f, f < vid_nfrm[b], no at-least-one rule.  With the selected      */
/*   positions P[0] < P[1] < ... and the same positions S[i] ordered by (h2, position):             */
/*   shuffled_orders[b, P[i]] = S[i], targets[b, S[i]] = P[i]; elsewhere f and -1.  Both [B, NF]    */
/*   int64.  NF <= 2048.                                                                           */
/* No atomics, nothing allocated, nothing read on the host: two runs give the same bits and every   */
/* launch can be captured.  Plain arguments: a backward-compatible addition, HERO_ABI_VERSION stays. */
/* ------------------------------------------------------------------------------------------ */
int hero_mlm_mask(const int64_t* input_ids, const int32_t* sub_nfrm, const int32_t* sub_ntok, const unsigned long long* seed_dev,
                  unsigned long long site, unsigned long long threshold, long long mask_id, long long v_lo, long long v_hi,
                  long long first_token, int64_t* ids_out, unsigned char* txt_mask_tgt, int64_t* txt_labels, int32_t* txt_mask_rows,
                  int32_t* count, int T, int max_sl, int out_size, hero_stream_t stream);
int hero_mfm_mask(const float* c_v_feats, const int32_t* vid_nfrm, const int32_t* vid_sub_off, const int32_t* sub_frm_off,
                  const int32_t* sub_frm, const unsigned long long* seed_dev, unsigned long long site, unsigned long long threshold,
                  unsigned char* c_v_masks, unsigned char* f_v_masks, float* feat_targets, int32_t* count, float* c_v_feats_out,
                  float* f_v_feats_out, int32_t* row_src, int T, int max_vl, int B, int NF, int D, hero_stream_t stream);
int hero_fom_shuffle(const int32_t* vid_nfrm, const unsigned long long* seed_dev, unsigned long long site, unsigned long long threshold,
                     int64_t* shuffled_orders, int64_t* targets, int B, int NF, hero_stream_t stream);

/* Consumers of the fixed-capacity draws (nothing has a mask-dependent shape; counts stay on the device).                    */
/* hero_mask_partition: mask [n] bytes 0 / non-zero, m = number set.  order [n] int32: order[r] = the r-th set index for      */
/*   r < m, the (r - m)-th unset index for r >= m (both ascending: the row order of the reference's cat([pos, neg]) in         */
/*   mfm_nce); rank [n] int32 = its inverse (rank[order[r]] = r); count [1] int32 = m.  One workgroup, 1 <= n <= 2^20.         */
/* hero_nce_pack_fwd: out [n, D] fp32 = the regressed rows in partition order, targets [n, D] fp32, count = m (clamped to     */
/*   [0, n]), 1 <= cap <= n.  Writes, in `dtype`, cand [round_up(n, 8), D]: cand[r] = targets[r] (r < m), out[r] (m <= r < n), */
/*   zero rows behind n; and masked [cap, D] = out[:cap].                                                                     */
/* hero_nce_pack_bwd: d_out [n, D] fp32 = (r < cap ? d_masked[r] : 0) + (r >= m ? d_cand[r] : 0); d_cand / d_masked in        */
/*   `dtype`, either may be NULL (zero); the targets receive no gradient.  D % 4 == 0, 16-byte aligned buffers.               */
/* All capturable.  Plain arguments: a backward-compatible addition, HERO_ABI_VERSION stays.                                  */
int hero_mask_partition(const unsigned char* mask, int n, int32_t* order, int32_t* rank, int32_t* count, hero_stream_t stream);
int hero_nce_pack_fwd(const float* out, const float* targets, const int32_t* count, void* cand, void* masked, int n, int cap, int D,
                      int dtype, hero_stream_t stream);
int hero_nce_pack_bwd(const void* d_cand, const void* d_masked, const int32_t* count, float* d_out, int n, int cap, int D, int dtype,
                      hero_stream_t stream);

/* Everything the model derives from the int64 index / mask tensors of a batch, in one launch: additive attention   */
/* masks (1 - m) * -10000 (model/layers.py:299-302), fp32 masks, int32 row indices, and f_gather_index as flat rows   */
/* of hero_gather_rows (>= 0: image row, <= -2: text row; model/encoder.py:271-279).  src int64, n elements.          */
enum { HERO_DERIVE_MASK_ADD = 0, HERO_DERIVE_F32 = 1, HERO_DERIVE_I32 = 2, HERO_DERIVE_FLAT_GATHER = 3 };
#define HERO_DERIVE_MAX 16
typedef struct HeroDerive {
  const int64_t* src;
  void* dst;        /* fp32 (MASK_ADD, F32) or int32 (I32, FLAT_GATHER), n elements */
  int64_t n;
  int mode;
  int p0, p1, p2;   /* FLAT_GATHER: row width of src, max_vl, max_sl */
} HeroDerive;
int hero_derive_multi(const HeroDerive* d, int n, hero_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Gradient exchange over RCCL (round 4) - replaces Horovod's allreduce_ / broadcast_ */
/* (utils/distributed.py:19-46, 103-151) and the negatives' allgather (model/pretrain.py:427-451).  */
/* Every collective is ENQUEUED on the caller's stream (no stream, thread or synchronisation of its  */
/* own: a captured step simply contains it).  librccl.so is dlopen-ed by the first call;             */
/* hero_comm_available() = 0 where it is missing.  One communicator per process = per GPU.          */
/* ------------------------------------------------------------------------------------------ */
typedef struct HeroCommBucket {
  void* buf;        /* device buffer, reduced in place                                          */
  size_t count;     /* elements                                                                 */
  int dtype;        /* HERO_F32 or HERO_BF16 (the wire format of hero_amd.utils.distributed.GradArena) */
  int pad_;
} HeroCommBucket;
int hero_comm_available(void);
int hero_comm_unique_id(void* id128);                          /* rank 0: 128 bytes to hand to every rank       */
int hero_comm_init(const void* id128, int rank, int world, void** comm_out);   /* collective; current device  */
int hero_comm_destroy(void* comm);
int hero_comm_rank(void* comm);
int hero_comm_world(void* comm);
int hero_comm_allreduce_buckets(void* comm, const HeroCommBucket* buckets, int n, hero_stream_t stream);  /* SUM, <= 64 buckets, one group */
int hero_comm_broadcast(void* comm, void* buf, size_t bytes, int root, hero_stream_t stream);
int hero_comm_allgather(void* comm, const void* send, void* recv, size_t bytes_per_rank, hero_stream_t stream);
/* recv = the ranks' buffers back to back; bytes_per_rank[world] is a HOST array, equal on every rank (the padded gather   */
/* + slice of model/pretrain.py:383-401 as one group of broadcasts)                                                       */
int hero_comm_allgather_var(void* comm, const void* send, void* recv, const size_t* bytes_per_rank, hero_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HERO_HIP_H_ */
