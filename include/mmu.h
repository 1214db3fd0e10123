/*
 * mmu.h -- C-ABI of libmmu_hip.so, the MI355X (gfx950) kernels of the MMBT
 * multimodal train / uncertainty-eval hot path.
 *
 * Reference being replaced (wooginawunan/multi-modal-uncertainty @ /root/reference,
 * pure PyTorch; its math lives in torchvision + pytorch_pretrained_bert 0.6.x):
 * every entry point below names the reference call it replaces (file:line).
 *
 * Conventions
 *   - Plain pointers + int64 sizes; no framework types.  All device buffers are
 *     owned by the caller; the library never allocates or frees device memory.
 *   - Work is enqueued on the caller's `stream` (a hipStream_t); no device sync.
 *   - Return 0 on success, nonzero on a bad argument / launch failure; the
 *     message is in mmu_last_error() (thread-local).
 *   - bf16 = IEEE bfloat16 bits (uint16), f32 = float.  Master weights, biases,
 *     LayerNorm params and all gradients of parameters are f32.
 *   - "additive key mask" = per (row, key) float added to the attention scores,
 *     0 for a real token and -10000 for a pad (src/mmbt.py:101-112).
 */
#ifndef MMU_H
#define MMU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mmu_stream_t; /* hipStream_t */

enum { MMU_BF16 = 0, MMU_F32 = 1 };

/* ------------------------------------------------------------------ status */
/* ABI version: bumped whenever an entry's argument list or buffer contract changes.  2 (round 5):
 * the residual stream's residue pointers inside mmu_batchnorm_fwd / _fwd_sums and the grad_scale
 * argument of mmu_bertadam_step.  3 (round 6): mmu_embed_bwd's workspace size is
 * mmu_embed_bwd_ws_floats().  4 (round 6): mmu_epilogue grows bn_x / bn_mask / bn_mean (the
 * BatchNorm-backward epilogues STORE_BNB / ADD_RES_BNB).  Still 4 with mmu_embed_bwd_ws_floats_h
 * and H = 1024 in mmu_embed_fwd / _bwd (a new symbol and a newly accepted value; no argument list
 * changed), and with the mmu_*_plan queries (new symbols).  Callers compare mmu_version() with the header they were built against. */
#define MMU_ABI_VERSION 4
int mmu_version(void);
const char* mmu_last_error(void);

/* Dropout under HIP-graph replay (round 5).  A captured launch replays the seed it was
 * captured with; with a device counter set here (uint64, caller-owned, NULL = off) every
 * dropout launch made afterwards folds *counter into its seed when it RUNS
 * (seed ^ counter * 0x9E3779B97F4A7C15), so a graph that advances the counter once per
 * replay draws fresh masks each step while forward and backward of one step agree.
 * A counter of 0 reproduces the eager masks bit for bit.  Process-wide setting.
 * (No reference counterpart: the reference draws torch's RNG per dropout call.) */
int mmu_set_seed_offset(const uint64_t* dev_counter);

/* Deterministic mode (new symbols, ABI stays 4).  Off: every entry launches what it always did.
 * On: no entry reaches a float atomicAdd; the column folds (mmu_colsum_reduce[_multi] and every
 * entry that folds through them), the column sums of mmu_gemm / mmu_colsum_bf16, mmu_embed_bwd
 * and mmu_ece_bins take fixed-order reductions whose result depends on the inputs and the shape
 * alone.  Host state, read when a launch is chosen: a captured graph keeps the mode it was
 * captured under.  Initial value: 1 if the environment holds MMU_DETERMINISTIC=1 at the first call
 * into the library, else 0.  Both work without a GPU.
 *   mmu_gemm with a plain colsum (not the *_STATS / *_BNB tables) always takes the partial-row
 *     path, whatever MMU_GEMM_CS_PART says; batch > 1 with a colsum is refused (mmu_last_error);
 *   mmu_colsum_bf16 over more than 1024 rows needs its scratch table;
 *   mmu_embed_bwd needs the larger workspace mmu_embed_bwd_ws_floats() reports while the mode is
 *     on (16-B aligned);
 *   mmu_uncertainty_decompose launches the same kernel in both modes: it has no atomics, its
 *     sums fold in a fixed lane and wave order, so its result depends on the inputs and the
 *     shape alone and is bitwise repeatable with the mode on or off; mmu_robustness_summary,
 *     mmu_uncertainty_decompose_scaled, mmu_temperature_nll and mmu_ensemble_diversity likewise;
 *     mmu_rank_table too launches one thing in both modes: it adds no float anywhere, and its column
 *     sums are 64-bit integer atomic adds, whose result does not depend on their order. */
int mmu_set_deterministic(int on); /* -> the previous value */
int mmu_get_deterministic(void);

/* ------------------------------------------------------------------ GEMM
 * C[m,n] (op)= sum_k A(m,k) * B(n,k), batched over `batch` with element strides.
 *   A(m,k) = A[m*lda + k] if a_kmajor else A[k*lda + m]      (bf16)
 *   B(n,k) = B[n*ldb + k] if b_kmajor else B[k*ldb + n]      (bf16)
 * Replaces the nn.Linear forward / backward products of pytorch_pretrained_bert
 * BertSelfAttention (query/key/value), BertSelfOutput.dense, BertIntermediate.dense,
 * BertOutput.dense (encoder call: src/mmbt.py:124-126) and the image projection
 * ImageBertEmbeddings.img_embeddings (src/mmbt.py:51,71).
 * Constraints: N % 128 == 0; K % 64 == 0 when an operand is K-major;
 *              M % 128 == 0 when A is M-major (not K-major).
 * Alignment (refused otherwise: the kernels access all of these as 16-B vectors): A, B, C, the
 * residual, aux, bias, res_ln_w / res_ln_b, bn_x, bn_mean and the float2 tables 16-B aligned;
 * lda, ldb, ldx and the ldc / ldr of bf16 rows multiples of 8, those of f32 rows multiples of 4;
 * for batch > 1 every batch stride a multiple of the same.  The plain colsum and res_ln_mean /
 * res_ln_rstd need 4 B only.
 */
enum {
  MMU_EPI_STORE = 0,        /* C = acc (+bias[n]) (+C if accumulate)                     */
  MMU_EPI_BIAS_GELU = 1,    /* z = acc+bias; C = gelu_erf(z); aux (optional) = gelu'(z)  */
  MMU_EPI_BIAS_DROP_RES = 2,/* C = residual + dropout(acc+bias); with c_dtype MMU_F32 the
                               residual is f32 too (the encoder's f32 hidden stream)    */
  MMU_EPI_DGELU = 3,        /* C = acc * aux   (aux = the forward's gelu'(z))            */
  MMU_EPI_ADD_RES = 4,      /* C = acc + residual                                        */
  MMU_EPI_BIAS_DROP_QGELU = 5,/* u = dropout(acc+bias); C = u*sigmoid(1.702u); aux (optional)
                               = keep/(1-p) * d(u*sigmoid(1.702u))/du: FLAVA ResidualAttentionBlock
                               mlp c_fc -> Dropout -> QuickGELU (src/model.py:183-185,196-198) */
  MMU_EPI_STORE_STATS = 6,    /* C = acc (+bias) in bf16, and `colsum` = a float2 table
                               [ceil(M/64)][N] of {sum, sum of squares} of the stored C per column
                               and 64-row block: the training BatchNorm statistics of a conv
                               output, produced by the conv's own epilogue (round 6;
                               mmu_batchnorm_fwd_parts consumes it).  batch 1, no split-K. */
  MMU_EPI_STORE_BNB = 7,
  MMU_EPI_ADD_RES_BNB = 8,  /* STORE / ADD_RES into a bf16 C that is the output gradient dY of a
                               training BatchNorm (+ReLU) whose input was bn_x [M, N] bf16 (ReLU
                               mask bn_mask [M, N/8] u8 as mmu_batchnorm_fwd wrote it, or NULL =
                               no ReLU; batch mean bn_mean [N] f32), and `colsum` = a float2 table
                               [ceil(M/64)][N] of {sum g, sum g (bn_x - mean)} per column and
                               64-row block, g = the stored C * mask: the reduction of that
                               BatchNorm's backward, produced by the epilogue of the product that
                               forms its dY (the next conv's data gradient; round 6,
                               mmu_batchnorm_bwd_parts consumes it).  batch 1, ldc == N, A K-major
                               and B N-major (the 1x1 conv dX = dY_next . W).                  */
};
typedef struct mmu_epilogue {
  int32_t kind;
  int32_t accumulate;       /* STORE only: C += result (f32 C)                         */
  const float* bias;        /* [N] f32 or NULL                                          */
  int64_t bias_bstride;
  const void* residual;     /* bf16 [M, ldr] (f32 for BIAS_DROP_RES into an f32 C)      */
  int64_t ldr, res_bstride;
  void* aux;                /* bf16 [M, ldx]: GELU derivative (written or read)         */
  int64_t ldx, aux_bstride;
  float* colsum;            /* f32 [N] per batch: += column sums of the final C (bias grads) */
  int64_t colsum_bstride;
  float drop_p;             /* BIAS_DROP_RES                                            */
  uint64_t seed;            /* dropout stream: element (z, m, n) uses counter (z*M+m)*N+n */
  float* workspace;         /* optional f32 scratch: lets a STORE/f32/no-bias product split K
                               over workgroups (weight gradients); slabs summed in slice
                               order, so results stay deterministic.
                               Stream-ordered: one workspace per stream.                */
  int64_t workspace_floats;
  /* BIAS_DROP_RES into an f32 C only (optional, all four or none): the f32 residual is the
     LayerNorm OUTPUT recomputed from its f32 input, residual[m][n] =
     (r[m][n] - res_ln_mean[m]) * res_ln_rstd[m] * res_ln_w[n] + res_ln_b[n], with r the
     `residual` rows -- the encoder passes the previous LayerNorm's input (kept for its
     backward anyway) instead of materialising its f32 output.                          */
  const float* res_ln_mean;
  const float* res_ln_rstd;
  const float* res_ln_w;
  const float* res_ln_b;
  int64_t res_ln_bstride;   /* batched products: w / b of batch item z at + z * res_ln_bstride
                               (mean / rstd at + z * M)                                  */
  const void* bn_x;         /* STORE_BNB / ADD_RES_BNB only (ABI 4): see those kinds      */
  const uint8_t* bn_mask;
  const float* bn_mean;
  const uint8_t* res_mask;  /* ADD_RES / ADD_RES_BNB (ABI 4, optional): the residual is gated by
                               a ReLU mask [M, N/8] u8 (bit e of byte (m, n/8) keeps residual[m][n+e];
                               needs ldr == N) -- an identity Bottleneck's skip gradient g = dY3 * mask3
                               read from bn3's dY and mask instead of a materialised dSkip      */
} mmu_epilogue;

int mmu_gemm(const void* A, int64_t lda, int a_kmajor,
             const void* B, int64_t ldb, int b_kmajor,
             void* C, int64_t ldc, int c_dtype,
             int64_t M, int64_t N, int64_t K,
             int64_t batch, int64_t strideA, int64_t strideB, int64_t strideC,
             const mmu_epilogue* epi, mmu_stream_t stream);

/* mmu_gemm whose dropout stream (BIAS_DROP_RES / BIAS_DROP_QGELU) is row-stepped: row m of the
 * (batched: z*M + m) output draws the decisions of row drop_row_offset + m * drop_row_step of a
 * dense [.., N] product, i.e. element (m, n) uses counter (drop_row_offset + m*drop_row_step)*N + n.
 * A compact problem holding every drop_row_step-th row of a dense one (the [CLS] rows of the last
 * encoder layer: row i = dense row i*L) thus drops exactly what the dense run drops there.  Nothing
 * but the counter changes; the seed offset of graph replays (mmu_set_seed_offset) is folded in as
 * in mmu_gemm.  drop_row_step >= 1, drop_row_offset >= 0; (1, 0) is mmu_gemm. */
int mmu_gemm_rows(const void* A, int64_t lda, int a_kmajor,
                  const void* B, int64_t ldb, int b_kmajor,
                  void* C, int64_t ldc, int c_dtype,
                  int64_t M, int64_t N, int64_t K,
                  int64_t batch, int64_t strideA, int64_t strideB, int64_t strideC,
                  const mmu_epilogue* epi, int64_t drop_row_step, int64_t drop_row_offset,
                  mmu_stream_t stream);

/* Sum `parts` rows of a [parts, N] f32 partial table into out[N] (+= if accumulate). */
int mmu_colsum_reduce(const float* partial, int64_t parts, int64_t N, float* out,
                      int accumulate, mmu_stream_t stream);
/* n (1..4) independent mmu_colsum_reduce jobs of one width N in one launch: job z sums parts[z]
 * rows of partial[z] into out[z] (host arrays of n entries; the pointers are device memory). */
int mmu_colsum_reduce_multi(int n, const float* const* partial, const int64_t* parts, float* const* out, int64_t N,
                            int accumulate, mmu_stream_t stream);
/* Column sums of a bf16 [M, N] matrix into out[N] f32 (+= if accumulate): the bias grads
 * of the FLAVA blocks' projections (src/model.py).  `partial` (may be NULL): f32 scratch
 * of at least ceil(M / 64) * N floats; with it the row blocks are sized for ~1 K
 * workgroups and fold through per-block partial rows (mmu_colsum_reduce), without it
 * 1024-row blocks add into out by float atomics. */
int mmu_colsum_bf16(const void* X, int64_t M, int64_t N, int64_t ldx, float* partial,
                    float* out, int accumulate, mmu_stream_t stream);

/* Batched bf16 transpose: for each of n_jobs jobs (a device table of 6 int64 per job:
 * src pointer, dst pointer, rows, cols, src row pitch, dst row pitch; a pitch of 0 means
 * dense: cols / rows), dst[c*dpitch + r] = src[r*spitch + c].  Keeps the K-major
 * (transposed) bf16 copies of the BERT layer weights that the data-gradient products
 * dX = dY.W read as their B operand (the backward of the nn.Linear layers inside
 * pytorch_pretrained_bert BertLayer, src/mmbt.py:124-126), and the flipped, transposed
 * 3x3 filters of the conv data gradient (one job per tap); max_rows / max_cols bound the
 * jobs' shapes (grid size). */
int mmu_transpose_bf16_batched(const int64_t* jobs, int n_jobs, int64_t max_rows, int64_t max_cols,
                               mmu_stream_t stream);

/* ------------------------------------------------------------------ attention
 * softmax(Q K^T / sqrt(64) + keymask) (dropout) V for 12 x 64 heads, Q/K/V read from
 * the token-major fused projection QKV[rows, ld_qkv] (q at col h*64, k at 768+h*64,
 * v at 1536+h*64).  Replaces pytorch_pretrained_bert BertSelfAttention scores /
 * softmax / dropout / context (inside the encoder call src/mmbt.py:124-126).
 *   O   [rows, ld_o] bf16 (col h*64)   LSE [batch*heads, L] f32 (natural log-sum-exp
 *   of the scaled+masked scores).  keymask [batch, L] f32 additive.
 *   dropmask (may be NULL): [batch*heads, L, ceil(L/64)] u64 keep bits of the
 *   attention-probs dropout (bit k of word j = key 64j+k kept), written when
 *   drop_p > 0 for the backward to read.
 */
int mmu_attention_fwd(const void* QKV, int64_t ld_qkv, const float* keymask,
                      void* O, int64_t ld_o, float* LSE,
                      int64_t batch, int64_t L, int64_t heads,
                      float drop_p, uint64_t seed, uint64_t* dropmask, mmu_stream_t stream);
/* dQKV [rows, ld_dqkv] bf16 from dO; `delta` workspace [batch*heads, L] f32;
 * dropmask = the forward's (required when drop_p > 0).
 * dbias_parts (may be NULL): f32 [(ceil(L/128) + 2 ceil(L/64)) * batch, heads*64] receives
 * per-block column sums of dQ (rows [0, nqb*batch)), dK (next nkb*batch rows) and dV (last
 * nkb*batch rows), every element written; summing each row range (mmu_colsum_reduce) gives
 * the Q / K / V bias gradients without another pass over dQKV. */
int mmu_attention_bwd(const void* QKV, int64_t ld_qkv, const float* keymask,
                      const void* O, int64_t ld_o, const void* dO, int64_t ld_do,
                      const float* LSE, float* delta, void* dQKV, int64_t ld_dqkv,
                      int64_t batch, int64_t L, int64_t heads,
                      float drop_p, uint64_t seed, const uint64_t* dropmask, float* dbias_parts,
                      mmu_stream_t stream);

/* Query row 0 only (the [CLS]-pooled model reads token 0 of its last encoder layer alone,
 * src/mmbt.py:124-128): the attention of query row 0 of every (batch, head) over all L keys.
 * Arguments and buffer layouts as mmu_attention_fwd / _bwd; QKV, O, dO, dQKV 16-B aligned, every
 * ld a multiple of 8.  The Q columns of QKV are read in row 0 of each batch item only.
 * Forward: writes O row 0 (per batch item: row b*L), LSE[bh][0] and, with drop_p > 0 and a
 * dropmask, the keep words [bh][0][0..ceil(L/64)) -- the addresses, values and dropout decisions
 * mmu_attention_fwd produces for that row (same seed, same stream); nothing else is written. */
int mmu_attention_row0_fwd(const void* QKV, int64_t ld_qkv, const float* keymask,
                           void* O, int64_t ld_o, float* LSE,
                           int64_t batch, int64_t L, int64_t heads,
                           float drop_p, uint64_t seed, uint64_t* dropmask, mmu_stream_t stream);
/* Backward for a dO that is non-zero in row 0 of each batch item only: reads row 0 of dO, O, LSE
 * and of the keep words (dropmask required when drop_p > 0); writes the dK and dV columns of dQKV
 * for ALL rows and the dQ columns of row 0 only (the dQ columns of the other rows -- zeros in the
 * dense result -- are left untouched).
 * dbias_sums (may be NULL): f32 [3][batch][heads*64], every element written: per batch item the
 * column sums over its rows of dQ (slab 0: dQ row 0 itself), dK (slab 1) and dV (slab 2); summing
 * each slab over the batch (mmu_colsum_reduce, parts = batch) gives the Q / K / V bias gradients. */
int mmu_attention_row0_bwd(const void* QKV, int64_t ld_qkv, const float* keymask,
                           const void* O, int64_t ld_o, const void* dO, int64_t ld_do,
                           const float* LSE, void* dQKV, int64_t ld_dqkv,
                           int64_t batch, int64_t L, int64_t heads,
                           float drop_p, const uint64_t* dropmask, float* dbias_sums,
                           mmu_stream_t stream);

/* ------------------------------------------------------------------ LayerNorm
 * y = LN(x) * w + b over the last dim (768), eps; x, y bf16 [rows, H]; saves
 * mean/rstd f32 [rows].  BertLayerNorm of BertSelfOutput / BertOutput
 * (src/mmbt.py:124-126).
 */
int mmu_layernorm_fwd(const void* X, const float* w, const float* b, void* Y,
                      float* mean, float* rstd, int64_t rows, int64_t H, float eps,
                      int64_t group_rows, int64_t param_stride, mmu_stream_t stream);
/* group_rows / param_stride: row r uses w/b + (r / group_rows) * param_stride, so the K
 * members of a deep ensemble normalise in one launch (group_rows <= 0: one group).
 * mean/rstd may both be NULL (inference). */
/* Backward of y = LN(x): dX = LN'(dY) (+ dRes), optional dXdrop = dropout_bwd(dX)
 * (same (seed, m*H+n) stream as the producing BIAS_DROP_RES epilogue), and partial
 * column sums [ceil(rows/rows_per_part), H] for dgamma, dbeta and dbias
 * (= column sum of dXdrop, or of dX when no dropout output). */
int mmu_layernorm_bwd(const void* dY, const void* X, const float* mean, const float* rstd,
                      const float* w, void* dX, void* dXdrop, float drop_p, uint64_t seed,
                      float* part_dw, float* part_db, float* part_dbias,
                      int64_t rows, int64_t H, int64_t rows_per_part, mmu_stream_t stream);

/* The encoder's f32 hidden stream (post-LN BertLayer, src/mmbt.py:124-126): the LN input
 * S = residual + dropout(branch) stays f32 (written by an f32 BIAS_DROP_RES epilogue), so
 * that the 24 residual adds of the 12 layers are never rounded to bf16.
 * mmu_layernorm_fwd_f32: X f32 [rows, H] -> Y bf16 (the next GEMM's operand) and, when
 * Y32 != NULL, Y32 f32 (the next residual); group_rows / param_stride as above.
 * mmu_layernorm_bwd_f32: mmu_layernorm_bwd with an f32 X. */
int mmu_layernorm_fwd_f32(const float* X, const float* w, const float* b, void* Y, float* Y32,
                          float* mean, float* rstd, int64_t rows, int64_t H, float eps,
                          int64_t group_rows, int64_t param_stride, mmu_stream_t stream);
int mmu_layernorm_bwd_f32(const void* dY, const float* X, const float* mean, const float* rstd,
                          const float* w, void* dX, void* dXdrop, float drop_p, uint64_t seed,
                          float* part_dw, float* part_db, float* part_dbias,
                          int64_t rows, int64_t H, int64_t rows_per_part, mmu_stream_t stream);

/* mmu_layernorm_bwd_f32 with a row-stepped dropout stream (see mmu_gemm_rows): row r of dXdrop
 * draws the decisions of row drop_row_offset + r * drop_row_step; (1, 0) is mmu_layernorm_bwd_f32. */
int mmu_layernorm_bwd_f32_rows(const void* dY, const float* X, const float* mean, const float* rstd,
                               const float* w, void* dX, void* dXdrop, float drop_p, uint64_t seed,
                               float* part_dw, float* part_db, float* part_dbias,
                               int64_t rows, int64_t H, int64_t rows_per_part,
                               int64_t drop_row_step, int64_t drop_row_offset, mmu_stream_t stream);

/* Pre-LN block backward (FLAVA ResidualAttentionBlock, src/model.py:210-212: x + f(LN(x))):
 * dX = LN'(dY) + dRes; part_dbias = column sums of that total dX (the bias gradient of the
 * Linear whose output was added to the residual stream).  No dropout output. */
int mmu_layernorm_bwd_res(const void* dY, const void* X, const float* mean, const float* rstd,
                          const float* w, const void* dRes, void* dX,
                          float* part_dw, float* part_db, float* part_dbias,
                          int64_t rows, int64_t H, int64_t rows_per_part, mmu_stream_t stream);

/* ------------------------------------------------------------------ FLAVA attention
 * nn.MultiheadAttention(x, x, x) with batch_first=False applied to an [S, N, E] tensor
 * (src/model.py:193,205-207; the block receives [B, L, E], so the sequence axis is the
 * BATCH: S = B samples, N = L token positions).  QKV [S*N, ld_qkv] bf16 = the in_proj
 * output, row s*N + n, q at col h*D, k at E + h*D, v at 2E + h*D (E = heads*D).
 * softmax(Q K^T / sqrt(D)) V per (n, h); no mask, no dropout (module defaults).
 *   O [S*N, ld_o] bf16 (col h*D); LSE2 [N*heads, S] f32 = log2-sum-exp2 of the scores
 *   scaled by log2(e)/sqrt(D) (for the backward).  D in {64, 128, 256}.
 * Refused (nonzero return, mmu_last_error): a null pointer; S, N or heads <= 0; another D;
 * ld_qkv < 3E or not a multiple of 8; ld_o < E or not a multiple of 4; N*heads > 65535;
 * S > INT32_MAX - 63 (rows and 64-row tiles are counted in int); QKV not 16-byte, O not 8-byte,
 * LSE2 not 4-byte aligned (16-B row loads, 8-B row stores). */
int mmu_seqattn_fwd(const void* QKV, int64_t ld_qkv, void* O, int64_t ld_o, float* LSE2,
                    int64_t S, int64_t N, int64_t heads, int64_t head_dim, mmu_stream_t stream);
/* dQKV [S*N, ld_dqkv] bf16 (every element written); delta workspace [N*heads, S] f32.
 * Refused: what the forward refuses of QKV, S, N, heads and D; ld_dqkv < 3E or not a multiple of
 * 4; ld_o < E or not a multiple of 4; ld_do < E or not a multiple of 8; QKV or dO not 16-byte,
 * O or dQKV not 8-byte, LSE2 or delta not 4-byte aligned; more than INT32_MAX delta blocks
 * (ceil(S*N*heads / 4), the x dimension of one grid). */
int mmu_seqattn_bwd(const void* QKV, int64_t ld_qkv, const void* O, int64_t ld_o,
                    const void* dO, int64_t ld_do, const float* LSE2, float* delta,
                    void* dQKV, int64_t ld_dqkv, int64_t S, int64_t N, int64_t heads,
                    int64_t head_dim, mmu_stream_t stream);

/* ------------------------------------------------------------------ embeddings
 * Modality-token embed + text gather + concat/gather, one pass
 * (ImageBertEmbeddings src/mmbt.py:58-83, BertEmbeddings src/mmbt.py:121,
 *  torch.cat src/mmbt.py:122, control gather src/mmbt.py:198-229).
 * Source sequence s of length S = n_img+2+T: s=0 [CLS], 1..n_img image proj rows,
 * n_img+1 [SEP] (positions 0..n_img+1, token type 0), then text t at position t,
 * type seg[b,t].  Output row (v,b,j) embeds source position idx[v*Lout + j]
 * (idx == NULL: identity, Lout == S) and is LayerNorm'ed.  X [V*B*Lout, H] bf16,
 * X32 (optional, may be NULL) the same rows in f32 (the encoder's f32 hidden stream);
 * keymask [V*B, Lout] f32 additive; mean/rstd (optional) f32 [V*B*Lout] for backward.
 * Dropout after the LN: drop_img on the image-segment rows (ImageBertEmbeddings.dropout,
 * args.dropout), drop_txt on text rows (BertEmbeddings.dropout 0.1); counter row*H+col.
 * Tables f32: word [vocab,H], pos [maxpos,H], type [2,H]; proj f32 [B, n_img, H].
 * H is 768 (bert-base) or 1024 (bert-large); any other width is refused.
 */
int mmu_embed_fwd(const int64_t* ids, const int64_t* seg, const int64_t* txt_mask,
                  const float* proj, const float* word, const float* pos, const float* type,
                  const float* ln_w, const float* ln_b, float eps,
                  int64_t cls_id, int64_t sep_id,
                  const int64_t* idx, int64_t V, int64_t B, int64_t T, int64_t n_img, int64_t Lout,
                  int64_t H, float drop_txt, float drop_img, uint64_t seed,
                  void* X, float* X32, float* keymask, float* mean, float* rstd, mmu_stream_t stream);
/* Backward of mmu_embed_fwd for the identity variant (training): recomputes the
 * pre-LN sums, LN backward, then scatters: word rows by atomics, position / type
 * / [CLS] / [SEP] by batch reduction, image rows to dproj f32 [B, n_img, H].
 * H is 768 or 1024, as for mmu_embed_fwd.
 * ws: f32 workspace of at least mmu_embed_bwd_ws_floats_h(B, T, n_img, H) floats;
 * mmu_embed_bwd_ws_floats(B, T, n_img) is that size at H = 768 (ABI 3; ABI 2 took
 * B*S*H + 2*ceil(B*S/64)*H, which is larger for every B > 1).  The _h query returns -1 for a
 * width mmu_embed_bwd refuses.
 * Deterministic mode: the size query returns the larger workspace of that mode (the text rows'
 * f32 gradients [B*T, H], the position partials [ceil(B/16), S, H], the segmented sum's carry
 * rows, the sort's pairs and counters) while the mode is on; the word rows are then summed per
 * id over the tokens in stable sorted order, in chunks of mmu_embed_bwd_det_chunk() tokens. */
int64_t mmu_embed_bwd_ws_floats(int64_t B, int64_t T, int64_t n_img);
int64_t mmu_embed_bwd_ws_floats_h(int64_t B, int64_t T, int64_t n_img, int64_t H);
int64_t mmu_embed_bwd_det_chunk(void);
int mmu_embed_bwd(const void* dX, const int64_t* ids, const int64_t* seg,
                  const float* proj, const float* word, const float* pos, const float* type,
                  const float* ln_w, const float* mean, const float* rstd,
                  int64_t cls_id, int64_t sep_id, int64_t B, int64_t T, int64_t n_img, int64_t H,
                  float drop_txt, float drop_img, uint64_t seed, float* d_word, float* d_pos, float* d_type, float* d_ln_w, float* d_ln_b,
                  float* d_proj, float* ws, mmu_stream_t stream);

/* Image transform tail of the Food-101 pipeline (src/dataset.py:488-498: ToTensor +
 * Normalize) on the device: in = uint8 crops [B,H,W,3] (HWC, as decoded), n = B*H*W*3;
 * out = (in/255 - mean[c]) / std[c] with c = index % 3, i.e. the channels-last
 * [B,3,H,W] image, f32 (out_dtype MMU_F32) or bf16 (MMU_BF16).  mean / std: 3 host floats. */
int mmu_image_normalize(const uint8_t* in, int64_t n, const float* mean, const float* stdv, void* out,
                        int out_dtype, mmu_stream_t stream);

/* MaxPool2d(3, stride 2, padding 1) of the ResNet stem (torchvision resnet child 3,
 * src/mmbt.py:19-21): x NHWC bf16 [B,H,W,C] -> y [B,OH,OW,C] + argmax (uint8 position 0..8
 * in the window, same layout as y); backward: dy + argmax -> dx [B,H,W,C] (every element
 * written).  C % 8 == 0, OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1. */
int mmu_maxpool_fwd(const void* x, int64_t B, int64_t H, int64_t W, int64_t C, void* y, uint8_t* argmax,
                    mmu_stream_t stream);
int mmu_maxpool_bwd(const void* dy, const uint8_t* argmax, int64_t B, int64_t H, int64_t W, int64_t C, void* dx,
                    mmu_stream_t stream);

/* AdaptiveAvgPool2d((n,1)) + flatten + transpose of the ResNet map
 * (src/mmbt.py:30,42-44): fmap NHWC bf16 [B,Hh,Ww,C] -> out f32 [B,n,C]; and its backward. */
int mmu_row_pool_fwd(const void* fmap, int64_t B, int64_t Hh, int64_t Ww, int64_t C, int64_t n,
                     float* out, mmu_stream_t stream);
int mmu_row_pool_bwd(const float* dout, int64_t B, int64_t Hh, int64_t Ww, int64_t C, int64_t n,
                     void* dfmap, mmu_stream_t stream);

/* ------------------------------------------------------------------ 3x3 conv weight gradient
 * dW (+)= dConv2d(3x3, stride 1, pad 1)/dW of the ResNet-152 bottleneck conv2 (torchvision
 * Bottleneck.conv2, src/mmbt.py:19-21) on channels-last bf16 maps: X [n_img*H*W, Cin] (the
 * conv input), dY [n_img*H*W, Cout] (its output gradient); dW f32 [Cout][3][3][Cin] (the
 * channels-last filter), += when accumulate.  One implicit-im2col MFMA GEMM (M = Cout,
 * N = 9 Cin, K = pixels; the B operand gathered per tap with zero padding), split-K over
 * the pixels into ws (f32, may be NULL: no split).  Cin % 256 == 0, Cout % 128 == 0. */
int mmu_conv3x3_wgrad(const void* dY, const void* X, float* dW, int64_t n_img, int64_t H, int64_t W,
                      int64_t Cin, int64_t Cout, int accumulate, float* ws, int64_t ws_floats,
                      mmu_stream_t stream);

/* 3x3 / stride-1 / pad-1 convolution as one implicit-im2col MFMA GEMM (the A operand
 * gathered per tap, padding read as zero): Y[pixel][n] = sum over taps t = 3 kh + kw and
 * channels c of X[pixel + (kh - 1, kw - 1)][c] * Wk[n][t * C + c], bf16 in / out,
 * f32 accumulate; X [n_img*H*W, C] and Y [n_img*H*W, N] NHWC rows.  The forward of
 * Bottleneck.conv2 is (X = x, Wk = the channels-last filter [Cout][3][3][Cin]); its data
 * gradient is (X = dY, Wk = the flipped filter transposed to [Cin][3][3][Cout]).
 * C % 64 == 0, N % 128 == 0, N >= 256.  `ws` (optional, ws_floats f32): when the output has
 * too few 256x256 tiles to fill the chip (small batches: e.g. layer3 at batch 32 is 25
 * tiles), the taps / channels are split over workgroups into f32 slabs of ws and summed in
 * slice order into Y (deterministic). */
int mmu_conv3x3_implicit(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W,
                         int64_t C, int64_t N, float* ws, int64_t ws_floats, mmu_stream_t stream);

/* The same two products for the strided convs of the ResNet-152 trunk (the first block of
 * layer2..4: Bottleneck.conv2 3x3 / stride 2 / pad 1 and the downsample 1x1 / stride 2,
 * src/mmbt.py:19-21): ksize 3 (pad 1) or 1 (pad 0), any stride 1..4; X [n_img*H*W, C] the
 * input map, Y / dY [n_img*Ho*Wo, N] with Ho = (H + 2 pad - ksize) / stride + 1 (Wo alike).
 * mmu_conv_implicit: forward (Wk [N][ksize][ksize][C]), C % 64 == 0, N % 64 == 0.
 * mmu_conv_wgrad: filter gradient dW f32 [Cout][ksize][ksize][Cin], Cin % 256 == 0,
 * Cout % 128 == 0.  mmu_conv3x3_* above are (ksize 3, stride 1) of these. */
int mmu_conv_implicit(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W, int64_t C,
                      int64_t N, int64_t ksize, int64_t stride, float* ws, int64_t ws_floats,
                      mmu_stream_t stream);
/* mmu_conv_implicit that also writes the training BatchNorm statistics of Y: stats = float2
 * [ceil(Npix / 64)][N] {sum, sum of squares} per output channel and 64-pixel block of the bf16
 * Y (MMU_EPI_STORE_STATS; with split-K they come from a pass over Y after its reduction). */
int mmu_conv_implicit_stats(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W, int64_t C,
                            int64_t N, int64_t ksize, int64_t stride, float* stats, float* ws, int64_t ws_floats,
                            mmu_stream_t stream);
/* mmu_conv3x3_implicit whose output is the data gradient dX of a 3x3 conv that a training
 * BatchNorm (+ReLU) fed: also writes that BatchNorm's backward reduction table (stats = float2
 * [ceil(Npix / 64)][N] {sum g, sum g (bn_x - bn_mean)}, g = dX * bn_mask; see
 * MMU_EPI_STORE_BNB).  bn_x [Npix, N] bf16, bn_mask [Npix, N/8] u8 or NULL, bn_mean [N] f32.
 * With split-K the table comes from a pass over dX after its reduction. */
int mmu_conv3x3_implicit_bnb(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W, int64_t C,
                             int64_t N, const void* bn_x, const uint8_t* bn_mask, const float* bn_mean,
                             float* stats, float* ws, int64_t ws_floats, mmu_stream_t stream);
int mmu_conv_wgrad(const void* dY, const void* X, float* dW, int64_t n_img, int64_t H, int64_t W, int64_t Cin,
                   int64_t Cout, int64_t ksize, int64_t stride, int accumulate, float* ws, int64_t ws_floats,
                   mmu_stream_t stream);

/* ResNet-152 stem convolution, 7x7 / stride 2 / pad 3, 3 -> 64 channels (torchvision resnet
 * child 0, the image encoder's conv embed: src/mmbt.py:19-21,42), on channels-last bf16:
 * X [n_img, H, W, 3], Wk [64][7][7][3] (the channels-last filter), Y [n_img, Ho, Wo, 64] with
 * Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1; f32 accumulate.  One persistent kernel: tiles of
 * 2 x 64 output pixels, the input patch in LDS, 16x16x32 bf16 MFMAs over the 3-channel taps
 * padded to 4 (K = 224). */
int mmu_stem_conv_fwd(const void* X, const void* Wk, void* Y, int64_t n_img, int64_t H, int64_t W,
                      mmu_stream_t stream);
/* Its filter gradient: dW f32 [64][7][7][3] (+)= sum over pixels of dY (x) im2col(X) (dY
 * [n_img, Ho, Wo, 64] bf16), += when accumulate.  Per-block f32 partials go to ws
 * (>= mmu_stem_conv_wgrad_ws_floats(n_img, H, W) floats) and are summed in block order. */
int64_t mmu_stem_conv_wgrad_ws_floats(int64_t n_img, int64_t H, int64_t W);
int mmu_stem_conv_wgrad(const void* dY, const void* X, float* dW, int64_t n_img, int64_t H, int64_t W,
                        int accumulate, float* ws, int64_t ws_floats, mmu_stream_t stream);

/* ------------------------------------------------------------------ BatchNorm (image trunk)
 * BatchNorm2d [+ residual add] [+ ReLU] of the ResNet-152 trunk (torchvision
 * Bottleneck bn1/bn2/bn3 + downsample, src/mmbt.py:19-21) on channels-last bf16
 * activations X [rows = N*H*W, C] (C % 8 == 0, C <= 2048):
 *   Y = act(X * scale + shift [+ skip]),  act = ReLU when relu != 0.
 * training: batch statistics (biased variance), running_mean / running_var updated
 *   with momentum (unbiased variance), *num_batches_tracked += 1 (each may be NULL);
 *   momentum < 0 = torch's momentum=None (cumulative moving average): the factor is
 *   1 / *num_batches_tracked, which the caller has ALREADY incremented for this pass (required,
 *   not incremented again here),
 *   save_mean / save_invstd [C] f32 written for the backward.
 * eval: running statistics.  weight / bias may be NULL (affine = False).
 * relu_mask (may be NULL; needs relu): [rows, C/8] u8 written with bit e of byte (r, c/8)
 *   = Y[r, c+e] > 0, for the backward to read instead of Y (1/16 of its bytes).
 * y_res / skip_res (may be NULL): the residual stream past bf16 -- y_res [rows, C] i8 is written
 *   with the 8-bit residue of each output, r = rint((v - Y) * 2^15 / 2^e) (v the f32 value, e
 *   the binary exponent of Y); a skip is then read as skip + skip_res * 2^(e(skip) - 15).  Two
 *   uses: a Bottleneck's bn3 (skip, relu, skip_res and y_res all given) and the downsample's
 *   BatchNorm (no skip, no relu, y_res only).
 * ws: device scratch of >= mmu_batchnorm_ws_bytes(C) bytes (per-block partial sums +
 * per-channel coefficients, ~8 MiB), 16-B aligned.
 */
int64_t mmu_batchnorm_ws_bytes(int64_t C);
int mmu_batchnorm_fwd(const void* X, const void* skip, void* Y, int64_t rows, int64_t C,
                      const float* weight, const float* bias, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, int training, float momentum, float eps, int relu,
                      float* save_mean, float* save_invstd, void* relu_mask, const void* skip_res, void* y_res,
                      void* ws, int64_t ws_bytes, mmu_stream_t stream);
/* Training-mode forward whose batch statistics were produced by the conv before it
 * (MMU_EPI_STORE_STATS / mmu_conv_implicit_stats: parts = float2 [nparts][C] block partials of
 * X's {sum, sum of squares} per channel): no statistics pass; finalize (running stats,
 * save_mean / save_invstd) and apply as mmu_batchnorm_fwd with training = 1. */
int mmu_batchnorm_fwd_parts(const void* X, const void* skip, void* Y, int64_t rows, int64_t C, const float* parts,
                            int64_t nparts, const float* weight, const float* bias, float* running_mean,
                            float* running_var, int64_t* num_batches_tracked, float momentum, float eps, int relu,
                            float* save_mean, float* save_invstd, void* relu_mask, const void* skip_res, void* y_res,
                            void* ws, int64_t ws_bytes, mmu_stream_t stream);
/* Training-mode backward.  g = dY * [Y > 0] when relu, from relu_mask when given (the
 * forward's mask), else from Y (the forward's output); g = dY without relu;
 * dX [rows, C] bf16; dSkip (may be NULL) = g, the gradient of the residual input;
 * dweight / dbias (may be NULL) f32 [C] are ACCUMULATED (+=). */
int mmu_batchnorm_bwd(const void* dY, const void* Y, const void* relu_mask, const void* X, int64_t rows,
                      int64_t C, const float* weight, const float* save_mean, const float* save_invstd, int relu,
                      void* dX, void* dSkip, float* dweight, float* dbias, void* ws, int64_t ws_bytes,
                      mmu_stream_t stream);

/* Training-mode backward whose reduction {sum g, sum g (x - mean)} was produced by the product
 * that formed dY (MMU_EPI_STORE_BNB / ADD_RES_BNB, mmu_conv3x3_implicit_bnb: parts = float2
 * [nparts][C] block partials): no reduction pass; finalize (dweight / dbias +=) and apply as
 * mmu_batchnorm_bwd. */
int mmu_batchnorm_bwd_parts(const void* dY, const void* Y, const void* relu_mask, const void* X, int64_t rows,
                            int64_t C, const float* parts, int64_t nparts, const float* weight,
                            const float* save_mean, const float* save_invstd, int relu, void* dX, void* dSkip,
                            float* dweight, float* dbias, void* ws, int64_t ws_bytes, mmu_stream_t stream);

/* Cross-rank (synchronised) BatchNorm: data-parallel training that keeps the reference's
 * whole-batch statistics (src/mmbt.py:19-21 normalises the trunk over the full batch of one
 * device; under DP the batch is split over ranks).  Each training pass is split at its
 * per-channel reduction and the caller sums `sums` over the ranks between the two calls
 * (one all-reduce of 2C+1 doubles; torch.nn.SyncBatchNorm's exchange):
 *   sums [2C+1] f64 = {s1[0..C), s2[0..C), rows}
 *   forward:  mmu_batchnorm_stats (s1 = sum x, s2 = sum x^2 over the local rows), exchange,
 *             mmu_batchnorm_fwd_sums (the training forward of mmu_batchnorm_fwd with the
 *             statistics of the exchanged sums: mean, biased variance over sums[2C] rows;
 *             running stats from the unbiased variance of the same)
 *   backward: mmu_batchnorm_bwd_reduce (s1 = sum g, s2 = sum g (x - mean); dweight / dbias
 *             += this rank's dgamma = s2 * invstd, dbeta = s1, may be NULL), exchange,
 *             mmu_batchnorm_bwd_sums (dX [, dSkip] from the exchanged sums).
 * Arguments otherwise as mmu_batchnorm_fwd / mmu_batchnorm_bwd. */
int mmu_batchnorm_stats(const void* X, int64_t rows, int64_t C, double* sums, void* ws, int64_t ws_bytes,
                        mmu_stream_t stream);
int mmu_batchnorm_fwd_sums(const void* X, const void* skip, void* Y, int64_t rows, int64_t C, const double* sums,
                           const float* weight, const float* bias, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, float momentum, float eps, int relu, float* save_mean,
                           float* save_invstd, void* relu_mask, const void* skip_res, void* y_res, void* ws,
                           int64_t ws_bytes, mmu_stream_t stream);
int mmu_batchnorm_bwd_reduce(const void* dY, const void* Y, const void* relu_mask, const void* X, int64_t rows,
                             int64_t C, const float* save_mean, const float* save_invstd, int relu, double* sums,
                             float* dweight, float* dbias, void* ws, int64_t ws_bytes, mmu_stream_t stream);
int mmu_batchnorm_bwd_sums(const void* dY, const void* Y, const void* relu_mask, const void* X, int64_t rows,
                           int64_t C, const double* sums, const float* weight, const float* save_mean,
                           const float* save_invstd, int relu, void* dX, void* dSkip, void* ws, int64_t ws_bytes,
                           mmu_stream_t stream);

/* ------------------------------------------------------------------ BertAdam
 * Fused multi-tensor BertAdam (pytorch_pretrained_bert 0.6.x, constructed at
 * train.py:142-147; stepped at src/framework.py:303): per-tensor clip
 * (max_grad_norm), m/v update without bias correction, decoupled weight decay
 * (group 0 only), lr * warmup_linear(step/t_total) with the per-tensor step read
 * before its increment, optional bf16 copy of the updated weight for the GEMMs.
 * table (int64, device): 7 per tensor {offset, numel, group (0 decay / 1 no decay),
 *   bf16_offset (-1 = none), active (0 = skipped like a None grad), first_chunk,
 *   n_chunks}, followed by 3 per chunk {tensor, start, len}.
 * steps int32 [n_tensors] (device, incremented); ws f32 >= n_chunks + 2*n_tensors.
 * grad_scale: the gradient the optimizer sees is grads * grad_scale (clip norm included) --
 * data parallelism's 1/world applied here instead of a separate pass over the summed grads.
 */
int mmu_bertadam_step(float* params, const float* grads, float* m, float* v, void* bf16_copy,
                      const int64_t* table, int32_t* steps, int64_t n_tensors, int64_t n_chunks,
                      float lr_decay, float lr_nodecay, float wd, float warmup, float t_total,
                      float b1, float b2, float eps, float max_grad_norm, float grad_scale,
                      float* ws, int64_t ws_floats, mmu_stream_t stream);

/* ------------------------------------------------------------------ uncertainty
 * logits f32 [S, R, C] (R = members x passes per sample) ->
 * p_bar f32 [S, C] = mean_r softmax(logits[s, r]); per-sample nll [S] = -log p_bar[y];
 * conf [S], correct [S].  ECE is then binned from conf/correct (mmu_ece_bins).
 * North-star metrics; softmax-then-mean convention of
 * notebooks/food101_robustness.py:25-36.
 */
int mmu_uncertainty(const float* logits, const int64_t* y, int64_t S, int64_t R, int64_t C,
                    float* p_bar, float* nll, float* conf, float* correct, mmu_stream_t stream);
/* 15-style equal-width bins: out f32 [3*n_bins] = (count, sum conf, sum correct). */
int mmu_ece_bins(const float* conf, const float* correct, int64_t S, int64_t n_bins,
                 float* out, mmu_stream_t stream);

/* Entropy / mutual-information split of the K-member x T-pass prediction, per sample.
 * logits f32, element (s, k, t, c) at logits[s*ss + k*sk + t*st + c]: element strides, class axis
 * contiguous, so the [K, T, S, C] tensor of one batched ensemble forward (ss = C, st = S*C,
 * sk = T*S*C) is read in place, and [S, K, T, C] too.  1 <= C <= 1024.  y int64 [S].
 * With p_kt = softmax(logits[s, k, t, :]), p_k = mean_t p_kt, p = mean_k p_k and
 * H[q] = -sum_c q_c ln q_c (nats, 0 ln 0 = 0), stats f32 [S, MMU_UNC_NSTAT] holds the columns
 * below; p_bar f32 [S, C] = p; member_nll f32 [S, K] = -ln max(p_k[y], 1e-12), or NULL.
 * Mutual information = MI_MEMBERS + MI_PASSES.  Argmax ties go to the lowest class.
 * A stride below the extent it steps over (st < C, or sk / ss overlapping another axis; axes of
 * extent 1 never step and are not looked at) is refused.  y outside [0, C) is the caller's error.
 * No reference counterpart (the reference stops at the softmax mean, notebooks/utils.py:22-23). */
enum {
  MMU_UNC_TOTAL = 0,       /* H[p]                                                         */
  MMU_UNC_ALEATORIC = 1,   /* mean_{k,t} H[p_kt]                                           */
  MMU_UNC_MI_MEMBERS = 2,  /* H[p] - mean_k H[p_k]: between-member disagreement            */
  MMU_UNC_MI_PASSES = 3,   /* mean_k H[p_k] - aleatoric: within-member MC-dropout disagreement */
  MMU_UNC_BRIER = 4,       /* sum_c (p_c - 1[c == y])^2                                    */
  MMU_UNC_NLL = 5,         /* -ln max(p_y, 1e-12), the floor of mmu_uncertainty            */
  MMU_UNC_CONF = 6,        /* max_c p_c                                                    */
  MMU_UNC_CORRECT = 7,     /* 1[argmax_c p_c == y]                                         */
  MMU_UNC_VOTE_DISAGREEMENT = 8, /* 1 - (largest count of argmax_c p_kt over the K*T rows) / (K*T) */
  MMU_UNC_NSTAT = 9
};
int mmu_uncertainty_decompose(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y,
                              int64_t S, int64_t K, int64_t T, int64_t C, float* stats, float* p_bar,
                              float* member_nll, mmu_stream_t stream);

/* Temperature scaling of the ensemble (new symbols, ABI stays 4).  Inverse temperature beta = 1 / tau,
 * one per member: beta in R^K, beta_k >= 0 and finite.  For sample s with rows z_kt in R^C and label y:
 *   p_kt(beta) = softmax(beta_k z_kt)     p_k = mean_t p_kt     p(beta) = mean_k p_k
 *   nll_s(beta) = -ln max(p(beta)_y, 1e-12)                      (the floor of mmu_uncertainty)
 * A label outside [0, C) gives p_y = 0, so nll = -ln 1e-12 (class indices are compared with y, never
 * indexed by it, as in mmu_robustness_summary).  "Shared" temperature: all beta_k equal; "per-member":
 * beta a free K-vector; beta = 1 is the unscaled pipeline.
 *
 * mmu_uncertainty_decompose_scaled: the table of mmu_uncertainty_decompose with z_kt replaced by
 * beta_k z_kt (all nine columns, p_bar and member_nll); inv_temp device f32 [K], or NULL = all ones.
 * With inv_temp NULL or all ones its outputs are bitwise those of mmu_uncertainty_decompose on the
 * same input (NULL launches the very same kernel; 1 * z is z).  Refusals as mmu_uncertainty_decompose.
 *
 * mmu_temperature_nll: the NLL of J candidate vectors in one read of the logits, addressed exactly as
 * in mmu_uncertainty_decompose (element strides, class axis contiguous: [K, T, S, C] in place and
 * [S, K, T, C]).  inv_temp device f32 [J, K] (row j = candidate j); 1 <= C <= 1024, 1 <= J <= 64.
 *   nll f32 [S, J]:      nll[s, j] = nll_s(inv_temp[j, :])
 *   nll_sum f64 [J]:     sum_s nll[s, j], accumulated in f64 in one fixed order (a second small launch
 *                        on the same stream), or NULL
 * A row is loaded once and its max taken once (max(beta z) = beta max z for beta >= 0); expf / logf, no
 * atomics, every sum in one fixed order: bitwise repeatable in both determinism modes, and a
 * candidate's figures do not depend on the other candidates of the launch.  Refused before any
 * launch: null logits / y / inv_temp / nll, non-positive S / K / T / C / J, C > 1024, J > 64, and the
 * stride checks of mmu_uncertainty_decompose.  The CONTENTS of inv_temp (finite, >= 0) are device
 * memory and the caller's contract. */
int mmu_uncertainty_decompose_scaled(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y,
                                     int64_t S, int64_t K, int64_t T, int64_t C, float* stats, float* p_bar,
                                     float* member_nll, const float* inv_temp, mmu_stream_t stream);
int mmu_temperature_nll(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y, int64_t S,
                        int64_t K, int64_t T, int64_t C, const float* inv_temp, int64_t J, float* nll,
                        double* nll_sum, mmu_stream_t stream);

/* Modality-reliance summary of the robustness stack, per sample (the analysis the reference does in
 * notebooks/food101_robustness.py + notebooks/utils.py on the saved [S, 3 + 2n, C] predictions:
 * label probability per variant, experimental shift against the mean control shift, accuracy from
 * the argmax of the head-mean logits; restated here, and the Jensen-Shannon columns added).
 * logits f32, element (s, v, k, c) at logits[s*ss + v*sv + k*sk + c]: element strides, class axis
 * contiguous, so the [V, B, C] tensor robustness_logits holds before its final transpose (ss = C,
 * sv = B*C, K = 1) is read in place, and [S, V, K, C] too.  V = 3 + 2n variants, n >= 1, in the
 * stack's order: 0 full, 1 image-only, 2 text-only, 3 .. 3+n-1 image controls, 3+n .. 3+2n-1 text
 * controls.  K heads / members (1 for MMBT).  1 <= C <= 1024, 5 <= V <= 1023 odd.  y int64 [S].
 * With p_v = mean_k softmax(logits[s, v, k, :]), H[q] = -sum_c q_c ln q_c (nats, 0 ln 0 = 0):
 *   p_label[v] = p_v[y]
 *   hit[v]     = 1[argmax_c mean_k logits[s, v, k, c] == y]   (the LOGITS' head mean; ties -> lowest class)
 *   js[v]      = H[(p_v + p_0) / 2] - (H[p_v] + H[p_0]) / 2   (Jensen-Shannon divergence from the full
 *                forward, in [0, ln 2]; the label-free companion of p_label[v] - p_label[0])
 * A label outside [0, C) gives p_label = 0 and hit = 0 (class indices are compared with y, never
 * indexed by it).  stats f32 [S, MMU_ROB_NSTAT] holds the columns below; per_variant f32 [S, 3, V]
 * = (p_label, js, hit), or NULL.  Strides are checked as in mmu_uncertainty_decompose.  One launch,
 * no atomics, every sum in one fixed order: bitwise repeatable in both determinism modes. */
enum {
  MMU_ROB_P_FULL = 0,            /* p_label[0]                                                  */
  MMU_ROB_DP_IMAGE = 1,          /* p_label[1] - p_label[0]                                     */
  MMU_ROB_DP_IMAGE_CONTROL = 2,  /* mean_i (p_label[3+i] - p_label[0]), i < n                   */
  MMU_ROB_SD_IMAGE_CONTROL = 3,  /* population std (ddof 0) of those n differences              */
  MMU_ROB_DP_TEXT = 4,           /* p_label[2] - p_label[0]                                     */
  MMU_ROB_DP_TEXT_CONTROL = 5,   /* mean_i (p_label[3+n+i] - p_label[0])                        */
  MMU_ROB_SD_TEXT_CONTROL = 6,   /* population std of those n differences                       */
  MMU_ROB_JS_IMAGE = 7,          /* js[1]                                                       */
  MMU_ROB_JS_IMAGE_CONTROL = 8,  /* mean_i js[3+i]                                              */
  MMU_ROB_JS_TEXT = 9,           /* js[2]                                                       */
  MMU_ROB_JS_TEXT_CONTROL = 10,  /* mean_i js[3+n+i]                                            */
  MMU_ROB_HIT_FULL = 11,         /* hit[0]                                                      */
  MMU_ROB_HIT_IMAGE = 12,        /* hit[1]                                                      */
  MMU_ROB_HIT_TEXT = 13,         /* hit[2]                                                      */
  MMU_ROB_ACC_IMAGE_CONTROL = 14,/* mean_i hit[3+i]                                             */
  MMU_ROB_ACC_TEXT_CONTROL = 15, /* mean_i hit[3+n+i]                                           */
  MMU_ROB_NSTAT = 16
};
int mmu_robustness_summary(const float* logits, int64_t ss, int64_t sv, int64_t sk, const int64_t* y,
                           int64_t S, int64_t V, int64_t K, int64_t C, float* stats, float* per_variant,
                           mmu_stream_t stream);

/* Ensemble diversity, per sample (new symbol, ABI stays 4): which members disagree with which, and by
 * how much.  The reference's "Prediction Diversity Analysis" (notebooks/analysis_round_1.py:68-113:
 * mute the true class, keep each sub-network's top-5 probabilities, Kendall tau between two
 * sub-networks), restated per sample; js and disagree have no counterpart.
 * logits and y as in mmu_uncertainty_decompose: f32, element (s, k, t, c) at
 * logits[s*ss + k*sk + t*st + c], class axis contiguous, [K, T, S, C] in place and [S, K, T, C];
 * y int64 [S].  2 <= K <= 16 members, 1 <= C <= 1024, 0 <= top <= 1024, mute_true 0 / 1.
 * With p_k = mean_t softmax(logits[s, k, t, :]) and H[q] = -sum_c q_c ln q_c (nats, 0 ln 0 = 0):
 *   member_arg int32 [S, K] = argmax_c p_k[c], ties to the lowest class.
 * For each pair (i, j), i < j, in itertools.combinations order, P = K (K - 1) / 2 of them,
 * pair f32 [S, P, MMU_DIV_NPAIR] holds
 *   js       = H[(p_i + p_j) / 2] - (H[p_i] + H[p_j]) / 2        (the form of mmu_robustness_summary)
 *   disagree = 1[member_arg_i != member_arg_j]
 *   tau      = Kendall tau-b between the truncated vectors x_i and x_j over the C classes.
 * Truncation (the reference's trunk_pred_top, its quirk included): m = min(top, C); thr_k is the m-th
 * largest value of p_k over all C classes, counted with multiplicity and with the TRUE CLASS INCLUDED
 * (the threshold comes from the unmuted row); x_k[c] = p_k[c] if p_k[c] >= thr_k, else 0; then, if
 * mute_true and 0 <= y < C, x_k[y] = 0.  top = 0: no truncation, every class is kept.  Ties at the
 * threshold keep every tied class, so more than top classes can be kept (equal logits: all C).
 * Kendall tau-b over the n0 = C (C - 1) / 2 class pairs a < b, with sx = sign(x_i[a] - x_i[b]) and
 * sy = sign(x_j[a] - x_j[b]):
 *   conc = #(sx sy > 0)   disc = #(sx sy < 0)   tx = #(sx = 0)   ty = #(sy = 0)
 *   tau = (conc - disc) / sqrt((n0 - tx) (n0 - ty)), the quotient formed in f64 and stored as f32;
 *   NaN when the denominator is 0 (C = 1, or a constant x).  This is scipy.stats.kendalltau's tau-b.
 * counts int32 [S, P, 4] = (conc, disc, tx, ty), or NULL; each at most 523,776, so exact.
 * The reference pools all S x C values of two sub-networks into one tau, which mixes the ordering
 * between samples with the ordering within one; here tau is per sample (average it over the samples
 * where it is defined).  For one sample the two coincide.
 * A label outside [0, C) mutes nothing (class indices are compared with y, never indexed by it).
 * One launch, expf / logf, no atomics, every sum in one fixed order: bitwise repeatable in both
 * determinism modes.  Refused before any launch: null logits / y / pair / member_arg, non-positive
 * S / T / C, C > 1024, K < 2, K > 16, top < 0, top > 1024, mute_true not 0 / 1, S over the grid limit
 * and the stride checks of mmu_uncertainty_decompose. */
enum {
  MMU_DIV_JS = 0,
  MMU_DIV_DISAGREE = 1,
  MMU_DIV_TAU = 2,
  MMU_DIV_NPAIR = 3
};
int mmu_ensemble_diversity(const float* logits, int64_t ss, int64_t sk, int64_t st, const int64_t* y,
                           int64_t S, int64_t K, int64_t T, int64_t C, int64_t top, int mute_true,
                           float* pair /* [S, P, MMU_DIV_NPAIR] */, int32_t* counts /* [S, P, 4] or NULL */,
                           int32_t* member_arg /* [S, K] */, mmu_stream_t stream);

/* Exact rank table over J score columns (new symbol, ABI stays 4): the integers every ranking metric
 * is a function of -- the AUC table and the epoch-ensemble AUC of the reference's
 * notebooks/hatefulmeme_robustness.py (AUC_table, ensemble_overtime), the AUROC of an uncertainty score
 * and its risk-coverage area.  The host forms each figure in fp64 from them (src/ranking.py), so a
 * result depends on the scores alone, not on summation order, launch shape or determinism mode.
 * Score (s, j) is x[s*ss + j*sj], f32, element strides: a contiguous [S, J] table and a [J, S] table
 * are both read in place.  group uint8 [S], contiguous: non-zero marks group 1 (the positives, or the
 * wrong samples), zero group 0.
 * rank int32 [J, S, MMU_RANK_NRANK], or NULL: for column j and sample i, comparing as IEEE f32,
 *   lt_g = #{i' in group g : x[i', j] <  x[i, j]}
 *   eq_g = #{i' in group g : x[i', j] == x[i, j]}, sample i itself included.
 * So -0 ties +0, +-inf are ordinary values, subnormals are distinct values (nothing is flushed), and a
 * NaN sample has all four counts 0 and is counted by nobody.
 * counts int64 [J, MMU_RANK_NCOUNT]: nan = the NaN scores of the column; n1, n0 = the non-NaN samples
 * per group; gt = sum over group 1 of lt_0 (the (positive, negative) pairs with the positive strictly
 * higher); eq = sum over group 1 of eq_0.  AUROC = (gt + eq / 2) / (n1 n0).
 * A count is at most S, a count sum at most S^2.  Every output element is written.
 * One sweep of S^2 compares per column: blocks of MMU_RANK_BLOCK_ROWS samples, the column streamed
 * through LDS in tiles of MMU_RANK_TILE candidates.  Refused before any launch: null x / group /
 * counts; non-positive S / J; S > 2^20 (the sweep is O(S^2) per column); J > 65535; a stride <= 0 on an
 * axis of extent > 1; overlapping axes (the larger stride must clear extent x the smaller); x or rank
 * not 4-byte aligned, counts not 8-byte aligned. */
enum { MMU_RANK_LT0 = 0, MMU_RANK_EQ0 = 1, MMU_RANK_LT1 = 2, MMU_RANK_EQ1 = 3, MMU_RANK_NRANK = 4 };
enum { MMU_RANK_N1 = 0, MMU_RANK_N0 = 1, MMU_RANK_GT = 2, MMU_RANK_EQ = 3, MMU_RANK_NAN = 4, MMU_RANK_NCOUNT = 5 };
enum { MMU_RANK_BLOCK_ROWS = 1024, MMU_RANK_TILE = 1024, MMU_RANK_MAX_S = 1 << 20, MMU_RANK_MAX_J = 65535 };
int mmu_rank_table(const float* x, int64_t ss, int64_t sj, const uint8_t* group, int64_t S, int64_t J,
                   int32_t* rank /* [J, S, 4] or NULL */, int64_t* counts /* [J, 5] */, mmu_stream_t stream);

/* ------------------------------------------------------------------ launch plans
 * What the host would decide for a product -- tiling, tile order, split-K, the split tail rows, the
 * column-sum path, the BatchNorm row blocks -- without launching it.  Each query runs the very
 * function the launch runs (csrc/plan.h; bn_grid of csrc/batchnorm.hip), makes no HIP call and
 * works without a GPU; a shape the launch would refuse is refused here with the same message
 * (mmu_last_error).  `plan` receives MMU_*_PLAN_FIELDS int64 values in the order listed.
 *
 * mmu_gemm_plan: the plan of mmu_gemm / mmu_gemm_rows for this shape, under the MMU_GEMM_*
 * environment knobs and the deterministic switch as they stand at the call, with both per-stream
 * scratch slots assumed available (a launch that cannot have one -- first use under stream capture,
 * a failed allocation -- drops the tail split / falls back to atomics).  has_bias / has_colsum: the
 * epilogue's bias / colsum pointers are given; workspace_floats: its split-K workspace (0: none).
 *    0 tiling      0 = 128 x 128, 1 = 256 x 256, 2 = 256 x 384
 *    1 tiles_m     2 tiles_n     tiles of the whole product in that tiling
 *    3 group_m     tile-order group height
 *    4 splitk      5 kchunk      K slices and their depth (1, K: unsplit)
 *    6 m_main      7 tail_rows   rows [m_main, M) are the split tail rows (M, 0: none); the main
 *                                tiling then runs m_main / 256 tile rows
 *    8 tail_split  9 tail_chunk  their K slices and depth (1, K: none)
 *   10 cs          column sums: 0 = none, 1 = float atomics, 2 = partial rows, 3 = the float2 table
 *   11 cs_rows    12 cs_parts    partial rows: rows per part on the main tiling (64 on the tail
 *                                rows), and the parts in all
 * mmu_conv_implicit_plan (mmu_conv_implicit[_stats], mmu_conv3x3_implicit[_bnb]):
 *    0 small (1 = the 128 x 128 kernel, 0 = 256 x 256)   1 M = n Ho Wo   2 K = ksize^2 C   3 Ho   4 Wo
 *    5 tiles_m   6 tiles_n   7 splitk   8 kchunk
 * mmu_conv_wgrad_plan (mmu_conv_wgrad, mmu_conv3x3_wgrad):
 *    0 K = n Ho Wo   1 Ho   2 Wo   3 tiles_m   4 tiles_n   5 few (1: <= 4 output tiles)   6 splitk   7 kchunk
 * mmu_batchnorm_plan (the row-block grid of every mmu_batchnorm_* reduction and apply pass):
 *    0 CH (channels per block)   1 rpi (rows per block iteration)   2 rpb (rows per block)
 *    3 blocks (grid.x = block partials per channel)   4 gy (grid.y = C / CH)
 *    5 clamped (1: rpb was raised so that blocks x C partial pairs fit the scratch)
 */
#define MMU_GEMM_PLAN_FIELDS 13
#define MMU_CONV_IMPLICIT_PLAN_FIELDS 9
#define MMU_CONV_WGRAD_PLAN_FIELDS 8
#define MMU_BATCHNORM_PLAN_FIELDS 6
int mmu_gemm_plan(int64_t M, int64_t N, int64_t K, int64_t batch, int64_t lda, int64_t ldb, int a_kmajor,
                  int b_kmajor, int c_dtype, int kind, int has_bias, int has_colsum, int64_t workspace_floats,
                  int64_t* plan);
int mmu_conv_implicit_plan(int64_t n_img, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ksize,
                           int64_t stride, int64_t ws_floats, int64_t* plan);
int mmu_conv_wgrad_plan(int64_t n_img, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t ksize,
                        int64_t stride, int64_t ws_floats, int64_t* plan);
int mmu_batchnorm_plan(int64_t rows, int64_t C, int64_t* plan);

/* ------------------------------------------------------------------ timing
 * Device-time of every mmu_gemm launch while enabled, bracketed by HIP events on
 * the launch stream (bench.py roofline).  Reads back (host sync) only in _read.
 */
int mmu_timing_enable(int on);
/* paused != 0: launches are not recorded (already recorded ones are kept) -- the
 * ResNet 1x1-conv products run through mmu_gemm but are not BERT-layer GEMMs. */
int mmu_timing_pause(int paused);
int mmu_timing_read(double* total_ms, int64_t* launches, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* MMU_H */
