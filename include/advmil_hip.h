/* C ABI of libadvmil_hip.so — the MI355X (gfx950) kernels underneath the AdvMIL plugin surface.
 *
 * The reference (liupei101/AdvMIL @ v1) is pure Python/PyTorch and has no FFI: its "operator
 * interface" for the generator+discriminator training path is the set of nn.Module forwards in
 * model/backbone.py, model/backbone_utils.py, model/GANSurv.py, model/model_utils.py and the loss
 * functions in loss/utils.py. Each entry point below names the reference code it replaces
 * (file:line into /root/reference). The Python host side (advmil_amd/) binds these with ctypes
 * and mirrors the reference's class names / ctor + forward signatures / state_dict keys.
 *
 * Conventions
 *  - all pointers are DEVICE pointers borrowed for the duration of the enqueue; row-major,
 *    contiguous unless a leading dimension is given; 16-byte aligned; fp32 unless noted.
 *  - every call is asynchronous on `stream` (a hipStream_t), never allocates, never syncs; it is
 *    safe under hipStreamBeginCapture (HIP graphs).
 *  - return value: 0 = ok, <0 = ADVMIL_E* (bad argument), >0 = hipError_t of the launch.
 *  - randomness (dropout, generator noise) is counter based: u = top 24 bits of hash32(key(seed, stream_id),
 *    element_index), key = splitmix64 mix of seed and stream id, hash32 = a two-round 32-bit multiply-xorshift
 *    mixer (csrc/common.h::rng_hash32); `seed` is a DEVICE pointer to a uint64 so a captured graph can be
 *    replayed with a fresh seed; `stream_id` distinguishes call sites. NULL seed or p == 0
 *    disables dropout. advmil_amd/synth.py restates the generator on the host.
 */
#ifndef ADVMIL_HIP_H
#define ADVMIL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* advmil_stream_t; /* hipStream_t */

enum { ADVMIL_ACT_NONE = 0, ADVMIL_ACT_RELU = 1, ADVMIL_ACT_TANH = 2, ADVMIL_ACT_SIGMOID = 3 };

int advmil_version(void);

/* ------------------------------------------------------------------------------------------
 * Dense contraction engine (fp32 MFMA v_mfma_f32_32x32x2_f32, exact fp32 accumulate).
 *   C[M,N] = epilogue( alpha * op(A)[M,K] . op(B)[K,N] )
 *   a_kc != 0 : A is [M,K] row-major (k contiguous, lda = row pitch); else A is [K,M] (m contiguous)
 *   b_kc != 0 : B is [N,K] row-major (a torch Linear weight);         else B is [K,N] (n contiguous)
 * replaces: nn.Linear / Conv2d(1x1) forwards (model/backbone.py:69,72-75,98,102;
 *   model/backbone_utils.py:16-17,35-44,150; model/model_utils.py:157-176) and the
 *   addmm/mm calls autograd issues for their backward.
 * epilogue, applied in this order per element (row m, col n):
 *   v = alpha*acc (+ bias[n]) (+ rowv[m]*colv[rowseg[m]*N + n]); v = act(v)  [act0 for n < act_split, else act1];
 *   v *= dropout(m*N+n); v *= (maskref[m*ldmask+n] > 0 ? mask_scale : 0) if maskref;
 *   C = v (+ C if accumulate).
 * splits > 1 partitions K across workgroups (needed when M*N is small and K is the bag length);
 * partials go to `ws` (advmil_gemm_f32_workspace_bytes) and a second launch reduces them.
 * Requirements: contiguous dims and leading dims multiples of 4 floats. */
typedef struct {
  const float* bias;
  int act0, act1, act_split;
  float drop_p;
  const uint64_t* seed;
  uint64_t stream_id;
  const float* rowv;
  const float* colv;
  const int32_t* rowseg; /* NULL, or the segment (bag) of each row: the rank-1 term reads colv[rowseg[m]*N + n] */
  const float* maskref;
  int ldmask;
  float mask_scale;
  int accumulate;    /* C += v. With splits > 1 (and advmil_merge_partials): while the launch stream is in DEFERRAL (advmil_defer_sums below -- opt-in
                      * per stream, never on by default) the `C += partials` fold is queued until the flush, so C must not be read or written by
                      * another launch before advmil_flush_sums / advmil_defer_sums(stream, 0); outside deferral the fold is issued at once. */
  float alpha;
  /* bf16x3 operand planes (all optional, ignored in exact mode). An fp32 matrix x can be accompanied by two bf16 matrices
   * hi = bf16(x), lo = bf16(x - hi) of the SAME shape and leading dimension (advmil_split_planes; the Adam kernel emits them
   * for the weights; c_hi/c_lo below for activations). When both planes of an operand are given (16-byte aligned, leading
   * dimension and contiguous extent multiples of 8) the engine stages them straight into LDS instead of re-splitting the fp32
   * values in every workgroup that re-reads them -- results are bit-identical to the on-the-fly split.
   * SINGLE-plane operand: a_hi (or b_hi) given with a_lo (b_lo) = NULL says the operand IS a bf16 matrix (a bag stored in bf16: the
   * x_storage = "bf16" mode of the ingest; the A / B pointer then only carries the pitch and is never dereferenced). Its products
   * are formed with two MFMAs instead of three -- built for A of the NT plane-fed forms (the embedding FCs over the slab) and B of
   * the TN plane-fed forms (the weight gradients dY^T X); the generic tiles 22 / 12 / 11 / 34 / 24 stage a zero lo plane. */
  const void* a_hi;
  const void* a_lo;
  const void* b_hi;
  const void* b_lo;
  void* c_hi; /* also write the planes of the final C values (pitch ldc) for the next contraction; with C == NULL in advmil_gemm_f32_tiled
               * (one pass, no accumulate, no second layer) the planes are written INSTEAD of C: a result consumed as an operand only */
  void* c_lo;
  /* Fused gate score (Attn_Net_Gated without its [rows, 2D] activations, model/backbone_utils.py:24-28; used by the no-grad
   * generator pass of the discriminator update, model_handler.py:398-400): B's rows are the two branches INTERLEAVED (row 2j = Wa_j,
   * row 2j+1 = Wb_j; bias likewise). Instead of C the launch writes, per row and per column block of the tile grid,
   * gate_out[m*gate_np + block] = sum_j tanh(c[2j]) * sigmoid(c[2j+1]) * gate_wc[j]; the score is the sum over blocks (+ bc).
   * gate_np = number of column blocks = n-tiles * waves along N (advmil_gemm_f32_gate_blocks). C may be NULL. No dropout, splits = 1. */
  const float* gate_wc;
  float* gate_out;
  int gate_np;
  /* Optional [M] device array: row m draws its dropout as row rng_row[m] (element index rng_row[m]*N + n). Under bag-parallel a
   * rank passes the rows its bags occupy in the single-process step slab, which makes the masks independent of the world size;
   * NULL = identity. The same optional argument exists on every entry point below that draws dropout / noise. */
  const int64_t* rng_row;
  /* Two layers over the same rows in one launch (plane-fed NT form, tile 85 only): B holds both layers' weight rows stacked
   * ([N, K]: layer 1 first); columns [0, n_split) of the product are layer 1 -- bias, output C (pitch ldc), planes c_hi/c_lo --,
   * columns [n_split, N) are layer 2 -- bias2[n - n_split], output c2[m*ldc2 + n - n_split], no planes. act_split = n_split selects
   * the two activations. n_split % 32 == 0; C, c2 and bias 16-byte aligned, ldc % 4 == 0 and ldc2 % 4 == 0, c_hi / c_lo 8-byte aligned
   * (ADVMIL_EINVAL otherwise: only the streaming epilogue routes layer 2); c2 = NULL = an ordinary launch. The generator's and the discriminator's first layers
   * over the step slab read X once this way (model/backbone.py:60-66 + model/model_utils.py:130-140). */
  float* c2;
  int64_t ldc2;
  int64_t n_split;
  const float* bias2;
  /* Column sums of the FINAL values, one partial row per (row tile, wave row) of the launch: colsum[p * N + n], p < advmil_gemm_f32_colsum_rows
   * (slab-sized bf16x3 tiles, whole tiles, splits = 1, no accumulate / dropout). With rowv + maskref in the same launch (rank-1 term, then
   * the mask) this is the fused backward of the first layer behind the gated-attention pool: dpre = (dG Wab + A dpooled) * (y > 0 ?
   * mask_scale : 0) and its bias gradient, instead of a separate pass over dh and y (model/backbone.py:79-86 autograd of ReLU + Dropout). */
  float* colsum;
  /* The mask as one bit per element instead of maskref: maskbits[m * ldbits + n / 32] bit n % 32 set = keep (x mask_scale), clear = 0
   * (advmil_act_dropout_bwd's `bits` output). Whole-tile launches of the slab-sized bf16x3 tiles only; may be combined with rowv. The
   * epilogue parks a wave's words in LDS before its first store: no per-element mask load inside the store loop. */
  const uint32_t* maskbits;
  int64_t ldbits;
  /* TRAINING form of the fused gate score (tiles 85 / 86, plain launches): gate_wc / gate_out / gate_np as above, but B's rows are the two
   * branches in BLOCKS of 32 (advmil_gate_interleave with pair32 = 1: [a_0..31 | b_0..31 | a_32..63 | ...]) and C IS written -- tanh on the
   * a blocks, sigmoid on the b blocks, in that blocked column order (advmil_gate_bwd with pair32 = 1 reads it back) --, while the row's
   * sum_j (a_j ka_j)(b_j kb_j) gate_wc[j] over each column block is reduced on the way into gate_out. ka / kb = drop_p-dropout keep
   * factors given as bits: gate_bits_a / gate_bits_b [M, ldgbits] uint32, bit j % 32 of word (m, j / 32) (advmil_dropout_planes draws them).
   * Attn_Net_Gated in train mode (model/backbone_utils.py:24-29) without a pass over its stored activations. */
  const uint32_t* gate_bits_a;
  const uint32_t* gate_bits_b;
  int64_t ldgbits;
  /* The M rows of this launch's result are in that pair-block order (dWab = dG^T h with dG from advmil_gate_bwd(pair32 = 1)) while C holds
   * [branch][unit] rows: accumulating split-K launches only (splits > 1, accumulate, no other epilogue term) -- the merge un-permutes. */
  int c_rows_pair32;
} advmil_epilogue_t;

size_t advmil_gemm_f32_workspace_bytes(int64_t M, int64_t N, int splits);
int advmil_gemm_f32(int a_kc, int b_kc, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                    const float* B, int64_t ldb, float* C, int64_t ldc, const advmil_epilogue_t* epi,
                    int splits, void* ws, size_t ws_bytes, advmil_stream_t stream);
/* Arithmetic of the fp32 engine (process-wide): 0 = exact fp32 MFMA; 1 = split-bf16 ("bf16x3"): every fp32 operand is
 * split into hi + lo bf16 in registers and a.b is formed as ah.bh + ah.bl + al.bh on the bf16 matrix pipe with fp32
 * accumulate -- dropped terms ~2^-17 |a||b| per product, 3/16 of the matrix-pipe time. Storage stays fp32 everywhere. */
/* lo may be NULL: only hi = bf16(x) is written (the rounding a bag undergoes on its way into a bf16 slab). */
int advmil_split_planes(const float* src, int64_t n, void* hi, void* lo, advmil_stream_t stream);
/* Glue of the fused gate score (epilogue.gate_wc): Wi[2D, D] = rows a0, b0, a1, b1, ... of the attention branches' weights Wa, Wb [D, D]
 * (reference model/backbone_utils.py Attn_Net_Gated: attention_a / attention_b), its planes (Wi_hi / Wi_lo, both or neither) and the
 * interleaved bias bi[2D]; and s[n] = sum_j partial[n][j] + bc[0] over the np per-column-block partials the epilogue wrote (bc may be NULL). */
int advmil_gate_interleave(const float* Wa, const float* Wb, const float* ba, const float* bb, int D, float* Wi, void* Wi_hi, void* Wi_lo,
                           float* bi, int pair32, advmil_stream_t stream);
int advmil_gate_partial_sum(const float* partial, int np, const float* bc, int64_t N, float* s, advmil_stream_t stream);
/* column blocks a launch with this tile writes per row in gate-score mode (see advmil_epilogue_t.gate_wc) */
int advmil_gemm_f32_gate_blocks(int tile, int64_t N);
/* partial rows a launch with this tile writes into epilogue.colsum for an M x N result (0: no column-sum form for this tile / these extents) */
int64_t advmil_gemm_f32_colsum_rows(int tile, int64_t M, int64_t N);
/* out[c] (+)= sum_{b < nblk} partial[b * stride + c], c < ncols: the merge of per-workgroup partial rows (deferrable: advmil_defer_sums) */
int advmil_merge_partials(const float* partial, int nblk, int64_t stride, int64_t ncols, float* out, int accumulate, advmil_stream_t stream);
int advmil_set_gemm_mode(int mode);
int advmil_get_gemm_mode(void);
/* The library's launch plan for a shape: block tile (see below) and K split count. Host callers size the workspace
 * from `splits` (advmil_gemm_f32_workspace_bytes) and pass both to advmil_gemm_f32_tiled. */
int advmil_gemm_f32_plan(int64_t M, int64_t N, int64_t K, int* tile, int* splits);
/* Same, knowing the operand layouts (the best tile differs between the NT forward form and the NN / TN backward forms; this is what
 * advmil_gemm_f32 itself uses). advmil_gemm_f32_plan is the a_kc = b_kc = 1 case. */
int advmil_gemm_f32_plan_layout(int a_kc, int b_kc, int64_t M, int64_t N, int64_t K, int* tile, int* splits);
/* bf16x3 mode, NT form (a_kc = b_kc = 1) with BOTH operands supplied as planes (a_hi..b_lo): the tile of the plane-fed kernel that
 * stages global -> LDS by LDS-DMA as a persistent kernel (82 / 83 = 256 x 128 / 192, 8 waves, one workgroup per CU walking the
 * tiles; M % 256 == 0, K % 32 == 0 and K >= 64, N % tile width == 0, planes < 4 GB each, splits = 1), or 0 when the shape does not
 * qualify. advmil_gemm_f32_tiled(tile = 0) makes the same choice; callers of the fused gate-score mode need the tile up front for
 * advmil_gemm_f32_gate_blocks and may pass 84 (256 x 256, instantiated for that mode only) when N % 256 == 0. Results are
 * bit-identical to the generic kernel's. */
int advmil_gemm_f32_plan_planes(int a_kc, int b_kc, int64_t M, int64_t N, int64_t K, int* tile);
/* TN form (A [K, M], B [K, N], both m-contiguous) with BOTH operands as planes -- the deep-K weight gradients dW = dY^T X over a
 * step slab (torch's addmm backward of nn.Linear / the 1x1 Conv, reference model/backbone.py:60-66, backbone_utils.py:158-168):
 * tile code (91 / 92 / 93 = 128x256 / 256x128 / 256x256, LDS-DMA fed split-K kernel) and split count to pass to
 * advmil_gemm_f32_tiled, or *tile = 0 when the shape does not qualify (then the ordinary plan applies). */
int advmil_gemm_f32_plan_tn_planes(int64_t M, int64_t N, int64_t K, int* tile, int* splits);
/* Same, with an explicit block tile: tile = 10*TM + TN selects (64*TM) x (64*TN) output tiles
 * (22 = 128x128, 23 = 128x192, 13 = 64x192, 12 = 64x128, 11 = 64x64; 43 = 256x192, 42 = 256x128, 34 = 192x256, 24 = 128x256 with 512 threads,
 * bf16x3 mode only -- in exact mode they fall back to 23 / 22); 0 = the plan's choice (what advmil_gemm_f32 uses). */
int advmil_gemm_f32_tiled(int a_kc, int b_kc, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                          const float* B, int64_t ldb, float* C, int64_t ldc, const advmil_epilogue_t* epi,
                          int splits, int tile, void* ws, size_t ws_bytes, advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused self-attention core of the ESAT layer (nn.MultiheadAttention inside nn.TransformerEncoderLayer,
 * model/backbone_utils.py:113-127, reached from DualTrans_HS.forward, model/backbone.py:188-196; the reference runs one
 * call per bag, model_handler.py:352, batch_size 1):  O = dropout(softmax(Q K^T / sqrt(head_dim))) V  per (bag, head).
 * Flash-style: the [L, L] scores never exist in HBM; the backward recomputes them from `lse`.
 *   qkv_hi / qkv_lo  [Ltot, 3*nhead*head_dim] bf16: the two bf16x3 operand planes (hi = bf16(x), lo = bf16(x - hi)) of the packed
 *        in-projection output (q | k | v; head h of q at columns h*head_dim ...), as advmil_split_planes or a contraction's
 *        c_hi / c_lo plane output produce them; 16-byte aligned, row pitch 3*nhead*head_dim. The kernels stream them into LDS by
 *        LDS-DMA and never see the fp32 values.
 *   out  [Ltot, nhead*head_dim];  lse [Ltot, nhead] = log2-domain log-sum-exp of the scaled scores (opaque to the caller)
 *   Rows are a slab of `nseg` bags, bag b = rows [ptr[b], ptr[b+1]) (device int64; NULL = one bag), longest bag <= max_len <= Ltot
 *   (a cap: it sizes the grids, and workgroups beyond a bag's own tiles return; advmil_mha_bwd1 refuses nseg > 65535);
 *   attention never crosses a bag. Any bag length >= 1 (ragged tails are masked). head_dim in {16, 32, 48, 64}: d_model / 8 heads
 *   of the bcb_dims load_backbone accepts (model/backbone.py:30-33; 384 -> 48 in the shipped config).
 * Dropout on the probabilities (train mode; NULL seed or p == 0 = off): one 32-bit hash per (query, 4 consecutive keys),
 *   keep(i, j) = byte (j & 3) of mix(rowkey + (j >> 2)*0x9E3779B9) >= floor(p*256),  mix(x): x ^= x >> 15; x *= 0x7feb352d; x ^= x >> 15
 *   (p quantised to 1/256 -- 0.25 is exact --, kept probabilities scaled by 256 / (256 - floor(256 p))),
 *   rowkey = high 32 bits of splitmix64(key(seed, stream_id) + (ptr[b] + rng_rowoff[b] + i)*nhead + h); rng_rowoff (device int64
 *   [nseg], NULL = zeros) lets a rank of a bag-parallel job address the row ids the single-process run would use.
 *   Host restatement: advmil_amd/synth.py::attn_dropout_keep.
 * Arithmetic: split-bf16 ("bf16x3": hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16, fp32 accumulate) in BOTH modes of
 *   advmil_set_gemm_mode -- ~2^-17 relative per product; softmax statistics and exponentials in fp32.
 * bwd: out / dout fp32 [Ltot, nhead*head_dim]; dqkv [Ltot, 3*nhead*head_dim] fp32 (every element written);
 *   ws >= advmil_mha_bwd_workspace_bytes (holds D = rowsum(dO * O) and the operand planes of dO). Deterministic (no atomics). */
int advmil_mha_fwd(const void* qkv_hi, const void* qkv_lo, int64_t Ltot, int nhead, int head_dim, int nseg, const int64_t* ptr,
                   int64_t max_len, float drop_p, const uint64_t* seed, uint64_t stream_id, const int64_t* rng_rowoff, float* out,
                   float* lse, advmil_stream_t stream);
/* The same forward with the log-sum-exp GIVEN (`lse` is read): the train-mode pass of an optimizer step behind the eval-mode pass over
 * the same q | k | v (the reference runs the generator twice per step with unchanged weights, model_handler.py:398-425; the softmax
 * statistics of the two passes are identical, only the dropout draw is new). Probabilities are exp2(s c - lse) directly: no running
 * maximum, no rescaling, no row sum. Dropout must be on (seed != NULL, drop_p > 0); same mask stream as advmil_mha_fwd. */
int advmil_mha_fwd_lse(const void* qkv_hi, const void* qkv_lo, int64_t Ltot, int nhead, int head_dim, int nseg, const int64_t* ptr,
                       int64_t max_len, float drop_p, const uint64_t* seed, uint64_t stream_id, const int64_t* rng_rowoff, float* out,
                       const float* lse, advmil_stream_t stream);
size_t advmil_mha_bwd_workspace_bytes(int64_t Ltot, int nhead, int head_dim);
int advmil_mha_bwd(const void* qkv_hi, const void* qkv_lo, const float* out, const float* dout, const float* lse, int64_t Ltot,
                   int nhead, int head_dim, int nseg, const int64_t* ptr, int64_t max_len, float drop_p, const uint64_t* seed,
                   uint64_t stream_id, const int64_t* rng_rowoff, float* dqkv, void* ws, size_t ws_bytes, advmil_stream_t stream);
/* The same backward in ONE pass over the scores (csrc/attn_bwd1.hip; round 6): keys stationary, dK / dV as above, and dQ from the
 * same score tiles -- dS goes through LDS once, each 256-key block leaves an unscaled partial slab [Ltot, nhead*head_dim] in the
 * workspace, and a reduce launch sums the blocks of a bag in block order into the q columns of dqkv. Five contractions instead of the
 * seven of advmil_mha_bwd (which recomputes S and dP for dQ), same arguments, same dropout stream, deterministic (no atomics); results
 * differ from advmil_mha_bwd's only in the summation order of dQ. ws >= advmil_mha_bwd1_workspace_bytes (D, the planes of dO and
 * ceil(max_len / 256) partial slabs). */
size_t advmil_mha_bwd1_workspace_bytes(int64_t Ltot, int nhead, int head_dim, int64_t max_len);
int advmil_mha_bwd1(const void* qkv_hi, const void* qkv_lo, const float* out, const float* dout, const float* lse, int64_t Ltot,
                    int nhead, int head_dim, int nseg, const int64_t* ptr, int64_t max_len, float drop_p, const uint64_t* seed,
                    uint64_t stream_id, const int64_t* rng_rowoff, float* dqkv, void* ws, size_t ws_bytes, advmil_stream_t stream);
/* Post-norm residual of the same layer (norm_first = False):  y = LayerNorm(x + dropout(o)) over rows of width d <= 512.
 * fwd also writes z = x + dropout(o), mean[R], rstd[R] for the backward; dropout element index = row*d + col on `stream_id`.
 * bwd: dx = LayerNorm'(dy); dob (may be NULL) = dx * keep; dgamma / dbeta = column sums (accumulate != 0 adds into them).
 * ws >= advmil_add_dropout_ln_bwd_workspace_bytes. */
/* y_hi / y_lo (both or neither): also the bf16x3 operand planes of y, for the plane-fed contraction that reads it next. */
int advmil_add_dropout_ln_fwd(const float* x, const float* o, const float* gamma, const float* beta, float eps, int64_t R,
                              int64_t d, float drop_p, const uint64_t* seed, uint64_t stream_id, const int64_t* rng_row, float* z,
                              float* y, float* mean, float* rstd, void* y_hi, void* y_lo, advmil_stream_t stream);
size_t advmil_add_dropout_ln_bwd_workspace_bytes(int64_t R, int64_t d);
int advmil_add_dropout_ln_bwd(const float* dy, const float* z, const float* gamma, const float* mean, const float* rstd, int64_t R,
                              int64_t d, float drop_p, const uint64_t* seed, uint64_t stream_id, const int64_t* rng_row, float* dx,
                              float* dob, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes,
                              advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gated-attention MIL pooling (Attn_Net_Gated + softmax + mm: model/backbone_utils.py:11-29,
 * model/backbone.py:81-85, 118-122, 163-167; GAPool: model/backbone_utils.py:47-56).
 *
 * gate_score: ab[N,2D] holds tanh-branch a (cols 0..D-1) and sigmoid-branch b (cols D..2D-1),
 *   post-activation, PRE-dropout. s[n] = sum_j (a*ka)(b*kb) wc[j] + bc[0], ka/kb the dropout
 *   factors (stream_a/stream_b, element index n*D+j).
 * softmax_pool_fwd: A = softmax(s) over the N instances; pooled[d] = sum_n A[n] h[n,d].
 *   ws >= advmil_softmax_pool_workspace_bytes. Deterministic two-stage reduction.
 * softmax_pool_bwd: ds[n] = A[n] * (dA[n] + dot(dpooled, h[n,:]) - sum_m A[m](dA[m] + dot(dpooled,h[m,:])));
 *   dA may be NULL. (dh gets A[n]*dpooled[d] through the rank-1 term of the gemm epilogue.)
 * gate_bwd: from ds -> dG[N,2D] = grads wrt the two pre-activations, plus dwc[D], dbc[1], dbias[2D]
 *   (column sums of dG).
 * pair32 (gate_bwd): ab and dG hold the branches in blocks of 32 columns ([a_0..31 | b_0..31 | a_32..63 | ...], the layout the fused training
 *   gate score stores: advmil_epilogue_t.gate_bits_a) instead of [a | b] halves; the parameter gradients keep their own order.
 * dG_hi / dG_lo (gate_bwd), out_hi / out_lo (act_dropout_bwd): optional (both or neither) bf16 [rows, cols] buffers that also receive
 *   the bf16x3 operand planes of the result, for the plane-fed contraction that reads it next.
 * `accumulate` (here and in the other backward entry points): non-zero ADDS the parameter gradients into the
 *   destination instead of overwriting it -- the destinations are then views of the flat gradient arena, which
 *   removes the per-parameter accumulate launches autograd would issue for every bag. */
int advmil_gate_score_fwd(const float* ab, const float* wc, const float* bc, float drop_p, const uint64_t* seed,
                          uint64_t stream_a, uint64_t stream_b, int64_t N, int64_t D, float* s, const int64_t* rng_row,
                          advmil_stream_t stream);
/* Segmented form: the N rows are a ragged slab of `nseg` bags, bag b = rows [seg_ptr[b], seg_ptr[b+1]) (device int64
 * array; NULL = one segment), max_len = longest segment. pooled / dpooled are [nseg, D]; A, s, ds are [N]. */
size_t advmil_softmax_pool_workspace_bytes(int64_t max_len, int64_t D, int nseg);
int advmil_softmax_pool_fwd(const float* s, const float* h, int64_t ldh, int64_t N, int64_t D, int nseg,
                            const int64_t* seg_ptr, int64_t max_len, float* A, float* pooled, void* ws, size_t ws_bytes,
                            advmil_stream_t stream);
/* Same, plus mean[nseg, D] = the per-bag UNWEIGHTED mean of h's rows from the same pass over h (the projection discriminator's region-level
 * inner product needs mean_r(fc_ins) beside the pooled fc_ins, GANSurv.py:96-98). D % 8 == 0. */
size_t advmil_softmax_pool_mean_workspace_bytes(int64_t max_len, int64_t D, int nseg);
int advmil_softmax_pool_mean_fwd(const float* s, const float* h, int64_t ldh, int64_t N, int64_t D, int nseg, const int64_t* seg_ptr,
                                 int64_t max_len, float* A, float* pooled, float* mean, void* ws, size_t ws_bytes, advmil_stream_t stream);
int advmil_softmax_pool_bwd(const float* dpooled, const float* dA, const float* A, const float* h, int64_t ldh,
                            int64_t N, int64_t D, int nseg, const int64_t* seg_ptr, int64_t max_len, float* ds, void* ws,
                            size_t ws_bytes, advmil_stream_t stream);
/* The same two calls with h held as its bf16x3 operand planes (h = h_hi + h_lo, exact in fp32; pitch ldh in elements, D % 8 == 0, planes
 * 16-byte aligned): the pooled tensor of a slab whose producing contraction wrote planes only (advmil_epilogue_t.c_hi with C == NULL) --
 * round 6: the generator's first layer keeps no fp32 copy of its [rows, 384] output. */
int advmil_softmax_pool_fwd_planes(const float* s, const void* h_hi, const void* h_lo, int64_t ldh, int64_t N, int64_t D, int nseg,
                                   const int64_t* seg_ptr, int64_t max_len, float* A, float* pooled, void* ws, size_t ws_bytes,
                                   advmil_stream_t stream);
int advmil_softmax_pool_bwd_planes(const float* dpooled, const float* dA, const float* A, const void* h_hi, const void* h_lo, int64_t ldh,
                                   int64_t N, int64_t D, int nseg, const int64_t* seg_ptr, int64_t max_len, float* ds, void* ws,
                                   size_t ws_bytes, advmil_stream_t stream);
/* Train-mode dropout of a tensor held as operand planes [M, N] (N % 32 == 0): out planes = split(dropout(in_hi + in_lo)), drawn at
 * (seed, stream_id, element index rng_row[m] * N + n) exactly as advmil_act_dropout_bwd's replay draws it, and bits[m * N / 32 + n / 32]
 * bit n % 32 = (out > 0) (NULL: no bits). The train-mode forward of a ReLU layer whose eval-mode output is memoized as planes
 * (model/backbone.py:60-66 run twice per optimizer step, model_handler.py:398-400 / 420-425).
 * gate_bits_a / gate_bits_b (optional, both or neither; uint32 [M, N / 32]): the KEEP bits of two more dropouts of rate gate_p over the same
 * [M, N] index space, streams gate_stream_a / _b -- the gated attention scorer's branch dropouts (model/backbone_utils.py:24-29), drawn here
 * for the fused training gate score (advmil_epilogue_t.gate_bits_a). */
int advmil_dropout_planes(const void* in_hi, const void* in_lo, int64_t M, int64_t N, float drop_p, const uint64_t* seed, uint64_t stream_id,
                          const int64_t* rng_row, void* out_hi, void* out_lo, void* bits, float gate_p, uint64_t gate_stream_a,
                          uint64_t gate_stream_b, void* gate_bits_a, void* gate_bits_b, advmil_stream_t stream);
/* dh[n, :] = A[n] * dpooled[rowseg[n], :] -- the backward of a pooling with constant weights (the per-bag mean of the region features in
 * the projection discriminator's region-level inner product, GANSurv.py:96-98). rowseg: int32 bag index per row, NULL = one bag. */
int advmil_seg_scale_rows(const float* dpooled, const float* A, const int32_t* rowseg, int64_t N, int64_t D, float* dh,
                          advmil_stream_t stream);
size_t advmil_gate_bwd_workspace_bytes(int64_t N, int64_t D);
int advmil_gate_bwd(const float* ab, const float* ds, const float* wc, float drop_p, const uint64_t* seed,
                    uint64_t stream_a, uint64_t stream_b, int64_t N, int64_t D, float* dG, float* dwc, float* dbc,
                    float* dbias, int accumulate, const int64_t* rng_row, void* dG_hi, void* dG_lo, int pair32, void* ws, size_t ws_bytes,
                    advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward of y = dropout(act(pre)) for the Linear layers: dpre = dy * keep * act'(y) and
 * dbias[n] = sum_m dpre[m,n] (NULL to skip). y is the stored post-dropout output.
 * replaces: autograd of ReLU/Tanh/Sigmoid/Dropout modules (model/backbone.py:70-75 etc.). */
size_t advmil_colsum_workspace_bytes(int64_t M, int64_t N);
/* bits (optional, N % 32 == 0): uint32 [M, N / 32], bit c % 32 of word (m, c / 32) = (dpre[m, c] > 0) -- with act NONE and dy = y = the
 * memoized pre-dropout activations this call IS the train-mode dropout of a ReLU layer, and the bits are that layer's ReLU-and-kept mask
 * for the backward (advmil_epilogue_t.maskbits): 1/32 of the bytes of reading the stored output back. */
int advmil_act_dropout_bwd(const float* dy, const float* y, int act, float drop_p, const uint64_t* seed,
                           uint64_t stream_id, int64_t M, int64_t N, float* dpre, float* dbias, int accumulate,
                           const int64_t* rng_row, void* out_hi, void* out_lo, void* bits, void* ws, size_t ws_bytes,
                           advmil_stream_t stream);
/* out[n] (+)= sum_m x[m,n] */
int advmil_colsum(const float* x, int64_t M, int64_t N, float* out, int accumulate, void* ws, size_t ws_bytes,
                  advmil_stream_t stream);

/* Deferred merges of parameter-gradient partials. Every backward entry point above that ADDS a parameter gradient into its destination
 * (`accumulate` != 0: the destinations are slots of the optimizer's flat gradient arena, model_handler.py:405-409 / 486-497 sum the
 * per-bag gradients the same way through autograd's accumulation) first leaves per-workgroup partial rows -- or split-K partial tiles:
 * advmil_gemm_f32 with splits > 1, alpha = 1 and no other epilogue term -- in the caller's workspace and then folds them with a second,
 * launch-bound kernel. advmil_defer_sums(stream, 1) puts `stream` into deferral: those folds are queued instead (up to 16; a fold into a
 * slot that already has one queued flushes first) and advmil_flush_sums(stream) / advmil_defer_sums(stream, 0) issue them as ONE launch.
 * Contract: every workspace handed to such a call stays alive and untouched until the flush, and nothing reads the destinations before
 * it. Non-accumulating folds are never deferred. advmil_pending_sums: queued folds (-1: the stream is not in deferral). */
int advmil_defer_sums(advmil_stream_t stream, int on);
int advmil_flush_sums(advmil_stream_t stream);
int advmil_pending_sums(advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Region embedding tail of AVGPoolPatchEmbedding (model/backbone_utils.py:158-168):
 * y[N,d] (the 1x1-conv / FC output) -> LayerNorm(d, eps) -> ReLU -> mean over each consecutive 16
 * rows -> emb[N/16,d]. Saves mean/rstd per row for the backward. N % 16 == 0 (backbone_utils.py:65).
 * bwd: demb[N/16,d] -> dy[N,d], dgamma[d], dbeta[d]; dycol (optional, [d]) += column sums of dy -- the bias gradient of the FC
 * that produced y, which otherwise costs a second pass over dy. dy_hi / dy_lo (both or neither): the bf16x3 operand planes of dy for
 * the weight-gradient contraction dy^T X that consumes it (advmil_epilogue_t.a_hi / a_lo); with them dy may be NULL (planes only). */
/* emb_hi / emb_lo (both or neither; d % 128 == 0): also the bf16x3 operand planes of emb (the ESAT in-projection reads it plane-fed). */
/* dup = 2 (d % 128 == 0): emb has 2 N / 16 rows, the embedding written twice ([emb; emb]: the discriminator update feeds the fake and the
 * real pass of the region level as one stacked batch, model_handler.py:373-401); the backward then takes demb [2 N / 16, d] and sums its
 * halves on load -- neither a concatenation nor an add launch. dup = 1: the plain call. */
int advmil_ln_relu_mean16_fwd(const float* y, const float* gamma, const float* beta, float eps, int64_t N, int64_t d,
                              float* emb, float* mean, float* rstd, void* emb_hi, void* emb_lo, int dup, advmil_stream_t stream);
size_t advmil_ln_relu_mean16_bwd_workspace_bytes(int64_t N, int64_t d);
int advmil_ln_relu_mean16_bwd(const float* demb, const float* y, const float* gamma, const float* beta,
                              const float* mean, const float* rstd, int64_t N, int64_t d, float* dy, float* dgamma,
                              float* dbeta, int accumulate, float* dycol, void* dy_hi, void* dy_lo, int dup, void* ws, size_t ws_bytes,
                              advmil_stream_t stream);

/* Plain row-wise LayerNorm(d) -> ReLU (the norm='layer' MLP inside GENConv; N arbitrary). Same kernels as above. */
int advmil_ln_relu_fwd(const float* y, const float* gamma, const float* beta, float eps, int64_t N, int64_t d, float* out,
                       float* mean, float* rstd, advmil_stream_t stream);
size_t advmil_ln_relu_bwd_workspace_bytes(int64_t N, int64_t d);
int advmil_ln_relu_bwd(const float* dout, const float* y, const float* gamma, const float* beta, const float* mean,
                       const float* rstd, int64_t N, int64_t d, float* dy, float* dgamma, float* dbeta, int accumulate,
                       void* ws, size_t ws_bytes, advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Residual block between the GENConv layers of a deep PatchGCN (DeepGCNLayer, block 'res'; model/backbone.py:148-168):
 *   out = keep / (1 - p) * (x + relu(LayerNorm(h)))      h[N, d] contiguous; x (row pitch ldx) and out (row pitch ldo) may be column
 *   blocks of a wider buffer. fwd also writes mean[N] and rstd[N] of h's rows for the backward.
 * The keep decision of element (m, n) is drawn at (seed, stream_id, rng_row[m] * d + n) (rng_row NULL: m) with the hash of
 * advmil_dropout_apply; the backward draws it again and stores no mask.
 * bwd: g = dout * keep / (1 - p) (dout: row pitch lddo); dx (row pitch lddx) = g, added onto dx when dx_accumulate != 0;
 *   dh[N, d] = LayerNorm'(g * (LayerNorm(h) > 0)); dgamma / dbeta = the column sums, through per-workgroup partial rows in ws merged
 *   in a fixed order (accumulate != 0 adds into them). ws >= advmil_gcn_res_bwd_workspace_bytes (a pure host function).
 * One row kernel each way, no host synchronisation (capturable).
 * Shapes: N > 0; 4 <= d <= 512 with d % 4 == 0; every pitch >= d and % 4 == 0; every pointer 16-byte aligned; 0 <= drop_p < 1, and
 * drop_p > 0 needs seed. Anything else: ADVMIL_EINVAL before any launch. */
int advmil_gcn_res_fwd(const float* h, const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, int64_t N,
                       int64_t d, float drop_p, const uint64_t* seed, uint64_t stream_id, const int64_t* rng_row, float* out,
                       int64_t ldo, float* mean, float* rstd, advmil_stream_t stream);
size_t advmil_gcn_res_bwd_workspace_bytes(int64_t N, int64_t d);
int advmil_gcn_res_bwd(const float* dout, int64_t lddo, const float* h, const float* gamma, const float* beta, const float* mean,
                       const float* rstd, int64_t N, int64_t d, float drop_p, const uint64_t* seed, uint64_t stream_id,
                       const int64_t* rng_row, float* dh, float* dx, int64_t lddx, int dx_accumulate, float* dgamma, float* dbeta,
                       int accumulate, void* ws, size_t ws_bytes, advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Region embedding tail of GAPoolPatchEmbedding (model/backbone_utils.py:171-202): gated-attention pooling of each consecutive 16
 * rows. s[N] = the rows' raw gate scores, z[N,d] (row pitch ldz) = the rows that are pooled (relu(LayerNorm(FC x))); region r is rows
 * [16 r, 16 r + 16), R = N / 16:
 *   A[16 r + i] = softmax_i s[16 r + i],   emb[r, :] = sum_i A[16 r + i] z[16 r + i, :]   (i ascending: the bits do not depend on the grid)
 * dup = 2: emb has 2 R rows, the embedding written twice ([emb; emb], as advmil_ln_relu_mean16_fwd does); the backward then takes
 * demb [2 R, d] and sums its halves on load.
 * bwd, g = demb[r] (+ demb[R + r]): ds[16 r + i] = A_i (z_i . g - sum_j A_j z_j . g), dz[16 r + i, :] (contiguous, pitch d) = A_i g,
 * added onto dz when dz_accumulate != 0 and written otherwise.
 * One launch each way: no workspace, no atomics, no segment arrays, no host synchronisation (capturable).
 * Shapes: N > 0, N % 16 == 0; 4 <= d <= 512 with d % 4 == 0 (the widths advmil_ln_relu_fwd takes, in 16-byte units); ldz >= d,
 * ldz % 4 == 0; dup 1 | 2; z, emb, demb, dz 16-byte aligned. Anything else: ADVMIL_EINVAL before any launch. */
int advmil_gapool16_fwd(const float* s, const float* z, int64_t ldz, int64_t N, int64_t d, float* A, float* emb, int dup,
                        advmil_stream_t stream);
int advmil_gapool16_bwd(const float* demb, const float* A, const float* z, int64_t ldz, int64_t N, int64_t d, int dup, float* ds,
                        float* dz, int dz_accumulate, advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * PatchGCN's GENConv softmax aggregation (model/backbone.py:139,157 -> torch_geometric.nn.GENConv, aggr='softmax',
 * learn_t; parity unpinned: restated from the published semantics). x[N,C]; the graph arrives as two int32 CSR images:
 *   by destination (rowptr_dst[N+1], col_src[E] = source of each in-edge)  -> forward
 *   by source      (rowptr_src[N+1], col_dst[E] = target of each out-edge) -> backward
 * fwd: out = agg + x, agg = sum_j softmax_j(t*m_j) m_j, m = relu(x)+eps; saves lse (log-sum-exp of t*m over the in-edges) and agg for
 *      the backward (both NULL: nothing is saved, an evaluation pass writes `out` only).
 * bwd: dx = dout + relu'(x) * sum_{j->i} dout_i w_ij (1 + t (m_j - agg_i)), w_ij = exp(t m_j - lse_i);
 *      dt[0] = sum_{j->i, c} dout_i w_ij m_j (m_j - agg_i), from the same edge walk (per-workgroup partials in `ws`, summed in a fixed
 *      order: run-to-run identical). ws_bytes >= advmil_genconv_bwd_workspace_bytes(N, C). No atomics in either direction. */
int advmil_genconv_fwd(const float* x, const int32_t* rowptr_dst, const int32_t* col_src, const float* t, float eps, int64_t N,
                       int64_t C, float* out, float* lse, float* agg, advmil_stream_t stream);
size_t advmil_genconv_bwd_workspace_bytes(int64_t N, int64_t C);
int advmil_genconv_bwd(const float* dout, const float* x, const float* agg, const float* lse, const int32_t* rowptr_src,
                       const int32_t* col_dst, const float* t, float eps, int64_t N, int64_t C, float* dx, float* dt, void* ws,
                       size_t ws_bytes, advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer + regulariser over a flat parameter arena (torch.optim.Adam, L2-in-grad weight decay:
 * optim/optim_factory.py:25-37,76-77; model/model_handler.py:104-107; L1: loss/utils.py:6-14).
 *   g = grad*grad_scale + l1_coef*sign(p) + wd[i]*p ; Adam(m, v) ; p -= lr/(1-b1^t) * m/(sqrt(v)/sqrt(1-b2^t)+eps)
 * `step` is a device int32 incremented by the kernel (graph-replay safe). wd may be NULL. The arenas are 16-byte aligned (planes: 8). p_hi / p_lo (both or neither): bf16 arenas of
 * n elements that receive the bf16x3 operand planes of the UPDATED weights, so the contractions never re-split a weight.
 * abs_sum: out[0] = sum |p| (for the logged Loss_G_total). */
/* tick != 0: the kernel's own second launch increments `step`; tick = 0: the caller increments it (advmil_step_seed_tick folds that into the
 * RNG seed's advance at the end of an optimizer step: one one-thread launch instead of two). */
/* abs_partial (NULL: skipped): advmil_adam_blocks(n) floats, abs_partial[i] = the i-th workgroup's share of sum |p| BEFORE the update (the logged
 * value of the L1 term, summed on the host when the log is read). clear_grad != 0: grad is zeroed behind its last read (the next step then
 * needs no fill launch; p.grad reads zero afterwards -- the captured step uses it, the eager handler does not). */
int advmil_adam_blocks(int64_t n);
int advmil_adam_step(float* p, float* grad, float* m, float* v, const float* wd, int64_t n, float lr,
                     float beta1, float beta2, float eps, float grad_scale, float l1_coef, int32_t* step, void* p_hi, void* p_lo,
                     int tick, float* abs_partial, int clear_grad, advmil_stream_t stream);
/* step[0] += 1, step2[0] += 1 (the two networks' counters; NULL: skipped) and seed[0] += inc (NULL: skipped) in one launch */
int advmil_step_seed_tick(int32_t* step, int32_t* step2, uint64_t* seed, uint64_t inc, advmil_stream_t stream);
int advmil_abs_sum(const float* p, int64_t n, float* out, void* ws, size_t ws_bytes, advmil_stream_t stream);
size_t advmil_abs_sum_workspace_bytes(int64_t n);

/* The other elementwise optimizers a handler can reach through create_optimizer (optim/optim_factory.py:76-89, optionally behind
 * optim/lookahead.py), one launch over the same arenas with the same options as advmil_adam_step (wd may be NULL, planes both or
 * neither, abs_partial of advmil_adam_blocks(n) floats, clear_grad, tick). g = grad*grad_scale + l1_coef*sign(p) first; then, t = step[0] + 1:
 *   ADAM     g += wd*p; Adam(s1 = m, s2 = v)                                        (torch.optim.Adam: the lookahead_adam base)
 *   ADAMW    p *= 1 - lr*wd; Adam moments of g; same step                           (torch.optim.AdamW)
 *   NADAM    g += wd*p; moments; mu_t = b1 (1 - 0.5 * 0.96^(t sd)); p -= lr (1-mu_t)/(1-M_t) g/den + lr mu_t+1/(1-M_t mu_t+1) m/den,
 *            den = sqrt(v/(1-b2^t)) + eps, M_t = prod mu_i                          (optim/nadam.py)
 *   RADAM    moments of g; p -= wd*lr*p; N = Nmax - 2t b2^t/(1-b2^t); N >= 5: rectified step over sqrt(v)+eps, else p -= lr/(1-b1^t) m
 *                                                                                   (optim/radam.py::RAdam)
 *   ADADELTA g += wd*p; s1 = square_avg, s2 = acc_delta, rho = beta1                (torch.optim.Adadelta)
 * The step-dependent scalars (b^t, N, the rectified step size, mu_t, M_t) are evaluated in double precision on the device from
 * `step`, so a captured launch replays; the elementwise arithmetic is fp32. NADAM keeps its running product M in m_sched[2] (device
 * doubles): the launch of step t reads m_sched[(t-1) & 1] and leaves M_t in m_sched[t & 1].
 * lookahead != 0 (optim/lookahead.py): lt = t - la_state[1] counts the wrapper's steps; when lt % la_k == 0 the slow arena is synced
 * in the same launch: lt <= la_state[0] (the sync that creates the slow buffer) slow = p; later slow += la_alpha (p - slow), p = slow.
 * The planes receive the post-sync weights. la_state: two device int32. */
enum { ADVMIL_OPT_ADAM = 0, ADVMIL_OPT_ADAMW = 1, ADVMIL_OPT_NADAM = 2, ADVMIL_OPT_RADAM = 3, ADVMIL_OPT_ADADELTA = 4 };
typedef struct {
  int32_t kind;                 /* ADVMIL_OPT_* */
  int32_t lookahead;
  int64_t n;
  float* p;
  float* grad;
  float* s1;
  float* s2;
  const float* wd;              /* per-element weight decay, or NULL */
  float* slow;                  /* lookahead: the slow arena (n floats) */
  double lr, beta1, beta2, eps; /* double: they enter the step-dependent scalars (ADADELTA: beta1 = rho) */
  double schedule_decay;        /* NADAM */
  float grad_scale, l1_coef;
  float la_alpha;
  int32_t la_k;
  int32_t tick;
  int32_t* step;
  const int32_t* la_state;      /* lookahead: {first sync step, step offset} */
  double* m_sched;              /* NADAM: two doubles */
  void* p_hi;
  void* p_lo;
  float* abs_partial;
  int32_t clear_grad;
} advmil_optim_t;
int advmil_optim_step(const advmil_optim_t* a, advmil_stream_t stream);

/* Bag ingest from the device-resident bag cache (replaces the per-bag, per-epoch `.cuda()` of model/model_handler.py:315 for a bag
 * that has been seen before): one launch copies rows_bytes of fp32 rows and, when the four plane pointers are given, plane_bytes of
 * each bf16 operand plane, device to device, into the step slab. All pointers and sizes multiples of 16 bytes; planes all or none.
 * dst_hi / dst_lo given with src_hi = src_lo = NULL: the planes are DERIVED from the fp32 rows on the way (hi = bf16(x), lo = bf16(x - hi),
 * as advmil_split_planes; plane_bytes = rows_bytes / 2) -- the cache then holds the fp32 rows only. src == dst rows is allowed in that
 * form (split in place of rows that just arrived over PCIe). */
int advmil_stage_bag(void* dst_rows, const void* src_rows, size_t rows_bytes, void* dst_hi, const void* src_hi, void* dst_lo,
                     const void* src_lo, size_t plane_bytes, advmil_stream_t stream);
/* advmil_stage_bag under a keep bitmap over the bag's 4x4 "square instances" (utils/func.py:14-40 random_mask_square_instance, way
 * mask_zero, applied on the device to the resident clean bag instead of by the dataset on the host: dataset/PatchWSI.py:80-81).
 * n_rows: rows of the bag, a multiple of 16; region r = rows [16 r, 16 r + 16) is kept when bit r & 31 of keep_bits[r >> 5] is set
 * (device array of ceil(n_rows / 16 / 32) words, 4-byte aligned). Kept regions are copied and their planes copied or derived exactly
 * as by advmil_stage_bag; masked regions are written as zeros in the rows and in both planes and are never read from the source.
 * Forms: rows + derived planes; the same with dst_rows = NULL (planes only: nothing is written but the planes; there is no
 * dst == src convention for that here); rows + held planes copied; rows only (elements of any size: rows_bytes / n_rows is the row
 * size); and in place, dst_rows == src_rows (kept regions stay, masked regions are zeroed, planes derived when asked for).
 * Pointers 16-byte aligned, planes all or none; ADVMIL_EINVAL before any launch otherwise. */
int advmil_stage_bag_masked(void* dst_rows, const void* src_rows, size_t rows_bytes, int64_t n_rows, void* dst_hi, const void* src_hi,
                            void* dst_lo, const void* src_lo, size_t plane_bytes, const uint32_t* keep_bits, advmil_stream_t stream);
/* fill out[i] = U[0,1) from the counter RNG (generator noise, utils/func.py:154-164) */
int advmil_uniform_fill(float* out, int64_t n, const uint64_t* seed, uint64_t stream_id, const int64_t* rng_row, int64_t width,
                        advmil_stream_t stream);
/* seed[0] += inc  (advance the step seed between graph replays) */
/* y = x * keep/(1-p) with keep drawn at flat index i of (seed, stream_id): nn.Dropout on the [B, d]-sized head tensors
 * (model/model_utils.py:106-176 make_mlp_layer; applied to dy it is the backward). In place (y == x) allowed.
 * rng_row / width (here and in advmil_uniform_fill): optional row map, the flat tensor is [n / width, width] and row r draws as
 * row rng_row[r] (see advmil_epilogue_t.rng_row); NULL = identity. */
int advmil_dropout_apply(const float* x, float* y, int64_t n, float p, const uint64_t* seed, uint64_t stream_id,
                         const int64_t* rng_row, int64_t width, advmil_stream_t stream);
int advmil_seed_advance(uint64_t* seed, uint64_t inc, advmil_stream_t stream);
/* Measurement aid (bench.py): dst[0] = the device's constant-rate wall clock, written by a one-thread launch in stream order, so two of
 * them bracket a kernel inside a captured step graph; advmil_clock_rate_khz() = ticks per millisecond (0: unknown). Not used by the step. */
int advmil_stamp_clock(int64_t* dst, advmil_stream_t stream);
int64_t advmil_clock_rate_khz(void);
/* The step's two scalar losses over <= bp_every_batch values, value and analytic gradient in one launch each.
 * D loss (loss/utils.py:182-203 real_fake_loss with the reference's means taken over the GLOBAL counts, model_handler.py:412):
 *   which 0 = bce as shipped, 1 = hinge, 2 = wasserstein; real_mask selects the real pairs (event bags with a visible label);
 *   out3 = {loss, sum mask*real, sum fake}; g_fake / g_real = d loss / d score.
 * G loss (model_handler.py:468-486): total = reg + coef*gen, reg = inv_nv * sum vis*recon_term (loss/utils.py:21-41), gen = -inv_nf*sum fake;
 *   out3 = {total, reg, gen}; g_pred / g_fake = d total / d (pred, fake). */
/* Linear layers with in_features == 1 or out_features == 1 on [B, .] head tensors (first layer of make_embedding_y_layer,
 * model_utils.py:178-186; prj_layer, GANSurv.py:78-84; the generator's output layer): y = act(x W^T + bias), x[B,K], W[N,K].
 * bwd: dx (may be NULL), dW / dbias (may be NULL; accumulate != 0 adds into them), dpre = dy * act'(y). */
int advmil_skinny_linear_fwd(const float* x, const float* W, const float* bias, int B, int K, int N, int act, float* y,
                             advmil_stream_t stream);
int advmil_skinny_linear_bwd(const float* x, const float* W, const float* y, const float* dy, int B, int K, int N, int act, float* dx,
                             float* dW, float* dbias, int accumulate, advmil_stream_t stream);
/* Linear (+ bias, activation, dropout) on [B, d] head / tail tensors, B <= 32 rows -- the generator's rho / hop MLP, the discriminator's
 * bag-level MLPs and label embedding (reference model/GANSurv.py:30-49, 89-105; model_utils.py:116-186): y = dropout(act(x W^T + bias)),
 * x[M, K] (pitch ldx), W[N, K]; fp32 FMA; K and ldx multiples of 4, x / W 16-byte aligned. Dropout draw = the contraction epilogue's
 * (element m * N + n of stream `stream_id`, row m replaced by rng_row[m] when given).
 * bwd: dpre = dy * keep * act'(y); dW[N, K] / dbias[N] (each may be NULL; acc_* != 0 adds into them); dx[M, K] (pitch lddx; NULL = not
 * needed; needs the workspace). One launch, two with dx. */
int advmil_small_linear_fwd(const float* x, int64_t ldx, const float* W, const float* bias, int M, int N, int K, int act, float drop_p,
                            const uint64_t* seed, uint64_t stream_id, const int64_t* rng_row, float* y, advmil_stream_t stream);
size_t advmil_small_linear_bwd_workspace_bytes(int M, int N);
int advmil_small_linear_bwd(const float* dy, const float* y, const float* x, int64_t ldx, const float* W, int M, int N, int K, int act,
                            float drop_p, const uint64_t* seed, uint64_t stream_id, const int64_t* rng_row, float* dW, int acc_w,
                            float* dbias, int acc_b, float* dx, int64_t lddx, void* ws, size_t ws_bytes, advmil_stream_t stream);
/* Projection head of the discriminator (reference model/GANSurv.py:78-105, PrjDiscriminator.forward): out[b] = <u[b], t[b]> + <src[b], w> + bias[0]
 * for [B, d] head tensors -- u = the (region-mean) x embedding, t = the label embedding, src = the prj_layer's input (NULL: no projection
 * layer). bwd: du / dt / dsrc [B, d], dw [d], dbias [1] (each may be NULL; accumulate != 0 adds into dw / dbias). */
int advmil_prj_head_fwd(const float* u, const float* t, const float* src, const float* w, const float* bias, int B, int d, float* out,
                        advmil_stream_t stream);
int advmil_prj_head_bwd(const float* dout, const float* u, const float* t, const float* src, const float* w, int B, int d, float* du,
                        float* dt, float* dsrc, float* dw, float* dbias, int accumulate, advmil_stream_t stream);
/* The discriminator's bag-level tail as ONE launch each way (reference model/GANSurv.py:89-105 PrjDiscriminator.forward after the region
 * level: hid_x = net_pair_one.fc2(emb_bag), hid_t = net_pair_two(t), out = <u, hid_t> + prj_layer(hid_x | hid_t), u = hid_x ('bag') or the
 * region-mean embedding ('instance', RLIP); model_utils.py:157-186 builds the two chains). B <= 32 rows (the bags of an optimizer step, or
 * 2 x 16 for the stacked fake | real pass), every width <= 256: one workgroup walks both chains with the activations in LDS -- the six
 * forward and up to twelve backward launches of 5-10 us each that these [B, d] layers cost as separate kernels become two.
 *   layer: y = dropout(act(x W^T + bias)), W [N, K] row-major; dropout element index row * N + col on `stream_id` (row through rng_row when
 *          given: advmil_epilogue_t.rng_row); `y` [B, N] is written by the forward and read by the backward.
 *   backward: dW / dbias (NULL = not wanted) are ADDED into (optimizer arena slots); dxin / dtin / du NULL = not wanted.
 * The two chains must end at the same width d; u [B, d] or NULL (= the x chain's output); prj_src 0 none, 1 = x chain output, 2 = y chain output. */
#define ADVMIL_TAIL_MAXL 3
typedef struct {
  const float* W;
  const float* bias;
  float* dW;
  float* dbias;
  float* y;
  int K, N, act;
  float drop_p;
  uint64_t stream_id;
} advmil_dense_layer_t;
typedef struct {
  int B, nx, ny, prj_src;
  const float* xin;
  const float* tin;
  advmil_dense_layer_t x[ADVMIL_TAIL_MAXL];
  advmil_dense_layer_t y[ADVMIL_TAIL_MAXL];
  const float* u;
  const float* w_prj;
  const float* b_prj;
  float* dw_prj;
  float* db_prj;
  const uint64_t* seed;
  const int64_t* rng_row;
  float* out;        /* forward: [B] */
  const float* dout; /* backward: [B] */
  float* dxin;
  float* dtin;
  float* du;
} advmil_dtail_t;
int advmil_dtail_fwd(const advmil_dtail_t* a, advmil_stream_t stream);
int advmil_dtail_bwd(const advmil_dtail_t* a, advmil_stream_t stream);
/* Several small deep-K weight-gradient contractions C_i (+)= A_i^T B_i (A_i [K, M], B_i [K, N] row-major: the TN form of advmil_gemm_f32) as
 * ONE launch: the three weight gradients behind the fused region network are 2-8 tiles x splits each -- side by side they overlap instead of
 * paying a launch + K-walk latency apiece. 64x64 tiles, split-K per member (>= 256 of K per workgroup), the engine's arithmetic mode and k
 * order: bit-identical to advmil_gemm_f32_tiled(tile 11) with the same split count. n <= 4; M, N, lda, ldb multiples of 4; the merges of the
 * partial tiles are deferrable (advmil_defer_sums) when accumulate != 0 and ldc == N. */
typedef struct {
  int64_t M, N, K;
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  float* C;
  int64_t ldc;
  int32_t accumulate;
} advmil_gemm_tn_call_t;
size_t advmil_gemm_tn_group_workspace_bytes(const advmil_gemm_tn_call_t* calls, int n);
int advmil_gemm_tn_group(const advmil_gemm_tn_call_t* calls, int n, void* ws, size_t ws_bytes, advmil_stream_t stream);
/* The generator's bag-level head as two launches each way (csrc/ghead.hip; reference model/GANSurv.py:13-46 `Generator.forward` behind the
 * backbone's pooling: ABMIL's `rho` = Linear(d0, d1) -> ReLU -> Dropout(p1) (model/backbone.py:66-70; d1 = 0: the backbone has none),
 * MLPs[0] = Linear(d1 | d0, d2) -> ReLU -> Dropout(p2), the noise [B, d2] concatenated, MLPs[1] = Linear(2 d2 | d2, 1), out_scale
 * (model/model_utils.py:124-140 make_noise_mlp_layer, hops = 1, noise = [0, 1]). fp32 FMA, fixed summation order.
 *   noise_mode 0: no noise input (W1 is [1, d2]); 1: zeros (W1 is [1, 2 d2], the noise half contributes nothing); 2: the caller's `noise`
 *   [B, d2]; 3: drawn in the kernel, U[0, 1) at site sid_noise, element rng_row(b) * d2 + n -- the draws of advmil_uniform_fill.
 *   out_act 0: identity, 1: sigmoid. Dropout: stream sid1 at element rng_row(b) * d1 + c (rho), sid2 at rng_row(b) * d2 + n (MLPs[0]).
 * fwd writes hs [B, d1 | d2] (the first hidden layer, post-dropout), h2 [B, d2] (d1 > 0 only), pred [B]; bwd reads them back with dpred [B],
 * writes dx [B, d0] (NULL: not wanted) and ADDS the weight / bias gradients in place (arena slots; NULL: not wanted).
 * B <= 32, d0 <= 512, d0 % 4 == 0, (d1 > 0 ? d1 : d2) % 16 == 0, d2 <= 256, d2 % 4 == 0; ws: advmil_ghead_workspace_bytes. */
typedef struct {
  int32_t B, d0, d1, d2;
  int32_t noise_mode, out_act;
  const float* x;
  int64_t ldx;
  const float* Wr; /* [d1, d0] */
  const float* br;
  const float* W0; /* [d2, d1 | d0] */
  const float* b0;
  const float* W1; /* [1, d2 | 2 d2] */
  const float* b1;
  float p1, p2;
  const uint64_t* seed;
  uint64_t sid1, sid2, sid_noise;
  const int64_t* rng_row;
  const float* noise;
  float* hs;
  float* h2;
  float* pred;
  const float* dpred;
  float* dx;
  int64_t lddx;
  float* dWr;
  float* dbr;
  float* dW0;
  float* db0;
  float* dW1;
  float* db1;
  float* ws;
  size_t ws_bytes;
} advmil_ghead_t;
size_t advmil_ghead_workspace_bytes(int B, int d0, int d1, int d2);
int advmil_ghead_fwd(const advmil_ghead_t* a, advmil_stream_t stream);
int advmil_ghead_bwd(const advmil_ghead_t* a, advmil_stream_t stream);
/* The same head with an output layer of width K (the wide form of csrc/ghead.hip; task disc_gansurv: hazards over K = time_bins bins):
 * MLPs[1] = Linear(2 d2 | d2, K), W1 [K, 2 d2 | d2] row-major, b1 [K], pred / dpred [B, K] contiguous, out_act applied per element, 1 <= K <= 32.
 * Every other field, the dropout / noise sites, their element indices and the bag-level row map are those of advmil_ghead_t; the same
 * decomposition (16-column slices of the first hidden layer, one workgroup per bag for the finish), fp32 FMA, fixed summation order, no
 * atomics, gradients ADDED in place. Alignment: 16 bytes for x, dx, Wr, W0, hs, ws, dWr, dW0 (float4 accesses); W1, b1, pred, dpred, dW1,
 * db1 and the bias / h2 pointers are read and written element by element. Same shape limits as advmil_ghead_t; a call whose slice kernel
 * would need more than 160 KB of LDS returns ADVMIL_EINVAL before any launch (no shape within the limits does).
 * ws: advmil_gheadk_workspace_bytes = slices * B * max(d0, d2, K) floats (d1 == 0: a slice's share of the output layer is [B, K]). */
typedef struct {
  int32_t B, d0, d1, d2;
  int32_t K; /* width of the output layer */
  int32_t noise_mode, out_act;
  int32_t reserved; /* 0 */
  const float* x;
  int64_t ldx;
  const float* Wr; /* [d1, d0] */
  const float* br;
  const float* W0; /* [d2, d1 | d0] */
  const float* b0;
  const float* W1; /* [K, d2 | 2 d2] */
  const float* b1; /* [K] */
  float p1, p2;
  const uint64_t* seed;
  uint64_t sid1, sid2, sid_noise;
  const int64_t* rng_row;
  const float* noise;
  float* hs;
  float* h2;
  float* pred; /* [B, K] */
  const float* dpred; /* [B, K] */
  float* dx;
  int64_t lddx;
  float* dWr;
  float* dbr;
  float* dW0;
  float* db0;
  float* dW1; /* [K, d2 | 2 d2] */
  float* db1; /* [K] */
  float* ws;
  size_t ws_bytes;
} advmil_gheadk_t;
size_t advmil_gheadk_workspace_bytes(int B, int d0, int d1, int d2, int K);
int advmil_gheadk_fwd(const advmil_gheadk_t* a, advmil_stream_t stream);
int advmil_gheadk_bwd(const advmil_gheadk_t* a, advmil_stream_t stream);
/* The discriminator's region-level network as one launch each way (reference model/model_utils.py:188-210 EmbedXLayer: fc1 = Linear(d, d/2)
 * -> ReLU -> Dropout -> Linear(d/2, d); model/backbone_utils.py:31-56 GAPool's scorer tanh(Linear(d, d)) * sigmoid(Linear(d, d)) -> Linear(d, 1))
 * over the R region rows of a step slab, d = 128 (the shipped disc_netx_out_dim; other widths keep the layer-by-layer path):
 *   h1 = dropout_p1(relu(e W1^T + b1)) [R, 64];  fc = h1 W2^T + b2 [R, 128];  ab = tanh | sigmoid (fc Wab^T + bab) [R, 256] (pre-dropout);
 *   s[r] = sum_j drop_pg(a_j) drop_pg(b_j) wc_j + bc.
 * bf16x3 arithmetic (split-bf16 products on the bf16 matrix pipe, fp32 accumulate, the contraction engine's order). Weights arrive as their
 * operand planes (hi = bf16(w), lo = bf16(w - hi), row-major [out, in]; Wab = the tanh branch's rows, then the sigmoid branch's).
 * Dropout draws: stream sid1 at element r * 64 + c for h1, streams sida / sidb at r * 128 + j for the two gate branches (row r through
 * rng_row when given) -- the draws of the separate launches. h1 / ab may be NULL (a pass nobody differentiates).
 * bwd: from ds[R] (gradient wrt the scores), A[R] and dpooled[nseg, 128] (the pooling's direct path A[r] dpooled[bag(r)]), dmean[nseg, 128] or
 * NULL (gradient wrt the per-bag mean of fc: + dmean[bag(r)] / len(bag(r))), dfc_add[R, 128] or NULL (any other gradient wrt fc):
 *   dG [R, 256], dfc [R, 128], dpre [R, 64] (= d h1 masked by the ReLU / dropout of h1), de [R, 128] (NULL: not wanted) are written;
 *   dwc[128], dbab[256], dbc[1], db2[128], db1[64] are ADDED into (arena slots; the merge of the per-workgroup partial rows is deferrable:
 *   advmil_defer_sums). The three weight gradients dWab = dG^T fc, dW2 = dfc^T h1, dW1 = dpre^T e stay contractions of the engine.
 *   WabT / W2T / W1T: operand planes of the TRANSPOSED weights ([128, 256], [64, 128], [128, 64]), made by advmil_dx_chain_prep.
 * One rule for both ways: a dropout is applied iff seed != NULL and its rate > 0. With seed == NULL neither the draws nor the
 * 1 / (1 - p) scales of p1 and pg happen, forward and backward alike, whatever the rates say. */
int advmil_dx_chain_fwd(const float* e, int64_t R, int d, const void* W1_hi, const void* W1_lo, const float* b1, const void* W2_hi,
                        const void* W2_lo, const float* b2, const void* Wab_hi, const void* Wab_lo, const float* bab, const float* wc,
                        const float* bc, float p1, float pg, const uint64_t* seed, uint64_t sid1, uint64_t sida, uint64_t sidb,
                        const int64_t* rng_row, float* h1, float* fc, float* ab, float* s, advmil_stream_t stream);
size_t advmil_dx_chain_bwd_workspace_bytes(int64_t R, int d);
int advmil_dx_chain_prep(const float* W1, const float* W2, const float* Wab, int d, void* W1T_hi, void* W1T_lo, void* W2T_hi, void* W2T_lo,
                         void* WabT_hi, void* WabT_lo, advmil_stream_t stream);
int advmil_dx_chain_bwd(int64_t R, int d, const float* ds, const float* A, const float* dpooled, const float* dmean, const int32_t* rowseg,
                        const int64_t* seg_ptr, const float* dfc_add, const float* h1, const float* ab, const float* wc, float p1, float pg,
                        const uint64_t* seed, uint64_t sida, uint64_t sidb, const int64_t* rng_row, const void* WabT_hi, const void* WabT_lo,
                        const void* W2T_hi, const void* W2T_lo, const void* W1T_hi, const void* W1T_lo, float* dG, float* dfc, float* dpre,
                        float* de, float* dwc, float* dbab, float* dbc, float* db2, float* db1, void* ws, size_t ws_bytes,
                        advmil_stream_t stream);
int advmil_gan_d_loss(const float* fake, int nf, const float* real, const float* real_mask, int nr, int which, float inv_nf,
                      float inv_nr, float* out3, float* g_fake, float* g_real, advmil_stream_t stream);
int advmil_gan_g_loss(const float* pred, const float* t, const float* e, const float* vis_mask, const float* fake, int n, float alpha,
                      float gamma, int l2, float coef, float inv_nf, float inv_nv, float* out3, float* g_pred, float* g_fake,
                      advmil_stream_t stream);
/* The discrete-time task (task: disc_gansurv), csrc/gan_disc.hip. One launch, one workgroup, fixed summation order; capturable.
 * advmil_gan_g_loss_disc: hz[B, K] hazards (dense rows), t[B] bin index carried as fp32, e[B], vis_mask[B] (0/1) or NULL = all visible,
 *   fake[B] scores. mle = inv_nv * sum_b vis_b SurvMLE_term(hz_b, t_b, e_b) (loss/utils.py:123-133: cumprod in bin order in fp32, both
 *   gathers, every log argument clamped at eps; a clamped argument has zero gradient), gen = -inv_nf * sum fake.
 *   out3 = {mle + coef * gen, mle, gen}; g_hz[B, K] = d mle / d hz (the adversarial part reaches hz through the discriminator's backward);
 *   g_fake[B] = -coef * inv_nf. inv_nv == 0: mle = 0 and g_hz = 0. 1 <= B <= 32, 1 <= K <= 32, else ADVMIL_EINVAL before any launch; every
 *   t must lie in [0, K): the caller's duty (a device array cannot be checked here; the kernel never forms an address outside a row).
 * advmil_mask_rows: out[B, K] = x[B, K] * mask[B, K] (dense rows, out distinct from x), B * K < 2^31. */
int advmil_gan_g_loss_disc(const float* hz, const float* t, const float* e, const float* vis_mask, const float* fake, int B, int K,
                           float alpha, float eps, float coef, float inv_nf, float inv_nv, float* out3, float* g_hz, float* g_fake,
                           advmil_stream_t stream);
int advmil_mask_rows(const float* x, const float* mask, int64_t B, int64_t K, float* out, advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Evaluator: concordance index for right-censored data, eval/cindex.py:79-143 (`_get_comparable`,
 * `_estimate_concordance_index`; python loops over samples there, all n^2 pair tests on the device here).
 * time[n], event[n] (!= 0: event observed), estimate[n] (risk: higher = earlier event; the reference passes -prediction,
 * eval/cindex.py:35,41). out6 (device, int64) = concordant, discordant, tied_risk, tied_time, comparable pairs, number of event
 * samples the reference would register (0 -> its NoComparablePairException). cindex = (concordant + 0.5*tied_risk) / comparable. */
int advmil_cindex_counts(const float* time, const float* event, const float* estimate, int64_t n, float tied_tol, int64_t* out6,
                         advmil_stream_t stream);

/* The same counts for B weighted resamples and M estimate rows at once (bootstrap of the concordance index). weights[B, ldw] (device,
 * int32, every entry >= 0): weights[b, i] = how often sample i occurs in resample b. estimate[M, lde]; lde, ldw >= n (elements).
 * out[M, B, 8] (device, int64): out[m, b, 0..5] is exactly what advmil_cindex_counts writes for the arrays in which sample i stands
 * weights[b, i] times (in any order) with estimate row m; out[m, b, 6] = sum_i w_i [event_i != 0] (event copies), out[m, b, 7] =
 * sum_i w_i (size of the resample). Per event anchor i with w_i > 0 and per j: the pair is comparable iff t_j > t_i, or t_j == t_i and
 * event_j == 0; each counter of the pair grows by w_i * w_j; events_with_entry += w_i * [sum_j w_j [t_j >= t_i] - 1 > 0] (j == i
 * included: copies of one sample are never comparable with each other, but they are entries of each other). Integer arithmetic in
 * 64-bit counters throughout (integer atomicAdd into `out`, which the call clears first): bit-identical from run to run and
 * independent of what `out` held; no workspace. 1 <= n, B <= 2^20, 1 <= M <= 64, tied_tol >= 0, weights / estimate 4-byte and out
 * 8-byte aligned, else ADVMIL_EINVAL before anything is enqueued. Asynchronous on `stream`, capturable.
 * advmil_cindex_counts_weighted_plan: the kernel's constants (pure host function): threads striding over j, resamples per chunk,
 * and the number of chunks beyond which one workgroup takes several. */
int advmil_cindex_counts_weighted(const float* time, const float* event, const float* estimate, int64_t lde, int M,
                                  const int32_t* weights, int64_t ldw, int B, int64_t n, float tied_tol, int64_t* out,
                                  advmil_stream_t stream);
int advmil_cindex_counts_weighted_plan(int* row_tile, int* resample_chunk, int* max_chunk_blocks);

/* ------------------------------------------------------------------------------------------
 * Risk-group stratification, csrc/strat.hip: the log-rank sums and the Kaplan-Meier curves of R rows over one cohort of n samples.
 * A row is a vector of group bits (a label permutation, a cut point) and / or of integer weights (a bootstrap resample); a weighted row
 * is by definition the unweighted computation on the arrays in which sample i stands weights[r, i] times.
 * The cohort, prepared once by the caller: order[n] (int32) = a stable ascending sort of the times, stime[k] = time[order[k]] (ascending:
 * the caller's duty, a device array cannot be checked here), sevent[k] = event[order[k]] (!= 0: event observed). The rows stay in the
 * caller's sample order and are read through `order`: groups[R, ldg] (uint8, 0 / not 0; ldg == 0: one row shared by all, else ldg >= n),
 * weights[R, ldw] (int32, every entry >= 0, ldw >= n; NULL: all ones). An entry of `order` outside [0, n) is read as 0: no address
 * outside a row is ever formed. sum_i weights[r, i] < 2^31 per row is the caller's duty. at[Q]: ascending query times, Q >= 0.
 * With w, e, g a row's weights, event flags and group bits, and over the distinct times t_j: d_j = sum of w e at t_j, n_j = sum of w
 * over time >= t_j, d1_j and n1_j their group-1 parts, n0_j = n_j - n1_j (all exact integers):
 *   counts[r, 0..5] (int64) = sum w e g (observed events of group 1), sum w e, sum w g, sum w, #{j: d_j > 0}, #{j: d_j > 0, n_j > 1};
 *   sums[r, 0..1] (double) = E1 = sum_{j: d_j > 0} d_j n1_j / n_j and V = sum_{j: d_j > 0, n_j > 1} (n1_j / n_j) (n0_j / n_j) d_j
 *     ((n_j - d_j) / (n_j - 1)) (the hypergeometric variance, from quotients: the product of the four counts overflows 64 bits);
 *   km[r, c, q] (double, only if Q > 0), c = group 0, group 1, pooled: prod_{t_j <= at[q]} (n^c_j - d^c_j) / n^c_j over the blocks with
 *     d^c_j > 0 -- an empty product is exactly 1, a factor with d == n exactly 0, a class with nobody at risk keeps its value;
 *   median[r, c] (double): the first event time at which that product is <= 0.5, +inf if it never is.
 * Every output slot is written. A row's outputs depend on that row's inputs only (not on R, its position or what the buffers held);
 * no atomics, a fixed order of every sum and product: the same bits from run to run. ws: 4-byte aligned, >=
 * advmil_logrank_rows_workspace_bytes(n, Q) (a pure host function; 0 for Q == 0, ws may then be NULL), else ADVMIL_EWORKSPACE.
 * 1 <= n, R <= 2^20, 0 <= Q <= 2^16, 4-byte (stime, sevent, order, weights, at, ws) and 8-byte (counts, sums, km, median) alignment,
 * else ADVMIL_EINVAL before anything is enqueued. Asynchronous on `stream`, capturable, no host synchronisation. */
size_t advmil_logrank_rows_workspace_bytes(int64_t n, int Q);
int advmil_logrank_rows(const float* stime, const float* sevent, const int32_t* order, int64_t n, const uint8_t* groups, int64_t ldg,
                        const int32_t* weights, int64_t ldw, int R, const float* at, int Q, int64_t* counts, double* sums, double* km,
                        double* median, void* ws, size_t ws_bytes, advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Time-dependent evaluation, csrc/timedep.hip: what the IPCW Brier score (Graf et al.) and the cumulative/dynamic AUC(t) (Uno et al.,
 * Hung & Chiang) are made of, for R rows of integer weights (bootstrap resamples) over one cohort of n samples at Q query times. A
 * weighted row is by definition the unweighted computation on the arrays in which sample i stands weights[r, i] times.
 * The cohort is prepared as for advmil_logrank_rows: order[n] (int32) = a stable ascending sort of the times, stime[k] = time[order[k]],
 * sevent[k] = event[order[k]] (!= 0: observed). Everything else stays in the caller's sample order and is read through `order` (an entry
 * outside [0, n) is read as 0): weights[R, ldw] (int32, >= 0, ldw >= n; NULL: all ones; every row sum < 2^31: the caller's duty),
 * surv[n, lds] (fp32, lds >= Q): surv[i, q] = the predicted probability that sample i survives at[q]; NULL: A = B = 0.
 * risk[n, ldr] (fp32, risk_cols = 1: one column for every q, or risk_cols = Q: column q for at[q]; ldr >= risk_cols); NULL: C = 0.
 * at[Q]: ascending (the caller's duty). No NaN anywhere (the caller's duty).
 * Over the distinct times u of a row's samples with w > 0: n(u) = sum w [y >= u], d(u) = sum w [e][y = u], c(u) = sum w [!e][y = u];
 *   G(t)    = prod_{u <= t, c(u) > 0} (n(u) - d(u) - c(u)) / (n(u) - d(u))   the censoring Kaplan-Meier estimate, right-continuous,
 *             events before censorings at a tied time;
 *   S_KM(t) = prod_{u <= t, d(u) > 0} (n(u) - d(u)) / n(u); an empty product is exactly 1.
 * With t = at[q], cases = {i: e_i, y_i <= t}, controls = {j: y_j > t}:
 *   counts[r, q, 0..1] (int64) = N_case = sum_cases w_i, N_ctrl = sum_controls w_j;
 *   rowcnt[r, 0..1]    (int64) = sum w, sum w e;
 *   sums[r, q, 0..5]  (double) = A  = sum_cases w_i surv[i, q]^2 / G(y_i),
 *                                B  = sum_controls w_j (1 - surv[j, q])^2,
 *                                G(at[q]), S_KM(at[q]),
 *                                Wc = sum_cases w_i / G(y_i),
 *                                C  = sum_cases (w_i / G(y_i)) K_i / 2, K_i = sum_controls w_j (2 [risk_i > risk_j] + [risk_i == risk_j])
 *                                     (fp32 comparisons; K_i is an exact integer below 2^32).
 *   Brier score(t) = (A + B / G(t)) / sum w, defined iff N_ctrl > 0; AUC(t) = C / (Wc N_ctrl), defined iff N_ctrl > 0 and N_case > 0.
 *   Where N_ctrl > 0 every G that is divided by is > 0 (a sample beyond t is still at risk). Where N_ctrl == 0, A, Wc and C are
 *   written as 0 (G(y_i) may be 0 there).
 * Every output slot is written. A row's outputs depend on that row's inputs only (not on R, its position or what the buffers held); no
 * atomics, a fixed order of every sum and product: the same bits from run to run. Each of A, B, G, S_KM, Wc, C is a sum of at most n
 * non-negative terms or a product of at most n factors of correctly rounded quotients of exact integers: relative error <= 2 n 2^-52.
 * ws: 8-byte aligned, >= advmil_ipcw_rows_workspace_bytes(n, R, Q) (a pure host function: R n doubles for G at every sorted sample's
 * own time, n + Q int32 rounded up to 8 bytes; 0 for a shape outside the limits), else ADVMIL_EWORKSPACE. 1 <= n <= 2^16, 1 <= R <= 2^20,
 * 1 <= Q <= 4096, 4-byte (stime, sevent, order, weights, at, surv, risk) and 8-byte (counts, rowcnt, sums, ws) alignment, else
 * ADVMIL_EINVAL before anything is enqueued. Asynchronous on `stream`, capturable, no host synchronisation.
 * advmil_ipcw_rows_plan: the walks' constants (pure host function): rows per workgroup and sorted samples per trip of the per-row walk,
 * threads = cases per round = controls per LDS tile of the pair pass, rows a pair-pass workgroup carries. */
size_t advmil_ipcw_rows_workspace_bytes(int64_t n, int R, int Q);
int advmil_ipcw_rows(const float* stime, const float* sevent, const int32_t* order, int64_t n, const int32_t* weights, int64_t ldw, int R,
                     const float* at, int Q, const float* surv, int64_t lds, const float* risk, int64_t ldr, int risk_cols,
                     int64_t* counts, int64_t* rowcnt, double* sums, void* ws, size_t ws_bytes, advmil_stream_t stream);
int advmil_ipcw_rows_plan(int* walk_rows, int* walk_trip, int* pair_tile, int* pair_rows);

/* ------------------------------------------------------------------------------------------
 * Global concordance, csrc/concord.hip: the pair counts of Harrell's C and of Antolini's time-dependent concordance, and the sums of
 * Uno's C, for R rows of integer weights (bootstrap resamples) over one cohort of n samples. What scikit-survival's
 * concordance_index_ipcw and pycox's EvalSurv.concordance_td answer, restated here so that neither package is needed. A weighted row is
 * by definition the unweighted computation on the arrays in which sample i stands weights[r, i] times.
 * The cohort is prepared as for advmil_ipcw_rows: order[n] (int32) = a stable ascending sort of the times, stime[k] = time[order[k]],
 * sevent[k] = event[order[k]] (!= 0: observed). Everything else stays in the caller's sample order and is read through `order` (an entry
 * outside [0, n) is read as 0): weights[R, ldw] (int32, >= 0, ldw >= n; NULL: all ones; every row sum < 2^31: the caller's duty).
 * Two comparison sources, either may be NULL, not both:
 *   risk[n] (fp32, higher = earlier event): i is WORSE than j iff risk_i > risk_j, they TIE iff risk_i == risk_j. Exact fp32
 *     comparisons: sksurv's tied_tol (1e-8 by default) is restated as 0;
 *   surv[n, lds] (fp32, lds >= Q, 1 <= Q <= 4096) with col[n] (int32): column col[i] holds every sample's predicted probability of
 *     surviving y_i. col[i] is read only where e_i = 1 and must lie in [0, Q) there (the caller's duty; a value outside is clamped, no
 *     address outside a row is formed). i is WORSE than j iff surv[i, col[i]] < surv[j, col[i]], they TIE iff the two are equal.
 * No NaN anywhere (the caller's duty). tau[T] (device, fp32, 1 <= T <= 8): truncation times, +inf = none.
 * The pair (i, j), i the case, is COMPARABLE iff e_i = 1 and (y_j > y_i or (y_j == y_i and e_j = 0)) -- sksurv's _get_comparable and
 * pycox's antolini rule. Per case i and row: Kcomp_i = sum_j w_j [comparable], Kconc_i = sum_j w_j [comparable][i worse than j],
 * Ktied_i = sum_j w_j [comparable][i ties j]; exact integers below 2^31. Source s = 0 is risk, s = 1 is surv:
 *   counts[r, s, 0..2] (int64) = sum_i w_i Kconc_i, sum_i w_i Ktied_i, sum_i w_i Kcomp_i over all cases. Exact. With surv: Antolini's
 *     C_td = conc / comp, adjusted (conc + tied / 2) / comp; with risk: Harrell's C = (conc + tied / 2) / comp under these tie rules;
 *   sums[r, s, t, 0..2] (double) = sum_{i: e_i = 1, y_i < tau[t], G(y_i) > 0} w_i G(y_i)^-2 (Kconc_i, Ktied_i, Kcomp_i): Uno's
 *     C(tau) = (conc + tied / 2) / comp on these. G is the Kaplan-Meier estimate of the censoring distribution OF THE ROW as defined for
 *     advmil_ipcw_rows (events before censorings at a tied time, right-continuous), at the sample's own time: the same bits;
 *   rowcnt[r, 0..1+T] (int64) = sum w, sum w e, and per tau the weight of the cases with y_i < tau[t] whose G(y_i) == 0 (an event tied
 *     with the censorings that end the row). Such cases are left out of the sums; a row with a non-zero count is UNDEFINED for that tau
 *     (sksurv raises there), and so is a row with comp == 0.
 *   The slots of an absent source are written as 0.
 * Every output slot is written. A row's outputs depend on that row's inputs only (not on R, its position or what the buffers held); no
 * atomics, a fixed order of every sum and product: the same bits from run to run.
 * Error of a double sum, u = 2^-53: G(y_i) is a product of at most n factors, each the correctly rounded quotient of exact integers,
 * joined by at most n - 1 rounded multiplications (a factor that is exactly 1 costs nothing): relative (2n - 1) u. A term squares it
 * (2 (2n - 1) u + u), divides w_i by it (u) and multiplies by the exact K_i (u): relative (4n + 1) u. Adding at most n non-negative
 * terms in any order costs (n - 1) u more: below 5 n u to first order, and with the second-order terms (5 n u < 4e-11) below
 * 3 n 2^-52 relative. (conc + tied / 2) / comp of three such sums: relative 3 * 3 n 2^-52 at the most.
 * ws: 8-byte aligned, >= advmil_concord_rows_workspace_bytes(n, R, T) (a pure host function: R n doubles for G, R ceil(n / 256)
 * (5 + 6 T) 8-byte partial sums, n int32 rounded up to 8 bytes; 0 for a shape outside the limits), else ADVMIL_EWORKSPACE.
 * 1 <= n <= 2^16, 1 <= R <= 2^20, 1 <= T <= 8, 4-byte (stime, sevent, order, weights, risk, surv, col, tau) and 8-byte (counts, rowcnt,
 * sums, ws) alignment, else ADVMIL_EINVAL before anything is enqueued. Asynchronous on `stream`, capturable, no host synchronisation.
 * advmil_concord_rows_plan: the walks' constants (pure host function): rows per workgroup and sorted samples per trip of the per-row walk,
 * threads = cases per tile = controls per LDS tile of the pair pass, rows a pair-pass workgroup carries. */
size_t advmil_concord_rows_workspace_bytes(int64_t n, int R, int T);
int advmil_concord_rows(const float* stime, const float* sevent, const int32_t* order, int64_t n, const int32_t* weights, int64_t ldw, int R,
                        const float* risk, const float* surv, int64_t lds, int Q, const int32_t* col, const float* tau, int T,
                        int64_t* counts, int64_t* rowcnt, double* sums, void* ws, size_t ws_bytes, advmil_stream_t stream);
int advmil_concord_rows_plan(int* walk_rows, int* walk_trip, int* pair_tile, int* pair_rows);

/* ------------------------------------------------------------------------------------------
 * Censoring-aware time error and D-calibration, csrc/calib.hip: how wrong a predicted TIME is when the censored samples' unknown event
 * times are replaced by a surrogate built from the cohort's Kaplan-Meier curve (the margin and the pseudo-observation of Qi et al.,
 * ICML 2023), next to the plain hinge (the reference's `mae`), and whether a predicted DISTRIBUTION is calibrated (D-calibration, Haider
 * et al., JMLR 2020), for R rows of integer weights (bootstrap resamples) over one cohort of n samples. The tail convention (the curve is
 * integrated to the row's largest time and no further) and the tie conventions below are THIS PROJECT'S; other packages extrapolate the
 * tail differently. A weighted row is by definition the unweighted computation on the arrays in which sample i stands weights[r, i] times.
 * The cohort is prepared as for advmil_concord_rows: order[n] (int32) = a stable ascending sort of the times, stime[k] = time[order[k]],
 * sevent[k] = event[order[k]] (!= 0: observed). Everything else stays in the caller's sample order and is read through `order` (an entry
 * outside [0, n) is read as 0): weights[R, ldw] (int32, >= 0, ldw >= n; NULL: all ones; every row sum < 2^31: the caller's duty).
 * Two sources, either may be NULL, not both:
 *   pred[n, ldp] (fp32, ldp >= P, 1 <= P <= 8): P columns of predicted times (the mean and the median of the samples, or two models);
 *   p_own[n] (fp32 in [0, 1]): the predicted probability of surviving one's own time, S_i(t_i); binned into `bins` = B bins.
 * 1 <= P <= 8 and 2 <= B <= 32 size the outputs and are checked whether or not the source is there. gamma (fp32, not NaN): the hinge
 * margin. Times >= 0 and no NaN anywhere are the caller's duty.
 * Per row: N = sum w; the distinct times with positive weight u_1 < ... < u_K, u_0 = 0; d_v = sum w e [t = u_v], n_v = sum w [t >= u_v].
 *   S(u_v) = prod_{x <= v} (1 - d_x / n_x): the event Kaplan-Meier curve of the row, right-continuous, events before censorings at a
 *     tie, 1 before u_1;
 *   theta = sum_v S(u_{v-1}) (u_v - u_{v-1}): the restricted mean to the row's largest time; A(u_k) = sum_{v > k} S(u_{v-1}) (u_v - u_{v-1});
 *   hinge, per column: sum_{e=1} w |t - y| + sum_{e=0} w max(0, t + gamma - y), over N. gamma = 1: the reference's `mae` (recon_loss at
 *     its default gamma, cur_alpha = 0); gamma = 0: the textbook hinge;
 *   margin: a censored sample of block k has the surrogate m = t + A(u_k) / S(u_k) (m = t where S(u_k) = 0) and the confidence
 *     omega = 1 - S(u_k); an event has m = t, omega = 1. Numerator sum w omega |m - y|, denominator sum w omega;
 *   pseudo-observation (only if with_po): for a censored sample of block k, theta^(-k) is the same restricted mean over the SAME grid
 *     u_1 .. u_K with every n_v, v <= k, lowered by one (a factor whose lowered n_v is 0 is 1); it depends on the block only. The
 *     surrogate is N theta - (N - 1) theta^(-k) -- what literally deleting one copy of the sample from the expanded arrays and
 *     integrating the new curve over the full row's grid gives; omega, numerator and denominator as for the margin;
 *   D-calibration: a sample's bin is k = min(B - 1, (int)(p * (float)B)), the product in fp32. An event adds w to bin k; a censored
 *     sample with p > 0 adds w (p - k / B) / p to bin k and w / (B p) to every bin below it (in double, from the fp32 p); a censored
 *     sample with p = 0 adds w to bin 0. The masses of a row sum to N.
 * Outputs:
 *   rowcnt[r, 0..3] (int64) = sum w, sum w e, K, the weight of the censored samples with S = 0 at their time. Exact. (Under these tie
 *     conventions a censored sample is still counted in n_v at its own time, so d_v < n_v there and the last count is 0: it is the guard
 *     of the `m = t where S = 0` clause, written so that a caller can see the clause was never taken);
 *   km[r, 0..2]    (double) = theta, S(u_K), u_K (a row without weight: 0, 1, 0);
 *   err[r, c, 0..2, 0..1] (double) = hinge, margin, pseudo-observation of column c, each numerator | denominator (the hinge's is N);
 *   dcal[r, 0..B-1] (double) = the bin masses.
 *   The slots of an absent source, and of the pseudo-observation when with_po == 0, are written as 0; with_po changes no other bit.
 *   Margin and pseudo-observation are undefined where their denominator is 0 (a row without an event).
 * Every output slot is written. A row's outputs depend on that row's inputs only (not on R, its position or what the buffers held); no
 * atomics, a fixed order of every sum and product: the same bits from run to run.
 * How theta^(-k) is formed: with g_v = (n_v - 1 - d_v) / (n_v - 1), S'_v = prod_{x <= v} g_x, theta'_k = sum_{v <= k} S'_{v-1}
 * (u_v - u_{v-1}) and T_k = sum_{v > k} (prod_{k < x < v} (1 - d_x / n_x)) (u_v - u_{v-1}) = A(u_k) / S(u_k) (one backward recurrence),
 * theta^(-k) = theta'_k + S'_k T_k: O(n) per row for all blocks together. A block of the cohort without weight in the row is a factor
 * of exactly 1 and splits an interval in two: the row walks the cohort's blocks.
 * Errors, u = 2^-53. Every factor is the correctly rounded quotient of exact integers; S, S' are products of at most n of them:
 * relative (2n - 1) u. An interval is the difference of two fp32 times in double (u); theta, theta' add at most n non-negative terms
 * S (u_v - u_{v-1}) ((2n + 1) u each, (n - 1) u for the sum in any order): relative 3 n u. T_k is a sum of non-negative products of
 * at most n factors and an interval, formed by composing maps y -> a + f y: a term passes at most n multiplications and n additions,
 * relative (3n + 1) u. All four: below 2 n 2^-52 relative. omega = 1 - S carries 2 n u ABSOLUTE; a term w omega |m - y| therefore an
 * absolute error below (5n + 5) u w (m + |y|), and a numerator (hinge and margin) at most 5 n 2^-52 sum w (m + |gamma| + |y|), its
 * denominator 2 n 2^-52 N. The pseudo-observation is N theta - (N - 1) theta^(-k), the difference of two numbers up to N u_K that are
 * each relative 4 n 2^-52 at the most: ABSOLUTE 8 n 2^-52 N u_K per surrogate, and 2^-52 n (8 N u_K sum_{e=0} w + 5 sum w (|s| + |y|))
 * for the numerator, s the surrogate. This loss of log2 N bits belongs to the DEFINITION of the pseudo-observation (it is there in
 * exact deletion carried out in double just as well), not to the kernel. A D-calibration mass adds at most n terms of magnitude <= w
 * (4 u w each) and at most B partial sums: ABSOLUTE (n + B + 4) 2^-52 N.
 * ws: 8-byte aligned, >= advmil_calib_rows_workspace_bytes(n, R, with_po) (a pure host function: R n (3 + 2 with_po) doubles; 0 for a
 * shape outside the limits), else ADVMIL_EWORKSPACE. 1 <= n <= 2^16, 1 <= R <= 2^20, with_po 0 or 1, 4-byte (stime, sevent, order,
 * weights, pred, p_own) and 8-byte (rowcnt, km, err, dcal, ws) alignment, else ADVMIL_EINVAL before anything is enqueued. Asynchronous
 * on `stream`, capturable, no host synchronisation.
 * advmil_calib_rows_plan: the walks' constants (pure host function): rows per workgroup and sorted samples per trip of the per-row walk,
 * rows per workgroup of the D-calibration pass. */
size_t advmil_calib_rows_workspace_bytes(int64_t n, int R, int with_po);
int advmil_calib_rows(const float* stime, const float* sevent, const int32_t* order, int64_t n, const int32_t* weights, int64_t ldw, int R,
                      const float* pred, int64_t ldp, int P, const float* p_own, int bins, float gamma, int with_po, int64_t* rowcnt,
                      double* km, double* err, double* dcal, void* ws, size_t ws_bytes, advmil_stream_t stream);
int advmil_calib_rows_plan(int* walk_rows, int* walk_trip, int* dcal_rows);

/* ------------------------------------------------------------------------------------------
 * Survival evaluators (eval/evaluator.py:11,133,213) and the two O(n^2) pair losses (loss/utils.py:43-80, 155-175), csrc/survk.hip.
 * fp32 inputs; every term is formed in fp32 (exp / log of a term: the hardware v_exp_f32 / v_log_f32, ~1 ulp), every sum is carried
 * in double; per-anchor logs and the rescaling of the softmax merge are double-precision libm. No floating-point atomics: partials go
 * to `ws` (>= the matching *_workspace_bytes(n), pure host functions) and a second launch merges them in a fixed order, so results
 * are bit-reproducible and independent of what `ws` and the outputs held. Every output slot is written. Asynchronous on `stream`,
 * capturable. 1 <= n <= 2^31 - 1. `which`: 0 bce as shipped | 1 hinge | 2 wasserstein (as advmil_gan_d_loss); `fake` may be NULL
 * (its slots are then 0).
 *
 * advmil_surv_metrics_cont -> out16 (device, double): 0 sum of recon_loss terms at `alpha`, 1 at alpha = 0, 2 sum of the `mae` terms
 *   (recon_loss defaults: gamma 1, l1, alpha 0), 3 sum of the discriminator's fake-only terms, 4 sum fake,
 *   5 sum_{e==1} |t-p| / end_time, 6 sum_{e==0} relu(t-p) / end_time, 7 sum_{e==1} (p-t) / end_time, 8 sum_{e==0} -relu(t-p) / end_time,
 *   9 #(e == 1), 10 #(e == 0), 11..15 zero. The caller forms the means.
 * advmil_surv_metrics_disc: hazards[n, bins] with row pitch ld (elements), 1 <= bins <= 256; t = bin index carried as fp32 (truncated
 *   toward zero). risk[n] = sum_k prod_{l<=k} (1 - h_l). out16: 0 sum of SurvMLE terms (loss/utils.py:123-133, both clamps at eps) at
 *   `alpha`, 1 at alpha = 0, 2 sum of fake-only terms, 3 sum fake, 4 number of rows whose bin index lies outside [0, bins-1] (such an
 *   index is never used as an address; the row adds nothing to slots 0-1), 5..15 zero.
 * advmil_ple_loss: SurvPLE.forward for 1-D T, E: out2[0] = -mean_i (theta_i - log sum_j [T_j >= T_i] exp theta_j) E_i with theta
 *   clamped at 10, out2[1] = sum E.
 * advmil_rank_loss_fwd: pairs (i, j) with t_i < t_j and e_i == 1, x = p_i - p_j, L = relu(gamma + x) (squared if l2); weights 1/#pairs
 *   or, with add_weight, softmax of x over the pairs. loss[0] (fp32) and state4 (double) = loss, #pairs or Z, max x (0 for uniform
 *   weights), #pairs. No pair: loss 0.
 * advmil_rank_loss_bwd: dpred[k] = gout[0] * (sum_j dx_kj - sum_i dx_ik), dx = w L' (uniform) or w (L' + L - loss) (softmax weights),
 *   from the forward's state4; no pair: all zeros. */
size_t advmil_surv_metrics_cont_workspace_bytes(int64_t n);
int advmil_surv_metrics_cont(const float* t, const float* e, const float* pred, const float* fake, int64_t n, float alpha, float gamma,
                             int l2, float end_time, int which, double* out16, void* ws, size_t ws_bytes, advmil_stream_t stream);
size_t advmil_surv_metrics_disc_workspace_bytes(int64_t n);
int advmil_surv_metrics_disc(const float* hazards, int64_t ld, const float* t, const float* e, const float* fake, int64_t n, int bins,
                             float alpha, float eps, int which, float* risk, double* out16, void* ws, size_t ws_bytes,
                             advmil_stream_t stream);
size_t advmil_ple_loss_workspace_bytes(int64_t n);
int advmil_ple_loss(const float* theta, const float* T, const float* E, int64_t n, double* out2, void* ws, size_t ws_bytes,
                    advmil_stream_t stream);
size_t advmil_rank_loss_workspace_bytes(int64_t n);
int advmil_rank_loss_fwd(const float* pred, const float* t, const float* e, int64_t n, float gamma, int l2, int add_weight,
                         double* state4, float* loss, void* ws, size_t ws_bytes, advmil_stream_t stream);
int advmil_rank_loss_bwd(const float* pred, const float* t, const float* e, int64_t n, float gamma, int l2, int add_weight,
                         const double* state4, const float* gout, float* dpred, advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * WSI graph construction (tools/patchgcn_graph_s2.py:70-90 of the reference, exact instead of HNSW), csrc/knn.hip.
 * Rows of the slab are partitioned into bags by seg_ptr (nseg + 1 int64 offsets, device; NULL with nseg == 1: one bag of N rows);
 * max_len = the longest bag, 1 <= max_len <= N. nbr[N, k] (int32): row i = the k nearest rows of i's OWN bag other than i itself, as
 * BAG-LOCAL ids, ascending by (squared distance, id). Self is excluded by index: a duplicate point at distance 0 is a neighbour.
 * 1 <= k <= 16, N < 2^31. A bag of <= k rows is memory-safe: the slots it cannot fill hold -1 and, in dist2, the largest finite value
 * of the type (INT64_MAX / FLT_MAX). dist2[N, k] may be NULL. No atomics, no N x N buffer: results are bit-reproducible and do not
 * depend on what the outputs or the workspace held. Asynchronous on `stream`, capturable.
 *
 * advmil_knn_spatial: xy[N, 2] int32 (8-byte aligned), |coordinate| < 2^30 (the caller's duty); squared distances exact in int64.
 * advmil_knn_latent: x_hi / x_lo = the bf16x3 operand planes of x[N, C] (advmil_split_planes), row pitch ldx >= C halfwords,
 *   ldx % 8 == 0, both 16-byte aligned, C % 32 == 0. One fused launch forms S = Xq . Xk^T tile by tile with the three-MFMA bf16x3
 *   product (whatever advmil_set_gemm_mode says, as the attention core) and ranks key j for query i by n_j - 2 s_ij, n_j = the fp32
 *   squared norm of row j from the planes (a small first launch, kept in `ws`); dist2 (fp32) = max(0, n_i + n_j - 2 s_ij).
 *   ws >= advmil_knn_latent_workspace_bytes(N, C, k) = 4 N bytes rounded up to 16 (ADVMIL_EWORKSPACE when shorter). */
int advmil_knn_spatial(const int32_t* xy, int64_t N, int k, int nseg, const int64_t* seg_ptr, int64_t max_len, int32_t* nbr,
                       int64_t* dist2, advmil_stream_t stream);
size_t advmil_knn_latent_workspace_bytes(int64_t N, int64_t C, int k);
int advmil_knn_latent(const void* x_hi, const void* x_lo, int64_t ldx, int64_t N, int64_t C, int k, int nseg, const int64_t* seg_ptr,
                      int64_t max_len, int32_t* nbr, float* dist2, void* ws, size_t ws_bytes, advmil_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batched k-means over the rows of a slab (the cluster ids of bcb_mode: cluster; tools/deepattnmisl_cluster.py of the reference runs
 * sklearn KMeans on the CPU), csrc/kmeans.hip. Conventions of the k-NN entry points above: bags by seg_ptr (NULL with nseg == 1: one
 * bag), every bag has its own K centres cent[nseg, K, C] (fp32, 16-byte aligned), a row meets its own bag's centres only. No atomics:
 * bit-reproducible, independent of what outputs and workspace held, and a bag gives the same bits alone and inside a slab.
 * 1 <= K <= 32, C % 32 == 0, N < 2^31. active[nseg] (int32, device; NULL = every bag): a bag with active[b] == 0 is not touched.
 * Asynchronous on `stream`.
 *
 * advmil_kmeans_assign: x_hi / x_lo = the bf16x3 operand planes of x[N, C], contract of advmil_knn_latent (pitch ldx >= C halfwords,
 *   ldx % 8 == 0, 16-byte aligned). The centres are split to hi / lo inside the launch and stay in LDS, which bounds
 *   K (C + 8) <= 37 856 (ADVMIL_EINVAL beyond). S = X . cent^T is the three-MFMA bf16x3 product whatever advmil_set_gemm_mode says;
 *   centre j is ranked for row i by c_j - 2 s_ij (c_j = fp32 squared norm of the split centre), ties to the lowest j.
 *   labels[N] (int32) is read AND written: changed[nseg] (may be NULL) = the rows of the bag whose label differs from the value labels
 *   held on entry, 0 for an inactive bag. dist2[N] (may be NULL) = max(0, n_i + c_j - 2 s_ij), n_i as in advmil_knn_latent.
 *   ws >= advmil_kmeans_assign_workspace_bytes = the row norms and the rows' moved flags (8 N bytes, each half rounded up to 16);
 *   norms_ready != 0: ws still holds the norms an earlier call on the same planes left there, the norm launch is skipped.
 * advmil_kmeans_update: x[N, C] fp32 (row pitch ldx >= C floats, ldx % 4 == 0, 16-byte aligned), labels as written by assign (a row
 *   whose label is outside [0, K) is skipped), max_len = the longest bag. cent_new[nseg, K, C] (may be cent itself) = per cluster
 *   (float)((double)sum / count), sum = the fp32 sum over the bag's rows in a fixed order: chunks of 128 rows counted from the BAG's
 *   first row, in row order inside a chunk, chunks folded in ascending order. A cluster without rows keeps its centre, count 0.
 *   count[nseg, K] int32; shift2[nseg] = sum_j ||cent_new_j - cent_j||^2. Inactive bag: cent_new = cent bit for bit, shift2 = 0,
 *   count not written. */
size_t advmil_kmeans_assign_workspace_bytes(int64_t N, int64_t C, int K);
int advmil_kmeans_assign(const void* x_hi, const void* x_lo, int64_t ldx, int64_t N, int64_t C, int K, int nseg, const int64_t* seg_ptr,
                         const int32_t* active, const float* cent, int norms_ready, int32_t* labels, float* dist2, int32_t* changed,
                         void* ws, size_t ws_bytes, advmil_stream_t stream);
size_t advmil_kmeans_update_workspace_bytes(int64_t max_len, int64_t C, int K, int nseg);
int advmil_kmeans_update(const float* x, int64_t ldx, int64_t N, int64_t C, int K, int nseg, const int64_t* seg_ptr, int64_t max_len,
                         const int32_t* active, const int32_t* labels, const float* cent, float* cent_new, int32_t* count, float* shift2,
                         void* ws, size_t ws_bytes, advmil_stream_t stream);

/* Greedy k-means++ seeding (sklearn's _kmeans_plusplus: every pick tries L = 2 + int(ln K) rows drawn from the D^2 distribution and
 * keeps the one that lowers the potential most), for every bag of the slab at once: one pick = advmil_kmeans_seed_cand, then
 * advmil_kmeans_seed_pick, ONE launch each whatever nseg and N are, nothing read back. Conventions of the entry points above (bags by
 * seg_ptr, max_len = the longest bag, nseg <= 65535, no atomics, a bag gives the same bits alone and inside a slab, asynchronous on
 * `stream`); 1 <= L <= 8. `ws` >= advmil_kmeans_seed_workspace_bytes(N, max_len, L, nseg) carries the state of the seeding from call
 * to call: the row norms (4 N bytes rounded up to 16) | the chunk potentials [nseg][ceil(max_len / 128)][L] float64. A workspace sized
 * for a larger L serves a smaller one.
 *
 * advmil_kmeans_seed_cand: planes as advmil_kmeans_assign. cand[nseg, L] (int32) = the bag-local rows on trial (an index outside its
 *   bag is clamped into it); the trial rows are read from the planes themselves. closest[N] fp32, NULL = +inf (the first centre: L = 1).
 *   d_il = max(0, n_i + n_cand - 2 s_il) with the bits advmil_kmeans_assign gives for the centre x[cand_l]; writes
 *   candmin[N, L] = min(closest_i, d_il) and, into ws, the float64 sum of candmin[:, l] over every chunk of 128 rows counted from the
 *   bag's first row, in row order. 2 L (C + 8) halfwords of LDS: ADVMIL_EINVAL where that exceeds the CU's. norms_ready as in assign.
 * advmil_kmeans_seed_pick: reads cand, candmin and ws as the candidate pass with the same (N, L, nseg, seg_ptr, max_len) left them.
 *   pot[nseg, L] (float64) = the chunk sums folded in ascending order; best = the first minimum of pot[b, :] (np.argmin);
 *   row_out[b * row_stride] (int64) = cand[b, best]; closest_i = candmin[i, best]. With L_next > 0 also the next pick's draws:
 *   cum = the float64 inclusive prefix sum of closest over the bag (the chunks before a row folded in ascending order, then row order
 *   inside its chunk; the last prefix equals pot[b, best] bit for bit), cand_next[b, l] = the first row with
 *   cum_i >= u[b * u_stride + l] * cum_last, the bag's last row when there is none (np.searchsorted side="left", clipped): a bag whose
 *   potential is 0 yields row 0. u float64 on the device, u_stride >= L_next doubles; cand_next[nseg, L_next] must not be cand.
 *   L_next == 0 (the last pick): u and cand_next are not read. */
size_t advmil_kmeans_seed_workspace_bytes(int64_t N, int64_t max_len, int L, int nseg);
int advmil_kmeans_seed_cand(const void* x_hi, const void* x_lo, int64_t ldx, int64_t N, int64_t C, int L, int nseg, const int64_t* seg_ptr,
                            int64_t max_len, const int32_t* cand, const float* closest, int norms_ready, float* candmin, void* ws,
                            size_t ws_bytes, advmil_stream_t stream);
int advmil_kmeans_seed_pick(int64_t N, int L, int nseg, const int64_t* seg_ptr, int64_t max_len, const int32_t* cand, const float* candmin,
                            const double* u, int64_t u_stride, int L_next, int64_t* row_out, int64_t row_stride, double* pot,
                            float* closest, int32_t* cand_next, const void* ws, size_t ws_bytes, advmil_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
