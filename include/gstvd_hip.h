/*
 * gstvd_hip.h -- C ABI of the MI355X (gfx950) kernels behind the gst-visdial enc_dec_a hot path.
 *
 * The reference (gicheonkang/gst-visdial) has NO native/FFI boundary: its hot path is eager
 * PyTorch inside models/vilbert_dialog.py, models/visual_dialog_{encoder,decoder,model}.py
 * (SURVEY.md section 8b).  This header is therefore the build's own boundary; every entry
 * point names the reference code it replaces.  Conventions:
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless noted;
 *   - the caller owns every buffer (no allocation inside), passes the hipStream_t to launch on;
 *   - return value: 0 = ok, <0 = invalid argument (GSTVD_E_*), >0 = hipError_t of the launch;
 *   - re-entrant, no global mutable state; safe under hipGraph stream capture
 *     (no sync / malloc / memcpy inside);
 *   - dtype: GSTVD_F32 (exact-fp32 parity mode, f32-input MFMA) or GSTVD_BF16 (bf16 storage,
 *     fp32 accumulate / statistics) -- the arithmetic type of activations;
 *   - dropout is counter based: keep(e) = hash(rng[0] (seed), rng[1] (step offset), site, e);
 *     `rng` points to two uint64 in device memory so a captured graph sees a fresh offset
 *     per replay; backward regenerates the mask instead of storing it.
 */
#ifndef GSTVD_HIP_H
#define GSTVD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gstvd_stream_t; /* hipStream_t */

enum { GSTVD_F32 = 0, GSTVD_BF16 = 1 };
enum {
  GSTVD_E_DTYPE = -1, GSTVD_E_SHAPE = -2, GSTVD_E_ALIGN = -3, GSTVD_E_NULL = -4, GSTVD_E_UNSUPPORTED = -5
};

/* ---- library info ----------------------------------------------------------------------- */
int gstvd_abi_version(void);            /* bumps on any signature change */
const char* gstvd_build_arch(void);     /* "gfx950" */

/* ---- GEMM: every nn.Linear forward / dgrad / wgrad on the path ---------------------------
 * C[m,n] = epi( alpha * sum_k A(m,k) * B(n,k) ),   batch = grid.z with element strides s*.
 *   A(m,k) = a_kmajor ? A[k*lda + m] : A[m*lda + k];   B(n,k) = b_kmajor ? B[k*ldb + n] : B[n*ldb + k]
 * forward  y = x W^T + b        : A=x,  B=W            (vilbert_dialog.py:381-383,417,446,459 ...)
 * dgrad    dx = dy W            : A=dy, B=W  b_kmajor
 * wgrad    dW = dy^T x          : A=dy a_kmajor, B=x b_kmajor, fp32 output, optional accumulate
 * Epilogue flags (bitmask), applied in this order:
 *   GSTVD_EPI_BIAS      += bias[n]                       (bias is always fp32)
 *   GSTVD_EPI_ADD       += addend[m,n]                   (dtype_out; residual / grad accumulate)
 *   GSTVD_EPI_GELU      aux[m,n] = gelu_erf'(v) (dtype_in); v = gelu_erf(v)   (vilbert_dialog.py:115-121)
 *   GSTVD_EPI_DGELU     v *= aux[m,n]   (aux as written by the forward GELU epilogue)
 *   GSTVD_EPI_DROPOUT   v *= keep(site, (z*M+m)*N+n) / (1-p)      (VLFusion dropout, visual_dialog_model.py:133)
 * Constraints: N % 4 == 0; row-major operands need K % (16/sizeof(T)) == 0 and 16-byte aligned rows;
 * k-major operands need their M (resp. N) extent % (16/sizeof(T)) == 0.  M and the k extent of
 * k-major operands are arbitrary (predicated / zero filled).
 */
enum { GSTVD_EPI_BIAS = 1, GSTVD_EPI_ADD = 2, GSTVD_EPI_GELU = 4, GSTVD_EPI_DGELU = 8, GSTVD_EPI_DROPOUT = 16,
       /* grouped weight-gradient launches only (gstvd_gemm_grouped with a k-major A, see gstvd_gemm_group_caps):
        * bias[m] (=|+=) sum_k A[k][m] -- the bias gradient dY^T.1 that autograd computes next to dW = dY^T X, taken from the
        * dY tiles the launch stages anyway (the tiles of column block 0 do it); COLSUM_ACC adds to bias instead of overwriting */
       GSTVD_EPI_COLSUM = 32, GSTVD_EPI_COLSUM_ACC = 64,
       /* gstvd_gemm_grouped_adamw only: C of this problem is a weight's slot of the flat gradient buffer and nothing else adds
        * to it this step -- the launch applies the AdamW update to the weight in its epilogue (see there) */
       GSTVD_EPI_ADAMW = 128 };

typedef struct {
  const void* A; const void* B; void* C;
  const float* bias; const void* addend; void* aux;
  int64_t M, N, K;
  int64_t lda, ldb, ldc, ldadd, ldaux;
  int64_t batch, sA, sB, sC, sAdd, sAux;
  int32_t dtype_in, dtype_out, a_kmajor, b_kmajor, epilogue;
  float alpha, dropout_p;
  uint32_t site;
  const uint64_t* rng;
} gstvd_gemm_t;
int gstvd_gemm(const gstvd_gemm_t* g, gstvd_stream_t s);

/* Split-K form of the same problem (bf16 inputs, batch = 1): for skinny, deep problems -- the decoder's 400-row
 * GEMMs with K >= 2304 and the LM-head input gradient (K = 30528) -- whose few 64x64 output tiles cannot keep the chip's
 * LDS fill paths busy.  `splits` workgroups share a tile, park fp32 partials in `ws`, the last to arrive adds them in
 * split order (result independent of arrival order) and runs the epilogue.  `ws`: caller-owned device scratch of at
 * least gstvd_gemm_splitk_ws_bytes() bytes (4 KiB of per-tile arrival counters, then the partials; at most 1024 tiles),
 * zero-filled once (the kernel leaves its counters zero; one scratch serves launches of any shape), never shared by
 * launches that may run concurrently (one per stream). */
int64_t gstvd_gemm_splitk_ws_bytes(int64_t M, int64_t N, int32_t splits);
int gstvd_gemm_splitk(const gstvd_gemm_t* g, int32_t splits, void* ws, int64_t ws_bytes, gstvd_stream_t s);

/* Grouped form: `table_dev` is a DEVICE array of nprob independent problems (batch ignored, = 1) that share dtypes
 * and operand layouts; they run as ONE launch over all their T x T tiles, T = gstvd_gemm_group_tile() (256).
 * tile_off_dev[i] = first tile id of problem i (ceil(M/T)*ceil(N/T) tiles each), device int32[nprob].  The engine uses it
 * for the deferred weight-gradient GEMMs of a whole backward pass (dW = dy^T x: a_kmajor = b_kmajor = 1, fp32 out, EPI_ADD
 * to accumulate), whose individual grids are too small to fill the chip.  bf16 inputs only.
 * block_map_dev (ABI 5; NULL = the library's own order): device int32[nblocks], nblocks >= total_tiles -- workgroup b runs
 * tile block_map_dev[b] (a tile id as in tile_off_dev), or nothing when the entry is negative; every tile id must appear
 * exactly once.  Workgroups b, b + 8, b + 16, ... share one XCD and its L2 (a speed fact, never a correctness one): the
 * caller that knows which problems share operand panels and run equally long (same K) queues them back to back on one XCD,
 * so that the ~32 tiles an XCD runs at a time stream the same panels in step -- autograd has no counterpart, it is pure
 * placement.
 * ABI 6: an entry's tile id is its bits 0-20 (total_tiles < 2^21); bits 21-30 of a non-negative entry are reserved and
 * ignored (round 5 measured a start barrier between the workgroups of a unit in them: fewer fetches, slower launch;
 * profiles/r05_group_sync_ab.txt). */
int gstvd_gemm_group_tile(void);
int gstvd_gemm_grouped(const gstvd_gemm_t* table_dev, const int32_t* tile_off_dev, int64_t nprob, int64_t total_tiles,
                       int32_t dtype_in, int32_t dtype_out, int32_t a_kmajor, int32_t b_kmajor,
                       const int32_t* block_map_dev, int64_t nblocks, gstvd_stream_t s);

/* ---- fused (bias-free) dropout + residual + LayerNorm, and the two embedding front ends -----
 * mode GSTVD_LN_RESID : h = drop_pre(x) + res ; y = drop_post(LN(h))   (BertSelfOutput/BertOutput/
 *        BertBiOutput, vilbert_dialog.py:416-420,458-462,735-742; HF BertSelfOutput/BertOutput)
 * mode GSTVD_LN_EMBED : h = word[ids] + pos[t] + type(seg)             (BertEmbeddingsDialog, :324-352)
 * mode GSTVD_LN_IMAGE : h = x + loc W_loc^T + b_loc                    (BertImageEmbeddings, :1420-1427)
 * LayerNorm is the TF-style (x-u)/sqrt(var+eps) of vilbert_dialog.py:283-296.
 * mean / rstd (fp32 [M]) are saved for backward.
 */
enum { GSTVD_LN_RESID = 0, GSTVD_LN_EMBED = 1, GSTVD_LN_IMAGE = 2 };

typedef struct {
  int32_t mode, dtype;
  int64_t M, H;                 /* rows, hidden (H % 4 == 0, H <= 2048) */
  const void* x; int64_t ldx;   /* RESID / IMAGE: [M,H] */
  const void* res; int64_t ldres; /* RESID: residual or NULL */
  const float* gamma; const float* beta; float eps;
  void* y; int64_t ldy;
  float* mean; float* rstd;
  float p_pre, p_post; uint32_t site_pre, site_post; const uint64_t* rng;
  /* EMBED */
  const int64_t* ids; const int64_t* segs; /* [M]; segs may be NULL (=0) */
  int64_t T; int32_t type_vocab;           /* position = row % T + pos_offset */
  const float* word; const float* pos; const float* tt; const float* tt_ext; /* fp32 tables, row stride H */
  /* IMAGE */
  const float* loc; const float* w_loc; const float* b_loc; /* loc [M,5] fp32, w_loc [H,5], b_loc [H] */
  int64_t pos_offset;                      /* EMBED: added to the position (KV-cached decode feeds one token per row) */
} gstvd_ln_t;
int gstvd_ln_fwd(const gstvd_ln_t* p, gstvd_stream_t s);

/* backward: dh = LN'(dy) ; dres = dh ; dx = drop_pre'(dh).
 * partial: fp32 [nblk, 3, H] scratch (nblk = gstvd_ln_bwd_blocks(M)) receiving per-block column sums of
 * (dy*xhat, dy, dx); reduce them with gstvd_colsum_partials.
 * EMBED mode scatters dh into dword/dpos (and dtt/dtt_ext for segment ids >= 2) with fp32 atomic adds instead of
 * writing dres/dx; its partial is [nblk, 4, H]: (dy*xhat, dy, dh of segment-0 rows, dh of segment-1 rows) -- the
 * caller adds vectors 2 and 3 to dtt rows 0 and 1 (no atomics onto those two hot rows). */
typedef struct {
  gstvd_ln_t f;                 /* the forward descriptor (y unused) */
  const void* dy; int64_t lddy;
  void* dres; int64_t lddres;   /* RESID: gradient wrt res (NULL allowed if res NULL); IMAGE: dh */
  void* dx; int64_t lddx;       /* RESID: gradient wrt x (may alias dres when p_pre == 0) */
  float* partial;
  float* dword; float* dpos; float* dtt; float* dtt_ext; /* EMBED */
  int64_t nblk;   /* number of [3|4][H] slabs `partial` holds = gstvd_ln_bwd_blocks_for(M, H, mode); 0 = gstvd_ln_bwd_blocks(M) */
} gstvd_ln_bwd_t;
int64_t gstvd_ln_bwd_blocks(int64_t M);                                    /* upper bound for every (H, mode) */
int64_t gstvd_ln_bwd_blocks_for(int64_t M, int64_t H, int32_t mode);       /* the geometry gstvd_ln_bwd uses when told so via nblk */
int gstvd_ln_bwd(const gstvd_ln_bwd_t* p, gstvd_stream_t s);
/* Measurement support: the (mangled) symbol of the device kernel that gstvd_ln_fwd (bwd == 0, desc: a gstvd_ln_t) or gstvd_ln_bwd
 * (bwd != 0, desc: a gstvd_ln_bwd_t) launches for this descriptor -- the launchers' own route decision (mode, type, 256-column
 * vectors per lane, rows per wave, waves per block), same checks and return codes as the launch; nothing is launched.
 * GSTVD_E_SHAPE when buf_len is too small for the name. */
int gstvd_ln_kernel_name(const void* desc, int32_t bwd, char* buf, int32_t buf_len);

/* LayerNorm folded into the Linear next to it, for latency-bound row counts (the decoder's M = rows x 25; csrc/gemm_rows.hip).
 * Both take a gstvd_gemm_t whose A operand is NOT read (A is produced in the kernel; M, K = the LayerNorm's M, H; bf16 operands,
 * batch 1, row-major or k-major B, every gstvd_gemm epilogue flag except COLSUM) and a RESID-mode LayerNorm descriptor:
 *   gstvd_gemm_ln_fwd   C = epi( LN(drop(x) + res) . B^T );  also writes ln->y / mean / rstd exactly as gstvd_ln_fwd would
 *                       (BertSelfOutput / BertOutput LayerNorm + the dense that reads it: transformers 4.16.2 modeling_bert,
 *                       call sites models/visual_dialog_decoder.py:300-311)
 *   gstvd_gemm_ln_bwd   C = epi( dx . B ), dx = what gstvd_ln_bwd(lb) writes to lb->dx (the LayerNorm's backward + the input
 *                       gradient of the Linear that produced the LayerNorm's input; autograd of the same modules); also writes
 *                       lb->dres, lb->dx and lb->partial = [ceil(M/R), 3, H] column partials, R = gstvd_gemm_ln_rows_per_block();
 *                       lb->nblk must be ceil(M/R)
 * Constraints: H = K a multiple of 64 and <= 768, M <= 1024, N >= 640 and N % 8 == 0.  GSTVD_E_UNSUPPORTED otherwise (the caller
 * runs the two kernels separately).  M <= 1024 is what the KERNEL accepts; the host policy (ops.gemm_ln_ok) only sends M <= 640
 * and at most 512 workgroups (one round of the chip) -- beyond that the two plain kernels are faster. */
int gstvd_gemm_ln_fwd(const gstvd_gemm_t* g, const gstvd_ln_t* ln, gstvd_stream_t s);
int gstvd_gemm_ln_bwd(const gstvd_gemm_t* g, const gstvd_ln_bwd_t* lb, gstvd_stream_t s);
int64_t gstvd_gemm_ln_rows_per_block(void);

/* out_j[c] (+)= sum_blk partial[blk, j, c]  for j in 0..nvec-1 ; out_j may be NULL (skipped) */
int gstvd_colsum_partials(const float* partial, int64_t nblk, int64_t nvec, int64_t H,
                          float* out0, float* out1, float* out2, int32_t accumulate, gstvd_stream_t s);

/* Batched form: every pending column reduction of a backward pass in ONE launch.  `table_dev` is a device
 * array of entries; entry i owns blocks [blk0_i, blk0_{i+1}) of the grid, one block per 64 output columns
 * of its nvec*H wide row; out_j[c] (+)= sum_{k<nblk} partial[k*stride + j*H + c]. */
typedef struct {
  const float* partial; float* out[3];
  int64_t nblk, stride, H;
  int32_t nvec, accumulate[3], blk0;
} gstvd_colsum_entry_t;
int gstvd_colsum_batched(const gstvd_colsum_entry_t* table_dev, int64_t nent, int64_t total_blocks, gstvd_stream_t s);
/* table-driven stage 1: entry i owns blocks [blk0_i, blk0_{i+1}), ceil(M/64) * ceil(N/256) blocks each;
 * scratch[slab, N] = sums over rows [64*slab, 64*slab+64) of x[M, N] (row stride ldx, all entries of one dtype) */
typedef struct { const void* x; float* scratch; int64_t ldx, M, N; int32_t blk0, pad_; } gstvd_slab_entry_t;
int gstvd_colsum_slabs_batched(const gstvd_slab_entry_t* table_dev, int64_t nent, int64_t total_blocks, int32_t dtype,
                               gstvd_stream_t s);
/* stage 1 of a plain column sum: scratch[slab, N] = per-64-row-slab sums of x[M, N] (reduce with the batched form) */
int gstvd_colsum_slabs(const void* x, int64_t ldx, int64_t M, int64_t N, int32_t dtype, float* scratch,
                       int64_t scratch_elems, gstvd_stream_t s);

/* out[c] (+)= sum_m x[m, c]   (bias gradients of QKV / FFN-up projections) */
int gstvd_colsum(const void* x, int64_t ldx, int64_t M, int64_t N, int32_t dtype, float* out,
                 float* scratch, int64_t scratch_elems, int32_t accumulate, gstvd_stream_t s);

/* dW_loc[h, j] (+)= sum_m dh[m,h] * loc[m,j]   (image_location_embeddings.weight grad) */
int gstvd_locgrad(const void* dh, int64_t lddh, const float* loc, int64_t M, int64_t H, int32_t dtype,
                  float* dw_loc, int32_t accumulate, gstvd_stream_t s);

/* ---- fused attention: softmax(Q K^T * scale + mask) V with dropout on the probabilities ------
 * (BertSelfAttention / BertImageSelfAttention / BertBiAttention, vilbert_dialog.py:380-407,507-534,
 *  646-712; HF 4.16.2 BertSelfAttention incl. the causal decoder mask and cross attention.)
 * Element (b, i, h, c) of Q lives at Q[(b*Lq + i)*ldq + h*d + c]; K, V, O, dO, dQ, dK, dV alike, so the
 * operands can be column slices of fused QKV buffers.
 * additive mask(b, i, j) = (key_mask[b, j] != 0 && (!causal || j <= i)) ? 0 : mask_neg;
 * LSE [B, nh, Lq] fp32 is saved by forward; backward recomputes P from it (nothing of size Lq x Lk is stored).
 * d in {32, 64, 128}.
 */
typedef struct {
  const void *Q, *K, *V; void* O; float* LSE;
  const float* key_mask;            /* [B, Lk] 1/0, or NULL = all ones */
  int64_t ldq, ldk, ldv, ldo;
  int32_t B, nh, Lq, Lk, d, causal, dtype;
  float mask_neg, scale, dropout_p; uint32_t site; const uint64_t* rng;
  /* backward only */
  const void* dO; int64_t lddo;
  void *dQ, *dK, *dV; int64_t lddq, lddk, lddv;
  float* delta;                      /* [B, nh, Lq] fp32 scratch: rowsum(dO * O) */
  int32_t kv_group;                  /* forward only: K, V and key_mask are shared by kv_group consecutive batch rows
                                        (their batch index is b / kv_group); 0 or 1 = one K/V per row.  Used to score the
                                        100 answer candidates of a dialog round against ONE encoder pass (evaluate_gen.py:45-92
                                        re-encodes the identical context 100 times). */
  int32_t q_bstride, kv_bstride;     /* forward only: rows between consecutive batch elements of Q/O resp. K/V (0 = Lq / Lk).
                                        Lets one decode step (Lq = 1) read a [B, Umax, H] K/V cache of which Lk rows are filled. */
  uint64_t* drop_bits;               /* (ABI 5) NULL, or the dropout keep bits of the probabilities: uint64
                                        [B, nh, ceil(Lq/16), ceil(Lk/16), 4] -- word r of tile (qt, kt): bit 16 g + i = "keep" of
                                        (query 16 qt + i, key 16 kt + 4 g + r).  Forward WRITES them when the pointer is set and
                                        dropout is on (the same draws it applies: nn.Dropout's mask, vilbert_dialog.py:398-401);
                                        the one-pass backward READS them instead of hashing every draw again (40 % of its vector
                                        instructions); the other backward kernels ignore them.  bf16, d = 64 only. */
} gstvd_attn_t;
int gstvd_attn_fwd(const gstvd_attn_t* a, gstvd_stream_t s);
int gstvd_attn_bwd(const gstvd_attn_t* a, gstvd_stream_t s);  /* dQ (+delta) then dK,dV */
/* Measurement / test support: the (mangled) symbol of the device kernel gstvd_attn_fwd (bwd == 0) or gstvd_attn_bwd (bwd != 0)
 * would launch for this descriptor, taken from the launchers' own route decision; same status codes as the launch.  Nothing is
 * launched.  The two-part backward's answer carries its block order: "<symbol> dq_first=0|1".  GSTVD_E_SHAPE when buf_len is
 * too small for the answer. */
int gstvd_attn_kernel_name(const gstvd_attn_t* a, int32_t bwd, char* buf, int32_t buf_len);
/* (entry point added for listwise candidate training, no signature changed: ABI stays 9)
 * The backward of a GROUPED forward launch, which gstvd_attn_bwd refuses: kv_group = G consecutive query rows share the K, V and
 * key_mask of row b / G.  Reads the descriptor as gstvd_attn_fwd left it (B query rows, B % G == 0) plus the backward fields.
 * dQ [B * Lq rows] and delta [B, nh, Lq] are per query row, bit for bit what gstvd_attn_bwd's two-part kernel gives with K, V and
 * the mask replicated G times.  dK, dV have (B / G) * Lk rows and are WRITTEN, not accumulated: row (e, k) is the sum over the
 * query rows e * G .. e * G + G - 1, added in ascending order by the one block that owns the key -- no atomics, the same bits
 * every run.  Dropout: the forward's draws, element index ((b * nh + h) * Lq + q) * round4(Lk) + k with b the query row;
 * drop_bits is ignored.  causal != 0, q_bstride != 0, kv_bstride != 0 or B % G != 0: GSTVD_E_UNSUPPORTED, nothing is written.
 * kv_group 0 or 1 is the ungrouped two-part backward.  d in {32, 64, 128}, bf16 and fp32. */
int gstvd_attn_group_bwd(const gstvd_attn_t* a, gstvd_stream_t s);
/* P = softmax_j(scale * q_i . k_j + mask(b, i, j)) in fp32, the probabilities gstvd_attn_fwd applies for the same descriptor:
 * p = __expf(s - m) times the correctly rounded 1 / sum (row maximum m and row sum taken by this call; one multiply, not a division),
 * with dropout off.  mask() as defined above gstvd_attn_t: key_mask, causal, mask_neg, kv_group.  Reads Q, K, key_mask only:
 * V, O, LSE, rng are not touched; the call does not depend on an earlier launch.  head_mean == 0: P [B, nh, Lq, Lk] contiguous;
 * head_mean != 0: P [B, Lq, Lk] = (p_0 + p_1 + ... + p_{nh-1}) * (1.0f / nh), heads added in ascending order in fp32 (nh <= 16).
 * Every element of P is written exactly once (a masked entry is written as the value the formula gives, 0.0f unless the whole row
 * is masked).  dropout_p != 0, q_bstride != 0 or kv_bstride != 0: GSTVD_E_UNSUPPORTED.  d in {32, 64, 128}, bf16 and fp32. */
int gstvd_attn_probs(const gstvd_attn_t* a, float* P, int32_t head_mean, gstvd_stream_t s);

/* ---- LM head loss: CrossEntropyLoss(ignore_index) of visual_dialog_decoder.py:70-77 ----------
 * logits [M, ldl >= V]; row_loss [M] (0 for ignored rows); stats (fp32[3], written by the call):
 * stats[0] = sum of row losses, stats[1] = number of non-ignored rows, stats[2] = mean loss
 * (= stats[0] / stats[1], NaN when every row is ignored, like torch); lse [M] saved.
 * A label outside [0, V) that is not ignore_index (the engines never produce one): the row's loss is 0 and its gradient row is
 * zero, like an ignored row's, but the row COUNTS in stats[1] (only label == ignore_index is left out of the count).
 * The three cross-entropy entries read logits and write dlogits in 4-element vectors; refused before any launch:
 * ldl < V or ldd < V or a leading dimension that is no multiple of 4 (GSTVD_E_SHAPE), a logits / dlogits pointer that is not
 * 16-byte (fp32) / 8-byte (bf16) aligned (GSTVD_E_ALIGN), a dtype that is neither GSTVD_F32 nor GSTVD_BF16 (GSTVD_E_DTYPE,
 * checked before the alignment, which depends on it). */
int gstvd_ce_fwd(const void* logits, int64_t ldl, const int64_t* labels, int64_t M, int64_t V,
                 int64_t ignore_index, int32_t dtype, float* row_loss, float* lse, float* stats,
                 gstvd_stream_t s);
/* dlogits[m, v] = (softmax - onehot) * gscale[0] / (mean ? stats[1] : 1) for kept rows, 0 otherwise;
 * columns V..ldd-1 are zero filled (they are the zero padded vocabulary rows of the LM head). */
int gstvd_ce_bwd(const void* logits, int64_t ldl, const int64_t* labels, const float* lse,
                 const float* stats, const float* gscale, int32_t mean, int64_t M, int64_t V,
                 int64_t ignore_index, int32_t dtype, void* dlogits, int64_t ldd, gstvd_stream_t s);
/* (entry points added for the FGSM attack evaluation, no signature changed: ABI stays 9)
 * The same under a PER-ROW upstream gradient, the backward of CrossEntropyLoss(reduction='none') (evaluate_gen_attack.py:121-130):
 * dlogits[m, v] = g[m] * (softmax - onehot) for kept rows with g[m] != 0 (g: device fp32 [M]); a row with g[m] == 0 or an
 * ignored label is stored as exact zeros (never 0 * inf); columns V..ldd-1 zero filled.  With g[m] = gscale / stats[1] on the
 * kept rows the result is gstvd_ce_bwd's mean form to the last bit (one row routine serves both). */
int gstvd_ce_bwd_rows(const void* logits, int64_t ldl, const int64_t* labels, const float* lse, const float* g, int64_t M,
                      int64_t V, int64_t ignore_index, int32_t dtype, void* dlogits, int64_t ldd, gstvd_stream_t s);
/* evaluate_gen_attack.py:131: out[i] = x[i] + eps * sign(g[i]) over fp32 [n], sign(+0) = sign(-0) = 0 (torch.sign), denormal g
 * counted by its sign bit; out may alias x; 16-byte aligned pointers. */
int gstvd_fgsm_step(const float* x, const float* g, float eps, float* out, int64_t n, gstvd_stream_t s);
/* evaluate_gen.py:94-106: score[m] = sum_u [tgt != 0] * (logits[m,u,tgt] - lse[m,u]) with tgt = ids shifted left */
int gstvd_answer_scores(const void* logits, int64_t ldl, const float* lse, const int64_t* dec_ids,
                        int64_t rows, int64_t U, int32_t dtype, float* scores, gstvd_stream_t s);
/* (entry point added for listwise candidate training, no signature changed: ABI stays 9)
 * Listwise ranking loss over the G answer candidates of each of E dialog rounds, one launch, no host synchronisation.
 * logits [E*G*U, ldl], lse [E*G*U], dec_ids [E*G, U] as for gstvd_answer_scores; relevance [E*G] fp32, >= 0.
 *   scores[i]     = gstvd_answer_scores' value, bit for bit
 *   t             = relevance / sum(relevance) per round; p = softmax over the round of scores * inv_temperature (fp32)
 *   round_loss[e] = -sum_{t_i > 0} t_i log p_i; a round whose relevance sums to 0 has loss 0, weights 0 and is not counted
 *   stats         = [sum of round_loss, counted rounds, mean (0 when no round counts)]
 *   g_tok[i, u]   = -(p_i - t_i) * inv_temperature / counted where dec_ids[i, u + 1] != 0, exactly 0 elsewhere: the upstream
 *                   gradient of the per-token cross entropies, as gstvd_ce_bwd_rows takes it (d mean loss / d ce[i, u]). */
int gstvd_rank_loss(const void* logits, int64_t ldl, const float* lse, const int64_t* dec_ids, const float* relevance,
                    int64_t E, int64_t G, int64_t U, float inv_temperature, int32_t dtype, float* scores, float* p,
                    float* round_loss, float* g_tok, float* stats, gstvd_stream_t s);

/* One sampling step of the decode loop (models/visual_dialog_model.py:96-108 after the n-gram filter has produced `banned`;
 * utils/decoding_utils.py:4-35 for the top-k rule): z = logits / temperature (banned -> -inf); top_k > 0: z below the k-th
 * largest z -> -inf (ties with it stay); out[b * out_stride] = first index whose cumulative softmax probability reaches
 * u[b] * total (inverse CDF -- the draw the oracle substitutes for the reference's torch.multinomial, whose stream is device
 * specific).  The id carries a non-zero weight whenever a token of the row does: it is the first position of non-zero weight
 * whose running sum reaches u * total, the LAST such position when rounding leaves every sum below it (never the clamp V - 1,
 * never a filtered or banned token next to a CDF step), and 0 for a row in which everything is banned.
 * logits [B, ld >= V] fp32 or bf16; banned: NULL or uint8 [B, banned_ld >= V]; u [B] in (0, 1).
 * ngram > 0 (ABI 5): the n-gram filter itself, utils/decoding_utils.py:38-77 (batch_ngram_blocking + _get_generated_ngrams), runs
 * in the same launch -- a token is banned when it would complete an n-gram that occurs in the row's history hist[b, 0..hist_T)
 * (int64 ids, row stride hist_ld; n-grams that contain one of the n_special ids in `special` are ignored) and whose first n-1
 * tokens are the row's last n-1 generated ids: ids_tm[(cur_len - (n-1) + j) * ids_stride + b], j < n-1, read from the TIME-MAJOR
 * id buffer [positions, ids_stride >= B].  Nothing is banned while cur_len < n-1 or hist_T < n (the reference's slice
 * semantics).  It composes with `banned` (either bans).
 * top_p in (0, 1) (ABI 6): nucleus filtering after top-k, utils/decoding_utils.py:22-34 -- a token stays when the softmax mass of
 * the tokens sorted in front of it (strictly larger logits) is <= top_p, i.e. the token that crosses top_p stays; equal logits
 * stay or go together (the reference leaves the order inside a tie to torch.sort).  0 or >= 1: off.  top_k is unbounded since
 * ABI 6 (k <= 16 walks the distinct values from the top, larger k bisects on the value). */
typedef struct {
  const void* logits; int64_t ld; int32_t dtype; int32_t B; int32_t V; int32_t top_k; float temperature;
  const float* u; int64_t* out; int64_t out_stride; const uint8_t* banned; int64_t banned_ld;
  const int64_t* hist; int64_t hist_ld; int32_t hist_T; int32_t ngram;
  const int64_t* ids_tm; int64_t ids_stride; int32_t cur_len; int32_t n_special; int32_t special[8];
  float top_p; int32_t reserved_;                                       /* ABI 6 */
} gstvd_sample_t;
int gstvd_sample_topk(const gstvd_sample_t* a, gstvd_stream_t s);
/* (entry point added for sample-and-rank decoding, no signature changed: ABI stays 9)
 * The same draw -- the rule above, the same ids -- and in the same launch the drawn id's log-probability
 *   logp[b * logp_stride] = (x[id] - max x) - log(sum_v exp(x[v] - max x))
 * in fp32 (expf / logf) over the row's RAW logits x[0..V): temperature, `banned`, the n-gram filter, top-k and top-p play no
 * part in it.  This is gstvd_beam_step's logp_j[v], so sampled and beam scores mean the same thing.  A row in which everything
 * is banned draws id 0 and reports the log-probability of id 0; columns V..ld are never read.  Refuses what gstvd_sample_topk
 * refuses, then logp == NULL (GSTVD_E_NULL) and logp_stride < 1 (GSTVD_E_SHAPE), before any launch. */
int gstvd_sample_topk_scored(const gstvd_sample_t* a, float* logp, int64_t logp_stride, gstvd_stream_t s);

/* backward of VLFusion's concat + dropout (visual_dialog_model.py:132-133): d_enc [B, R+T, H] ->
 * d_v [B*R, H] (vision rows first) and d_t [B*T, H], each multiplied by the dropout mask its forward GEMM
 * epilogue applied (element index (b*R + r)*H + n under site_v, (b*T + t)*H + n under site_t). */
int gstvd_vl_split(const void* d_enc, int64_t B, int64_t R, int64_t T, int64_t H, int32_t dtype, void* d_v, void* d_t,
                   float p, uint32_t site_v, uint32_t site_t, const uint64_t* rng, gstvd_stream_t s);

/* ---- element-wise plumbing --------------------------------------------------------------------*/
int gstvd_cast(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t n, gstvd_stream_t s);
/* (ABI 7) dst[e] = bf16(src[e]) for e in the union of `nranges` ranges of two flat buffers that share their indexing: ranges_dev =
 * device int64[nranges][2] (start, length; start % 4 == 0), blk0_dev = device int32[nranges + 1], the exclusive prefix sum of the
 * ranges' block counts ceil(length / 1024); total_blocks = blk0_dev[nranges].  The N > 1 gradient path: the weight-gradient
 * launch writes the bf16 all-reduce payload of every GEMM weight itself, this casts the REST of a slice (biases, LayerNorm, embedding
 * tables: ~5 % of it) instead of a pass over the whole fp32 gradient buffer (train_gen.py:324: the reduce-add of DataParallel). */
int gstvd_cast_ranges(const float* src, void* dst_bf16, const int64_t* ranges_dev, const int32_t* blk0_dev, int64_t nranges,
                      int64_t total_blocks, gstvd_stream_t s);
int gstvd_scale(float* x, const float* factor, int64_t n, gstvd_stream_t s);   /* x *= factor[0] */
int gstvd_rng_advance(uint64_t* rng, gstvd_stream_t s);                        /* rng[1] += 1 */
/* materialise a dropout mask (1/(1-p) or 0) for tests: out[e] for e in [0, n) */
int gstvd_dropout_mask(float* out, int64_t n, float p, uint32_t site, const uint64_t* rng, gstvd_stream_t s);

/* fused AdamW over flat fp32 buffers with pytorch_transformers-1.2.0 semantics (train_gen.py:16,247:
 * eps inside sqrt(v)+eps, bias correction, decoupled decay applied after the update) and, optionally,
 * refresh of the bf16 shadow weights in the same pass.  lr/wd are per-element-segment tables:
 * seg_end[i] is the exclusive end offset of segment i; hp[2*i] = lr, hp[2*i+1] = weight decay (lr 0 = skip).
 * The call updates flat elements [begin, n): the backward pipeline applies the optimizer slice by slice, as soon
 * as a slice's gradients are final, overlapped with the rest of backward. */
int gstvd_adamw(float* param, const float* grad, float* m, float* v, void* shadow_bf16, int64_t n,
                const int64_t* seg_end, const float* hp, int64_t nseg, float beta1, float beta2, float eps,
                const float* step /* device scalar, 1-based */, float grad_scale, int64_t begin, gstvd_stream_t s);
/* Same update with the gradient taken from a bf16 buffer: flat element i reads grad_bf16[i - grad_origin].  Used at N>1
 * when the gradient slice travels over RCCL in bf16: the all-reduced bf16 slice feeds AdamW directly instead of being
 * expanded back into the fp32 gradient buffer first (saves 8 B/param of HBM traffic per step). */
int gstvd_adamw_bf16grad(float* param, const void* grad_bf16, int64_t grad_origin, float* m, float* v, void* shadow_bf16,
                         int64_t n, const int64_t* seg_end, const float* hp, int64_t nseg, float beta1, float beta2, float eps,
                         const float* step, float grad_scale, int64_t begin, gstvd_stream_t s);

/* The update of a chosen set of 1024-element blocks of the flat buffers: block_list_dev[b] = index of a block (elements
 * [1024 k, 1024 k + 1024), absolute), nblocks of them; of those, elements outside [begin, n) and elements of segments with
 * seg_skip_dev[segment] != 0 are left alone (seg_skip_dev NULL = none).  It is the remainder pass behind
 * gstvd_gemm_grouped_adamw: biases, LayerNorm and embedding parameters, and any weight whose gradient was accumulated from
 * several producers. */
int gstvd_adamw_blocks(float* param, const float* grad, float* m, float* v, void* shadow_bf16, int64_t n,
                       const int64_t* seg_end, const float* hp, int64_t nseg, float beta1, float beta2, float eps,
                       const float* step, float grad_scale, int64_t begin, const int32_t* block_list_dev, int64_t nblocks,
                       const uint8_t* seg_skip_dev, gstvd_stream_t s);

/* Weight gradients and their AdamW update as ONE launch (single-GPU training: no all-reduce stands between a gradient and its
 * update; train_gen.py:324-329 loss.backward(); optimizer.step(); optimizer.zero_grad()).  A grouped launch like
 * gstvd_gemm_grouped (bf16 operands, both k-major, fp32 accumulators); for every problem that carries GSTVD_EPI_ADAMW the
 * tile's epilogue does not store dW but runs the update of gstvd_adamw on its 256 x 256 weights straight from the
 * accumulators: g = alpha * acc * grad_scale; reads param / m / v, writes param / m / v and the bf16 shadow weights -- 26
 * bytes per weight instead of 4 (dW out) + 30 (AdamW pass), and the HBM-bound update runs under the MFMA-bound K-loops of the
 * other workgroups instead of after them.  Such a problem's C must point INTO the flat gradient buffer `grad_base` (its flat
 * index addresses param / m / v / shadow), with ldc % 4 == 0 and a flat index % 4 == 0; its `addend` field carries the DEVICE
 * address of the weight's (lr, weight decay) pair -- two consecutive floats, e.g. &hp[2 * segment] of gstvd_adamw's table, read at
 * run time so that a schedule step needs no new table; it carries no other epilogue flag than COLSUM / COLSUM_ACC.  write_grad
 * != 0 also stores dW (the `.grad` the caller may want to look at).  Problems without the flag get the plain epilogue.  Same
 * arithmetic per element as gstvd_gemm_grouped followed by gstvd_adamw: results are bit-identical. */
typedef struct {
  const float* grad_base; float* param; float* m; float* v; void* shadow_bf16;
  const float* step; float beta1, beta2, eps, grad_scale;
  int32_t write_grad;
} gstvd_adamw_fuse_t;
int gstvd_gemm_grouped_adamw(const gstvd_gemm_t* table_dev, const int32_t* tile_off_dev, int64_t nprob, int64_t total_tiles,
                             const gstvd_adamw_fuse_t* f, const int32_t* block_map_dev, int64_t nblocks, gstvd_stream_t s);
/* measurement support: the (mangled) symbol of the kernel gstvd_gemm_grouped_adamw launches (rocprofv3 traces key on it) */
int gstvd_gemm_grouped_adamw_kernel_name(char* buf, int32_t buf_len);

/* Decode step (one token per row, models/visual_dialog_model.py:87-92 with the KV cache of this build): the LayerNorm that
 * closes a BERT sub-layer (transformers 4.16.2 BertSelfOutput / BertOutput, eps 1e-12) folded into the Linear that consumes it:
 * C = epi(LN(A; gamma, beta, eps) . B^T) for M <= 16 rows, K <= 1024, bf16 operands; epilogue flags BIAS / ADD / GELU as in
 * gstvd_gemm.  y_out (or NULL): bf16 [M, ldy >= K] receives LN(A), the residual input of the sub-layer's closing Linear.
 * GSTVD_E_UNSUPPORTED for any other shape (the caller then runs gstvd_ln_fwd + gstvd_gemm). */
int gstvd_gemv_ln(const gstvd_gemm_t* g, const float* gamma, const float* beta, float eps, void* y_out, int64_t ldy, gstvd_stream_t s);
/* bit 0: gstvd_gemm_grouped honours GSTVD_EPI_COLSUM (always set: the producer / consumer kernel is the one it launches) */
int32_t gstvd_gemm_group_caps(void);
/* Measurement support: the (mangled) symbol of the device kernel that gstvd_gemm (splits <= 1) or gstvd_gemm_splitk
 * (splits >= 2) would launch for this descriptor -- the dispatch runs, the launch is replaced by recording its target.
 * bench.py's roofline.kernel comes from here.  Nothing is launched; pointers in the descriptor are not dereferenced. */
int gstvd_gemm_kernel_name(const gstvd_gemm_t* g, int32_t splits, char* buf, int32_t buf_len);
int gstvd_gemm_grouped_kernel_name(int32_t dtype_in, int32_t dtype_out, int32_t a_kmajor, int32_t b_kmajor, char* buf, int32_t buf_len);

/* ---- (ABI 9) NSP head of the discriminative enc_only model: poolers + fusion + bi_seq_relationship + 2-way softmax ------------
 * What evaluate_disc.py:79-83 ranks by, in ONE launch on the encoder's final activations:
 *   t0 = xt[b * t_rows * ldt + 0 .. H),  v0 = xv[b * v_rows * ldv + 0 .. Hv)       first token / region of batch row b, read in
 *                                                                                  place (models/vilbert_dialog.py:924,938)
 *   pt = relu(Wt t0 + bt),  pv = relu(Wv v0 + bv)                                  BertTextPooler / BertImagePooler, :915-941
 *   f  = pt * pv  (fusion 0, 'mul')  or  pt + pv  (fusion 1, 'sum')                BertPreTrainingHeads.forward, :1030-1033
 *                                                                                  (its Dropout is the identity in eval)
 *   z  = Wn f + bn                    -> z[b * ldz + 0..1], fp32                   cls.bi_seq_relationship, :1038
 *   prob0 = exp(z0 - m) / (exp(z0 - m) + exp(z1 - m)), m = max(z0, z1)  -> prob0[b]  F.softmax(.., 1)[:, 0], evaluate_disc.py:81-83
 * dtype = type of xt, xv, wt [Hb, ldwt >= H], wv [Hb, ldwv >= Hv]: GSTVD_BF16 (fp32 accumulation on the MFMA) or GSTVD_F32 (the
 * f32-input MFMA).  bt, bv [Hb], wn [2, ldwn >= Hb], bn [2] are fp32 in both; pt, pv and f never leave fp32 registers.
 * One workgroup owns 16 batch rows and all Hb columns: no cross-workgroup reduction, sums in a fixed order, bit-reproducible.
 * Constraints: B >= 1; H, Hv, Hb multiples of 16 and <= 1024; row strides multiples of 8 (bf16) / 4 (fp32) elements; every
 * pointer 16-byte aligned.  kernel_name (HOST pointer or NULL): receives the mangled symbol of the kernel the call launched. */
typedef struct {
  const void* xt; int64_t ldt; int64_t t_rows;
  const void* xv; int64_t ldv; int64_t v_rows;
  const void* wt; int64_t ldwt; const void* wv; int64_t ldwv;
  const float* bt; const float* bv; const float* wn; int64_t ldwn; const float* bn;
  float* z; int64_t ldz; float* prob0;
  int32_t B, H, Hv, Hb, dtype, fusion;
  char* kernel_name; int32_t kernel_name_len; int32_t reserved_;
} gstvd_nsp_head_t;
int gstvd_nsp_head(const gstvd_nsp_head_t* a, gstvd_stream_t s);

/* ---- training heads of the enc_only model (train_disc.py; entry points added, no signature changed: ABI stays 9) --------------
 * Row compaction.  The MLM and masked-region losses read only the masked rows; every other row's gradient is exactly zero, so
 * the heads run on the gathered rows and the [B*T, vocab] logits of the reference never exist.
 *   gather : dst[i, 0..H) = src[idx[i], 0..H),  i < n            (src [M, lds >= H], dst [n, ldd >= H]; idx outside [0, M): zeros)
 *   scatter: dst[idx[i], 0..H) (=|+=) src[i, 0..H)               (dst [M, ldd]; idx distinct -- one writer per row, no atomics)
 *            accumulate = 0: the FIRST writer of dst -- every row of dst[0..M) that no index names is zero filled;
 *            accumulate = 1: adds to what dst holds (the pooler also sends a gradient to row 0 of every batch row).
 * H % 4 == 0, strides % 4 == 0, n >= 1 (a zero-row launch is the caller's to skip). */
int gstvd_rows_gather(const void* src, int64_t lds, int64_t M, const int64_t* idx, int64_t n, int64_t H, int32_t dtype,
                      void* dst, int64_t ldd, gstvd_stream_t s);
int gstvd_rows_scatter(const void* src, int64_t lds, const int64_t* idx, int64_t n, int64_t H, int32_t dtype, void* dst,
                       int64_t ldd, int64_t M, int32_t accumulate, gstvd_stream_t s);

/* x[m, 0..N) *= a[m, 0..N) in place (both dtype, N % 4 == 0): d(GELU output) -> d(pre-activation) with the gelu' that the
 * GSTVD_EPI_GELU epilogue saved, for the head transforms whose LayerNorm follows the GELU directly (vilbert_dialog.py:955-959). */
int gstvd_rows_mul(void* x, int64_t ldx, const void* a, int64_t lda, int64_t M, int64_t N, int32_t dtype, gstvd_stream_t s);

/* Masked-region loss (models/vilbert_dialog.py:1496-1501): per row i of scores [rows, lds >= C] (dtype) against the fp32 target
 * row target[(target_row ? target_row[i] : i) * ldt + 0..C):
 *   row_loss[i] = sum_c t * (log t - log_softmax(scores[i])[c]), terms with t == 0 exactly 0 (torch.xlogy);  lse[i] saved;
 *   labels (int64 [rows] or NULL = all rows count): rows whose label != 1 give 0 and are not counted;
 *   stats[0] = sum_i row_loss[i], stats[1] = counted rows, stats[2] = stats[0] / stats[1]    (one block, fixed order).
 * Backward: dscores[i, c] = scale * (softmax(scores[i])[c] * sum_c t - t[c]), scale = gscale[0] (NULL: 1), / stats[1] with
 * `mean`; the row's ACTUAL target sum is used; columns [C, ldd) are zero filled.  Any C (1601: the tail is handled inside). */
int gstvd_kl_fwd(const void* scores, int64_t lds, const float* target, int64_t ldt, const int64_t* target_row,
                 const int64_t* labels, int64_t rows, int64_t C, int32_t dtype, float* row_loss, float* lse, float* stats,
                 gstvd_stream_t s);
int gstvd_kl_bwd(const void* scores, int64_t lds, const float* target, int64_t ldt, const int64_t* target_row,
                 const int64_t* labels, const float* lse, const float* stats, const float* gscale, int32_t mean,
                 int64_t rows, int64_t C, int32_t dtype, void* dscores, int64_t ldd, gstvd_stream_t s);

/* NSP head, training form (models/vilbert_dialog.py:1026-1041,1509-1510).  Forward = gstvd_nsp_head's arithmetic in the same
 * order (p = 0: the same z bits) with the Dropout(p) of BertPreTrainingHeads on the fused value, drawn at element b * Hb + n of
 * (rng, site), plus the soft-label loss:
 *   z = Wn drop(f) + bn;  row_loss[b] = -(l[b,0] * log_softmax(z[b])[0] + l[b,1] * log_softmax(z[b])[1]),  labels [B, ldl >= 2] fp32
 *   stats = (sum_b row_loss, B, sum / B);  saved for backward: pt, pv [B, Hb] fp32 (dense), keep [B, Hb] uint8 (1 = kept).
 * Backward of gscale[0] * stats[2] (gscale NULL: 1):
 *   dwn [2, lddwn], dbn [2] (=|+=, acc_w / acc_b), and the gradients in front of the two ReLUs dpt, dpv [B, lddp] (dtype);
 *   the labels' row sums are used as they are (soft labels [s, 1 - s], not assumed to add up to 1).
 * Constraints as gstvd_nsp_head; 0 <= p < 1.  The backward entry reads pt .. labels, wn, gscale and writes dwn .. dpv only. */
typedef struct {
  const void* xt; int64_t ldt; int64_t t_rows;
  const void* xv; int64_t ldv; int64_t v_rows;
  const void* wt; int64_t ldwt; const void* wv; int64_t ldwv;
  const float* bt; const float* bv; const float* wn; int64_t ldwn; const float* bn;
  const float* labels; int64_t ldl;
  float* z; int64_t ldz;
  float* pt; float* pv; uint8_t* keep; float* row_loss; float* stats;
  const float* gscale; float* dwn; int64_t lddwn; float* dbn; void* dpt; void* dpv; int64_t lddp;
  const uint64_t* rng; float p; uint32_t site;
  int32_t B, H, Hv, Hb, dtype, fusion, acc_w, acc_b;
  char* kernel_name; int32_t kernel_name_len; int32_t reserved_;
} gstvd_nsp_train_t;
int gstvd_nsp_train_fwd(const gstvd_nsp_train_t* a, gstvd_stream_t s);
int gstvd_nsp_train_bwd(const gstvd_nsp_train_t* a, gstvd_stream_t s);

/* ---- beam-search answer decoding (entry points added, no signature changed: ABI stays 9) --------------------------------------
 * The reference ships no beam search (its _reorder_cache, visual_dialog_decoder.py:177-181, is never called), so this is the
 * specification.  B dialog rows, K beams (1..8), V vocabulary; beam j of dialog b is decoder row b * K + j.  Per beam an fp32
 * score s[b,j] (the sum of its tokens' log-probabilities) and a flag done[b,j]; in front of the first generated position
 * s[b,0] = 0, s[b,j>0] = -inf, nothing done.
 * One step:
 *   a live beam j offers every v in [0, V) with score s[b,j] + logp_j[v],
 *       logp_j[v] = (z[v] - max z) - log sum_v exp(z[v] - max z)     in fp32 over the beam row's raw logits z (no temperature, no
 *                                                                    top-k / top-p);
 *   a done beam j offers exactly one candidate, (j, pad), with its score s[b,j] unchanged;
 *   the K best candidates of the dialog row become the new beams IN ORDER: higher score first, equal scores by smaller j, then by
 *       smaller v; scores of -inf sort last under the same index rule;
 *   new beam i:  parent[b,i] = j,  token = v -> ids_tm[pos * ids_stride + b*K + i]  (the TIME-MAJOR id buffer [positions,
 *       ids_stride >= B*K]: the next token step's embedding reads the row as it is),  score_out[b,i] = the candidate's score,
 *       done_out[b,i] = done_in[b,j] || v == eos.
 * logits [B*K, ld >= V] fp32 or bf16; score_in / score_out fp32 [B, K], done_in / done_out / parent int32 [B, K]; in and out state
 * are separate buffers (ping-pong, nothing is updated in place).  workspace: caller-owned, 8 * B * K * K bytes ([B, K, K] pairs of
 * (fp32 score, int32 token): the K best continuations of every live beam, which phase A -- one workgroup per beam row, the row in
 * registers -- leaves for phase B -- one wave per dialog row, which merges them under the rule).  Two launches, no allocation, no
 * synchronisation.  Refused before any launch: K outside 1..8 (GSTVD_E_SHAPE), V > 31744 (GSTVD_E_UNSUPPORTED), a null pointer. */
typedef struct {
  const void* logits; int64_t ld; int32_t dtype; int32_t B; int32_t K; int32_t V;
  const float* score_in; const int32_t* done_in;
  float* score_out; int32_t* done_out; int32_t* parent;
  int64_t* ids_tm; int64_t ids_stride; int32_t positions; int32_t pos;
  void* workspace;
  int32_t eos; int32_t pad;
} gstvd_beam_step_t;
int gstvd_beam_step(const gstvd_beam_step_t* a, gstvd_stream_t s);

/* The self-attention caches of the surviving beams, all decoder layers in ONE launch: for every layer l < n_layers
 *   dst[l][b*K + i, 0..t, H..3H) = src[l][b*K + parent[b,i], 0..t, H..3H)
 * over the fused Q|K|V caches [B*K, Umax, ld >= 3H] (row_stride >= Umax * ld elements between decoder rows): only the K and V
 * columns move, only positions <= t; the Q columns and later positions of dst are left alone, src is only read.  src[l] != dst[l]:
 * the caller keeps two cache sets that swap roles every step, so a permutation never reads a row it has already overwritten.
 * 16-byte copies: H * sizeof(T), ld * sizeof(T), row_stride * sizeof(T) and every pointer multiples of 16 (GSTVD_E_ALIGN). */
typedef struct {
  const void* src[16]; void* dst[16];
  const int32_t* parent;
  int64_t row_stride; int64_t ld;
  int32_t n_layers; int32_t B; int32_t K; int32_t H; int32_t Umax; int32_t t; int32_t dtype; int32_t reserved_;
} gstvd_beam_reorder_t;
int gstvd_beam_reorder(const gstvd_beam_reorder_t* a, gstvd_stream_t s);

/* ---- self-training glue (entry points added, no signature changed: ABI stays 9) ------------------------------------------------
 * Both entries are one launch each, without atomics, workspace, allocation or host synchronisation (capture-safe).
 *
 * gstvd_context_append: the context splice of the generation loop (generate.py:145-160, 214-228) for all B rows at once.
 * ctx_ids int64 [B, T] (row stride ld_ctx), segments int64 [B, T] or NULL, att_mask fp32 [B, T] or NULL, ctx_len int64 [B],
 * new_ids int64 [B, U] (row stride ld_new), n_out int64 [B] or NULL, abnormal / full int32 [B].  Row b:
 *   n = the number of non-zero entries of new_ids[b],  start = ctx_len[b];
 *   start + n <= T:  ctx_ids[b, start + c] = new_ids[b, c] for c < n -- the FIRST n entries, a zero among them included (the
 *                    reference copies ids[:n]);  n_eff = n;
 *   else start < T:  ctx_ids[b, start] = sep_id;  n_eff = 1;  abnormal[b] = 1;
 *   else (the context is full already):  nothing of the row is written;  n_eff = 0;  abnormal[b] = full[b] = 1  (the reference
 *                    raises here; the caller reads `full` once, after its loop, and raises then).  A negative ctx_len[b] is
 *                    handled as a full row;
 *   over [start, start + n_eff):  segments = segment_value when given,  att_mask[p] = (ctx_ids[b, p] != 0) when given;
 *   ctx_len[b] += n_eff;  n_out[b] = n_eff when given.
 * abnormal is OR-ed and full is set: the kernel never clears either.  Refused before the launch: a null required pointer
 * (GSTVD_E_NULL); T < 1, U < 1 or a row stride below its row (GSTVD_E_SHAPE). */
typedef struct {
  int64_t* ctx_ids; int64_t ld_ctx;
  int64_t* segments; int64_t ld_seg;
  float* att_mask; int64_t ld_att;
  int64_t* ctx_len;
  const int64_t* new_ids; int64_t ld_new;
  int64_t B; int64_t T; int64_t U;
  int64_t sep_id; int64_t segment_value;
  int64_t* n_out; int32_t* abnormal; int32_t* full;
} gstvd_context_append_t;
int gstvd_context_append(const gstvd_context_append_t* a, gstvd_stream_t s);

/* gstvd_dialog_rows: the student's train rows of B generated dialogs of R rounds -- what dataloader/dataloader_cc12m_gen.py:104-248
 * builds through utils/data_utils.py:34-71 (encode_input) from re-tokenised text, computed from the token ids for all B * R rows.
 * Inputs: cap int64 [B, Lc] (row stride ld_cap); ques, ans int64 [B, R, U] (row stride ld_utt between the B * R rows); ppl fp32
 * [B, R]; valid int32 [B] or NULL; u_tok fp32 [B, R, T] (row stride ld_u; may be NULL when mask_prob == 0).
 * Outputs, over the B * R rows: enc_ids, enc_seg, enc_mlm int64 [., T] and enc_att fp32 [., T] (row stride ld_enc, in elements of
 * each); enc_sep int64 [., S] (ld_sep); enc_hist_len int64 [.]; dec_ids, dec_labels int64 [., Ud] and dec_att fp32 [., Ud]
 * (ld_dec).  Every output element is written exactly once: nothing needs zeroing in front.
 *   Utterances.  The caption: the entries of cap[b] in front of its first zero.  Question / answer k: the entries of ques[b, k] /
 *     ans[b, k] that are not among special[0 .. n_special), in order (what tokenizer.decode(skip_special_tokens=True) keeps).  An
 *     utterance may be empty.
 *   Context of round j (0-based): caption, q0, a0, ..., q(j-1), a(j-1), qj -- 2j + 2 utterances, answers uncut -- under
 *     encode_input with start_segment 1: [CLS] opens the row, every utterance is followed by [SEP], the segment starts at 1 and
 *     flips after every utterance ([CLS] and each [SEP] carry their utterance's segment), the row is cut at T (which may lose the
 *     last [SEP]) and padded with 0.  enc_sep: the running positions of the separators, the first S of them, 0-padded, NOT cut at
 *     T (positions >= T are listed).  enc_hist_len = 2j + 1.  enc_att = (enc_ids != 0), after the masking.
 *   Mask noise.  An utterance token at (untruncated) position p < T is masked iff (double)u_tok[b, j, p] < mask_prob (strict, in
 *     double): enc_ids = mask, enc_mlm = the token (no 80 / 10 / 10 rule).  Everything else -- [CLS], [SEP], padding -- has
 *     enc_mlm = -1.
 *   Target of round j.  The answer's first Ud - 2 tokens; dec_ids = [CLS] answer [SEP], 0-padded to Ud; dec_att = (dec_ids != 0)
 *     at this point (1 through the [SEP] slot); dec_labels = dec_ids shifted left by one -- all 0 when
 *     select_data && (double)ppl[b, j] >= threshold (literal: a NaN perplexity keeps its labels) or when valid is given and
 *     valid[b] == 0; last, [SEP] -> 0 in dec_ids.
 * Refused before the launch: a null required pointer, mask_prob > 0 without u_tok (GSTVD_E_NULL); R < 1, 2R > S, R > 32, U or Lc
 * outside 1..64, T < 2, Ud < 3, n_special outside 0..8, a row stride below its row (GSTVD_E_SHAPE). */
typedef struct {
  const int64_t* cap; int64_t ld_cap;
  const int64_t* ques; const int64_t* ans; int64_t ld_utt;
  const float* ppl; const int32_t* valid;
  const float* u_tok; int64_t ld_u;
  int64_t* enc_ids; int64_t* enc_seg; int64_t* enc_mlm; float* enc_att; int64_t ld_enc;
  int64_t* enc_sep; int64_t ld_sep; int64_t* enc_hist_len;
  int64_t* dec_ids; int64_t* dec_labels; float* dec_att; int64_t ld_dec;
  double mask_prob; double threshold;
  int64_t cls; int64_t sep; int64_t mask; int64_t special[8];
  int32_t B; int32_t R; int32_t U; int32_t Lc; int32_t T; int32_t S; int32_t Ud; int32_t n_special; int32_t select_data;
  int32_t reserved_;
} gstvd_dialog_rows_t;
int gstvd_dialog_rows(const gstvd_dialog_rows_t* a, gstvd_stream_t s);

/* ---- vocabulary arg-max of the masked-LM fill-in (utils/text_attack.py:30-56; entry points added, no signature changed: ABI
 * stays 9).  One total order in both forms: the larger value wins, equal values go to the SMALLER column.  Inputs are assumed
 * finite: a NaN never wins, and a row without a single finite-or-infinite winner reports column 0 with value -inf.
 *
 * rows_argmax: logits [n, ld >= V] (GSTVD_F32 or GSTVD_BF16) -> idx[r] = arg-max over columns 0..V-1 (int64), val[r] its value
 * (fp32).  Columns V..ld-1 are never read.  n >= 1 (a zero-row launch is the caller's to skip).
 *
 * vocab_argmax: the tied decoder's product fused in.  X [n, ldx >= H] bf16, W [>= V, ldw >= H] bf16 row-major (one table row per
 * vocabulary entry, the "NT" form), bias fp32 [>= V]:
 *     z[r, v] = (sum_k x[r, k] * w[v, k], accumulated in fp32) + bias[v] in fp32;   idx[r], val[r] as above over v = 0..V-1.
 * The [n, V] logits are never stored: a first launch of MFMA tiles (64 rows x 64 vocabulary columns) leaves one (value, column)
 * pair per row and tile in `ws` ([n, ceil(V / 64)] pairs of 8 bytes, gstvd_vocab_argmax_ws_bytes(n, V) bytes, 8-byte aligned), a
 * second launch reduces a row's pairs.  No atomics: the result is deterministic.  Table rows and bias entries at or beyond V are
 * never read.  GSTVD_E_UNSUPPORTED for a dtype other than GSTVD_BF16, an H that is no multiple of 32, n > 2^20 or V > 2^30: the
 * caller then runs gstvd_gemm into a [n, >= V] buffer and gstvd_rows_argmax (also the fp32-precision path).  ldx, ldw multiples of
 * 8 and X, W 16-byte aligned (GSTVD_E_ALIGN); ws_bytes below the helper's answer, n < 1, V < 1: GSTVD_E_SHAPE. */
int gstvd_rows_argmax(const void* logits, int64_t ld, int64_t n, int64_t V, int32_t dtype, int64_t* idx, float* val,
                      gstvd_stream_t s);
int64_t gstvd_vocab_argmax_ws_bytes(int64_t n, int64_t V);
int gstvd_vocab_argmax(const void* X, int64_t ldx, const void* W, int64_t ldw, const float* bias, int64_t n, int64_t V, int64_t H,
                       int32_t dtype, void* ws, int64_t ws_bytes, int64_t* idx, float* val, gstvd_stream_t s);

/* ---- soft pseudo-labels of the self-training loop (entry points added, no signature changed: ABI stays 9) ------------------------
 * The reference closes its self-training loop through JSON text and hands the student one sampled token per position; this is the
 * build's own rule.  The teacher hands over the K best tokens of every position with their log-probabilities (sparse: 12 K bytes
 * per token), the student trains on the hard-label cross entropy mixed with the KL divergence to that distribution.
 *
 * topk_logp (teacher): per row m of logits [M, ldl >= V] (GSTVD_F32 or GSTVD_BF16) with lse[m] as gstvd_ce_fwd saved it:
 *   ids [M, K] int64, logp [M, K] fp32 (dense), logp = x[id] - lse[m] in fp32; the K largest entries of the row under the total order
 *   (value descending, then smaller id), best first; -inf logits take part in the same order, so a row with fewer than K finite
 *   values ends in -inf entries.  Inputs are assumed free of NaN (a NaN never wins).  The row is read once and lives in registers.
 *   K < 1, K > 16 or K > V: GSTVD_E_SHAPE; V > 32768: GSTVD_E_UNSUPPORTED; ldl, alignment and dtype as the cross-entropy entries.
 *
 * distill_fwd (student), after gstvd_ce_fwd on the same logits and labels, whose row_loss it takes as ce_row_loss:
 *   a token is KEPT exactly when the cross entropy keeps it (label != ignore_index and inside [0, V)); a kept token HAS A SOFT LABEL
 *   when soft_ids[m, 0] >= 0 and every one of its K ids lies in [0, V) (no logit is ever read through an id outside it).
 *   Kept with a soft label:  q = softmax_k(soft_logp[m, :] * inv_tau) over the K entries (fp32, max-subtracted),
 *     lse_tau[m] = logsumexp_v(x[m, v] * inv_tau) over the full vocabulary,
 *     row_kd[m]  = sum_k q_k * (log q_k - (x[m, id_k] * inv_tau - lse_tau[m])), terms with q_k == 0 exactly 0;
 *   elsewhere row_kd[m] = lse_tau[m] = 0.  Duplicate ids in one row count as separate entries.
 *   row_loss[m] = (1 - a_m) * ce_row_loss[m] + a_m * tau^2 * row_kd[m], a_m = alpha where the token has a soft label, 0 otherwise
 *   (a_m == 0: ce_row_loss[m] itself, bit for bit);  stats_out = [sum of row_loss, rows with label != ignore_index, their quotient]
 *   by the cross entropy's reduction, so stats_out[1] is its stats[1].  soft_ids [M, K] int64, soft_logp [M, K] fp32, dense.
 *   1 <= K <= 16, 0 <= alpha <= 1, 0 < inv_tau < inf, else GSTVD_E_SHAPE; ldl, alignment, dtype as the cross-entropy entries.
 *
 * distill_bwd: ONE launch writes dlogits [M, ldd] once; gs = gscale[0] (NULL: 1), count = stats[1]:
 *   d[m, v] = gs / count * ( (1 - a_m) * (softmax(x)[v] - [v == label]) + a_m * tau * (softmax(x / tau)[v] - sum_k q_k [v == id_k]) )
 *   columns V..ldd-1 zero filled, rows that are not kept stored as zeros; a token with a_m == 0 goes through the cross entropy's own
 *   row routine: its row is the bits gstvd_ce_bwd's mean form writes.  lse as gstvd_ce_fwd saved it, lse_tau as distill_fwd did. */
int gstvd_topk_logp(const void* logits, int64_t ldl, const float* lse, int64_t M, int64_t V, int64_t K, int32_t dtype, int64_t* ids,
                    float* logp, gstvd_stream_t s);
int gstvd_distill_fwd(const void* logits, int64_t ldl, const int64_t* labels, const int64_t* soft_ids, const float* soft_logp,
                      int64_t M, int64_t V, int64_t K, int64_t ignore_index, float alpha, float inv_tau, int32_t dtype,
                      const float* ce_row_loss, float* row_loss, float* row_kd, float* lse_tau, float* stats_out, gstvd_stream_t s);
int gstvd_distill_bwd(const void* logits, int64_t ldl, const int64_t* labels, const int64_t* soft_ids, const float* soft_logp,
                      const float* lse, const float* lse_tau, const float* stats, const float* gscale, int64_t M, int64_t V,
                      int64_t K, int64_t ignore_index, float alpha, float inv_tau, int32_t dtype, void* dlogits, int64_t ldd,
                      gstvd_stream_t s);

/* ---- coreference text attack (utils/text_attack.py:58-116; entry points added, no signature changed: ABI stays 9) ---------------
 * cos_topk: the K nearest neighbours by cosine of n source rows of a table of UNIT rows, without the V x V matrix the reference
 * stores.  Ehat fp32 [>= V, ld >= D] row-major; src int32 [n], or NULL: source r is row r and n must equal V.
 *   idx int32 [n, K], val fp32 [n, K] (dense): row r holds the K best targets t in [0, V), t != src[r], with
 *   dot(Ehat[src[r]], Ehat[t]) >= threshold, under ONE total order -- the larger value first, equal values to the SMALLER index (the
 *   order of the vocabulary arg-max above) -- best first; unused slots hold idx = -1, val = 0.  threshold = -inf: no cut.  A source
 *   index outside [0, V) reads no memory and gives a row of unused slots.  Inputs are assumed finite.  Columns D..ld-1 and rows at
 *   or beyond V are never read.
 * The products run on the f32-input MFMA (exact fp32, one rounding per product).  A pair's D products are added in one fixed order
 * (k = 16 s + 4 g + e: s ascending, then e = 0..3, then g = 0..3) on both routes, so both return the same bits:
 *   GSTVD_COS_TOPK_MANY: a workgroup owns 32 source rows and streams all V targets past them, keeping every row's running K best;
 *                        the workspace is not used (ws may be NULL);
 *   GSTVD_COS_TOPK_FEW : the targets are split over workgroups; every split leaves a partial list per row in `ws`
 *                        (gstvd_cos_topk_ws_bytes(n, V, K) bytes, 8-byte aligned), a second launch merges them;
 *   GSTVD_COS_TOPK_AUTO: gstvd_cos_topk_route(n, V) -- MANY from 16384 source rows on, where its workgroups alone fill the chip.
 * No atomics, every output element is written once, the result does not depend on the order workgroups finish in.
 * Refused before the launch: a null Ehat / idx / val, or ws on the FEW route (GSTVD_E_NULL); n < 1, V < 1, D < 1, ld < D, K outside
 * 1..16, src NULL with n != V, a NaN threshold, an unknown route, ws_bytes below the helper's answer (GSTVD_E_SHAPE); D > 512 (the
 * source rows of a workgroup live in LDS; 300, the counter-fitted vectors' width, fits), V or n > 2^30 (GSTVD_E_UNSUPPORTED); D or
 * ld no multiple of 4, Ehat not 16-byte aligned (GSTVD_E_ALIGN). */
enum { GSTVD_COS_TOPK_AUTO = 0, GSTVD_COS_TOPK_MANY = 1, GSTVD_COS_TOPK_FEW = 2 };
int32_t gstvd_cos_topk_route(int64_t n, int64_t V);
int64_t gstvd_cos_topk_ws_bytes(int64_t n, int64_t V, int32_t K);
int gstvd_cos_topk(const float* Ehat, int64_t ld, int64_t V, int64_t D, const int32_t* src, int64_t n, int32_t K, float threshold,
                   int32_t route, void* ws, int64_t ws_bytes, int32_t* idx, float* val, gstvd_stream_t s);

/* subseq_replace: substitutions of wordpiece id sequences inside one utterance of a context row, all rows in one launch, one
 * workgroup per row; the attack's substitute_word (utils/text_attack.py:93-100) on ids instead of decoded text.
 * Row r's substitutions are subs[row_ptr[r] .. row_ptr[r + 1]) (row_ptr int32 [n + 1]); substitution i is the four int32
 * subs[4 i ..] = (u, off, La, Lb): inside utterance u replace a = pieces[off .. off + La) by b = pieces[off + La .. off + La + Lb)
 * (pieces int64 [n_pieces]), 1 <= La, Lb <= 16.  An entry outside these bounds is skipped, never read through.
 *  1. a row's substitutions apply in order, each to the result of the one before;
 *  2. utterance u is the tokens strictly between the u-th and the (u + 1)-th `sep` of the row as it stands; for u = 0 the left
 *     boundary is position 0 (where `cls` stands; the position is the boundary whatever it holds).  Fewer than u + 1 separators:
 *     the substitution does nothing;
 *  3. matches are taken left to right, greedy, non-overlapping, wholly inside the utterance.  With cont (uint8 [n_vocab], 1 for a
 *     "##" continuation piece; ids outside [0, n_vocab) count as 0) a match also needs cont[first matched token] == 0 and the token
 *     behind the match to be the utterance's end or a piece with cont == 0;
 *  4. every match is replaced by b, the tail shifts, tokens pushed past T are dropped, a shorter row is filled with `pad`;
 *  5. out_ids int64 [n, ld_out >= T] and n_replaced int32 [n] (matches replaced, all substitutions of the row) are always written;
 *  6. segments int64, sep_indices int64 [n, ld_sep >= max_sep], att_mask fp32 are written when non-NULL, recomputed from out_ids
 *     by encode_input's rules (utils/data_utils.py:41-71): segments[q] = start_seg[r * ld_start] (NULL: 0) XOR (number of
 *     separators in front of q, mod 2), 0 on pads; sep_indices = the first max_sep separator positions, then 0; att_mask =
 *     (out_ids != pad).
 * No atomics, no workspace, every output element written once; ids is never written (ids == out_ids is refused).
 * Refused before the launch: null ids / out_ids / n_replaced / row_ptr, null subs or pieces with n_subs > 0 (GSTVD_E_NULL); n < 1,
 * T < 1, a row stride below its row, cont with n_vocab < 1, sep_indices with max_sep < 1 (GSTVD_E_SHAPE); T > 1024
 * (GSTVD_E_UNSUPPORTED). */
typedef struct {
  const int64_t* ids; int64_t ld_ids;
  int64_t* out_ids; int64_t ld_out; int32_t* n_replaced;
  const int32_t* row_ptr; const int32_t* subs; const int64_t* pieces;
  const uint8_t* cont; int64_t n_vocab;
  int64_t cls; int64_t sep; int64_t pad;
  int64_t* segments; int64_t ld_seg; const int64_t* start_seg; int64_t ld_start;
  int64_t* sep_indices; int64_t ld_sep; float* att_mask; int64_t ld_att;
  int32_t n; int32_t T; int32_t n_subs; int32_t n_pieces; int32_t max_sep; int32_t reserved_;
} gstvd_subseq_replace_t;
int gstvd_subseq_replace(const gstvd_subseq_replace_t* a, gstvd_stream_t s);

/* ---- discriminative rows (entry point added, no signature changed: ABI stays 9) ------------------------------------------------
 * gstvd_disc_rows: N rows of the discriminative (enc_only) model -- what dataloader/dataloader_visdial_disc.py builds per dialog
 * with a tokenizer and Python lists (train rows :125-288, eval rows :299-401) through utils/data_utils.py:34-71 (encode_input) --
 * from token-id pools, in ONE launch without atomics, workspace, allocation or host synchronisation (capture-safe).  Every output
 * element is written exactly once: nothing needs zeroing in front.
 * Pools (int64, 0-padded, no [CLS] / [SEP] inside): cap [D, Lc] (row stride ld_cap); ques, ans [D, R, U] (row stride ld_utt
 * between the D * R rows; ans = the ground-truth answers); opts [D, R, O, U] (row stride ld_opt between the D * R * O rows);
 * gt_index int64 [D, R]; dense_scores double [D, R, O] or NULL.  An utterance is the entries in front of the row's first 0 (all of
 * them when there is none); it may be empty and then contributes a lone [SEP].
 * Row list: row_dialog, row_round, row_slot int32 [N].  Uniforms: u_tok fp32 [N, T] (row stride ld_u; may be NULL when
 * mask_prob == 0), u_neg fp32 [N] (train mode).
 * Outputs over the N rows: tokens, segments, mask int64 [N, T] and att fp32 [N, T] (one row stride ld_row, in elements of each);
 * sep_indices int64 [N, S] (ld_sep); hist_len int64 [N]; neg_option int32 [N]; nsp_labels fp32 [N, 2] (contiguous).
 *   Row (d, j, x): the utterances caption, q0, a0, ..., q(j-1), a(j-1), qj, x -- 2j + 3 of them.
 *   pruneRounds (:84-93) with tot_rounds: j + 2 > tot_rounds drops the first 2j + 3 - 2 * tot_rounds utterances and the row starts at
 *     segment 0; otherwise nothing is dropped and it starts at segment 1.  hist_len = (utterances kept) - 1.
 *   encode_input: [CLS] opens the row, every utterance is followed by [SEP], the segment flips after every utterance ([CLS] and each
 *     [SEP] carry their utterance's segment), the row is cut at T (which may lose the last [SEP], or more) and padded with 0
 *     (segments 0, mask -1).  sep_indices: the running separator positions, 0-padded to S, NOT cut at T.
 *   att[t] = (t < sep_indices[hist_len] + 1): train_disc.py:97-99 (sequence_mask of the row's untruncated length).
 *   [MASK] noise: an utterance token at position p < T is masked iff (double)u_tok[r, p] < mask_prob (strict, in double): tokens =
 *     mask_id and mask = the original id (no 80 / 10 / 10 rule); everything else has mask = -1.
 *   Eval mode (train == 0; :299-326): x = option c of round j with c = gt if slot == 0, else the (slot - 1)-th index of
 *     {0..O-1} \ {gt} in increasing order; 0 <= slot < num_options.  neg_option[r] = c; nsp_labels is not touched (may be NULL).
 *   Train mode (train != 0; :125-183, 218-246):
 *     slot 0: x = ans[d, j];  neg_option = -1;  nsp_labels = [1, 0].
 *     slot >= 1: a negative.  Candidates C = the first num_options - 1 indices of {0..O-1} \ {gt}.
 *       tot_len = len(cap) + 2 + sum over k <= j of (len q_k + 1 + len a_k + 1) -- the loader's running length, which counts the
 *       ground-truth answer of round j although the negative replaces it (kept as it is).  c in C is feasible iff
 *       T >= tot_len + len(opt_c) + 1.  With F = the feasible candidates in increasing order and u = u_neg[r]:
 *         F not empty:  c = F[min(floor((double)u * |F|), |F| - 1)], x = opt_c whole;
 *         F empty:      c = C[min(floor((double)u * |C|), |C| - 1)], x = the first len(a_j) tokens of opt_c
 *       (a negative index counts as 0).  The loader's random.choice / remove loop draws c from the same distribution -- the first
 *       feasible element of a uniform random permutation of C, or its last element when none is feasible -- from another stream.
 *       neg_option = c;  nsp_labels = [0, 1], or with dense_scores [(float)s, (float)(1.0 - s)], s = dense_scores[d, j, c], the
 *       subtraction in double (torch.tensor([score, 1.0 - score]), :240-243).
 *   A row whose d, j or slot is out of range, or whose gt_index[d, j] is outside [0, O), reads no pool: it is written as padding
 *     (tokens, segments, att, sep_indices, hist_len 0; mask -1; neg_option -1; nsp_labels [0, 0]).
 * Limits: 1 <= U, Lc <= 64; R >= 1 and 2R + 1 <= S <= 64 (S = 25, the loader's max_sep_len: R <= 12); 2 <= num_options <= O <= 100;
 * tot_rounds >= 1; T >= 2.  Refused before the launch, nothing written: a null required pointer, mask_prob > 0 without u_tok, train
 * mode without u_neg or nsp_labels (GSTVD_E_NULL); a shape outside the limits, N < 0 or above 2^31 - 1, a row stride below its row
 * (GSTVD_E_SHAPE). */
typedef struct {
  const int64_t* cap; int64_t ld_cap;
  const int64_t* ques; const int64_t* ans; int64_t ld_utt;
  const int64_t* opts; int64_t ld_opt;
  const int64_t* gt_index; const double* dense_scores;
  const int32_t* row_dialog; const int32_t* row_round; const int32_t* row_slot;
  const float* u_tok; int64_t ld_u; const float* u_neg;
  int64_t* tokens; int64_t* segments; int64_t* mask; float* att; int64_t ld_row;
  int64_t* sep_indices; int64_t ld_sep; int64_t* hist_len;
  int32_t* neg_option; float* nsp_labels;
  double mask_prob;
  int64_t cls; int64_t sep; int64_t mask_id;
  int64_t N;
  int32_t D; int32_t R; int32_t O; int32_t U; int32_t Lc; int32_t T; int32_t S;
  int32_t tot_rounds; int32_t num_options; int32_t train;
} gstvd_disc_rows_t;
int gstvd_disc_rows(const gstvd_disc_rows_t* a, gstvd_stream_t s);

/* ---- generative rows (entry point added, no signature changed: ABI stays 9) -----------------------------------------------------
 * gstvd_gen_rows: the rows of the generative (enc_dec) model -- what dataloader/dataloader_visdial_gen.py builds per dialog with a
 * tokenizer and Python lists (eval rows :295-458, test rows :507-603, teacher rows :123-293) through utils/data_utils.py:34-71
 * (encode_input) -- from token-id pools, in ONE launch without atomics, workspace, allocation or host synchronisation
 * (capture-safe).  Every output element is written exactly once: nothing needs zeroing in front.
 * Pools (int64, 0-padded, no [CLS] / [SEP] inside): cap [D, Lc] (row stride ld_cap); ques, ans [D, R, U] (row stride ld_utt
 * between the D * R rows; ans = the ground-truth answers); opts [D, Ro, O, U] with Ro == R or Ro == 1 (row stride ld_opt between
 * the D * Ro * O rows); gt_index int64 [D, R].  opts is read in the modes EVAL and TEST only, gt_index in EVAL only; each may be
 * NULL elsewhere.  An utterance is the entries in front of the row's first 0 (all of them when there is none); it may be empty and
 * then contributes a lone [SEP].
 * One launch takes two independent row lists; either may be empty (n == 0), and then its pointers may be NULL.
 * Encoder rows: enc_dialog, enc_round int32 [n_enc]; u_tok fp32 [n_enc, T] (row stride ld_u; may be NULL when mask_prob == 0).
 *   Outputs: tokens, segments, mlm int64 [n_enc, T] and att fp32 [n_enc, T] (one row stride ld_row, in elements of each);
 *   sep_indices int64 [n_enc, S] (ld_sep); hist_len int64 [n_enc].
 *   Context of (d, j): caption, q0, a0, ..., q(j-1), a(j-1), qj -- 2j + 2 utterances; in mode TRAIN_Q caption, q0, a0, ...,
 *     a(j-1) -- 2j + 1 utterances (the questioner's context ends at the previous answer).  hist_len = utterances - 1.  The gen
 *     loader never calls pruneRounds: the row starts at segment 1 and nothing is dropped.
 *   encode_input: [CLS] opens the row, every utterance is followed by [SEP], the segment flips after every utterance ([CLS] and each
 *     [SEP] carry their utterance's segment), the row is cut at T (which may lose the last [SEP], or more) and padded with 0
 *     (segments 0, mlm -1).  sep_indices: the running separator positions, 0-padded to S, NOT cut at T.
 *   [MASK] noise: an utterance token at position p < T is masked iff (double)u_tok[r, p] < mask_prob (strict, in double): tokens =
 *     mask_id and mlm = the original id (no 80 / 10 / 10 rule); everything else has mlm = -1.
 *   att[t] = (tokens[t] != 0), after the noise.
 *   A row whose d or j is out of range reads no pool: it is written as padding (tokens, segments, att, sep_indices, hist_len 0;
 *     mlm -1).
 * Decoder rows: dec_dialog, dec_round, dec_slot int32 [n_dec].
 *   Outputs: dec_ids int64 [n_dec, Ud] and dec_att fp32 [n_dec, Ud] (one row stride ld_dec); dec_option int32 [n_dec]; in the train
 *   modes dec_labels int64 [n_dec, Ud] (ld_dec; not touched and may be NULL otherwise).
 *   The target x, cut to its first Ud - 2 tokens; the row is [CLS] x [SEP], 0-padded to Ud; dec_att = (row != 0) at this point.
 *     GSTVD_GEN_EVAL (:303-355, :390-399): x = option c of round j with c = gt if slot == 0, else the (slot - 1)-th index of
 *       {0..O-1} \ {gt} in increasing order; 0 <= slot < num_options; dec_option = c; dec_ids = the row ([SEP] kept).
 *     GSTVD_GEN_TEST (:519-557): x = option `slot` of round j (of the pool's only round when Ro == 1), original order; 0 <= slot <
 *       num_options; gt_index is not read; dec_option = slot; dec_ids = the row.
 *     GSTVD_GEN_TRAIN_A (:164-169, :226-230): x = ans[d, j]; the slot must be 0; dec_option = -1; dec_labels[:-1] = row[1:],
 *       dec_labels[-1] = 0; then every element of dec_ids equal to sep becomes 0.
 *     GSTVD_GEN_TRAIN_Q (:142-147): x = ques[d, j]; otherwise as TRAIN_A.
 *   A row whose d, j or slot is out of range, or (EVAL) whose gt_index[d, j] is outside [0, O), reads no pool: it is written as
 *     padding (dec_ids, dec_att, dec_labels 0; dec_option -1).
 * Limits: 1 <= U, Lc <= 64; R >= 1 and 2R <= S <= 64 (S = 25, the loader's max_sep_len: R <= 12); T >= 2; Ud >= 3; in EVAL and TEST
 * 2 <= num_options <= O <= 100 and Ro in {R, 1}.  Refused before the launch, nothing written, in this order: a null required pointer,
 * mask_prob > 0 without u_tok (GSTVD_E_NULL); a mode that is none, a shape outside the limits, n_enc or n_dec < 0 or their sum above
 * 2^31 - 1 (GSTVD_E_SHAPE); a row stride below its row (GSTVD_E_SHAPE). */
enum { GSTVD_GEN_EVAL = 0, GSTVD_GEN_TEST = 1, GSTVD_GEN_TRAIN_A = 2, GSTVD_GEN_TRAIN_Q = 3 };
typedef struct {
  const int64_t* cap; int64_t ld_cap;
  const int64_t* ques; const int64_t* ans; int64_t ld_utt;
  const int64_t* opts; int64_t ld_opt;
  const int64_t* gt_index;
  const int32_t* enc_dialog; const int32_t* enc_round;
  const float* u_tok; int64_t ld_u;
  int64_t* tokens; int64_t* segments; int64_t* mlm; float* att; int64_t ld_row;
  int64_t* sep_indices; int64_t ld_sep; int64_t* hist_len;
  const int32_t* dec_dialog; const int32_t* dec_round; const int32_t* dec_slot;
  int64_t* dec_ids; int64_t* dec_labels; float* dec_att; int64_t ld_dec;
  int32_t* dec_option;
  double mask_prob;
  int64_t cls; int64_t sep; int64_t mask_id;
  int64_t n_enc; int64_t n_dec;
  int32_t D; int32_t R; int32_t Ro; int32_t O; int32_t U; int32_t Lc; int32_t T; int32_t S; int32_t Ud;
  int32_t num_options; int32_t mode; int32_t reserved_;
} gstvd_gen_rows_t;
int gstvd_gen_rows(const gstvd_gen_rows_t* a, gstvd_stream_t s);

/* ---- ranking metrics (entry point added, no signature changed: ABI stays 9) ------------------------------------------------------
 * gstvd_rank_metrics: L score lists of O options -> the rank of every option, the rank of the ground truth, the NDCG ratio of the
 * list and additions to a device-resident accumulator: what utils/visdial_metrics.py computes on the host per batch
 * (scores_to_ranks :21-39, SparseGTMetrics :41-117, NDCG :119-195).  No workspace, allocation or host synchronisation; safe to
 * capture, and a captured call may be replayed on other contents.  Every output element is written exactly once; the accumulator is
 * only ever added to, in stream order.
 * Operands: scores fp32 [L, O] (dense rows, row stride ld_scores); gt_index int64 [L] or NULL; relevance fp32 [n_rel, O] (dense
 * rows, row stride ld_rel) or NULL; rel_index int32 [L] or NULL: the relevance row of list l, -1 = none; NULL = row l (then
 * n_rel == L); discounts fp32 [n_discounts >= O], required with relevance: discounts[p] = log2(p + 2), computed by the caller on the
 * host (torch.log2(torch.arange(O).float() + 2)) so that no device log2 enters a result.
 * Outputs, each may be NULL: ranks int64 [L, O] (row stride ld_ranks); gt_rank int32 [L] (needs gt_index); ndcg fp32 [L] (needs
 * relevance, and relevance needs it); acc int64 [GSTVD_RANK_ACC_SLOTS].
 *   Rank rule: the stable descending sort.  Keys compare as fp32 values, except that NaN is the largest key with all NaNs equal,
 *     and -0.0 == +0.0.   rank[i] = 1 + #{j : key_j > key_i} + #{j < i : key_j == key_i}
 *     (= torch.sort(dim=1, descending=True, stable=True); the reference's scores.sort(1, descending=True) is not stable, so the rank
 *     of tied options is implementation-defined there).
 *   Sparse rule: 0 <= gt_index[l] < O: gt_rank[l] = rank[gt_index[l]], acc[N_SPARSE] += 1, acc[HIST + gt_rank[l]] += 1.
 *     Otherwise gt_rank[l] = 0, acc[N_GT_SKIPPED] += 1 and the histogram is unchanged.  Without gt_index none of this happens.
 *   NDCG rule, list l with relevance row r = rel_index[l] (or l), 0 <= r < n_rel:  k = #{i : rel[r, i] != 0};
 *       dcg   = sum over p = 0 .. k-1 of rel[r, option of rank p + 1] / discounts[p]
 *       ideal = the same sum with the options ordered by the rank rule applied to rel[r, :]
 *     every term ONE fp32 division; the terms added in ascending p, sequentially, in double; each sum then rounded to fp32;
 *     ndcg[l] = the fp32 quotient dcg / ideal.  k == 0: ndcg[l] = NaN (the reference's 0 / 0).  A finite ndcg[l] adds 1 to
 *     acc[N_NDCG]; a non-finite one (k == 0, or an ideal sum of 0 or a non-finite relevance) adds 1 to acc[N_NDCG_EMPTY] and stays
 *     out of the sum -- a stated departure: the reference adds the NaN and poisons its running sum.
 *     r outside [0, n_rel): ndcg[l] = NaN, no relevance is read, acc[N_REL_SKIPPED] += 1 unless r == -1.
 *   Accumulator: the counts and the histogram are integer slots (integer atomics: order-independent).  acc[NDCG_SUM] holds the bit
 *     pattern of a double: a call adds to it the sum of its finite ndcg[l] taken in ascending l, sequentially, in double -- one
 *     lane of a one-wave launch behind the lists, no float atomics: the same bits on every run.  acc[N_CALLS] += 1 per call.
 * Limits: 1 <= O <= GSTVD_RANK_MAX_OPTIONS, 1 <= L <= 2^31 - 1.  Refused before the launch, nothing written: scores NULL, relevance
 * without discounts or ndcg, gt_rank without gt_index, ndcg without relevance (GSTVD_E_NULL); a shape outside the limits, a row
 * stride below O, n_discounts < O, n_rel < 1, rel_index NULL with n_rel != L (GSTVD_E_SHAPE). */
enum { GSTVD_RANK_MAX_OPTIONS = 128 };
enum { GSTVD_RANK_N_SPARSE = 0, GSTVD_RANK_N_GT_SKIPPED = 1, GSTVD_RANK_N_NDCG = 2, GSTVD_RANK_N_NDCG_EMPTY = 3,
       GSTVD_RANK_N_REL_SKIPPED = 4, GSTVD_RANK_N_CALLS = 5, GSTVD_RANK_NDCG_SUM = 6, /* slot 7 is not used */
       GSTVD_RANK_HIST = 8,           /* hist[0 .. GSTVD_RANK_MAX_OPTIONS]: hist[r] = lists whose ground truth has rank r */
       GSTVD_RANK_ACC_SLOTS = 8 + GSTVD_RANK_MAX_OPTIONS + 1 };
typedef struct {
  const float* scores; int64_t ld_scores;
  const int64_t* gt_index;
  const float* relevance; int64_t ld_rel; int64_t n_rel;
  const int32_t* rel_index;
  const float* discounts; int64_t n_discounts;
  int64_t* ranks; int64_t ld_ranks;
  int32_t* gt_rank; float* ndcg; int64_t* acc;
  int64_t L;
  int32_t O; int32_t reserved_;
} gstvd_rank_metrics_t;
int gstvd_rank_metrics(const gstvd_rank_metrics_t* a, gstvd_stream_t s);

/* ---- in-domain image filter (entry points added, no signature changed: ABI stays 9) ----------------------------------------------
 * The first stage of GST (preprocessing/clip_in_domain_filtering.py, from the feature matrix on): fit a multivariate normal to the
 * image features of the dialog data (cov_mean :54-90), score other images by its log density (MultivariateNormal.log_prob
 * :183,192) and cut at a threshold.  Feature rows x[n, :] are GSTVD_F16 (IEEE half: what CLIP emits; these two entries alone take
 * it) or GSTVD_F32, dense rows with a free row stride ldx >= D, D % 16 == 0, 16 <= D <= GSTVD_GAUSS_MAX_D.  Every product and sum
 * below is in float64.
 *
 * gstvd_gauss_fit on x [N, D], N >= 2.  Two passes over the rows, two launches on the caller's stream:
 *     mean[i] = (sum_n x[n, i]) / N
 *     S[i, j] = sum_n (x[n, i] - mean[i]) * (x[n, j] - mean[j])
 *     cov     = fact * S,  fact = 1.0 / (N - 1), applied once, behind the sum
 *   mean double [D]; cov double [D, D], dense, written in full: the elements with i >= j are computed, cov[j, i] is a copy of
 *   cov[i, j], so the matrix is symmetric to the bit.  The rows are cut into slabs of GSTVD_GAUSS_FIT_SLAB; the first launch leaves
 *   one column sum per slab in the workspace, the second adds them in ascending slab order (every workgroup the same way), centres
 *   the rows on their way into the fp64 MFMA and leaves one 64 x 64 partial tile of S per (lower tile, slab) in the workspace; the
 *   workgroup that finishes a tile's last slab adds that tile's partials in ascending slab order.  No floating-point atomics: the
 *   same input gives the same bits on every run.  workspace: gstvd_gauss_fit_ws_bytes(N, D) bytes, 8-byte aligned, caller-owned,
 *   contents free on entry (the first launch initialises what the second counts in).
 *
 * gstvd_gauss_logprob on x [M, D], M >= 1, one launch:
 *     z = W (x[m, :] - mean),   q = sum_i z_i^2,   out[m] = (-0.5 * (klog2pi + q)) - half_log_det
 *   W = L^-1 for cov = L L^T (lower triangular; the caller factors on the host, in float64), klog2pi = D * log(2 pi),
 *   half_log_det = sum_i log L[i, i].  z is never stored.  Only the lower triangle of W is read (the products with the zeros above
 *   the diagonal are skipped, in 16 x 4 blocks): w_packed holds it in the order the kernel's operand registers take it,
 *     w_packed[128 * t * (t + 1) + 64 * s + 16 * c + r] = W[16 t + r, 4 s + c]   t < D/16, s < 4 t + 4, c < 4, r < 16
 *   gstvd_gauss_w_packed_elems(D) = 128 * (D/16) * (D/16 + 1) doubles.  A row's result depends on that row alone: not on M, nor on
 *   where the row stands in the batch.  A NaN or Inf feature gives a NaN or Inf result and nothing is raised (torch's
 *   MultivariateNormal validates its argument and raises: a stated departure).  out double [M].
 *   Cut, optional, same launch: keep uint8 [M]: keep[m] = (out[m] >= threshold), so a NaN score is never kept; n_kept: one int64
 *   that the kept rows of the call are ADDED to (integer atomic; zero it in front of a loop, read it once behind it).  Either may
 *   be NULL.
 * Both: no allocation, no synchronisation, safe under stream capture.  Refused before a launch, nothing written: a NULL operand
 * (GSTVD_E_NULL), a dtype other than the two (GSTVD_E_DTYPE), D outside the rule, N < 2 or N > 2^28, M < 1 or M > 2^31 - 1,
 * ldx < D, a workspace smaller than gstvd_gauss_fit_ws_bytes (GSTVD_E_SHAPE), a misaligned workspace (GSTVD_E_ALIGN). */
enum { GSTVD_F16 = 2 };
enum { GSTVD_GAUSS_MAX_D = 1024, GSTVD_GAUSS_FIT_SLAB = 4096 };
typedef struct {
  const void* x; int64_t ldx; int64_t N;
  double* mean; double* cov;
  void* workspace; int64_t workspace_bytes;
  int32_t D; int32_t dtype;
} gstvd_gauss_fit_t;
int64_t gstvd_gauss_fit_ws_bytes(int64_t N, int32_t D);     /* < 0: N or D outside the rule */
int gstvd_gauss_fit(const gstvd_gauss_fit_t* a, gstvd_stream_t s);
typedef struct {
  const void* x; int64_t ldx; int64_t M;
  const double* mean; const double* w_packed;
  double klog2pi; double half_log_det; double threshold;
  double* out; uint8_t* keep; int64_t* n_kept;
  int32_t D; int32_t dtype;
} gstvd_gauss_logprob_t;
int64_t gstvd_gauss_w_packed_elems(int32_t D);              /* < 0: D outside the rule */
int gstvd_gauss_logprob(const gstvd_gauss_logprob_t* a, gstvd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* GSTVD_HIP_H */
