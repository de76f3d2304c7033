// LM-head cross entropy (visual_dialog_decoder.py:70-77), candidate scoring (evaluate_gen.py:94-106) and the listwise loss over the scores.
// HBM-bound: 16-byte vector accesses, one workgroup per logits row, deterministic reductions; the row arithmetic is ce_row.h's.
#include "loss_reduce.h"
#include "ce_row.h"

template <typename T>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const T* logits, int64_t ldl, const int64_t* labels, int64_t V,
                                                     int64_t ignore, float* row_loss, float* lse_out) {
  __shared__ float red[4];
  const int64_t m = blockIdx.x;
  const T* x = logits + m * ldl;
  const float lse = ce_row_lse(x, V, red, RowPlain{});
  if (threadIdx.x == 0) {
    lse_out[m] = lse;
    const int64_t lab = labels[m];
    row_loss[m] = ce_counts(lab, ignore, V) ? lse - to_f(x[lab]) : 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const T* logits, int64_t ldl, const int64_t* labels, const float* lse,
                                                     const float* stats, const float* gscale, int mean, int64_t V,
                                                     int64_t ignore, T* dl, int64_t ldd) {
  const int64_t m = blockIdx.x;
  const int64_t lab = labels[m];
  const bool keep = ce_counts(lab, ignore, V);
  const float gs = loss_grad_scale(gscale, mean, stats);
  ce_bwd_row(logits + m * ldl, dl + m * ldd, lab, keep, lse[m], gs, V, ldd);
}

// Backward of CrossEntropyLoss(reduction='none') (visual_dialog_decoder.py:76) under a per-token upstream gradient g[m]
// (evaluate_gen_attack.py:126-130: mean over the sequence, times the candidate's relevance).  A row whose g is zero is STORED as
// zeros, never multiplied: 0 * exp(...) of a logit that overflowed would be NaN.
template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_rows_kernel(const T* logits, int64_t ldl, const int64_t* labels, const float* lse,
                                                          const float* g, int64_t V, int64_t ignore, T* dl, int64_t ldd) {
  const int64_t m = blockIdx.x;
  const int64_t lab = labels[m];
  const float gs = g[m];
  const bool keep = ce_counts(lab, ignore, V) && gs != 0.f;
  ce_bwd_row(logits + m * ldl, dl + m * ldd, lab, keep, lse[m], gs, V, ldd);
}

// score[row] = sum_u [tgt != 0] (logits[row,u,tgt] - lse[row,u]),  tgt = ids[row,u+1] (0 for the last u)
template <typename T>
__global__ __launch_bounds__(64) void answer_scores_kernel(const T* logits, int64_t ldl, const float* lse,
                                                           const int64_t* ids, int64_t U, float* scores) {
  const int64_t row = blockIdx.x;
  const float a = answer_score_row(logits, ldl, lse, ids, U, row, threadIdx.x);
  if (threadIdx.x == 0) scores[row] = a;
}

// Listwise ranking loss over the G candidates of each of E rounds (gstvd_rank_loss), ONE workgroup, one launch:
//   1. score[i] of every candidate row, a wave per row through answer_score_row, as answer_scores_kernel forms it;
//   2. count = rounds whose relevance is not all zero (every thread learns it: block_reduce);
//   3. a wave per round: t = rel / sum(rel), logp = log_softmax(score * inv_temperature), loss_e = -sum_{t_i > 0} t_i logp_i, and the
//      upstream gradient of the round's per-token cross entropies, g_tok[i, u] = -(p_i - t_i) * inv_temperature / count where the
//      shifted target is not [PAD] (score_i = -sum_u ce[i, u]), exact zeros elsewhere and for a round that does not count;
//   4. stats = [sum of loss_e, count, mean] by loss_reduce.h's rule (thread-strided sums, then block_reduce): fixed order, no atomics.
// The sum of a round's relevance is the serial sum i = 0 .. G - 1 wherever it is formed, so "counts" is one decision.
DEVFN float rank_rel_sum(const float* rel, int64_t G) {
  float s = 0.f;
  for (int64_t i = 0; i < G; ++i) s += rel[i];
  return s;
}
template <typename T>
__global__ __launch_bounds__(256) void rank_loss_kernel(const T* logits, int64_t ldl, const float* lse, const int64_t* ids, const float* rel,
                                                        int64_t E, int64_t G, int64_t U, float inv_t, float* scores, float* p_out,
                                                        float* round_loss, float* g_tok, float* stats) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t row = wave; row < E * G; row += 4) {
    const float a = answer_score_row(logits, ldl, lse, ids, U, row, lane);
    if (lane == 0) scores[row] = a;
  }
  float n = 0.f;
  for (int64_t e = threadIdx.x; e < E; e += 256) n += rank_rel_sum(rel + e * G, G) > 0.f ? 1.f : 0.f;
  const float count = block_reduce(n, red, false);            // (its barriers also publish the scores to the whole workgroup)
  for (int64_t e = wave; e < E; e += 4) {
    const float* sc = scores + e * G;
    const float rsum = rank_rel_sum(rel + e * G, G);
    const bool counts = rsum > 0.f;
    float mx = -INFINITY;
    for (int64_t i = lane; i < G; i += 64) mx = fmaxf(mx, sc[i] * inv_t);
    mx = wave_max(mx);
    float se = 0.f;
    for (int64_t i = lane; i < G; i += 64) se += expf(sc[i] * inv_t - mx);
    const float lz = mx + logf(wave_sum(se));                 // log sum exp of the round's scaled scores
    float le = 0.f;
    for (int64_t i = lane; i < G; i += 64) {
      const float logp = sc[i] * inv_t - lz, t = counts ? rel[e * G + i] / rsum : 0.f;
      p_out[e * G + i] = expf(logp);
      if (t > 0.f) le -= t * logp;                            // (t == 0 with logp == -inf adds nothing)
    }
    le = wave_sum(le);
    if (lane == 0) round_loss[e] = counts ? le : 0.f;
    for (int64_t j = lane; j < G * U; j += 64) {
      const int64_t i = j / U, u = j - i * U;
      const int64_t tgt = (u + 1 < U) ? ids[(e * G + i) * U + u + 1] : 0;
      float gv = 0.f;
      if (counts && tgt != 0) gv = -(expf(sc[i] * inv_t - lz) - rel[e * G + i] / rsum) * inv_t / count;
      g_tok[(e * G + i) * U + u] = gv;
    }
  }
  __syncthreads();                                            // round_loss is complete
  float s = 0.f;
  for (int64_t e = threadIdx.x; e < E; e += 256) s += round_loss[e];
  s = block_reduce(s, red, false);
  if (threadIdx.x == 0) { stats[0] = s; stats[1] = count; stats[2] = count > 0.f ? s / count : 0.f; }
}

// ---- C ABI ----------------------------------------------------------------------------------------------
extern "C" int gstvd_ce_fwd(const void* logits, int64_t ldl, const int64_t* labels, int64_t M, int64_t V, int64_t ignore_index,
                            int32_t dtype, float* row_loss, float* lse, float* stats, gstvd_stream_t stream) {
  if (const int rc = ce_row_args(!logits || !labels || !row_loss || !lse || !stats, M, V, false, dtype, logits, ldl)) return rc;
  hipStream_t s = (hipStream_t)stream;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(ce_fwd_kernel<T>, dim3((unsigned)M), dim3(256), 0, s, (const T*)logits, ldl, labels, V, ignore_index, row_loss, lse));
  GSTVD_LAUNCH_CHECK();
  hipLaunchKernelGGL(row_loss_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)row_loss, labels, ignore_index, 0, M, stats);   // rows with label != ignore count
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_ce_bwd(const void* logits, int64_t ldl, const int64_t* labels, const float* lse, const float* stats,
                            const float* gscale, int32_t mean, int64_t M, int64_t V, int64_t ignore_index, int32_t dtype,
                            void* dlogits, int64_t ldd, gstvd_stream_t stream) {
  if (const int rc = ce_row_args(!logits || !labels || !lse || !stats || !dlogits, M, V, false, dtype, logits, ldl, dlogits, ldd)) return rc;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(ce_bwd_kernel<T>, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, (const T*)logits, ldl, labels, lse, stats, gscale, mean, V, ignore_index, (T*)dlogits, ldd));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_ce_bwd_rows(const void* logits, int64_t ldl, const int64_t* labels, const float* lse, const float* g, int64_t M,
                                 int64_t V, int64_t ignore_index, int32_t dtype, void* dlogits, int64_t ldd, gstvd_stream_t stream) {
  if (const int rc = ce_row_args(!logits || !labels || !lse || !g || !dlogits, M, V, false, dtype, logits, ldl, dlogits, ldd)) return rc;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(ce_bwd_rows_kernel<T>, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, (const T*)logits, ldl, labels, lse, g, V, ignore_index, (T*)dlogits, ldd));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_answer_scores(const void* logits, int64_t ldl, const float* lse, const int64_t* dec_ids, int64_t rows,
                                   int64_t U, int32_t dtype, float* scores, gstvd_stream_t stream) {
  if (!logits || !lse || !dec_ids || !scores) return GSTVD_E_NULL;
  if (rows <= 0 || U <= 0) return GSTVD_E_SHAPE;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(answer_scores_kernel<T>, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, (const T*)logits, ldl, lse, dec_ids, U, scores));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_rank_loss(const void* logits, int64_t ldl, const float* lse, const int64_t* dec_ids, const float* relevance,
                               int64_t E, int64_t G, int64_t U, float inv_temperature, int32_t dtype, float* scores, float* p,
                               float* round_loss, float* g_tok, float* stats, gstvd_stream_t stream) {
  if (!logits || !lse || !dec_ids || !relevance || !scores || !p || !round_loss || !g_tok || !stats) return GSTVD_E_NULL;
  if (E <= 0 || G <= 0 || U <= 0 || !(inv_temperature > 0.f)) return GSTVD_E_SHAPE;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(rank_loss_kernel<T>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const T*)logits, ldl, lse, dec_ids, relevance, E, G, U,
                                               inv_temperature, scores, p, round_loss, g_tok, stats));
  GSTVD_LAUNCH_CHECK();
  return 0;
}
