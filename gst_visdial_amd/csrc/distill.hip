// Soft pseudo-labels of the self-training loop (no reference counterpart; include/gstvd_hip.h states the rules in full): the K best
// teacher tokens of every position with their log-probabilities (gstvd_topk_logp), and the student's loss against them mixed with
// the hard-label cross entropy (gstvd_distill_fwd / gstvd_distill_bwd).  Conventions of loss.hip: one workgroup per logits row,
// 4-element vector accesses, deterministic reductions, the row arithmetic of ce_row.h, stats by loss_reduce.h's rule.
#include "loss_reduce.h"
#include "ce_row.h"
#include "select.h"

namespace {

constexpr int KMAX = 16;

// ---- teacher side ----------------------------------------------------------------------------------------------------------------
constexpr int TNT = 1024, TNW = TNT / 64;
constexpr int TVEC = 8;                                       // 4-vectors per thread: V <= 8 * 4 * 1024 (checked by the host entry)

// The row in registers as in beam.hip's phase A, read once in 4-vectors (slot j = element (tid + (j >> 2) * TNT) * 4 + (j & 3)); its
// K best by select.h's rounds.
template <typename T>
__global__ __launch_bounds__(TNT) void topk_logp_kernel(const T* logits, int64_t ldl, const float* lse, int V, int K, int64_t* ids,
                                                        float* logp) {
  __shared__ float smv[TNW];
  __shared__ int smi[TNW];
  const int tid = threadIdx.x;
  const int64_t m = blockIdx.x;
  const T* x = logits + m * ldl;
  float zr[TVEC * 4];
#pragma unroll
  for (int j = 0; j < TVEC; ++j) {
    const f32x4 v = ld4_guard(x, (tid + j * TNT) * 4, V, -INFINITY);
#pragma unroll
    for (int e = 0; e < 4; ++e) zr[j * 4 + e] = v[e];
  }
  const float l = lse[m];
  // (only a row with NaNs runs out of candidates: K <= V is checked)
  const Sel mine = sel_topk_rounds<TNW>(zr, [tid](int j) { return (tid + (j >> 2) * TNT) * 4 + (j & 3); }, V, K, smv, smi);
  if (tid < K) {
    ids[m * K + tid] = (int64_t)mine.i;
    logp[m * K + tid] = mine.v - l;
  }
}

// ---- student side ----------------------------------------------------------------------------------------------------------------
// A token has a soft label when its first id is not negative and every one of its K ids lies in [0, V): one decision, taken the
// same way by the forward and the backward, before any logit is read through an id.
DEVFN bool soft_row_ok(const int64_t* sid, int K, int64_t V) {
  bool ok = sid[0] >= 0;
  for (int k = 0; k < K; ++k) ok = ok && sid[k] >= 0 && sid[k] < V;
  return ok;
}

// q_k = softmax over the K entries of soft_logp * inv_tau, max-subtracted: e_k / sum with the sum formed serially k = 0 .. K - 1
// wherever it is formed, so the forward and the backward hold the same q.  -> sum, max (q_k = expf(s_k - max) / sum)
DEVFN void soft_q_norm(const float* sl, int K, float inv_tau, float& smax, float& z) {
  smax = -INFINITY;
  for (int k = 0; k < K; ++k) smax = fmaxf(smax, sl[k] * inv_tau);
  z = 0.f;
  for (int k = 0; k < K; ++k) z += expf(sl[k] * inv_tau - smax);
}

template <typename T>
__global__ __launch_bounds__(256) void distill_fwd_kernel(const T* logits, int64_t ldl, const int64_t* labels, const int64_t* soft_ids,
                                                          const float* soft_logp, int64_t V, int K, int64_t ignore, float alpha,
                                                          float inv_tau, const float* ce_loss, float* row_loss, float* row_kd,
                                                          float* lse_tau) {
  __shared__ float red[4];
  const int64_t m = blockIdx.x;
  const int64_t* sid = soft_ids + m * K;
  if (!(ce_counts(labels[m], ignore, V) && soft_row_ok(sid, K, V))) {   // block-uniform
    if (threadIdx.x == 0) { row_loss[m] = ce_loss[m]; row_kd[m] = 0.f; lse_tau[m] = 0.f; }
    return;
  }
  const T* x = logits + m * ldl;
  const float lt = ce_row_lse(x, V, red, RowTimes{inv_tau});   // inv_tau > 0: the scaled maximum is the maximum of the scaled row
  if (threadIdx.x == 0) {
    const float* sl = soft_logp + m * K;
    float smax, z;
    soft_q_norm(sl, K, inv_tau, smax, z);
    const float lz = logf(z);
    float kd = 0.f;
    for (int k = 0; k < K; ++k) {
      const float sk = sl[k] * inv_tau - smax;
      const float q = expf(sk) / z;
      if (q > 0.f) kd += q * ((sk - lz) - (to_f(x[sid[k]]) * inv_tau - lt));     // (q == 0: the term is exactly 0, never 0 * inf)
    }
    const float tau = 1.f / inv_tau;
    lse_tau[m] = lt;
    row_kd[m] = kd;
    row_loss[m] = alpha == 0.f ? ce_loss[m] : (1.f - alpha) * ce_loss[m] + alpha * (tau * tau) * kd;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void distill_bwd_kernel(const T* logits, int64_t ldl, const int64_t* labels, const int64_t* soft_ids,
                                                          const float* soft_logp, const float* lse, const float* lse_tau,
                                                          const float* stats, const float* gscale, int64_t V, int K, int64_t ignore,
                                                          float alpha, float inv_tau, T* dl, int64_t ldd) {
  __shared__ float sq[KMAX];
  __shared__ int64_t si[KMAX];
  const int64_t m = blockIdx.x;
  const int64_t lab = labels[m];
  const bool keep = ce_counts(lab, ignore, V);
  const float gs = loss_grad_scale(gscale, 1, stats);
  const T* x = logits + m * ldl;
  T* d = dl + m * ldd;
  const int64_t* sid = soft_ids + m * K;
  if (!(keep && alpha != 0.f && soft_row_ok(sid, K, V))) {    // block-uniform: the cross entropy's own row, bit for bit
    ce_bwd_row(x, d, lab, keep, lse[m], gs, V, ldd);
    return;
  }
  if (threadIdx.x < K) {
    const float* sl = soft_logp + m * K;
    float smax, z;
    soft_q_norm(sl, K, inv_tau, smax, z);
    sq[threadIdx.x] = expf(sl[threadIdx.x] * inv_tau - smax) / z;
    si[threadIdx.x] = sid[threadIdx.x];
  }
  __syncthreads();
  const float l = lse[m], lt = lse_tau[m];
  const float wc = 1.f - alpha, wk = alpha * (1.f / inv_tau);
  for (int64_t c = threadIdx.x * 4; c < ldd; c += 1024) {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (c < V) {
      const f32x4 v = ld4_guard(x, c, V, 0.f);
      f32x4 qs = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < K; ++k) {                           // duplicate ids count as separate entries: their q add up, k ascending
        const int64_t off = si[k] - c;
        if (off >= 0 && off < 4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) qs[e] += off == e ? sq[k] : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < V)
          o[e] = gs * (wc * (__expf(v[e] - l) - ((c + e) == lab ? 1.f : 0.f)) + wk * (__expf(v[e] * inv_tau - lt) - qs[e]));
    }
    st4(d + c, o);
  }
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
// The student entries' own shape terms: K entries per token, the mixing weight and a finite positive 1 / tau.
static bool soft_args_bad(int64_t K, float a, float it) { return K < 1 || K > KMAX || !(a >= 0.f && a <= 1.f) || !(it > 0.f) || isinf(it); }

extern "C" int gstvd_topk_logp(const void* logits, int64_t ldl, const float* lse, int64_t M, int64_t V, int64_t K, int32_t dtype,
                               int64_t* ids, float* logp, gstvd_stream_t stream) {
  if (const int rc = ce_row_args(!logits || !lse || !ids || !logp, M, V, K < 1 || K > KMAX || K > V, dtype, logits, ldl)) return rc;
  if (V > TVEC * 4 * TNT) return GSTVD_E_UNSUPPORTED;         // a row lives in 32 registers per thread
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(topk_logp_kernel<T>, dim3((unsigned)M), dim3(TNT), 0, (hipStream_t)stream, (const T*)logits, ldl, lse, (int)V, (int)K, ids, logp));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_distill_fwd(const void* logits, int64_t ldl, const int64_t* labels, const int64_t* soft_ids, const float* soft_logp,
                                 int64_t M, int64_t V, int64_t K, int64_t ignore_index, float alpha, float inv_tau, int32_t dtype,
                                 const float* ce_row_loss, float* row_loss, float* row_kd, float* lse_tau, float* stats_out,
                                 gstvd_stream_t stream) {
  if (const int rc = ce_row_args(!logits || !labels || !soft_ids || !soft_logp || !ce_row_loss || !row_loss || !row_kd || !lse_tau || !stats_out, M, V,
                                 soft_args_bad(K, alpha, inv_tau), dtype, logits, ldl)) return rc;
  hipStream_t s = (hipStream_t)stream;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(distill_fwd_kernel<T>, dim3((unsigned)M), dim3(256), 0, s, (const T*)logits, ldl, labels, soft_ids, soft_logp, V, (int)K,
                                               ignore_index, alpha, inv_tau, ce_row_loss, row_loss, row_kd, lse_tau));
  GSTVD_LAUNCH_CHECK();
  hipLaunchKernelGGL(row_loss_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)row_loss, labels, ignore_index, 0, M, stats_out);   // the cross entropy's count, by its rule
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_distill_bwd(const void* logits, int64_t ldl, const int64_t* labels, const int64_t* soft_ids, const float* soft_logp,
                                 const float* lse, const float* lse_tau, const float* stats, const float* gscale, int64_t M, int64_t V,
                                 int64_t K, int64_t ignore_index, float alpha, float inv_tau, int32_t dtype, void* dlogits, int64_t ldd,
                                 gstvd_stream_t stream) {
  if (const int rc = ce_row_args(!logits || !labels || !soft_ids || !soft_logp || !lse || !lse_tau || !stats || !dlogits, M, V,
                                 soft_args_bad(K, alpha, inv_tau), dtype, logits, ldl, dlogits, ldd)) return rc;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(distill_bwd_kernel<T>, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, (const T*)logits, ldl, labels, soft_ids, soft_logp, lse, lse_tau,
                                               stats, gscale, V, (int)K, ignore_index, alpha, inv_tau, (T*)dlogits, ldd));
  GSTVD_LAUNCH_CHECK();
  return 0;
}
