// What the kernels over logits rows share (loss.hip, distill.hip): ONE rule for "this token counts", the 256-thread row log-sum-exp,
// one row of the cross entropy's gradient, the guarded 4-element load, the answer score of a candidate row, and the argument checks
// of the C entries that take such rows.  Forward and backward call the same function, so they take the same decision and hold the
// same bits: distill_bwd_kernel mixes lse (ce_fwd_kernel) and lse_tau (distill_fwd_kernel) on one row, and sends a token without a
// soft label through ce_bwd_row, so that row is the bits gstvd_ce_bwd writes.
// Not here, on purpose: kl_fwd_kernel's normaliser (disc_train.hip: scalar loads, because C = 1601 has no 4-element alignment, and
// expf, not __expf), rank_loss_kernel's log-sum-exp over a round's scores and select.h's sel_row_norm (other layouts, expf).
#pragma once
#include "common.h"
#include <math.h>

// A token counts towards the loss when its label is not the ignore index and names a column of the row.
DEVFN bool ce_counts(int64_t lab, int64_t ignore, int64_t V) { return !(lab == ignore || lab < 0 || lab >= V); }

// Pre-scales of ce_row_lse, a compile-time choice: RowPlain adds no instruction, RowTimes{k} (k > 0) is v * k.
struct RowPlain { DEVFN float operator()(float v) const { return v; } };
struct RowTimes { float k; DEVFN float operator()(float v) const { return v * k; } };

// log sum_c exp(pre(x[c])) of one row by the 256 threads of a workgroup, result in every thread: 4-element vectors up to V & ~3,
// a scalar tail, block_reduce max, the maximum pre-scaled ONCE (pre is monotone), __expf(pre(v) - max) summed lane -> wave ->
// waves in wave order, then max + logf(sum).  red: 4 floats of LDS; every thread must call (barriers inside).
template <typename T, typename Pre> DEVFN float ce_row_lse(const T* x, int64_t V, float* red, Pre pre) {
  const int64_t V4 = V & ~(int64_t)3;
  float mx = -INFINITY;
  for (int64_t c = threadIdx.x * 4; c < V4; c += 1024) {
    f32x4 v = ld4(x + c);
    mx = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  }
  for (int64_t c = V4 + threadIdx.x; c < V; c += 256) mx = fmaxf(mx, to_f(x[c]));
  mx = pre(block_reduce(mx, red, true));
  float s = 0.f;
  for (int64_t c = threadIdx.x * 4; c < V4; c += 1024) {
    f32x4 v = ld4(x + c);
    s += __expf(pre(v[0]) - mx) + __expf(pre(v[1]) - mx) + __expf(pre(v[2]) - mx) + __expf(pre(v[3]) - mx);
  }
  for (int64_t c = V4 + threadIdx.x; c < V; c += 256) s += __expf(pre(to_f(x[c])) - mx);
  s = block_reduce(s, red, false);
  return mx + logf(s);
}

// Elements c .. c + 3 of a row of V: one vector load where all four exist, else element by element with `fill` past the end.
// c % 4 == 0 and the row 4-element aligned (ce_row_args); I is the caller's index type, so its address arithmetic stays its own.
template <typename T, typename I> DEVFN f32x4 ld4_guard(const T* x, I c, I V, float fill) {
  if (c + 3 < V) return ld4(x + c);
  f32x4 v = {fill, fill, fill, fill};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (c + e < V) v[e] = to_f(x[c + e]);
  return v;
}

// One row of dlogits = (softmax - onehot) * gs, columns V..ldd zero; `keep` false: the whole row zero.  Shared by the mean form
// and the per-row form of loss.hip, so the two agree to the last bit wherever their scales do.  The vector branch and the guarded
// element branch stay written out: as ld4_guard + one guarded loop ce_bwd measured 21.1 against 19.6 us (profiles/loss_refactor_timing.txt).
template <typename T>
DEVFN void ce_bwd_row(const T* x, T* d, int64_t lab, bool keep, float l, float gs, int64_t V, int64_t ldd) {
  for (int64_t c = threadIdx.x * 4; c < ldd; c += 1024) {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (keep) {
      if (c + 3 < V) {
        f32x4 v = ld4(x + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (__expf(v[e] - l) - ((c + e) == lab ? 1.f : 0.f)) * gs;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e < V) o[e] = (__expf(to_f(x[c + e]) - l) - ((c + e) == lab ? 1.f : 0.f)) * gs;
      }
    }
    st4(d + c, o);
  }
}

// score = sum_u [tgt != 0] (logits[row, u, tgt] - lse[row, u]), tgt = ids[row, u + 1] (0 for the last u), by ONE wave: lane l adds
// u = l, l + 64, ... in that order, then wave_sum; result in every lane.  answer_scores_kernel and rank_loss_kernel: the same bits.
template <typename T>
DEVFN float answer_score_row(const T* logits, int64_t ldl, const float* lse, const int64_t* ids, int64_t U, int64_t row, int64_t lane) {
  float a = 0.f;
  for (int64_t u = lane; u < U; u += 64) {
    const int64_t tgt = (u + 1 < U) ? ids[row * U + u + 1] : 0;
    if (tgt != 0) a += to_f(logits[(row * U + u) * ldl + tgt]) - lse[row * U + u];
  }
  return wave_sum(a);
}

// The cross-entropy and distillation entries read logits (and write dlogits) in 4-element vectors: 16 bytes of fp32, 8 bytes of bf16
static inline bool ce_misaligned(const void* p, int32_t dtype) { return ((uintptr_t)p & (dtype == GSTVD_BF16 ? 7 : 15)) != 0; }

// The argument checks of an entry over M logits rows of V, in the order the C ABI promises: NULL, SHAPE (with the entry's own terms,
// `own_shape_bad`: K, alpha, inv_tau), DTYPE, ALIGN.  dlogits / ldd: the gradient rows of a backward entry, or NULL / 0.  0: launch.
static inline int ce_row_args(bool any_null, int64_t M, int64_t V, bool own_shape_bad, int32_t dtype, const void* logits, int64_t ldl,
                              const void* dlogits = nullptr, int64_t ldd = 0) {
  if (any_null) return GSTVD_E_NULL;
  if (M <= 0 || V <= 0 || (ldl % 4) || ldl < V || (dlogits && ((ldd % 4) || ldd < V)) || own_shape_bad) return GSTVD_E_SHAPE;
  if (dtype != GSTVD_BF16 && dtype != GSTVD_F32) return GSTVD_E_DTYPE;
  if (ce_misaligned(logits, dtype) || (dlogits && ce_misaligned(dlogits, dtype))) return GSTVD_E_ALIGN;
  return 0;
}
