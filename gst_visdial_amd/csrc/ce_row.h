// One row of the cross entropy's gradient, shared by the cross-entropy entries (loss.hip) and the distillation backward
// (distill.hip): a token that carries no soft label goes through this routine there, so its row is the bits gstvd_ce_bwd writes.
#pragma once
#include "common.h"

// One row of dlogits = (softmax - onehot) * gs, columns V..ldd zero; `keep` false: the whole row zero.  Shared by the mean form
// and the per-row form of loss.hip, so the two agree to the last bit wherever their scales do.
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

// The cross-entropy and distillation entries read logits (and write dlogits) in 4-element vectors: 16 bytes of fp32, 8 bytes of bf16
static inline bool ce_misaligned(const void* p, int32_t dtype) { return ((uintptr_t)p & (dtype == GSTVD_BF16 ? 7 : 15)) != 0; }
