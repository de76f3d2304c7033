// The stand-alone fused AdamW pass and its three entries.  HBM-bound: 16-byte streaming accesses, one lr / weight-decay lookup per vector.
#include "common.h"

// AdamW: pytorch_transformers==1.2.0 optimization.AdamW.step (train_gen.py:16,247).  Segments are 4-element aligned
// (the flat layout aligns every tensor to 64 elements), so one lookup serves a 16-byte vector.
// GT = float: grad is the flat fp32 gradient buffer (same indexing as param).  GT = bf16: grad points at the bf16 copy of
// the slice that was just all-reduced; element i of the flat buffers is grad[i - gorigin].
template <typename GT>
__global__ __launch_bounds__(256) void adamw_kernel(float* param, const GT* grad, float* m, float* v, bf16* shadow, int64_t n,
                                                    const int64_t* seg_end, const float* hp, int64_t nseg, float b1, float b2,
                                                    float eps, const float* step, float gscale, int64_t base, int64_t gorigin,
                                                    const int32_t* blocks, const uint8_t* seg_skip) {
  // the launch covers flat elements [base, n) of the buffers (pointers are the buffers' starts), or -- `blocks` given -- the
  // listed 1024-element blocks; segment ends are absolute
  __shared__ float s_bc;
  const int64_t i0 = blocks ? (int64_t)blocks[blockIdx.x] * 1024 : base + (int64_t)blockIdx.x * 1024;   // block-uniform: scalar loads below
  const int64_t i = i0 + threadIdx.x * 4;
  if (threadIdx.x == 0) s_bc = adamw_bias_correction(b1, b2, step[0]);     // once per block
  // streaming operands first (their latency overlaps the segment lookup); nothing here is re-read, keep it out of L2's way
  const bool vec = i + 3 < n;
  f32x4 g4 = {0.f, 0.f, 0.f, 0.f}, m4 = g4, v4 = g4, p4 = g4;
  if (vec) {
    g4 = ld4_stream(grad + (i - gorigin));
    m4 = __builtin_nontemporal_load((const f32x4*)(m + i));
    v4 = __builtin_nontemporal_load((const f32x4*)(v + i));
    p4 = __builtin_nontemporal_load((const f32x4*)(param + i));
  }
  int64_t lo = adamw_segment(seg_end, nseg, i0);        // first segment whose end > i0
  __syncthreads();
  if (i >= n || i < base) return;                    // (i < base: only with a block list, whose blocks may straddle the range's start)
  while (lo < nseg - 1 && seg_end[lo] <= i) ++lo;     // at most a few steps inside a 1024-element block
  const float lr = hp[2 * lo], wd = hp[2 * lo + 1];
  const float bc = s_bc;
  if (vec && seg_end[lo] >= i + 4) {
    if (lr == 0.f || (seg_skip && seg_skip[lo])) return;   // padding / frozen segment / updated by the weight-gradient launch
    adamw_update4(p4, m4, v4, g4, gscale, lr, wd, bc, b1, b2, eps);
    __builtin_nontemporal_store(m4, (f32x4*)(m + i));
    __builtin_nontemporal_store(v4, (f32x4*)(v + i));
    __builtin_nontemporal_store(p4, (f32x4*)(param + i));
    if (shadow) st4(shadow + i, p4);
    return;
  }
  int64_t seg = lo;
  for (int e = 0; e < 4 && i + e < n; ++e) {
    const int64_t k = i + e;
    while (seg < nseg - 1 && seg_end[seg] <= k) ++seg;
    const float lr_ = hp[2 * seg], wd_ = hp[2 * seg + 1];
    if (lr_ == 0.f || (seg_skip && seg_skip[seg])) continue;
    f32x4 g1 = {(float)grad[k - gorigin], 0.f, 0.f, 0.f}, m1 = {m[k], 0.f, 0.f, 0.f}, v1 = {v[k], 0.f, 0.f, 0.f}, p1 = {param[k], 0.f, 0.f, 0.f};
    adamw_update4(p1, m1, v1, g1, gscale, lr_, wd_, bc, b1, b2, eps);
    m[k] = m1[0]; v[k] = v1[0]; param[k] = p1[0];
    if (shadow) shadow[k] = (bf16)p1[0];
  }
}

// ---- C ABI ----------------------------------------------------------------------------------------------
// One launch of `nblk` blocks over [begin, n), or over the listed blocks; each entry makes its own checks first.
template <typename GT>
static int adamw_launch(int64_t nblk, gstvd_stream_t stream, float* param, const GT* grad, int64_t gorigin, float* m, float* v,
                        void* shadow_bf16, int64_t n, const int64_t* seg_end, const float* hp, int64_t nseg, float beta1, float beta2,
                        float eps, const float* step, float grad_scale, int64_t begin, const int32_t* blocks, const uint8_t* seg_skip) {
  hipLaunchKernelGGL(adamw_kernel<GT>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, param, grad, m, v, (bf16*)shadow_bf16, n,
                     seg_end, hp, nseg, beta1, beta2, eps, step, grad_scale, begin, gorigin, blocks, seg_skip);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_adamw(float* param, const float* grad, float* m, float* v, void* shadow_bf16, int64_t n,
                           const int64_t* seg_end, const float* hp, int64_t nseg, float beta1, float beta2, float eps,
                           const float* step, float grad_scale, int64_t begin, gstvd_stream_t stream) {
  if (!param || !grad || !m || !v || !seg_end || !hp || !step) return GSTVD_E_NULL;
  if (n <= 0 || nseg <= 0 || begin < 0 || begin >= n || (begin % 4)) return GSTVD_E_SHAPE;
  return adamw_launch((n - begin + 1023) / 1024, stream, param, grad, 0, m, v, shadow_bf16, n, seg_end, hp, nseg, beta1, beta2, eps, step,
                      grad_scale, begin, nullptr, nullptr);
}

extern "C" int gstvd_adamw_bf16grad(float* param, const void* grad_bf16, int64_t grad_origin, float* m, float* v, void* shadow_bf16,
                                    int64_t n, const int64_t* seg_end, const float* hp, int64_t nseg, float beta1, float beta2,
                                    float eps, const float* step, float grad_scale, int64_t begin, gstvd_stream_t stream) {
  if (!param || !grad_bf16 || !m || !v || !seg_end || !hp || !step) return GSTVD_E_NULL;
  if (n <= 0 || nseg <= 0 || begin < 0 || begin >= n || (begin % 4) || grad_origin > begin || (grad_origin % 4)) return GSTVD_E_SHAPE;
  if ((uintptr_t)grad_bf16 & 7) return GSTVD_E_ALIGN;
  return adamw_launch((n - begin + 1023) / 1024, stream, param, (const bf16*)grad_bf16, grad_origin, m, v, shadow_bf16, n, seg_end, hp, nseg,
                      beta1, beta2, eps, step, grad_scale, begin, nullptr, nullptr);
}

extern "C" int gstvd_adamw_blocks(float* param, const float* grad, float* m, float* v, void* shadow_bf16, int64_t n,
                                  const int64_t* seg_end, const float* hp, int64_t nseg, float beta1, float beta2, float eps,
                                  const float* step, float grad_scale, int64_t begin, const int32_t* block_list_dev, int64_t nblocks,
                                  const uint8_t* seg_skip_dev, gstvd_stream_t stream) {
  if (!param || !grad || !m || !v || !seg_end || !hp || !step || !block_list_dev) return GSTVD_E_NULL;
  if (n <= 0 || nseg <= 0 || begin < 0 || begin >= n || (begin % 4) || nblocks < 0 || nblocks > (n + 1023) / 1024) return GSTVD_E_SHAPE;
  if (nblocks == 0) return 0;
  return adamw_launch(nblocks, stream, param, grad, 0, m, v, shadow_bf16, n, seg_end, hp, nseg, beta1, beta2, eps, step, grad_scale, begin,
                      block_list_dev, seg_skip_dev);
}
