// Training heads of the discriminative (enc_only) model, the parts that are not a GEMM / LayerNorm / cross entropy:
//   * row compaction (gstvd_rows_gather / gstvd_rows_scatter): the MLM and masked-region losses read only the masked rows
//     (train_disc.py: ~10-15 % of the tokens, 1-2 regions per image), every other row's gradient is exactly zero, so the heads
//     run on the gathered rows and their input gradient is scattered back into the stream's gradient buffer;
//   * the masked-region loss (gstvd_kl_fwd / gstvd_kl_bwd): KLDivLoss(reduction='none')(log_softmax(scores, 2), target) summed
//     over the regions with image_label == 1 and divided by their number (models/vilbert_dialog.py:1496-1501).
// One workgroup per row, sums in a fixed order (lane -> wave -> waves in wave order; one block for the sum over rows): no atomics,
// bit-reproducible.
#include "loss_reduce.h"
#include <math.h>

// ---- row gather / scatter ----------------------------------------------------------------------------------------------------
// dst[i, :] = src[idx[i], :]; an index outside [0, M) gives a zero row (never an out-of-bounds read)
template <typename T>
__global__ __launch_bounds__(256) void rows_gather_kernel(const T* src, int64_t lds, int64_t M, const int64_t* idx, int64_t H, T* dst,
                                                          int64_t ldd) {
  const int64_t i = blockIdx.x, r = idx[i];
  const bool in = r >= 0 && r < M;
  const T* s = src + (in ? r : 0) * lds;
  T* d = dst + i * ldd;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int64_t c = threadIdx.x * 4; c < H; c += 1024) st4(d + c, in ? ld4(s + c) : zero);
}

template <typename T>
__global__ __launch_bounds__(256) void rows_zero_kernel(T* dst, int64_t ldd, int64_t H) {
  T* d = dst + (int64_t)blockIdx.x * ldd;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int64_t c = threadIdx.x * 4; c < H; c += 1024) st4(d + c, zero);
}

// dst[idx[i], :] (=|+=) src[i, :]; distinct indices: every destination row has one writer.  An index outside [0, M) is skipped.
template <typename T>
__global__ __launch_bounds__(256) void rows_scatter_kernel(const T* src, int64_t lds, const int64_t* idx, int64_t H, T* dst, int64_t ldd,
                                                           int64_t M, int acc) {
  const int64_t i = blockIdx.x, r = idx[i];
  if (r < 0 || r >= M) return;
  const T* s = src + i * lds;
  T* d = dst + r * ldd;
  for (int64_t c = threadIdx.x * 4; c < H; c += 1024) {
    f32x4 v = ld4(s + c);
    if (acc) v += ld4(d + c);
    st4(d + c, v);
  }
}

// x[m, :] *= a[m, :]: the LayerNorm of a head transform sits directly behind the GELU (Linear -> GELU -> LayerNorm,
// models/vilbert_dialog.py:955-959), so its backward hands over d(GELU output); this turns it into d(pre-activation) with the
// gelu' the forward epilogue saved, the form every weight / input gradient GEMM of the engine expects
template <typename T>
__global__ __launch_bounds__(256) void rows_mul_kernel(T* x, int64_t ldx, const T* a, int64_t lda, int64_t N) {
  T* xr = x + (int64_t)blockIdx.x * ldx;
  const T* ar = a + (int64_t)blockIdx.x * lda;
  for (int64_t c = threadIdx.x * 4; c < N; c += 1024) st4(xr + c, ld4(xr + c) * ld4(ar + c));
}

// ---- masked-region KL loss ----------------------------------------------------------------------------------------------------
// row i of the scores belongs to target row trow[i] (or i); labels (or NULL = every row counts): a row whose label is not 1
// contributes nothing.  The class tail (C % 4 != 0, C = 1601) is handled here: scalar accesses, nothing is padded by the caller --
// so this normaliser (expf) is not ce_row.h's ce_row_lse, and the two entries keep their own checks (no stride % 4, no alignment step).
template <typename T>
__global__ __launch_bounds__(256) void kl_fwd_kernel(const T* scores, int64_t lds, const float* target, int64_t ldt, const int64_t* trow,
                                                     const int64_t* labels, int64_t C, float* row_loss, float* lse_out) {
  __shared__ float red[4];
  const int64_t m = blockIdx.x;
  const T* x = scores + m * lds;
  const float* t = target + (trow ? trow[m] : m) * ldt;
  float mx = -INFINITY;
  for (int64_t c = threadIdx.x; c < C; c += 256) mx = fmaxf(mx, to_f(x[c]));
  mx = block_reduce(mx, red, true);
  float s = 0.f;
  for (int64_t c = threadIdx.x; c < C; c += 256) s += expf(to_f(x[c]) - mx);
  s = block_reduce(s, red, false);
  const float lse = mx + logf(s);
  float a = 0.f;
  for (int64_t c = threadIdx.x; c < C; c += 256) {
    const float tv = t[c];
    // torch's xlogy convention: the t == 0 terms are exactly 0 whatever the score
    if (tv != 0.f) a += tv * (logf(tv) - (to_f(x[c]) - lse));
  }
  a = block_reduce(a, red, false);
  if (threadIdx.x == 0) {
    lse_out[m] = lse;
    row_loss[m] = (labels && labels[m] != 1) ? 0.f : a;
  }
}

// d scores = scale * (softmax * sum_c t - t), scale = gscale[0] (/ stats[1] with `mean`); columns [C, ldd) are zero filled
template <typename T>
__global__ __launch_bounds__(256) void kl_bwd_kernel(const T* scores, int64_t lds, const float* target, int64_t ldt, const int64_t* trow,
                                                     const int64_t* labels, const float* lse, const float* stats, const float* gscale,
                                                     int mean, int64_t C, T* dsc, int64_t ldd) {
  __shared__ float red[4];
  const int64_t m = blockIdx.x;
  const T* x = scores + m * lds;
  const float* t = target + (trow ? trow[m] : m) * ldt;
  T* d = dsc + m * ldd;
  const bool keep = !labels || labels[m] == 1;
  float ts = 0.f;
  for (int64_t c = threadIdx.x; c < C; c += 256) ts += t[c];
  ts = block_reduce(ts, red, false);            // the row's ACTUAL target sum (not assumed to be 1)
  const float gs = loss_grad_scale(gscale, mean, stats);
  const float l = lse[m];
  for (int64_t c = threadIdx.x; c < ldd; c += 256) {
    float o = 0.f;
    if (keep && c < C) o = (expf(to_f(x[c]) - l) * ts - t[c]) * gs;
    d[c] = from_f<T>(o);
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------
static int rows_args(const void* a, const void* b, const int64_t* idx, int64_t n, int64_t H, int64_t lda, int64_t ldb, int64_t M,
                     int32_t dtype) {
  if (!a || !b || !idx) return GSTVD_E_NULL;
  if (dtype != GSTVD_BF16 && dtype != GSTVD_F32) return GSTVD_E_DTYPE;
  if (n <= 0 || n > 0x7fffffffLL || H <= 0 || (H % 4) || M <= 0 || lda < H || ldb < H || (lda % 4) || (ldb % 4)) return GSTVD_E_SHAPE;
  const uintptr_t al = dtype == GSTVD_BF16 ? 7 : 15;
  if (((uintptr_t)a | (uintptr_t)b) & al) return GSTVD_E_ALIGN;
  if ((uintptr_t)idx & 7) return GSTVD_E_ALIGN;
  return 0;
}

extern "C" int gstvd_rows_gather(const void* src, int64_t lds, int64_t M, const int64_t* idx, int64_t n, int64_t H, int32_t dtype,
                                 void* dst, int64_t ldd, gstvd_stream_t stream) {
  const int rc = rows_args(src, dst, idx, n, H, lds, ldd, M, dtype);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(rows_gather_kernel<T>, dim3((unsigned)n), dim3(256), 0, s, (const T*)src, lds, M, idx, H, (T*)dst, ldd));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_rows_scatter(const void* src, int64_t lds, const int64_t* idx, int64_t n, int64_t H, int32_t dtype, void* dst,
                                  int64_t ldd, int64_t M, int32_t accumulate, gstvd_stream_t stream) {
  const int rc = rows_args(src, dst, idx, n, H, lds, ldd, M, dtype);
  if (rc) return rc;
  if (M > 0x7fffffffLL) return GSTVD_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const int acc = accumulate ? 1 : 0;
  if (!acc) {       // first writer: the rows no index names are zero, written here (same stream: ordered before the scatter)
    GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(rows_zero_kernel<T>, dim3((unsigned)M), dim3(256), 0, s, (T*)dst, ldd, H));
    GSTVD_LAUNCH_CHECK();
  }
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(rows_scatter_kernel<T>, dim3((unsigned)n), dim3(256), 0, s, (const T*)src, lds, idx, H, (T*)dst, ldd, M, acc));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_rows_mul(void* x, int64_t ldx, const void* a, int64_t lda, int64_t M, int64_t N, int32_t dtype, gstvd_stream_t stream) {
  if (!x || !a) return GSTVD_E_NULL;
  if (dtype != GSTVD_BF16 && dtype != GSTVD_F32) return GSTVD_E_DTYPE;
  if (M <= 0 || M > 0x7fffffffLL || N <= 0 || (N % 4) || ldx < N || lda < N || (ldx % 4) || (lda % 4)) return GSTVD_E_SHAPE;
  if (((uintptr_t)x | (uintptr_t)a) & (dtype == GSTVD_BF16 ? 7 : 15)) return GSTVD_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(rows_mul_kernel<T>, dim3((unsigned)M), dim3(256), 0, s, (T*)x, ldx, (const T*)a, lda, N));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_kl_fwd(const void* scores, int64_t lds, const float* target, int64_t ldt, const int64_t* target_row,
                            const int64_t* labels, int64_t rows, int64_t C, int32_t dtype, float* row_loss, float* lse, float* stats,
                            gstvd_stream_t stream) {
  if (!scores || !target || !row_loss || !lse || !stats) return GSTVD_E_NULL;
  if (rows <= 0 || rows > 0x7fffffffLL || C <= 0 || lds < C || ldt < C) return GSTVD_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(kl_fwd_kernel<T>, dim3((unsigned)rows), dim3(256), 0, s, (const T*)scores, lds, target, ldt, target_row, labels, C, row_loss, lse));
  GSTVD_LAUNCH_CHECK();
  hipLaunchKernelGGL(row_loss_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)row_loss, labels, (int64_t)1, 1, rows, stats);   // rows with label == 1 (no labels: all) count
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_kl_bwd(const void* scores, int64_t lds, const float* target, int64_t ldt, const int64_t* target_row,
                            const int64_t* labels, const float* lse, const float* stats, const float* gscale, int32_t mean,
                            int64_t rows, int64_t C, int32_t dtype, void* dscores, int64_t ldd, gstvd_stream_t stream) {
  if (!scores || !target || !lse || !stats || !dscores) return GSTVD_E_NULL;
  if (rows <= 0 || rows > 0x7fffffffLL || C <= 0 || lds < C || ldt < C || ldd < C) return GSTVD_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(kl_bwd_kernel<T>, dim3((unsigned)rows), dim3(256), 0, s, (const T*)scores, lds, target, ldt, target_row, labels, lse, stats, gscale, mean, C, (T*)dscores, ldd));
  GSTVD_LAUNCH_CHECK();
  return 0;
}
