// In-domain image filter: the arithmetic of preprocessing/clip_in_domain_filtering.py from the feature matrix on -- the Gaussian fit
// (cov_mean :54-90) and the log density of every scored image (MultivariateNormal.log_prob :183,192) -- in float64 on the fp64 MFMA.
// include/gstvd_hip.h states the rule in full.
//
//   gauss_colsum_kernel   (fit, launch 1) grid (column groups of 64, row slabs): four row lanes per column add the slab's rows in
//                         double; one column sum per slab goes to the workspace.  Block (0, 0) zeroes the tile tickets launch 2 counts in.
//   gauss_syrk_kernel     (fit, launch 2) grid (lower 64 x 64 tiles, row slabs), four waves, one 32 x 32 quadrant each.  Every block adds
//                         the slab column sums of its 128 columns in ascending slab order (mean = sum / N), centres and widens the rows on
//                         their way into the operand registers and leaves its partial tile in the workspace; the block that draws a tile's
//                         last ticket adds the partials in ascending slab order, scales once by fact and writes the tile and its mirror.
//   gauss_logprob_kernel  32 rows per workgroup, staged in LDS in their own dtype.  A wave owns 16-row blocks of W (dealt out in a snake so
//                         the triangle's work is even) and walks their K-steps up to the diagonal; z lives in the accumulator only, its
//                         squares are added per lane, over the four lane groups, then over the waves in wave order.
//
// fp64 MFMA 16x16x4 fragments: A[row l & 15][k l >> 4], B[k l >> 4][col l & 15], one double per lane; C/D col = l & 15,
// row = (l >> 4) + 4 * reg -- NOT the f32 map ((l >> 4) * 4 + reg).
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;
typedef _Float16 f16;

constexpr int SLAB = GSTVD_GAUSS_FIT_SLAB;
constexpr int TILE = 64;                                      // covariance tile of a workgroup
constexpr int TILE_ELEMS = TILE * TILE;
constexpr int LP_ROWS = 32;                                   // scored rows of a workgroup: two MFMA column blocks

DEVFN double widen(float v) { return (double)v; }
DEVFN double widen(f16 v) { return (double)v; }
DEVFN f64x4 mfma_f64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

struct FitWs {                                                // the workspace, cut up
  double* colsum;                                             // [nslab][D]
  double* part;                                               // [ntiles][nslab][TILE_ELEMS], fragment order
  uint32_t* ticket;                                           // [ntiles]
};

template <typename T>
__global__ __launch_bounds__(256) void gauss_colsum_kernel(const T* x, int64_t ldx, int64_t N, int D, FitWs ws, int ntiles) {
  __shared__ double red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + tx;
  const int64_t n0 = (int64_t)blockIdx.y * SLAB, n1 = n0 + SLAB < N ? n0 + SLAB : N;
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (int t = threadIdx.x; t < ntiles; t += 256) ws.ticket[t] = 0;
  double s = 0.0;
  if (col < D)
    for (int64_t n = n0 + ty; n < n1; n += 4) s += widen(x[n * ldx + col]);
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && col < D) ws.colsum[(int64_t)blockIdx.y * D + col] = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
}

template <typename T>
__global__ __launch_bounds__(256) void gauss_syrk_kernel(gstvd_gauss_fit_t a, FitWs ws, int nslab, double fact) {
  __shared__ double s_sh[2 * TILE + 1];                       // means of the tile's row and column features; [128]: "I am last"
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wi = w >> 1, wj = w & 1, r = lane & 15, kq = lane >> 4;
  const int D = a.D;
  const int t = blockIdx.x, slab = blockIdx.y;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  const int tj = t - ti * (ti + 1) / 2;                       // ti >= tj: a lower tile
  const T* x = (const T*)a.x;

  if (threadIdx.x < 2 * TILE) {
    const int col = (threadIdx.x < TILE ? ti * TILE : tj * TILE - TILE) + threadIdx.x;
    double s = 0.0;
    if (col < D) {
      for (int sl = 0; sl < nslab; ++sl) s += ws.colsum[(int64_t)sl * D + col];
      s = s / (double)a.N;
      if (slab == 0 && tj == 0 && threadIdx.x < TILE) a.mean[col] = s;      // every column once: the row features of the tiles (ti, 0)
    }
    s_sh[threadIdx.x] = s;
  }
  __syncthreads();

  int ci[2], cj[2];
  double mi[2], mj[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    ci[h] = ti * TILE + wi * 32 + h * 16 + r;
    cj[h] = tj * TILE + wj * 32 + h * 16 + r;
    mi[h] = s_sh[wi * 32 + h * 16 + r];
    mj[h] = s_sh[TILE + wj * 32 + h * 16 + r];
  }
  f64x4 acc[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[p][q] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int64_t n0 = (int64_t)slab * SLAB, n1 = n0 + SLAB < a.N ? n0 + SLAB : a.N;
  if (!(ti == tj && wi < wj)) {                               // a quadrant above the diagonal is never written
    const int rows = (int)(n1 - n0);
    const T* row = x + (n0 + kq) * a.ldx;
    for (int nb = 0; nb < rows; nb += 16, row += 16 * a.ldx) {   // four K-steps a turn: sixteen loads in flight, then sixteen MFMAs
      double xa[4][2], xb[4][2];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool live = nb + 4 * u + kq < rows;
        const T* ru = row + 4 * u * a.ldx;
#pragma unroll
        for (int h = 0; h < 2; ++h) {                         // a dead row or column is a centred zero, not -mean
          xa[u][h] = (live && ci[h] < D) ? widen(ru[ci[h]]) - mi[h] : 0.0;
          xb[u][h] = (live && cj[h] < D) ? widen(ru[cj[h]]) - mj[h] : 0.0;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int q = 0; q < 2; ++q) acc[p][q] = mfma_f64(xa[u][p], xb[u][q], acc[p][q]);
    }
  }

  // ---- the partial tile, in fragment order; release; ticket
  double* mine = ws.part + ((int64_t)t * nslab + slab) * TILE_ELEMS;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) mine[(((w * 4 + p * 2 + q) * 4 + g) << 6) + lane] = acc[p][q][g];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t drawn = __hip_atomic_fetch_add(ws.ticket + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = drawn == (uint32_t)(nslab - 1);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_sh[2 * TILE] = last ? 1.0 : 0.0;
  }
  __syncthreads();
  if (s_sh[2 * TILE] == 0.0) return;

  // ---- the tile's last block: partials in ascending slab order, one scaling, the tile and its mirror
  const double* all = ws.part + (int64_t)t * nslab * TILE_ELEMS;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = ti * TILE + wi * 32 + p * 16 + kq + 4 * g, j = cj[q];
        if (i >= D || j >= D || i < j) continue;
        const int e = (((w * 4 + p * 2 + q) * 4 + g) << 6) + lane;
        double s = 0.0;
        for (int sl = 0; sl < nslab; ++sl) s += all[(int64_t)sl * TILE_ELEMS + e];
        const double v = fact * s;
        a.cov[(int64_t)i * D + j] = v;
        a.cov[(int64_t)j * D + i] = v;
      }
}

template <typename T>
__global__ __launch_bounds__(256) void gauss_logprob_kernel(gstvd_gauss_logprob_t a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int D = a.D, LD = D + (int)(16 / sizeof(T));          // 16 bytes of row padding: the 16 rows of an operand read spread over the banks
  double* s_mean = (double*)smem;                             // [D]
  double* s_q = s_mean + D;                                   // [4 waves][LP_ROWS]
  T* xs = (T*)(s_q + 4 * LP_ROWS);                            // [LP_ROWS][LD]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * LP_ROWS;
  const T* x = (const T*)a.x;

  for (int e = threadIdx.x; e < LP_ROWS * D; e += 256) {
    const int row = e / D, c = e - row * D;
    const int64_t m = m0 + row;
    xs[row * LD + c] = m < a.M ? x[m * a.ldx + c] : (T)0;
  }
  for (int c = threadIdx.x; c < D; c += 256) s_mean[c] = a.mean[c];
  __syncthreads();

  const int nt = D >> 4;
  double q0 = 0.0, q1 = 0.0;
  const T* x0 = xs + r * LD + kq;
  const T* x1 = x0 + 16 * LD;
  for (int g = 0; 4 * g < nt; ++g) {
    const int it = 4 * g + ((g & 1) ? 3 - w : w);             // the snake: wave w's blocks cost as much as wave 3 - w's
    if (it >= nt) continue;
    f64x4 z0 = {0.0, 0.0, 0.0, 0.0}, z1 = {0.0, 0.0, 0.0, 0.0};
    const double* wp = a.w_packed + (int64_t)128 * it * (it + 1) + lane;
    const int nks = 4 * it + 4;                               // K-steps up to and with the diagonal block
    for (int k4 = 0; k4 < nks; k4 += 4) {                     // nks % 4 == 0: four K-steps a turn, their loads in flight together
      double av[4], b0[4], b1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ks = k4 + u;
        av[u] = wp[ks << 6];
        const double mk = s_mean[4 * ks + kq];
        b0[u] = widen(x0[4 * ks]) - mk;
        b1[u] = widen(x1[4 * ks]) - mk;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        z0 = mfma_f64(av[u], b0[u], z0);
        z1 = mfma_f64(av[u], b1[u], z1);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { q0 += z0[e] * z0[e]; q1 += z1[e] * z1[e]; }
  }
  q0 += __shfl_xor(q0, 16, WAVE); q0 += __shfl_xor(q0, 32, WAVE);
  q1 += __shfl_xor(q1, 16, WAVE); q1 += __shfl_xor(q1, 32, WAVE);
  if (kq == 0) { s_q[w * LP_ROWS + r] = q0; s_q[w * LP_ROWS + 16 + r] = q1; }
  __syncthreads();
  if (threadIdx.x < LP_ROWS) {
    const int64_t m = m0 + threadIdx.x;
    bool kept = false;
    if (m < a.M) {
      const double q = ((s_q[threadIdx.x] + s_q[LP_ROWS + threadIdx.x]) + s_q[2 * LP_ROWS + threadIdx.x]) + s_q[3 * LP_ROWS + threadIdx.x];
      const double lp = (-0.5 * (a.klog2pi + q)) - a.half_log_det;
      a.out[m] = lp;
      kept = lp >= a.threshold;
      if (a.keep) a.keep[m] = kept ? 1 : 0;
    }
    if (a.n_kept) {
      const int n = __popcll(__ballot(kept));
      if (threadIdx.x == 0 && n > 0) atomicAdd((unsigned long long*)a.n_kept, (unsigned long long)n);
    }
  }
}

bool gauss_dim_ok(int32_t D) { return D >= 16 && D <= GSTVD_GAUSS_MAX_D && D % 16 == 0; }
int64_t gauss_nslab(int64_t N) { return (N + SLAB - 1) / SLAB; }

template <typename T> int fit_go(const gstvd_gauss_fit_t& a, hipStream_t s) {
  const int nslab = (int)gauss_nslab(a.N), tiles = (a.D + TILE - 1) / TILE, ntiles = tiles * (tiles + 1) / 2;
  FitWs ws;
  ws.colsum = (double*)a.workspace;
  ws.part = ws.colsum + (int64_t)nslab * a.D;
  ws.ticket = (uint32_t*)(ws.part + (int64_t)ntiles * nslab * TILE_ELEMS);
  hipLaunchKernelGGL(gauss_colsum_kernel<T>, dim3((a.D + 63) / 64, nslab), dim3(256), 0, s, (const T*)a.x, a.ldx, a.N, a.D, ws, ntiles);
  GSTVD_LAUNCH_CHECK();
  hipLaunchKernelGGL(gauss_syrk_kernel<T>, dim3(ntiles, nslab), dim3(256), 0, s, a, ws, nslab, 1.0 / (double)(a.N - 1));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

template <typename T> int logprob_go(const gstvd_gauss_logprob_t& a, hipStream_t s) {
  const size_t fixed = ((size_t)GSTVD_GAUSS_MAX_D + 4 * LP_ROWS) * sizeof(double);
  const size_t lds = ((size_t)a.D + 4 * LP_ROWS) * sizeof(double) + (size_t)LP_ROWS * (a.D * sizeof(T) + 16);
  if (lds > 48 * 1024) {
    static int rc = (int)hipFuncSetAttribute((const void*)gauss_logprob_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(fixed + LP_ROWS * (GSTVD_GAUSS_MAX_D * sizeof(T) + 16)));
    if (rc) return rc;
  }
  hipLaunchKernelGGL(gauss_logprob_kernel<T>, dim3((unsigned)((a.M + LP_ROWS - 1) / LP_ROWS)), dim3(256), lds, s, a);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int64_t gstvd_gauss_fit_ws_bytes(int64_t N, int32_t D) {
  if (!gauss_dim_ok(D) || N < 2 || N > ((int64_t)1 << 28)) return -1;
  const int64_t nslab = gauss_nslab(N), tiles = (D + TILE - 1) / TILE, ntiles = tiles * (tiles + 1) / 2;
  return 8 * (nslab * D + ntiles * nslab * TILE_ELEMS) + 4 * ntiles;
}

extern "C" int gstvd_gauss_fit(const gstvd_gauss_fit_t* a, gstvd_stream_t s) {
  if (!a || !a->x || !a->mean || !a->cov || !a->workspace) return GSTVD_E_NULL;
  if (a->dtype != GSTVD_F16 && a->dtype != GSTVD_F32) return GSTVD_E_DTYPE;
  const int64_t need = gstvd_gauss_fit_ws_bytes(a->N, a->D);
  if (need < 0 || a->ldx < a->D || a->workspace_bytes < need) return GSTVD_E_SHAPE;
  if ((uintptr_t)a->workspace % 8 || (uintptr_t)a->mean % 8 || (uintptr_t)a->cov % 8) return GSTVD_E_ALIGN;
  return a->dtype == GSTVD_F16 ? fit_go<f16>(*a, (hipStream_t)s) : fit_go<float>(*a, (hipStream_t)s);
}

extern "C" int64_t gstvd_gauss_w_packed_elems(int32_t D) {
  if (!gauss_dim_ok(D)) return -1;
  const int64_t t = D / 16;
  return 128 * t * (t + 1);
}

extern "C" int gstvd_gauss_logprob(const gstvd_gauss_logprob_t* a, gstvd_stream_t s) {
  if (!a || !a->x || !a->mean || !a->w_packed || !a->out) return GSTVD_E_NULL;
  if (a->dtype != GSTVD_F16 && a->dtype != GSTVD_F32) return GSTVD_E_DTYPE;
  if (!gauss_dim_ok(a->D) || a->M < 1 || a->M > 0x7fffffff || a->ldx < a->D) return GSTVD_E_SHAPE;
  if ((uintptr_t)a->mean % 8 || (uintptr_t)a->w_packed % 8 || (uintptr_t)a->out % 8 || (a->n_kept && (uintptr_t)a->n_kept % 8))
    return GSTVD_E_ALIGN;
  return a->dtype == GSTVD_F16 ? logprob_go<f16>(*a, (hipStream_t)s) : logprob_go<float>(*a, (hipStream_t)s);
}
