// NSP head of the discriminative (enc_only) model, one launch (gstvd_nsp_head in include/gstvd_hip.h):
//   first-token gather -> the two poolers (Linear + ReLU) -> mul / sum fusion -> bi_seq_relationship -> 2-way softmax
// (models/vilbert_dialog.py:915-941,1026-1041; evaluate_disc.py:79-83).
//
//  * a workgroup owns 16 batch rows and ALL Hb pooler columns: row 0 of each batch row is copied from the encoder's activation
//    buffers straight into LDS (no [B, H] staging tensor in memory), the pooler weights stream from global memory into MFMA
//    fragments exactly once per workgroup (a full 128-byte line of a weight row per fragment load);
//  * the MFMA runs with the WEIGHTS on the accumulator rows: a lane ends up with pt and pv of 4 consecutive columns of one
//    batch row, so bias, ReLU, fusion and the 2-wide classifier are lane-local fp32 arithmetic -- pt, pv, f never leave registers;
//  * the classifier's sum over the Hb columns: in the lane over its column tiles, then over the four 16-lane rows of the wave,
//    then over the waves through LDS in wave order -- fixed order, no atomics, no cross-workgroup reduction: bit-reproducible.
#include "gemm_common.h"

struct NspP {
  const char* xt; const char* xv; const char* wt; const char* wv;
  const float* bt; const float* bv; const float* wn; const float* bn;
  float* z; float* prob0;
  int64_t ldt, ldv, sbt, sbv, ldwt, ldwv, ldwn, ldz;      // sb*: elements between the first rows of consecutive batch rows
  int B, H, Hv, Hb, sum;
};

constexpr int NSP_ROWS = 16, NSP_WAVES = 8;
template <typename T> struct NspCfg;
template <> struct NspCfg<bf16> { static constexpr int VE = 8, PAD = 8; };      // LDS rows padded by 16 bytes
template <> struct NspCfg<float> { static constexpr int VE = 4, PAD = 4; };

// acc[r] += sum_k W[n0 + 4g + r][k] * X[li][k]: `wrow` = row n0 + li of the weights (global), `xrow` = row li of the LDS image.
// The k index a lane feeds to an MFMA step is permuted the same way for both operands (lane group g takes 16 consecutive k of
// every 64: a whole cache line of the weight row per step across the four groups), which leaves every product in the sum.
// Four steps are issued together (clamped addresses + selects instead of branches for the tail), so a lane has eight 16-byte
// weight loads in flight: the loop is bound by the latency of the weight stream, nothing else.
DEVFN void nsp_dot(f32x4& acc, const bf16* wrow, const bf16* xrow, int K, int g) {
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const bf16x8 zero = __builtin_bit_cast(bf16x8, (s16x8){0, 0, 0, 0, 0, 0, 0, 0});
  for (int k0 = 0; k0 < K; k0 += 256) {
    bf16x8 w[8], x[8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 64 * u + 16 * g;
      const bool in = k < K;               // K % 16 == 0: a lane's 16 elements are all inside or all outside
      const int kc = in ? k : 0;
      w[2 * u] = *(const bf16x8*)(wrow + kc);
      w[2 * u + 1] = *(const bf16x8*)(wrow + kc + 8);
      x[2 * u] = *(const bf16x8*)(xrow + kc);
      x[2 * u + 1] = *(const bf16x8*)(xrow + kc + 8);
      if (!in) { w[2 * u] = zero; w[2 * u + 1] = zero; x[2 * u] = zero; x[2 * u + 1] = zero; }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = mfma_bf16_k32(w[u], x[u], acc);
  }
}
DEVFN void nsp_dot(f32x4& acc, const float* wrow, const float* xrow, int K, int g) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 64) {
    f32x4 w[4], x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 16 * u + 4 * g;
      const bool in = k < K;               // K % 16 == 0
      const int kc = in ? k : 0;
      w[u] = *(const f32x4*)(wrow + kc);
      x[u] = *(const f32x4*)(xrow + kc);
      if (!in) { w[u] = zero; x[u] = zero; }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = mfma_f32_k4(w[u][e], x[u][e], acc);
  }
}

// row 0 of batch rows m0 .. m0 + 15 -> LDS image [16][K + PAD] (rows past B: zeros)
template <typename T>
DEVFN void nsp_stage(T* img, const char* x, int64_t sb, int K, int64_t m0, int B, int tid) {
  constexpr int VE = NspCfg<T>::VE, PAD = NspCfg<T>::PAD;
  const int vpr = K / VE;
  for (int v = tid; v < NSP_ROWS * vpr; v += NSP_WAVES * 64) {
    const int r = v / vpr, c = (v % vpr) * VE;
    u32x4 val = {0u, 0u, 0u, 0u};
    if (m0 + r < B) val = *(const u32x4*)(x + ((m0 + r) * sb + c) * (int64_t)sizeof(T));
    *(u32x4*)(img + r * (K + PAD) + c) = val;
  }
}

template <typename T>
__global__ __launch_bounds__(NSP_WAVES * 64) void nsp_head_kernel(NspP p) {
  constexpr int PAD = NspCfg<T>::PAD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* xs_t = (T*)smem;
  T* xs_v = xs_t + NSP_ROWS * (p.H + PAD);
  float* zpart = (float*)(xs_v + NSP_ROWS * (p.Hv + PAD));        // [wave][row][2]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int64_t m0 = (int64_t)blockIdx.x * NSP_ROWS;

  nsp_stage<T>(xs_t, p.xt, p.sbt, p.H, m0, p.B, tid);
  nsp_stage<T>(xs_v, p.xv, p.sbv, p.Hv, m0, p.B, tid);
  __syncthreads();

  // lane: batch row m0 + li, pooler columns n0 + 4g .. + 3 of every column tile of its wave
  float z0 = 0.f, z1 = 0.f;
  for (int n0 = wave * 16; n0 < p.Hb; n0 += NSP_WAVES * 16) {
    f32x4 at = {0.f, 0.f, 0.f, 0.f}, av = at;
    nsp_dot(at, (const T*)p.wt + (int64_t)(n0 + li) * p.ldwt, xs_t + li * (p.H + PAD), p.H, g);
    nsp_dot(av, (const T*)p.wv + (int64_t)(n0 + li) * p.ldwv, xs_v + li * (p.Hv + PAD), p.Hv, g);
    const int n = n0 + 4 * g;
    const f32x4 b1 = *(const f32x4*)(p.bt + n), b2 = *(const f32x4*)(p.bv + n);
    const f32x4 w0 = *(const f32x4*)(p.wn + n), w1 = *(const f32x4*)(p.wn + p.ldwn + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pt = fmaxf(at[r] + b1[r], 0.f), pv = fmaxf(av[r] + b2[r], 0.f);
      const float f = p.sum ? pt + pv : pt * pv;
      z0 += f * w0[r];
      z1 += f * w1[r];
    }
  }
  z0 = rows_sum(z0);
  z1 = rows_sum(z1);
  if (g == 0) { zpart[(wave * NSP_ROWS + li) * 2] = z0; zpart[(wave * NSP_ROWS + li) * 2 + 1] = z1; }
  __syncthreads();
  if (tid < NSP_ROWS && m0 + tid < p.B) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int w = 0; w < NSP_WAVES; ++w) { s0 += zpart[(w * NSP_ROWS + tid) * 2]; s1 += zpart[(w * NSP_ROWS + tid) * 2 + 1]; }
    s0 += p.bn[0];
    s1 += p.bn[1];
    const int64_t m = m0 + tid;
    p.z[m * p.ldz] = s0;
    p.z[m * p.ldz + 1] = s1;
    // one value per batch row: evaluated in double, so the fp32 result is the correctly rounded one (denormal tail included)
    const double mx = (double)fmaxf(s0, s1);
    const double e0 = exp((double)s0 - mx), e1 = exp((double)s1 - mx);
    p.prob0[m] = (float)(e0 / (e0 + e1));
  }
}

template <typename T>
static int nsp_launch(const NspP& p, char* name, int32_t name_len, hipStream_t s) {
  constexpr int PAD = NspCfg<T>::PAD;
  const int lds = NSP_ROWS * (p.H + PAD + p.Hv + PAD) * (int)sizeof(T) + NSP_WAVES * NSP_ROWS * 2 * 4;
  auto k = nsp_head_kernel<T>;
  static int attr_rc = ensure_lds(k, NSP_ROWS * (1024 + PAD) * 2 * (int)sizeof(T) + NSP_WAVES * NSP_ROWS * 2 * 4);
  if (attr_rc) return attr_rc;
  if (name) {
    const int rc = copy_kernel_name((const void*)k, name, name_len);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k, dim3((unsigned)((p.B + NSP_ROWS - 1) / NSP_ROWS)), dim3(NSP_WAVES * 64), lds, s, p);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_nsp_head(const gstvd_nsp_head_t* a, gstvd_stream_t stream) {
  if (!a || !a->xt || !a->xv || !a->wt || !a->wv || !a->bt || !a->bv || !a->wn || !a->bn || !a->z || !a->prob0) return GSTVD_E_NULL;
  if (a->dtype != GSTVD_BF16 && a->dtype != GSTVD_F32) return GSTVD_E_DTYPE;
  if (a->fusion != 0 && a->fusion != 1) return GSTVD_E_UNSUPPORTED;
  if (a->kernel_name && a->kernel_name_len <= 1) return GSTVD_E_SHAPE;
  const int dims[3] = {a->H, a->Hv, a->Hb};
  for (int d : dims)
    if (d <= 0 || d % 16 || d > 1024) return GSTVD_E_SHAPE;
  if (a->B <= 0 || a->t_rows <= 0 || a->v_rows <= 0) return GSTVD_E_SHAPE;
  if (a->ldt < a->H || a->ldv < a->Hv || a->ldwt < a->H || a->ldwv < a->Hv || a->ldwn < a->Hb || a->ldz < 2) return GSTVD_E_SHAPE;
  const int ve = a->dtype == GSTVD_BF16 ? 8 : 4;
  if ((a->ldt % ve) || (a->ldv % ve) || (a->ldwt % ve) || (a->ldwv % ve) || (a->ldwn % 4)) return GSTVD_E_ALIGN;
  if (((uintptr_t)a->xt | (uintptr_t)a->xv | (uintptr_t)a->wt | (uintptr_t)a->wv | (uintptr_t)a->bt | (uintptr_t)a->bv |
       (uintptr_t)a->wn) & 15)
    return GSTVD_E_ALIGN;
  if (((uintptr_t)a->bn | (uintptr_t)a->z | (uintptr_t)a->prob0) & 3) return GSTVD_E_ALIGN;
  NspP p;
  p.xt = (const char*)a->xt; p.xv = (const char*)a->xv; p.wt = (const char*)a->wt; p.wv = (const char*)a->wv;
  p.bt = a->bt; p.bv = a->bv; p.wn = a->wn; p.bn = a->bn; p.z = a->z; p.prob0 = a->prob0;
  p.ldt = a->ldt; p.ldv = a->ldv; p.sbt = a->t_rows * a->ldt; p.sbv = a->v_rows * a->ldv;
  p.ldwt = a->ldwt; p.ldwv = a->ldwv; p.ldwn = a->ldwn; p.ldz = a->ldz;
  p.B = a->B; p.H = a->H; p.Hv = a->Hv; p.Hb = a->Hb; p.sum = a->fusion;
  hipStream_t s = (hipStream_t)stream;
  return a->dtype == GSTVD_BF16 ? nsp_launch<bf16>(p, a->kernel_name, a->kernel_name_len, s)
                                : nsp_launch<float>(p, a->kernel_name, a->kernel_name_len, s);
}
