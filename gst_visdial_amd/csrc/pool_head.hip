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
#include "loss_reduce.h"

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

// Training form (gstvd_nsp_train_fwd; train_disc.py, models/vilbert_dialog.py:1026-1041,1509-1510): the same launch plus what
// backward needs -- pt, pv [B, Hb] fp32, the keep flags of the Dropout(0.1) in front of the classifier (drawn from the engine's
// counter stream at element b * Hb + n) -- and, in place of prob0, the soft-label loss
//   row_loss[b] = -(l[b, 0] * log_softmax(z[b])[0] + l[b, 1] * log_softmax(z[b])[1]),   stats = (sum_b, B, sum_b / B).
struct NspTrainP : NspP {
  const float* labels; int64_t ldl;
  float* pt; float* pv; uint8_t* keep; float* row_loss;
  float p; uint32_t site; const uint64_t* rng;
};
template <bool TRAIN> struct NspArgs { typedef NspP type; };
template <> struct NspArgs<true> { typedef NspTrainP type; };

// ONE body for both forms: what TRAIN adds sits under `if constexpr`, so the inference instantiation neither carries nor reads a
// training field, and z is accumulated by the same instructions in the same order in both -- with p = 0 the same bits.
template <typename T, bool TRAIN>
__global__ __launch_bounds__(NSP_WAVES * 64) void nsp_head_kernel(typename NspArgs<TRAIN>::type q) {
  const NspP& p = q;
  constexpr int PAD = NspCfg<T>::PAD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* xs_t = (T*)smem;
  T* xs_v = xs_t + NSP_ROWS * (p.H + PAD);
  float* zpart = (float*)(xs_v + NSP_ROWS * (p.Hv + PAD));        // [wave][row][2]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int64_t m0 = (int64_t)blockIdx.x * NSP_ROWS;
  DropKey dk;
  if constexpr (TRAIN) dk = make_drop(q.p, q.site, q.rng);

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
    const int64_t m = m0 + li;
    f32x4 fac, pt4, pv4;
    uint32_t kb = 0;
    if constexpr (TRAIN) fac = drop_factor4(dk, (uint64_t)(m * p.Hb + n));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pt = fmaxf(at[r] + b1[r], 0.f), pv = fmaxf(av[r] + b2[r], 0.f);
      float f = p.sum ? pt + pv : pt * pv;
      if constexpr (TRAIN) {
        pt4[r] = pt; pv4[r] = pv;
        if (dk.on) f *= fac[r];
        kb |= (fac[r] != 0.f ? 1u : 0u) << (8 * r);
      }
      z0 += f * w0[r];
      z1 += f * w1[r];
    }
    if constexpr (TRAIN) {
      if (m < p.B) {
        *(f32x4*)(q.pt + m * p.Hb + n) = pt4;
        *(f32x4*)(q.pv + m * p.Hb + n) = pv4;
        *(uint32_t*)(q.keep + m * p.Hb + n) = kb;
      }
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
    if constexpr (TRAIN) {
      const double lse = mx + log(e0 + e1);
      const double l0 = (double)q.labels[m * q.ldl], l1 = (double)q.labels[m * q.ldl + 1];
      q.row_loss[m] = (float)(-(l0 * ((double)s0 - lse) + l1 * ((double)s1 - lse)));
    } else {
      p.prob0[m] = (float)(e0 / (e0 + e1));
    }
  }
}

template <typename T, bool TRAIN>
static int nsp_launch(const typename NspArgs<TRAIN>::type& q, char* name, int32_t name_len, hipStream_t s) {
  constexpr int PAD = NspCfg<T>::PAD;
  const int lds = NSP_ROWS * (q.H + PAD + q.Hv + PAD) * (int)sizeof(T) + NSP_WAVES * NSP_ROWS * 2 * 4;
  auto k = nsp_head_kernel<T, TRAIN>;
  static int attr_rc = ensure_lds(k, NSP_ROWS * (1024 + PAD) * 2 * (int)sizeof(T) + NSP_WAVES * NSP_ROWS * 2 * 4);
  if (attr_rc) return attr_rc;
  if (name) {
    const int rc = copy_kernel_name((const void*)k, name, name_len);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k, dim3((unsigned)((q.B + NSP_ROWS - 1) / NSP_ROWS)), dim3(NSP_WAVES * 64), lds, s, q);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

// The conditions both entry points share, as four steps in the order the return codes are tested; an entry point puts its own
// conditions into the step they belong to (`null_own`: one of its own pointers is NULL; `shape_own`; `own16` / `own4`: its own
// pointers that must be 16- / 4-byte aligned, or-ed together).  gstvd_nsp_head_t and gstvd_nsp_train_t name the shared fields alike.
template <typename A>
static int nsp_fwd_check(const A* a, bool null_own, bool shape_own, uintptr_t own16, uintptr_t own4) {
  if (!a->xt || !a->xv || !a->wt || !a->wv || !a->bt || !a->bv || !a->wn || !a->bn || !a->z || null_own) return GSTVD_E_NULL;
  if (a->dtype != GSTVD_BF16 && a->dtype != GSTVD_F32) return GSTVD_E_DTYPE;
  if (a->fusion != 0 && a->fusion != 1) return GSTVD_E_UNSUPPORTED;
  if (a->kernel_name && a->kernel_name_len <= 1) return GSTVD_E_SHAPE;
  const int dims[3] = {a->H, a->Hv, a->Hb};
  for (int d : dims)
    if (d <= 0 || d % 16 || d > 1024) return GSTVD_E_SHAPE;
  if (a->B <= 0 || a->t_rows <= 0 || a->v_rows <= 0) return GSTVD_E_SHAPE;
  if (a->ldt < a->H || a->ldv < a->Hv || a->ldwt < a->H || a->ldwv < a->Hv || a->ldwn < a->Hb || a->ldz < 2 || shape_own) return GSTVD_E_SHAPE;
  const int ve = a->dtype == GSTVD_BF16 ? 8 : 4;
  if ((a->ldt % ve) || (a->ldv % ve) || (a->ldwt % ve) || (a->ldwv % ve) || (a->ldwn % 4)) return GSTVD_E_ALIGN;
  if (((uintptr_t)a->xt | (uintptr_t)a->xv | (uintptr_t)a->wt | (uintptr_t)a->wv | (uintptr_t)a->bt | (uintptr_t)a->bv |
       (uintptr_t)a->wn | own16) & 15)
    return GSTVD_E_ALIGN;
  if (((uintptr_t)a->bn | (uintptr_t)a->z | own4) & 3) return GSTVD_E_ALIGN;
  return 0;
}

template <typename A>
static void nsp_pack(NspP& p, const A* a, float* prob0) {
  p.xt = (const char*)a->xt; p.xv = (const char*)a->xv; p.wt = (const char*)a->wt; p.wv = (const char*)a->wv;
  p.bt = a->bt; p.bv = a->bv; p.wn = a->wn; p.bn = a->bn; p.z = a->z; p.prob0 = prob0;
  p.ldt = a->ldt; p.ldv = a->ldv; p.sbt = a->t_rows * a->ldt; p.sbv = a->v_rows * a->ldv;
  p.ldwt = a->ldwt; p.ldwv = a->ldwv; p.ldwn = a->ldwn; p.ldz = a->ldz;
  p.B = a->B; p.H = a->H; p.Hv = a->Hv; p.Hb = a->Hb; p.sum = a->fusion;
}

extern "C" int gstvd_nsp_head(const gstvd_nsp_head_t* a, gstvd_stream_t stream) {
  if (!a) return GSTVD_E_NULL;
  const int rc = nsp_fwd_check(a, !a->prob0, false, 0, (uintptr_t)a->prob0);
  if (rc) return rc;
  NspP p;
  nsp_pack(p, a, a->prob0);
  GSTVD_FOR_DTYPE(a->dtype, T, return (nsp_launch<T, false>(p, a->kernel_name, a->kernel_name_len, (hipStream_t)stream)));
}

extern "C" int gstvd_nsp_train_fwd(const gstvd_nsp_train_t* a, gstvd_stream_t stream) {
  if (!a) return GSTVD_E_NULL;
  const int rc = nsp_fwd_check(a, !a->labels || !a->pt || !a->pv || !a->keep || !a->row_loss || !a->stats,
                               a->ldl < 2 || !(a->p >= 0.f && a->p < 1.f) || (a->p > 0.f && !a->rng), (uintptr_t)a->pt | (uintptr_t)a->pv,
                               (uintptr_t)a->labels | (uintptr_t)a->row_loss | (uintptr_t)a->stats | (uintptr_t)a->keep);
  if (rc) return rc;
  NspTrainP q;
  nsp_pack(q, a, nullptr);
  q.labels = a->labels; q.ldl = a->ldl; q.pt = a->pt; q.pv = a->pv; q.keep = a->keep; q.row_loss = a->row_loss;
  q.p = a->p; q.site = a->site; q.rng = a->rng;
  hipStream_t s = (hipStream_t)stream;
  GSTVD_FOR_DTYPE(a->dtype, T, {
    const int lrc = nsp_launch<T, true>(q, a->kernel_name, a->kernel_name_len, s);
    if (lrc) return lrc;
  });
  hipLaunchKernelGGL(row_loss_reduce_kernel, dim3(1), dim3(64), 0, s, (const float*)a->row_loss, (const int64_t*)nullptr, (int64_t)0, 0,
                     (int64_t)a->B, a->stats);      // every row counts
  GSTVD_LAUNCH_CHECK();
  return 0;
}

// Backward of loss = gscale * sum_b row_loss[b] / B down to the gradients in front of the two ReLUs:
//   dz[b, j] = gscale / B * (softmax(z[b])[j] * (l[b, 0] + l[b, 1]) - l[b, j])           (soft labels: their sum is not assumed 1)
//   d wn[j, n] (=|+=) sum_b dz[b, j] * fd[b, n],   d bn[j] (=|+=) sum_b dz[b, j],            fd = dropout(f)
//   df[b, n] = keep * (dz[b, 0] wn[0, n] + dz[b, 1] wn[1, n]);  mul: dpt = df * pv, dpv = df * pt;  sum: both df;  x [pre-ReLU > 0]
// A workgroup owns 64 columns; its four waves take the batch rows b = w, w + 4, ... and their partial sums meet in LDS in wave
// order: fixed order, no atomics.
struct NspBwdP {
  const float* pt; const float* pv; const uint8_t* keep; const float* z; int64_t ldz; const float* labels; int64_t ldl;
  const float* wn; int64_t ldwn; const float* gscale;
  float* dwn; int64_t lddwn; float* dbn; void* dpt; void* dpv; int64_t lddp;
  int B, Hb, sum, acc_w, acc_b; float p;
};

template <typename T>
__global__ __launch_bounds__(256) void nsp_train_bwd_kernel(NspBwdP q) {
  __shared__ float part[4][64][2];
  __shared__ float partb[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + lane;
  const bool in = n < q.Hb;
  const float w0 = in ? q.wn[n] : 0.f, w1 = in ? q.wn[q.ldwn + n] : 0.f;
  const float scale = (q.gscale ? q.gscale[0] : 1.f) / (float)q.B;
  const float ks = q.p > 0.f ? 1.f / (1.f - q.p) : 1.f;
  float a0 = 0.f, a1 = 0.f, sb0 = 0.f, sb1 = 0.f;
  for (int b = wave; b < q.B; b += 4) {
    const float z0 = q.z[(int64_t)b * q.ldz], z1 = q.z[(int64_t)b * q.ldz + 1];
    const float l0 = q.labels[(int64_t)b * q.ldl], l1 = q.labels[(int64_t)b * q.ldl + 1];
    const float mx = fmaxf(z0, z1);
    const float e0 = expf(z0 - mx), e1 = expf(z1 - mx);
    const float inv = 1.f / (e0 + e1), sl = l0 + l1;
    const float dz0 = scale * (e0 * inv * sl - l0), dz1 = scale * (e1 * inv * sl - l1);
    sb0 += dz0;
    sb1 += dz1;
    if (in) {
      const int64_t e = (int64_t)b * q.Hb + n;
      const float pt = q.pt[e], pv = q.pv[e];
      const float kf = q.keep[e] ? ks : 0.f;
      const float fd = (q.sum ? pt + pv : pt * pv) * kf;
      a0 += dz0 * fd;
      a1 += dz1 * fd;
      const float df = (dz0 * w0 + dz1 * w1) * kf;
      const float gt = pt > 0.f ? (q.sum ? df : df * pv) : 0.f;
      const float gv = pv > 0.f ? (q.sum ? df : df * pt) : 0.f;
      ((T*)q.dpt)[(int64_t)b * q.lddp + n] = from_f<T>(gt);
      ((T*)q.dpv)[(int64_t)b * q.lddp + n] = from_f<T>(gv);
    }
  }
  part[wave][lane][0] = a0;
  part[wave][lane][1] = a1;
  if (lane == 0) { partb[wave][0] = sb0; partb[wave][1] = sb1; }
  __syncthreads();
  if (wave == 0) {
    if (in) {
      float s0 = part[0][lane][0], s1 = part[0][lane][1];
#pragma unroll
      for (int w = 1; w < 4; ++w) { s0 += part[w][lane][0]; s1 += part[w][lane][1]; }
      q.dwn[n] = q.acc_w ? q.dwn[n] + s0 : s0;
      q.dwn[q.lddwn + n] = q.acc_w ? q.dwn[q.lddwn + n] + s1 : s1;
    }
    if (blockIdx.x == 0 && lane < 2) {
      float s = partb[0][lane];
#pragma unroll
      for (int w = 1; w < 4; ++w) s += partb[w][lane];
      q.dbn[lane] = q.acc_b ? q.dbn[lane] + s : s;
    }
  }
}

extern "C" int gstvd_nsp_train_bwd(const gstvd_nsp_train_t* a, gstvd_stream_t stream) {
  if (!a || !a->pt || !a->pv || !a->keep || !a->z || !a->labels || !a->wn || !a->dwn || !a->dbn || !a->dpt || !a->dpv) return GSTVD_E_NULL;
  if (a->dtype != GSTVD_BF16 && a->dtype != GSTVD_F32) return GSTVD_E_DTYPE;
  if (a->fusion != 0 && a->fusion != 1) return GSTVD_E_UNSUPPORTED;
  if (a->B <= 0 || a->Hb <= 0 || (a->Hb % 16) || a->Hb > 1024 || a->ldwn < a->Hb || a->lddwn < a->Hb || a->lddp < a->Hb || a->ldz < 2 ||
      a->ldl < 2)
    return GSTVD_E_SHAPE;
  if (!(a->p >= 0.f && a->p < 1.f)) return GSTVD_E_SHAPE;
  NspBwdP q;
  q.pt = a->pt; q.pv = a->pv; q.keep = a->keep; q.z = a->z; q.ldz = a->ldz; q.labels = a->labels; q.ldl = a->ldl;
  q.wn = a->wn; q.ldwn = a->ldwn; q.gscale = a->gscale;
  q.dwn = a->dwn; q.lddwn = a->lddwn; q.dbn = a->dbn; q.dpt = a->dpt; q.dpv = a->dpv; q.lddp = a->lddp;
  q.B = a->B; q.Hb = a->Hb; q.sum = a->fusion; q.acc_w = a->acc_w; q.acc_b = a->acc_b; q.p = a->p;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((a->Hb + 63) / 64));
  GSTVD_FOR_DTYPE(a->dtype, T, hipLaunchKernelGGL(nsp_train_bwd_kernel<T>, grid, dim3(256), 0, s, q));
  GSTVD_LAUNCH_CHECK();
  return 0;
}
