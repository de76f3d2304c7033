// Attention maps: P = softmax(scale * Q K^T + mask) on its own, fp32, for the descriptor of an attention launch (gstvd_attn_probs).
// The fused kernels of attention.hip never hold a probability outside registers; this one writes them all
// (B * nh * Lq * Lk * 4 bytes), so its layout is chosen for the stores.
//
//   * geometry of the forward: a workgroup of four waves owns 64 queries of one (batch row, head), a wave 16 of them; the keys
//     stream through the LDS row image in chunks of 64 (Stage64, one register stage ahead), and the score tile of 16 keys x 16
//     queries is the forward's own first product (attn_common.h: same operand images, same MFMA, same scale and mask terms);
//   * the score row is computed TWICE and never kept: sweep 1 takes the row maximum m and the row sum l = sum exp(s - m) (running
//     maximum, rescaled per 64-key chunk, all fp32), sweep 2 forms the scores again -- bit for bit the same -- and writes
//     exp(s - m) * (1 / l).  Any key count runs with the same registers; the second sweep costs one more QK^T, 1 / 3 of the forward's
//     MFMA work (at the product shapes a launch is 7-25 us of dependent chunk rounds: timings in DESIGN.md section 8);
//   * stores: the accumulator puts the QUERY on the lane (four consecutive keys per lane), P rows are contiguous in the KEY.  Each
//     wave therefore turns its 16 x 64 tile through a private LDS tile (rows of 68 floats) and stores it with the key on the lane:
//     a 16-byte piece per lane, 256 contiguous bytes per row and four rows per instruction when the rows are 16-byte aligned
//     (Lk % 4 == 0), else one float per lane, 64 consecutive keys of one row per instruction;
//   * head mean: the workgroup walks the heads itself, in ascending order, and adds their probabilities in registers
//     (p_0 + p_1 + ...) * (1 / nh) -- one writer per element, no atomics, the same bits every run.
//   Nothing but Q, K and the key mask is read.
#include "common.h"
#include "attn_common.h"

// Floats per row of a wave's LDS tile: 64 keys + 4.  The 16-byte write of lane (li, g) goes to 4-bank slot (li + g + 4 t) mod 8 of the
// 32 write banks; ds_write_b128 is serviced in groups of 8 CONSECUTIVE lanes (eight li, one g): eight different slots, no conflict
// (lanes (li, g) and (li - 1, g + 1) share a slot but sit 15 lanes apart, in different groups).  The 16-byte read-back (row 4 j + g,
// key 4 li) has one 2-way conflict per 16-lane group of ds_read_b128 (5 LDS cycles for 4); the 4-byte read-back has none.
constexpr int PMAP_PROW = 68;
constexpr int PMAP_TILE = 16 * PMAP_PROW;                     // floats of one wave's tile

// scores of the 64-key chunk at c0 for this lane's query: val[t][r] = s * scale + mask of key c0 + 16 t + 4 g + r (-inf past the end)
template <typename T, int D>
DEVFN void pmap_scores(const gstvd_attn_t& a, const char* sK, const float* smask, const RowFrag<T, D>& qf, int c0, int q, int lane,
                       float (&val)[4][4]) {
  const int g = lane >> 4;
  const int ntile = (a.Lk - c0 + 15) / 16 < 4 ? (a.Lk - c0 + 15) / 16 : 4;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < ntile) {
      const f32x4 s = first_product<T, D>(sK, t * 16, qf, lane);
      f32x4 madd = *(const f32x4*)(smask + t * 16 + 4 * g);
      if (a.causal) {
#pragma unroll
        for (int r = 0; r < 4; ++r) madd[r] = causal_add(a, madd[r], c0 + t * 16 + 4 * g + r, q);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) val[t][r] = __builtin_fmaf(s[r], a.scale, madd[r]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) val[t][r] = -INFINITY;
    }
  }
}

// sweep 1, one chunk: running maximum (over the query's four lanes) and this lane's part of the row sum
DEVFN void pmap_stats_update(const float (&val)[4][4], float& m_run, float& l_part) {
#pragma clang fp contract(off)
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, val[t][r]);
  mx = rows_max(mx);
  const float m_new = fmaxf(m_run, mx);
  float ps = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) ps += __expf(val[t][r] - m_new);
  l_part = l_part * __expf(m_run - m_new) + ps;
  m_run = m_new;
}

// sweep 2, one chunk of one head: p = exp(s - m) * (1 / l), stored into (first head) or added to acc.  No contraction: the sum
// over heads is the plain fp32 sum of the values the per-head launch writes.
template <bool FIRST> DEVFN void pmap_probs(const float (&val)[4][4], float m, float inv, f32x4 (&acc)[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __expf(val[t][r] - m) * inv;
      acc[t][r] = FIRST ? p : acc[t][r] + p;
    }
}

template <typename T, int D, bool MEAN>
__global__ __launch_bounds__(256) void pmap_kernel(gstvd_attn_t a, float* __restrict__ P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  float* smask = (float*)(smem + Img<T, D>::BYTES);
  float* sP = smask + 64;
  float* sstat = sP + 4 * PMAP_TILE;                          // MEAN: [nh][64 queries][m, 1 / l]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int b = blockIdx.z;
  const int q0w = blockIdx.x * 64 + wave * 16, q = q0w + li;
  const bool qv = q < a.Lq;
  const int bk = a.kv_group > 1 ? b / a.kv_group : b;
  const int nhl = MEAN ? a.nh : 1, h0 = MEAN ? 0 : blockIdx.y;
  const int nch = (a.Lk + 63) / 64;
  const T* Qrow = (const T*)a.Q + ((int64_t)b * a.Lq + (qv ? q : 0)) * a.ldq;
  const T* Kb = (const T*)a.K + (int64_t)bk * a.Lk * a.ldk;

  // the K rows and mask terms of a chunk are loaded one chunk ahead of their use; the order of the chunks: sweep 1 head by head,
  // sweep 2 chunk by chunk with the heads inside (items 0 .. 2 * nhl * nch - 1)
  Stage64<T, D> st;
  float mreg = 0.f;
  const int nitem = nhl * nch;
  auto item = [&](int i, int& hh, int& c0) {
    if (i < nitem) { hh = i / nch; c0 = (i - hh * nch) * 64; }
    else { const int j = i - nitem; c0 = (j / nhl) * 64; hh = j - (j / nhl) * nhl; }
  };
  auto load = [&](int i) {
    int hh, c0;
    item(i, hh, c0);
    st.load(Kb + (h0 + hh) * D, a.ldk, c0, a.Lk, tid);
    if (tid < 64) mreg = key_add(a, bk, c0 + tid);
  };
  auto commit = [&](int i) {
    __syncthreads();
    st.store(sK, nullptr, tid);
    if (tid < 64) smask[tid] = mreg;
    __syncthreads();
    if (i + 1 < 2 * nitem) load(i + 1);
  };

  RowFrag<T, D> qf;
  float val[4][4];
  float m_one = 0.f, inv_one = 0.f;                            // !MEAN: the statistics stay in registers
  load(0);
  // ---- sweep 1: row maximum and row sum of every head
  for (int hh = 0; hh < nhl; ++hh) {
    qf.load(Qrow + (h0 + hh) * D, qv, g);
    float m_run = -1e30f, l_part = 0.f;
    for (int c = 0; c < nch; ++c) {
      commit(hh * nch + c);
      pmap_scores<T, D>(a, sK, smask, qf, c * 64, q, lane, val);
      pmap_stats_update(val, m_run, l_part);
    }
    const float inv = 1.0f / rows_sum(l_part);
    if (MEAN) {
      if (g == 0) { sstat[(hh * 64 + wave * 16 + li) * 2] = m_run; sstat[(hh * 64 + wave * 16 + li) * 2 + 1] = inv; }
    } else {
      m_one = m_run; inv_one = inv;
    }
  }
  // ---- sweep 2: the probabilities, chunk by chunk
  const float rn = 1.0f / (float)a.nh;
  const bool vec = (a.Lk & 3) == 0 && ((uintptr_t)P & 15) == 0;
  float* tp = sP + wave * PMAP_TILE;
  const int64_t prow0 = MEAN ? (int64_t)b * a.Lq : ((int64_t)b * a.nh + h0) * a.Lq;      // P row of query 0
  for (int c = 0; c < nch; ++c) {
    const int c0 = c * 64;
    f32x4 acc[4];
    for (int hh = 0; hh < nhl; ++hh) {
      commit(nitem + c * nhl + hh);                           // (its second barrier also orders the sstat writes of sweep 1)
      float m = m_one, inv = inv_one;
      if (MEAN) {
        qf.load(Qrow + hh * D, qv, g);
        m = sstat[(hh * 64 + wave * 16 + li) * 2];
        inv = sstat[(hh * 64 + wave * 16 + li) * 2 + 1];
      }
      pmap_scores<T, D>(a, sK, smask, qf, c0, q, lane, val);
      if (hh == 0) pmap_probs<true>(val, m, inv, acc);
      else pmap_probs<false>(val, m, inv, acc);
    }
    if (MEAN) {
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] *= rn;
    }
    // the wave's 16 queries x 64 keys: query on the lane -> key on the lane (the tile was last read before the barriers of `commit`)
#pragma unroll
    for (int t = 0; t < 4; ++t) *(f32x4*)(tp + li * PMAP_PROW + t * 16 + 4 * g) = acc[t];
    __syncthreads();
    const int nk = a.Lk - c0 < 64 ? a.Lk - c0 : 64;
    if (vec) {
      const int k = 4 * li;                                   // (nk % 4 == 0 here)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * j + g;
        if (q0w + r < a.Lq && k < nk) *(f32x4*)(P + (prow0 + q0w + r) * a.Lk + c0 + k) = *(const f32x4*)(tp + r * PMAP_PROW + k);
      }
    } else {
#pragma unroll 4
      for (int r = 0; r < 16; ++r)
        if (q0w + r < a.Lq && lane < nk) P[(prow0 + q0w + r) * a.Lk + c0 + lane] = tp[r * PMAP_PROW + lane];
    }
  }
}

template <typename K> static int pmap_lds_attr(K kernel, int bytes) {
  if (bytes <= 48 * 1024) return 0;
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return e == hipSuccess ? 0 : (int)e;
}

constexpr int PMAP_MAX_HEADS = 16;                            // head mean: LDS for the statistics of this many heads

template <typename T, int D, bool MEAN> static int pmap_launch(const gstvd_attn_t& a, float* P, hipStream_t s) {
  constexpr int lds = Img<T, D>::BYTES + 64 * 4 + 4 * PMAP_TILE * 4 + (MEAN ? PMAP_MAX_HEADS * 64 * 2 * 4 : 0);
  static int rc = pmap_lds_attr(pmap_kernel<T, D, MEAN>, lds);
  if (rc) return rc;
  dim3 grid((unsigned)((a.Lq + 63) / 64), (unsigned)(MEAN ? 1 : a.nh), (unsigned)a.B);
  hipLaunchKernelGGL((pmap_kernel<T, D, MEAN>), grid, dim3(256), lds, s, a, P);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
template <typename T, int D> static int pmap_m(const gstvd_attn_t& a, float* P, int32_t head_mean, hipStream_t s) {
  return head_mean ? pmap_launch<T, D, true>(a, P, s) : pmap_launch<T, D, false>(a, P, s);
}
template <typename T> static int pmap_d(const gstvd_attn_t& a, float* P, int32_t head_mean, hipStream_t s) {
  if (a.d == 32) return pmap_m<T, 32>(a, P, head_mean, s);
  if (a.d == 64) return pmap_m<T, 64>(a, P, head_mean, s);
  return pmap_m<T, 128>(a, P, head_mean, s);
}

extern "C" int gstvd_attn_probs(const gstvd_attn_t* a, float* P, int32_t head_mean, gstvd_stream_t stream) {
  if (!a || !a->Q || !a->K || !P) return GSTVD_E_NULL;
  if (a->dtype != GSTVD_F32 && a->dtype != GSTVD_BF16) return GSTVD_E_DTYPE;
  if (a->d != 32 && a->d != 64 && a->d != 128) return GSTVD_E_UNSUPPORTED;
  if (a->dropout_p != 0.f || a->q_bstride != 0 || a->kv_bstride != 0) return GSTVD_E_UNSUPPORTED;
  if (a->B <= 0 || a->nh <= 0 || a->Lq <= 0 || a->Lk <= 0 || a->B > 65535 || a->nh > 65535) return GSTVD_E_SHAPE;
  if (a->kv_group > 1 && a->B % a->kv_group) return GSTVD_E_SHAPE;
  if (head_mean && a->nh > PMAP_MAX_HEADS) return GSTVD_E_UNSUPPORTED;
  const int ve = a->dtype == GSTVD_BF16 ? 8 : 4;
  if ((a->ldq % ve) || (a->ldk % ve)) return GSTVD_E_ALIGN;
  if ((((uintptr_t)a->Q | (uintptr_t)a->K) & 15) || ((uintptr_t)P & 3)) return GSTVD_E_ALIGN;
  return a->dtype == GSTVD_BF16 ? pmap_d<bf16>(*a, P, head_mean, (hipStream_t)stream) : pmap_d<float>(*a, P, head_mean, (hipStream_t)stream);
}
