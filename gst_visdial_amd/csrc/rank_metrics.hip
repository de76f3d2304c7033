// Ranking metrics on the device: what utils/visdial_metrics.py does on the host per batch (scores_to_ranks :21-39, SparseGTMetrics
// :41-117, NDCG :119-195) -- ranks of every option, the rank of the ground truth, the NDCG ratio of a list and the additions to a
// device-resident accumulator -- without workspace, allocation or host synchronisation.  include/gstvd_hip.h states the rule in full.
//
//   rank_metrics_kernel   one wave per list, four lists per 256-thread workgroup.  A lane owns options i and i + 64.  The ordered
//                         keys of the list sit in LDS; a rank is a count against the broadcast keys (O compares per owned key, no
//                         sort network; equal keys keep their index order: the stable descending sort).  With a relevance row the
//                         same count over the relevance keys gives the ideal order; both term arrays are laid out by position in
//                         LDS and lanes 0 and 1 add them in ascending position, sequentially, in double.  Integer atomics carry
//                         the counts and the histogram.  Every output element is written once.
//   rank_ndcg_sum_kernel  one wave behind it (same stream): the finite ndcg[l] in ascending l, sequentially, in double, added to the
//                         accumulator's sum by one lane -- the same bits on every run, no float atomics.
#include "common.h"

namespace {

constexpr int OMAX = GSTVD_RANK_MAX_OPTIONS;                  // 128: two owned options per lane
constexpr int LISTS = 4;                                      // waves (lists) of a workgroup

// Ordered key of a score: a > b as keys <=> a sorts in front of b.  NaN is the largest key and all NaNs are equal; -0 == +0.
DEVFN uint32_t rank_key(float x) {
  uint32_t b = __builtin_bit_cast(uint32_t, x);
  if (x != x) return 0xffffffffu;
  if (b == 0x80000000u) b = 0;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// 1-based rank of the key at index i among the n keys in LDS: 1 + #{greater} + #{equal, in front}
DEVFN int rank_of(const uint32_t* keys, int n, uint32_t ki, int i) {
  int c = 1;
  for (int j = 0; j < n; ++j) {
    const uint32_t kj = keys[j];
    c += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
  }
  return c;
}

DEVFN void acc_add(int64_t* acc, int slot, int v) { atomicAdd((unsigned long long*)(acc + slot), (unsigned long long)v); }

__global__ __launch_bounds__(LISTS * WAVE) void rank_metrics_kernel(gstvd_rank_metrics_t a) {
  __shared__ uint32_t s_keys[LISTS][OMAX];
  __shared__ float s_dcg[LISTS][OMAX];
  __shared__ float s_ideal[LISTS][OMAX];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
  const int64_t l = (int64_t)blockIdx.x * LISTS + w;
  const bool live = l < a.L;                                  // wave-uniform; a dead wave only meets the barriers
  const int O = a.O;
  uint32_t* keys = s_keys[w];
  const int i0 = lane, i1 = lane + WAVE;

  if (live && l == 0 && lane == 0 && a.acc) acc_add(a.acc, GSTVD_RANK_N_CALLS, 1);

  // ---- keys of the scores
  uint32_t k0 = 0, k1 = 0;
  if (live) {
    const float* sc = a.scores + l * a.ld_scores;
    if (i0 < O) { k0 = rank_key(sc[i0]); keys[i0] = k0; }
    if (i1 < O) { k1 = rank_key(sc[i1]); keys[i1] = k1; }
  }
  __syncthreads();
  int r0 = 0, r1 = 0;
  if (live) {
    if (i0 < O) r0 = rank_of(keys, O, k0, i0);
    if (i1 < O) r1 = rank_of(keys, O, k1, i1);
    if (a.ranks) {
      int64_t* out = a.ranks + l * a.ld_ranks;
      if (i0 < O) out[i0] = r0;
      if (i1 < O) out[i1] = r1;
    }
    // ---- ground truth: the lane that owns it
    if (a.gt_index) {
      const int64_t gt = a.gt_index[l];
      if (gt >= 0 && gt < O) {
        if (lane == (int)(gt & (WAVE - 1))) {
          const int r = gt >= WAVE ? r1 : r0;
          if (a.gt_rank) a.gt_rank[l] = r;
          if (a.acc) { acc_add(a.acc, GSTVD_RANK_N_SPARSE, 1); acc_add(a.acc, GSTVD_RANK_HIST + r, 1); }
        }
      } else if (lane == 0) {
        if (a.gt_rank) a.gt_rank[l] = 0;
        if (a.acc) acc_add(a.acc, GSTVD_RANK_N_GT_SKIPPED, 1);
      }
    }
  }
  __syncthreads();                                            // the score keys are read: the relevance keys take their place

  // ---- relevance row of the list (wave-uniform)
  int64_t row = -1;
  bool has_rel = false;
  if (live && a.relevance) {
    row = a.rel_index ? (int64_t)a.rel_index[l] : l;
    has_rel = row >= 0 && row < a.n_rel;
    if (!has_rel && lane == 0) {
      a.ndcg[l] = __builtin_nanf("");
      if (row != -1 && a.acc) acc_add(a.acc, GSTVD_RANK_N_REL_SKIPPED, 1);
    }
  }
  float v0 = 0.f, v1 = 0.f;
  int k = 0;
  if (has_rel) {
    const float* rel = a.relevance + row * a.ld_rel;
    if (i0 < O) { v0 = rel[i0]; k0 = rank_key(v0); keys[i0] = k0; }
    if (i1 < O) { v1 = rel[i1]; k1 = rank_key(v1); keys[i1] = k1; }
    k = __popcll(__ballot(i0 < O && v0 != 0.f)) + __popcll(__ballot(i1 < O && v1 != 0.f));
  }
  __syncthreads();
  if (has_rel) {
    // position p = rank - 1 < k holds the term rel / discounts[p]: by predicted rank (dcg), by the relevance's own rank (ideal)
    if (i0 < O) {
      const int p = r0 - 1, q = rank_of(keys, O, k0, i0) - 1;
      if (p < k) s_dcg[w][p] = v0 / a.discounts[p];
      if (q < k) s_ideal[w][q] = v0 / a.discounts[q];
    }
    if (i1 < O) {
      const int p = r1 - 1, q = rank_of(keys, O, k1, i1) - 1;
      if (p < k) s_dcg[w][p] = v1 / a.discounts[p];
      if (q < k) s_ideal[w][q] = v1 / a.discounts[q];
    }
  }
  __syncthreads();
  if (has_rel) {
    // lanes 0 (dcg) and 1 (ideal): ascending position, sequentially, in double; rounded to fp32; one fp32 quotient
    double s = 0.0;
    if (lane < 2) {
      const float* t = lane == 0 ? s_dcg[w] : s_ideal[w];
      for (int p = 0; p < k; ++p) s += (double)t[p];
    }
    const float mine = (float)s;
    const float ideal = __shfl(mine, 1, WAVE);
    if (lane == 0) {
      const float q = k > 0 ? mine / ideal : __builtin_nanf("");
      a.ndcg[l] = q;
      if (a.acc) acc_add(a.acc, __builtin_isfinite(q) ? GSTVD_RANK_N_NDCG : GSTVD_RANK_N_NDCG_EMPTY, 1);
    }
  }
}

__global__ __launch_bounds__(WAVE) void rank_ndcg_sum_kernel(const float* ndcg, int64_t L, int64_t* acc) {
  const int lane = threadIdx.x;
  double s = 0.0;                                             // wave-uniform: every lane adds the same values in the same order
  for (int64_t base = 0; base < L; base += WAVE) {
    const float v = base + lane < L ? ndcg[base + lane] : __builtin_nanf("");
    const int n = L - base < WAVE ? (int)(L - base) : WAVE;
    for (int i = 0; i < n; ++i) {
      const float x = __shfl(v, i, WAVE);
      if (__builtin_isfinite(x)) s += (double)x;
    }
  }
  if (lane == 0) {
    const double t = __builtin_bit_cast(double, acc[GSTVD_RANK_NDCG_SUM]) + s;
    acc[GSTVD_RANK_NDCG_SUM] = __builtin_bit_cast(int64_t, t);
  }
}

}  // namespace

extern "C" int gstvd_rank_metrics(const gstvd_rank_metrics_t* a, gstvd_stream_t s) {
  if (!a || !a->scores) return GSTVD_E_NULL;
  if (a->relevance && (!a->discounts || !a->ndcg)) return GSTVD_E_NULL;
  if ((a->gt_rank && !a->gt_index) || (a->ndcg && !a->relevance)) return GSTVD_E_NULL;   // an output nothing would fill
  if (a->L < 1 || a->L > 0x7fffffff || a->O < 1 || a->O > OMAX || a->ld_scores < a->O) return GSTVD_E_SHAPE;
  if (a->ranks && a->ld_ranks < a->O) return GSTVD_E_SHAPE;
  if (a->relevance && (a->n_rel < 1 || a->ld_rel < a->O || a->n_discounts < a->O || (!a->rel_index && a->n_rel != a->L)))
    return GSTVD_E_SHAPE;
  const unsigned blocks = (unsigned)((a->L + LISTS - 1) / LISTS);
  hipLaunchKernelGGL(rank_metrics_kernel, dim3(blocks), dim3(LISTS * WAVE), 0, (hipStream_t)s, *a);
  GSTVD_LAUNCH_CHECK();
  if (a->relevance && a->acc) {
    hipLaunchKernelGGL(rank_ndcg_sum_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)s, (const float*)a->ndcg, a->L, a->acc);
    GSTVD_LAUNCH_CHECK();
  }
  return 0;
}
