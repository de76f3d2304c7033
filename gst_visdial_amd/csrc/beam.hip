// Beam-search answer decoding on the device: the beam step (the K best of the K x V continuations of a dialog row) and the
// reorder of the self-attention K/V caches of the surviving beams.  Neither needs the host, so the whole beam loop replays from
// one captured graph, like the sampling loop (sample.hip).
//
// The step rule (there is no reference implementation; include/gstvd_hip.h states it in full):
//   live beam j, every v in [0, V):  score s[b,j] + logp_j[v],  logp_j[v] = (z[v] - max z) - log sum exp(z - max z)  in fp32
//   done beam j: ONE candidate (j, PAD) with score s[b,j]
//   the K best become the new beams in order: higher score first, then smaller j, then smaller v (-inf scores under the same rule)
// Phase A (one 1024-thread workgroup per beam row, the row in registers as in sample_topk_kernel): max, log-sum-exp, the row's
// candidate scores, and its K best under (score, v) in K rounds of block arg-max -> workspace [B, K, K] of (score, v).
// Phase B (one wave per dialog row): ranks the <= K * K candidates under the full rule; the lane of rank i < K writes new beam i.
#include "select.h"

namespace {

constexpr int NT = 1024, NWV = NT / 64;
constexpr int SEG = 31;                                       // V <= 31 * 1024 (checked by the host entry), as in sample.hip
constexpr int KMAX = 8;

struct Cand { float s; int32_t v; };                          // one workspace entry

template <typename T>
__global__ __launch_bounds__(NT) void beam_topk_kernel(gstvd_beam_step_t a) {
  __shared__ float smf[NWV];
  __shared__ float smv[NWV];
  __shared__ int smi[NWV];
  const int tid = threadIdx.x, r = blockIdx.x, V = a.V, K = a.K;
  Cand* ws = (Cand*)a.workspace + (int64_t)r * K;
  if (a.done_in[r] != 0) return;                              // phase B reads nothing of a done beam's workspace rows
  const float s_in = a.score_in[r];
  if (!(s_in > -INFINITY)) {
    // a live beam without a finite score (the beams j > 0 in front of the first step): every candidate scores -inf, so the
    // rule orders them by v alone
    if (tid < K) { Cand c; c.s = -INFINITY; c.v = tid; ws[tid] = c; }
    return;
  }
  const T* row = (const T*)a.logits + (int64_t)r * a.ld;
  float zr[SEG];
#pragma unroll
  for (int j = 0; j < SEG; ++j) {
    const int i = tid + j * NT;
    zr[j] = i < V ? to_f(row[i]) : -INFINITY;
  }
  float m, lse;
  sel_row_norm<NWV>(zr, V, smf, m, lse);
  // the candidates' scores, in the spec's own association: s + ((z - max) - lse)
#pragma unroll
  for (int j = 0; j < SEG; ++j) zr[j] = (tid + j * NT < V) ? s_in + ((zr[j] - m) - lse) : -INFINITY;

  // select.h's sel_topk_rounds, written out: through the function the bf16 kernel measured 40.6-40.7 us per step against 40.2 with
  // the loop here (profiles/select_refactor_timing.txt).  Keep the two in step.  (V < K runs out of candidates: never with a real
  // vocabulary.)
  Sel prev{INFINITY, -1}, mine{-INFINITY, 0};
  for (int round = 0; round < K; ++round) {
    Sel b{-INFINITY, SEL_NONE};
#pragma unroll
    for (int j = 0; j < SEG; ++j) {
      const int i = tid + j * NT;
      const bool ok = i < V && sel_before(prev.v, prev.i, zr[j], i) && sel_before(zr[j], i, b.v, b.i);
      b = Sel{ok ? zr[j] : b.v, ok ? i : b.i};
    }
    b = sel_block_best<NWV>(b, smv, smi);
    if (b.i >= V) b = Sel{-INFINITY, V - 1};
    if (tid == round) mine = b;
    prev = b;
  }
  if (tid < K) { Cand c; c.s = mine.v; c.v = mine.i; ws[tid] = c; }
}

// One wave per dialog row: lane j * K + i holds candidate i of beam j.
__global__ __launch_bounds__(64) void beam_merge_kernel(gstvd_beam_step_t a) {
  __shared__ float cs[KMAX * KMAX];
  __shared__ int cv[KMAX * KMAX];
  __shared__ int cok[KMAX * KMAX];
  const int lane = threadIdx.x, b = blockIdx.x, K = a.K, n = K * K;
  const int j = lane / K, i = lane - j * K;
  float s = -INFINITY;
  int v = 0, ok = 0, dn = 0;
  if (lane < n) {
    const int r = b * K + j;
    dn = a.done_in[r] != 0;
    if (dn) {                                                 // a done beam: one candidate, its score unchanged
      ok = i == 0;
      s = a.score_in[r];
      v = a.pad;
    } else {
      const Cand c = ((const Cand*)a.workspace)[(int64_t)r * K + i];
      ok = 1; s = c.s; v = c.v;
    }
  }
  cs[lane] = s; cv[lane] = v; cok[lane] = ok;
  __syncthreads();
  if (!ok) return;
  // rank under (score desc, beam asc, token asc); candidates of one beam differ in v, so the order is total and the ranks of the
  // >= K valid candidates are 0, 1, 2, ... without repeats: every output slot has exactly one writer
  int rank = 0;
  for (int q = 0; q < n; ++q) {
    const float qs = cs[q];
    const int qj = q / K, qv = cv[q];
    const bool first = qs > s || (qs == s && (qj < j || (qj == j && qv < v)));
    rank += (cok[q] && q != lane && first) ? 1 : 0;
  }
  if (rank < K) {
    const int o = b * K + rank;
    a.ids_tm[(int64_t)a.pos * a.ids_stride + o] = (int64_t)v;
    a.parent[o] = j;
    a.score_out[o] = s;
    a.done_out[o] = (dn || v == a.eos) ? 1 : 0;
  }
}

// dst[l][b*K + i, 0..t, H..3H) = src[l][b*K + parent[b,i], 0..t, H..3H): grid (B*K, layers), 16-byte pieces
constexpr int RNT = 256;
__global__ __launch_bounds__(RNT) void beam_reorder_kernel(gstvd_beam_reorder_t a, int vec_per_pos, int esize) {
  const int o = blockIdx.x, l = blockIdx.y, K = a.K;
  const int b = o / K;
  const int j = a.parent[o];
  if ((unsigned)j >= (unsigned)K) return;                     // (never from gstvd_beam_step; no read outside the row group)
  const int64_t rs = a.row_stride * esize, ps = a.ld * esize;                              // bytes
  const char* __restrict__ src = (const char*)a.src[l] + (int64_t)(b * K + j) * rs + (int64_t)a.H * esize;
  char* __restrict__ dst = (char*)a.dst[l] + (int64_t)o * rs + (int64_t)a.H * esize;
  const int total = (a.t + 1) * vec_per_pos;
#pragma unroll 4
  for (int x = threadIdx.x; x < total; x += RNT) {
    const int p = x / vec_per_pos, c = x - p * vec_per_pos;
    const int64_t off = (int64_t)p * ps + (int64_t)c * 16;
    *(u32x4*)(dst + off) = *(const u32x4*)(src + off);
  }
}

}  // namespace

extern "C" int gstvd_beam_step(const gstvd_beam_step_t* a, gstvd_stream_t stream) {
  if (!a || !a->logits || !a->score_in || !a->done_in || !a->score_out || !a->done_out || !a->parent || !a->ids_tm || !a->workspace)
    return GSTVD_E_NULL;
  if (a->dtype != GSTVD_F32 && a->dtype != GSTVD_BF16) return GSTVD_E_DTYPE;
  if (a->K < 1 || a->K > KMAX) return GSTVD_E_SHAPE;
  if (a->V > SEG * 1024) return GSTVD_E_UNSUPPORTED;          // the sampler's limit: a row lives in 31 registers per thread
  if (a->B <= 0 || a->V <= 0 || a->ld < a->V || a->pos < 0 || a->pos >= a->positions || a->ids_stride < (int64_t)a->B * a->K ||
      (int64_t)a->B * a->K > 0x7fffffff / KMAX)
    return GSTVD_E_SHAPE;
  if (a->score_in == a->score_out || a->done_in == a->done_out) return GSTVD_E_SHAPE;      // ping-pong: nothing in place
  hipStream_t s = (hipStream_t)stream;
  if (a->dtype == GSTVD_BF16) hipLaunchKernelGGL((beam_topk_kernel<bf16>), dim3((unsigned)(a->B * a->K)), dim3(NT), 0, s, *a);
  else hipLaunchKernelGGL((beam_topk_kernel<float>), dim3((unsigned)(a->B * a->K)), dim3(NT), 0, s, *a);
  GSTVD_LAUNCH_CHECK();
  hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)a->B), dim3(64), 0, s, *a);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_beam_reorder(const gstvd_beam_reorder_t* a, gstvd_stream_t stream) {
  if (!a || !a->parent) return GSTVD_E_NULL;
  if (a->n_layers < 1 || a->n_layers > 16) return GSTVD_E_SHAPE;
  for (int l = 0; l < a->n_layers; ++l)
    if (!a->src[l] || !a->dst[l]) return GSTVD_E_NULL;
  if (a->dtype != GSTVD_F32 && a->dtype != GSTVD_BF16) return GSTVD_E_DTYPE;
  const int esize = a->dtype == GSTVD_BF16 ? 2 : 4;
  if (a->K < 1 || a->K > KMAX || a->B <= 0 || a->H <= 0 || a->Umax <= 0 || a->t < 0 || a->t >= a->Umax || a->ld < 3 * (int64_t)a->H ||
      a->row_stride < (int64_t)a->Umax * a->ld || (int64_t)a->B * a->K > 0x7fffffff / KMAX)
    return GSTVD_E_SHAPE;
  if (((int64_t)a->H * esize) % 16 || (a->ld * esize) % 16 || (a->row_stride * esize) % 16) return GSTVD_E_ALIGN;
  for (int l = 0; l < a->n_layers; ++l) {
    if (((uintptr_t)a->src[l] | (uintptr_t)a->dst[l]) & 15) return GSTVD_E_ALIGN;
    if (a->src[l] == a->dst[l]) return GSTVD_E_SHAPE;         // two cache sets: a permutation never reads an overwritten row
  }
  const int vec_per_pos = (int)(2 * (int64_t)a->H * esize / 16);
  hipLaunchKernelGGL(beam_reorder_kernel, dim3((unsigned)(a->B * a->K), (unsigned)a->n_layers), dim3(RNT), 0, (hipStream_t)stream,
                     *a, vec_per_pos, esize);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
