// What the selection kernels share (beam.hip, distill.hip, vocab_argmax.hip, synonym.hip, sample.hip): ONE order on (value, index)
// pairs, its wave and workgroup arg-max, the K best of a row held in registers, and the row normaliser of the log-probabilities.
//
// The order -- part of the C ABI's contract (include/gstvd_hip.h): the larger value first, then the SMALLER index.  -inf == -inf
// falls through to the index; a NaN compares false both ways, so it never wins and never displaces.  SEL_NONE is the index of
// "nothing yet": with -inf it stands behind every real pair.
//
// Not here, on purpose: sample.hip's fkey and rank_metrics.hip's rank_key are DIFFERENT maps (fkey must be invertible for the
// bisections; rank_key sends NaN to the top and merges +-0), and sample.hip's reduce_maxcount reduces (max, count), not
// (value, index).  vocab_argmax.hip's row16_best is this order over a DPP row and stays with the MFMA layout it serves.
#pragma once
#include "common.h"
#include <math.h>

constexpr int SEL_NONE = 0x7fffffff;
struct Sel { float v; int i; };                   // a pair; also the layout of the kernels' workspace entries

// (a, ia) stands in front of (b, ib)
DEVFN bool sel_before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }
// b, or (v, i) if that stands in front: two selects, no branch.  Pairs travel BY VALUE through these helpers: with reference
// parameters hipcc compiled beam_topk_kernel's scan into exec-masked moves, 5 us of 40 per launch (profiles/select_refactor_timing.txt).
DEVFN Sel sel_take(Sel b, float v, int i) {
  const bool t = sel_before(v, i, b.v, b.i);
  return Sel{t ? v : b.v, t ? i : b.i};
}

// Best over the 64 lanes, result in every lane.
DEVFN Sel sel_wave_best(Sel b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) b = sel_take(b, __shfl_xor(b.v, o, 64), __shfl_xor(b.i, o, 64));
  return b;
}

// Best over the NW waves of a workgroup, result in every thread: the wave's best, then the waves' pairs through smv / smi (one slot
// per wave) in wave order 0, 1, 2, ...  The leading barrier lets consecutive calls share the slots, as block_reduce does.
template <int NW> DEVFN Sel sel_block_best(Sel b, float* smv, int* smi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  b = sel_wave_best(b);
  __syncthreads();
  if (lane == 0) { smv[wave] = b.v; smi[wave] = b.i; }
  __syncthreads();
  b = Sel{smv[0], smi[0]};
#pragma unroll
  for (int w = 1; w < NW; ++w) b = sel_take(b, smv[w], smi[w]);
  return b;
}

// The K best of a row whose elements live in NR registers per thread (slot j of this thread holds element at(j)), in K rounds of
// workgroup arg-max: each round takes the best pair that stands strictly behind the previous round's winner.  Nothing is marked in
// the registers (a dynamic index into zr[] would send the row to scratch; the constant, fully unrolled indexing keeps it in VGPRs);
// slots with at(j) >= V never qualify, whatever they hold.  A row that runs out yields (-inf, V - 1).  Thread `round` returns
// winner `round`; every thread must call (barriers inside).  topk_logp_kernel calls it; beam_topk_kernel holds the same loop written
// out, because its bf16 form measured 1 % slower through the call.
template <int NW, int NR, typename At> DEVFN Sel sel_topk_rounds(const float (&zr)[NR], At at, int V, int K, float* smv, int* smi) {
  Sel prev{INFINITY, -1}, mine{-INFINITY, 0};
  for (int round = 0; round < K; ++round) {                   // uniform: every thread holds the same prev
    Sel b{-INFINITY, SEL_NONE};
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int i = at(j);
      const bool ok = i < V && sel_before(prev.v, prev.i, zr[j], i) && sel_before(zr[j], i, b.v, b.i);
      b = Sel{ok ? zr[j] : b.v, ok ? i : b.i};
    }
    b = sel_block_best<NW>(b, smv, smi);
    if (b.i >= V) b = Sel{-INFINITY, V - 1};
    if ((int)threadIdx.x == round) mine = b;
    prev = b;
  }
  return mine;
}

// max x and log sum exp(x - max x) of a row in fp32 with fmaxf / expf / logf, element tid + j * NW * 64 in register zr[j]; slots
// at or past V play no part, whatever they hold.  This is THE normaliser of gstvd_beam_step's logp_j[v] and of
// gstvd_sample_topk_scored's logp; the callers spell the score in the spec's association, (x - max) - lse.
template <int NW, int SEG> DEVFN void sel_row_norm(const float (&zr)[SEG], int V, float* red, float& mx, float& lse) {
  const int tid = threadIdx.x;
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < SEG; ++j) m = fmaxf(m, (tid + j * NW * 64 < V) ? zr[j] : -INFINITY);
  mx = block_reduce(m, red, true);
  float e = 0.f;
#pragma unroll
  for (int j = 0; j < SEG; ++j) e += (tid + j * NW * 64 < V) ? expf(zr[j] - mx) : 0.f;
  lse = logf(block_reduce(e, red, false));
}
