// The last launch of every loss (gstvd_ce_fwd, gstvd_kl_fwd, gstvd_nsp_train_fwd):
//   stats[0] = sum of the row losses, stats[1] = number of counted rows, stats[2] = their quotient.
// ONE block; a thread sums the rows tid, tid + blockDim.x, ..., then block_reduce: the block size fixes the order of the additions
// and with it every bit of stats, so each caller keeps its own (256, 256, 64).  A row counts when
//   labels == NULL (every row), or eq ? labels[i] == value : labels[i] != value.
// The backward scales every row by loss_grad_scale (ce_bwd_kernel, distill_bwd_kernel, kl_bwd_kernel).  Not here, on purpose:
// nsp_train_bwd_kernel (pool_head.hip) divides by its argument B -- it takes no stats pointer; reading one would add a load.
#pragma once
#include "common.h"

// Upstream gradient of one row loss: gscale[0] (1 without one), divided by the number of counted rows, stats[1], for a mean loss.
DEVFN float loss_grad_scale(const float* gscale, int mean, const float* stats) {
  const float gs = gscale ? gscale[0] : 1.f;
  return mean ? gs / stats[1] : gs;
}

static __global__ __launch_bounds__(256) void row_loss_reduce_kernel(const float* row_loss, const int64_t* labels, int64_t value, int eq,
                                                                     int64_t M, float* stats) {
  __shared__ float red[4];
  float s = 0.f, n = 0.f;
  for (int64_t i = threadIdx.x; i < M; i += blockDim.x) {
    s += row_loss[i];
    n += (!labels || (labels[i] == value) == (eq != 0)) ? 1.f : 0.f;
  }
  s = block_reduce(s, red, false);
  n = block_reduce(n, red, false);
  if (threadIdx.x == 0) { stats[0] = s; stats[1] = n; stats[2] = s / n; }
}
