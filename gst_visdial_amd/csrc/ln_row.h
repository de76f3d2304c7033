// The row arithmetic of the LayerNorm family, once: ln_fwd_kernel / ln_bwd_kernel (layernorm.hip) and the two prologues of
// gemm_rows_kernel (gemm_rows.hip) all go through these helpers, which is why the fused launches agree with the stand-alone
// kernels bit for bit (y, mean, rstd, dres, dx).  One wave owns a row; lane l holds NV vectors of four columns in registers,
// vector i at columns 4 l + 256 i.  Everything is __forceinline__: a call site's registers and schedule are its own.
// (gemv16_ln_kernel, gemv.hip, keeps its own statistics: its one-round E[x^2] - mean^2 form is a documented choice, not a copy.)
#pragma once
#include "common.h"

// the lane's vector i: its first column c, and whether it lies inside a row of H columns
struct LnCol { int c; bool in; };
DEVFN LnCol ln_col(int lane, int i, int H) {
  const int c = lane * 4 + i * 256;
  return {c, c < H};
}

// dropout factors of the four elements at (row, c .. c + 3) of an [M, H] site
DEVFN f32x4 ln_drop(const DropKey& k, int64_t row, int64_t H, int c) { return drop_factor4(k, (uint64_t)(row * H + c)); }

// pre-LayerNorm row of the residual form, in place: h = x on entry, h = x * drop_pre (+ res(), asked for only where there is a
// residual) on return
template <typename R> DEVFN void ln_resid(f32x4& h, f32x4 drop, bool has_res, R res) {
  h *= drop;
  if (has_res) h += res();
}

DEVFN float ln_sum4(f32x4 v) { return v[0] + v[1] + v[2] + v[3]; }
// a row's mean of a quantity from the lanes' partial sums
DEVFN float ln_row_mean(float lane_sum, int H) { return wave_sum(lane_sum) / (float)H; }

// Two-pass statistics of a row: mean = ln_row_mean(s), s the lane's sum of ln_sum4(h[i]) in ascending i; then
// rstd = ln_rstd(v), v the lane's sum of ln_var_term(h[i], mean, NV == 1) in ascending i.
// The squares: the one-vector kernels (H <= 256) have always summed a vector's four through fused multiply-adds, the wider ones
// round each square first -- which is why the two disagree in rstd's last bit on a narrow row.  Spelled out, with contraction off,
// so that neither depends on what the optimizer makes of the expression at a given call site.
DEVFN float ln_var_term(f32x4 h, float mean, bool one_vector) {
  const f32x4 d = h - mean;
  {
#pragma clang fp contract(off)
    if (one_vector) return __builtin_fmaf(d[3], d[3], __builtin_fmaf(d[2], d[2], __builtin_fmaf(d[0], d[0], d[1] * d[1])));
    return ln_sum4(d * d);
  }
}
DEVFN float ln_rstd(float v, int H, float eps) { return 1.0f / sqrtf(ln_row_mean(v, H) + eps); }

DEVFN f32x4 ln_xhat(f32x4 h, float mean, float rstd) { return (h - mean) * rstd; }
DEVFN f32x4 ln_y(f32x4 h, float mean, float rstd, f32x4 gamma, f32x4 beta) { return gamma * ln_xhat(h, mean, rstd) + beta; }

// backward, one vector: xhat (formed in front of the dy load at both call sites); then gy = dy * gamma, and s1 / s2 collect the
// lane's sums of gy and gy * xhat ...
DEVFN void ln_bwd_sums(f32x4 dyv, f32x4 gamma, f32x4 xh, f32x4& gy, float& s1, float& s2) {
  gy = dyv * gamma;
  s1 += ln_sum4(gy);
  s2 += ln_sum4(gy * xh);
}
// ... and with c1 / c2 = the row means of s1 / s2 (ln_row_mean) the gradient of the pre-LayerNorm row; dx = dh * ln_drop(pre)
DEVFN f32x4 ln_bwd_dh(f32x4 gy, f32x4 xh, float c1, float c2, float rstd) { return (gy - c1 - xh * c2) * rstd; }
