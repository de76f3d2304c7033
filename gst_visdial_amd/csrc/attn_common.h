// Operand images, register fragments, the first product and the mask terms of the attention kernels: shared by attention.hip
// (forward, backward, decode) and attn_maps.hip (the probabilities on their own), so that both form a score the same way.
#pragma once
#include "common.h"
#include <math.h>

template <typename T, int D> struct Img {
  static constexpr bool BF = sizeof(T) == 2;
  static constexpr int RB = BF ? D * 2 : (D + 4) * 4;        // row bytes
  static constexpr int BYTES = 64 * RB;                       // 64-row chunk
  // bf16 row image: 16-byte slot s of row r at slot s ^ (r & mask)
  static DEVFN int row_off(int row, int slot) {
    constexpr int NS = D / 8, MASK = (NS < 16 ? NS : 16) - 1;
    return row * RB + ((slot ^ (row & MASK)) << 4);
  }
  // bf16 transposed-read image: 32-byte block b of row r at block b ^ (r / rows_per_bank_row)
  static DEVFN int tr_off(int row, int col) {
    constexpr int NB = D / 16, RPB = 128 / D >= 1 ? 128 / D : 1;
    int blk = ((col >> 4) ^ (row / RPB)) & (NB - 1);
    return row * RB + (blk << 5) + ((col & 15) << 1);
  }
  static DEVFN int f32_off(int row, int col) { return row * RB + col * 4; }
};

// Copy of rows [r0, r0+64) x D of a [rows, ld] matrix into LDS image(s), rows >= rmax zero filled, in two phases for software
// pipelining: `load` issues the chunk's global loads into registers (they stay in flight while the previous chunk is being
// consumed), `store` writes them into the LDS image(s) after the barrier.
template <typename T, int D> struct Stage64 {
  static constexpr int VE = 16 / sizeof(T), VPR = D / VE, TOT = 64 * VPR, NV = TOT / 256;
  static_assert(TOT % 256 == 0, "chunk must split evenly over 256 threads");
  u32x4 v[NV];
  DEVFN void load(const T* g, int64_t ld, int r0, int rmax, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256, row = idx / VPR, cv = idx % VPR;
      v[i] = (u32x4){0u, 0u, 0u, 0u};
      if (r0 + row < rmax) v[i] = *(const u32x4*)(g + (int64_t)(r0 + row) * ld + cv * VE);
    }
  }
  DEVFN void store(char* img_row, char* img_tr, int tid) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256, row = idx / VPR, cv = idx % VPR;
      if (Img<T, D>::BF) {
        if (img_row) *(u32x4*)(img_row + Img<T, D>::row_off(row, cv)) = v[i];
        if (img_tr) *(u32x4*)(img_tr + Img<T, D>::tr_off(row, cv * 8)) = v[i];
      } else {
        *(u32x4*)(img_row + row * Img<T, D>::RB + cv * 16) = v[i];
      }
    }
  }
};

// per-lane register copy of one row of a [rows, ld] matrix laid out as the MFMA operand that contracts over d:
//   bf16: NF = D/32 fragments of 8 (d = kk*32 + 8g + j);  f32: NF = D/4 scalars (d = g*(D/4) + ks)
template <typename T, int D> struct RowFrag;
template <int D> struct RowFrag<bf16, D> {
  static constexpr int NF = D / 32;
  bf16x8 f[NF];
  DEVFN void load(const bf16* rowp, bool valid, int g) {
#pragma unroll
    for (int kk = 0; kk < NF; ++kk) {
      typedef __attribute__((ext_vector_type(8))) short s16x8;
      s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      f[kk] = valid ? *(const bf16x8*)(rowp + kk * 32 + 8 * g) : __builtin_bit_cast(bf16x8, z);
    }
  }
  DEVFN float dot(const bf16* rowp, bool valid, int g) const {   // sum_j f * other (same positions)
    float a = 0.f;
    if (valid) {
#pragma unroll
      for (int kk = 0; kk < NF; ++kk) {
        bf16x8 o = *(const bf16x8*)(rowp + kk * 32 + 8 * g);
#pragma unroll
        for (int j = 0; j < 8; ++j) a += (float)f[kk][j] * (float)o[j];
      }
    }
    return a;
  }
};
template <int D> struct RowFrag<float, D> {
  static constexpr int NF = D / 4;
  float f[NF];
  DEVFN void load(const float* rowp, bool valid, int g) {
#pragma unroll
    for (int v = 0; v < NF / 4; ++v) {
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (valid) t = *(const f32x4*)(rowp + g * NF + v * 4);
      f[v * 4 + 0] = t[0]; f[v * 4 + 1] = t[1]; f[v * 4 + 2] = t[2]; f[v * 4 + 3] = t[3];
    }
  }
  DEVFN float dot(const float* rowp, bool valid, int g) const {
    float a = 0.f;
    if (valid) {
#pragma unroll
      for (int ks = 0; ks < NF; ++ks) a += f[ks] * rowp[g * NF + ks];
    }
    return a;
  }
};

// first product: acc(16x16) = sum_d Arow[x = xb + (lane&15)][d] * frag[d]  (A from the LDS row image)
template <typename T, int D>
DEVFN f32x4 first_product(const char* img_row, int xb, const RowFrag<T, D>& fr, int lane) {
  const int g = lane >> 4, li = lane & 15;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) {
      bf16x8 a = *(const bf16x8*)(img_row + Img<T, D>::row_off(xb + li, kk * 4 + g));
      acc = mfma_bf16_k32(a, fr.f[kk], acc);
    }
  } else {
    constexpr int NF = D / 4;
#pragma unroll
    for (int ks = 0; ks < NF; ++ks) {
      float a = *(const float*)(img_row + Img<T, D>::f32_off(xb + li, g * NF + ks));
      acc = mfma_f32_k4(a, fr.f[ks], acc);
    }
  }
  return acc;
}

__host__ DEVFN int round4(int x) { return (x + 3) & ~3; }

// additive mask term of key `key` of batch row bk: 0 (valid), mask_neg (masked out), -inf (past the end => p = 0)
DEVFN float key_add(const gstvd_attn_t& a, int bk, int key) {
  if (key >= a.Lk) return -INFINITY;
  return (a.key_mask == nullptr || a.key_mask[(int64_t)bk * a.Lk + key] != 0.f) ? 0.f : a.mask_neg;
}
// causal x padding: a key after the query gets mask_neg only when its term is still 0 -- the term is added once
DEVFN float causal_add(const gstvd_attn_t& a, float add, int key, int q) { return (key > q && add == 0.f) ? a.mask_neg : add; }

// Row 0 of Q / K / V (and, on demand, row q of O / dO) of (batch row b, head h).  STRIDED (forward, decode): kv_group query rows share the keys of batch
// row bk, and q_bstride / kv_bstride sequence positions separate two batch rows; the backward takes neither (attn_check).
template <typename T, int D, bool STRIDED> struct HeadBase {
  const T *Q, *K, *V;
  int bk, h;
  int64_t qrow0;                                              // first query row of batch row b
  DEVFN HeadBase(const gstvd_attn_t& a, int b, int h_) : h(h_) {
    bk = STRIDED && a.kv_group > 1 ? b / a.kv_group : b;
    const int64_t kbs = STRIDED && a.kv_bstride > 0 ? a.kv_bstride : a.Lk;
    qrow0 = (int64_t)b * (STRIDED && a.q_bstride > 0 ? a.q_bstride : a.Lq);
    Q = (const T*)a.Q + qrow0 * a.ldq + h * D;
    K = (const T*)a.K + (int64_t)bk * kbs * a.ldk + h * D;
    V = (const T*)a.V + (int64_t)bk * kbs * a.ldv + h * D;
  }
  DEVFN T* O(const gstvd_attn_t& a, int64_t q) const { return (T*)a.O + (qrow0 + q) * a.ldo + h * D; }             // row q of O
  DEVFN const T* dO(const gstvd_attn_t& a, int64_t q) const { return (const T*)a.dO + (qrow0 + q) * a.lddo + h * D; }
};
