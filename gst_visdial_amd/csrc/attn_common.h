// Operand images, register fragments, the first product and the mask terms of the attention kernels: shared by attention.hip
// (forward, backward, decode) and attn_maps.hip (the probabilities on their own), so that both form a score the same way; the
// second products, the dropout draws and the two bodies of the two-part backward: shared by attention.hip and attn_group.hip
// (the backward of a launch whose kv_group query rows share one K / V row).
#pragma once
#include "common.h"
#include <math.h>
#include <type_traits>

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

// second product: acc[i](16x16) += sum_{r<4} X[row = xb + 4g + r][col = i*16 + (lane&15)] * w[r]
//   (A = X^T read transposed from the row-major image, B = the in-register tile w)
template <typename T, int D>
DEVFN void second_product(f32x4 (&acc)[D / 16], const char* img_tr, int xb, const float (&w)[4], int lane) {
  const int g = lane >> 4, li = lane & 15;
  if constexpr (sizeof(T) == 2) {
    const s16x4 b = pack_bf16x4(w[0], w[1], w[2], w[3]);
#pragma unroll
    for (int i = 0; i < D / 16; ++i) {
      s16x4 a = lds_tr16(img_tr + Img<T, D>::tr_off(xb + 4 * g + (li >> 2), i * 16 + 4 * (lane & 3)));
      acc[i] = mfma_bf16_k16(a, b, acc[i]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < D / 16; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float a = *(const float*)(img_tr + Img<T, D>::f32_off(xb + 4 * g + r, i * 16 + li));
        acc[i] = mfma_f32_k4(a, w[r], acc[i]);
      }
    }
  }
}

// The second product of TWO 16-row tiles (rows xb.. and xb+16..).  bf16: ONE 16x16x32 MFMA per 16 output columns -- k-slot 8g+j
// of the instruction is row 4g+j of the first tile (j < 4) or of the second (j >= 4), i.e. the A operand is the concatenation
// of the two transposed reads the tiles would have issued separately and the B operand that of their in-register weights.
template <typename T, int D>
DEVFN void second_product_pair(f32x4 (&acc)[D / 16], const char* img_tr, int xb, const float (&w0)[4], const float (&w1)[4], int lane) {
  if constexpr (sizeof(T) == 2) {
    const int g = lane >> 4, li = lane & 15;
    const bf16x8 b = {(bf16)w0[0], (bf16)w0[1], (bf16)w0[2], (bf16)w0[3], (bf16)w1[0], (bf16)w1[1], (bf16)w1[2], (bf16)w1[3]};
#pragma unroll
    for (int i = 0; i < D / 16; ++i) {
      const s16x4 lo = lds_tr16(img_tr + Img<T, D>::tr_off(xb + 4 * g + (li >> 2), i * 16 + 4 * (lane & 3)));
      const s16x4 hi = lds_tr16(img_tr + Img<T, D>::tr_off(xb + 16 + 4 * g + (li >> 2), i * 16 + 4 * (lane & 3)));
      typedef __attribute__((ext_vector_type(8))) short s16x8;
      const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      acc[i] = mfma_bf16_k32(__builtin_bit_cast(bf16x8, v), b, acc[i]);
    }
  } else {
    second_product<T, D>(acc, img_tr, xb, w0, lane);
    second_product<T, D>(acc, img_tr, xb + 16, w1, lane);
  }
}

// Dropout draws.  E32: the launch has fewer than 2^33 score elements, so the high word of every pair index is zero and its
// term of drop_draw (a quarter-rate integer multiply per draw) vanishes -- same stream, cheaper arithmetic.
template <bool E32> DEVFN uint32_t draw_pair(const DropKey& k, uint64_t e2) {
  if (E32) return drop_hash((uint32_t)e2, k.key);
  return drop_draw(k, e2);
}
template <bool E32> DEVFN f32x4 drop_factor4e(const DropKey& k, uint64_t e) {      // four consecutive elements, e % 4 == 0
  f32x4 f = {1.f, 1.f, 1.f, 1.f};
  if (!k.on) return f;
  const uint32_t r0 = draw_pair<E32>(k, e >> 1), r1 = draw_pair<E32>(k, (e >> 1) + 1);
  f[0] = (r0 & 0xffffu) >= k.thr ? k.scale : 0.f;
  f[1] = (r0 >> 16) >= k.thr ? k.scale : 0.f;
  f[2] = (r1 & 0xffffu) >= k.thr ? k.scale : 0.f;
  f[3] = (r1 >> 16) >= k.thr ? k.scale : 0.f;
  return f;
}
// The dK/dV lane layout (one key per lane, four consecutive queries): draw index set-up and the factors of one tile.
// e2lane: pair index (element index >> 1) of (query 4g of the chunk at c0 = 0, this lane's key); Lkp = round4(Lk) is even, so a
// step of one query is a step of `half` = Lkp / 2 pairs.  Not clamped for keys past the end: the partner lane may be a valid key
// and takes our draws.
struct PairDraw {
  uint64_t half, e2lane;
  bool odd;
  DEVFN PairDraw(int64_t stat0, int Lk, int g, int key)
      : half((uint64_t)(round4(Lk) >> 1)), e2lane(((uint64_t)stat0 + (uint64_t)(4 * g)) * half + (uint64_t)(key >> 1)), odd((key & 1) != 0) {}
  DEVFN uint64_t chunk(int c0) const { return e2lane + (uint64_t)c0 * half; }   // the same for the chunk at query c0
};
// The two keys of a pair sit in neighbouring lanes (li, li ^ 1): the even lane draws for rows r = 0, 1 of the tile q0 rows
// below pair index e2 (the chunk's base, formed once per chunk), the odd lane for rows 2, 3, and one quad permute hands each its
// partner's draws.  f stays as it is without dropout.
template <bool E32> DEVFN void pair_drop_factors(const DropKey& dk, uint64_t e2, int q0, uint64_t half, bool odd, float (&f)[4]) {
  if (!dk.on) return;
  const int r0 = odd ? 2 : 0;
  const uint32_t mine0 = draw_pair<E32>(dk, e2 + (uint64_t)(q0 + r0) * half);
  const uint32_t mine1 = draw_pair<E32>(dk, e2 + (uint64_t)(q0 + r0 + 1) * half);
  const uint32_t other0 = (uint32_t)__builtin_amdgcn_mov_dpp((int)mine0, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
  const uint32_t other1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)mine1, 0xB1, 0xf, 0xf, true);
  const uint32_t d0 = odd ? other0 : mine0, d1 = odd ? other1 : mine1, d2 = odd ? mine0 : other0, d3 = odd ? mine1 : other1;
  const uint32_t sh = odd ? 16u : 0u;
  f[0] = ((d0 >> sh) & 0xffffu) >= dk.thr ? dk.scale : 0.f;
  f[1] = ((d1 >> sh) & 0xffffu) >= dk.thr ? dk.scale : 0.f;
  f[2] = ((d2 >> sh) & 0xffffu) >= dk.thr ? dk.scale : 0.f;
  f[3] = ((d3 >> sh) & 0xffffu) >= dk.thr ? dk.scale : 0.f;
}

// K + V + additive-mask registers of one 64-key chunk (forward, dQ): `load` issues the global loads, `store` fills the LDS images
template <typename T, int D> struct KVStage {
  Stage64<T, D> k, v;
  float m;
  DEVFN void load(const gstvd_attn_t& a, const T* Kb, const T* Vb, int bk, int c0, int tid) {
    k.load(Kb, a.ldk, c0, a.Lk, tid);
    v.load(Vb, a.ldv, c0, a.Lk, tid);
    if (tid < 64) m = key_add(a, bk, c0 + tid);
  }
  DEVFN void store(char* k_row, char* k_tr, char* v_row, char* v_tr, float* smask, int tid) const {
    k.store(k_row, k_tr, tid);
    v.store(v_row, v_tr, tid);
    if (tid < 64) smask[tid] = m;
  }
};

// fewer than 2^33 score elements: the dropout draws of the launch take 32-bit index arithmetic (draw_pair); also part of the route
__host__ DEVFN bool attn_small_index_space(const gstvd_attn_t& a) {
  return (uint64_t)a.B * (uint64_t)a.nh * (uint64_t)a.Lq * (uint64_t)round4(a.Lk) < (1ull << 33);
}

// =====================================================================================================
// backward, part 1: dQ (and delta = rowsum(dO * O)); same tiling as forward
// =====================================================================================================
// GROUPED: K, V and the key mask of query row b are those of row b / kv_group (HeadBase STRIDED; gstvd_attn_group_bwd admits no
// batch strides); everything that is indexed by the query row -- Q, O, dO, LSE, delta, dQ, the draws -- is as without it.
template <typename T, int D, bool E32, bool GROUPED = false>
DEVFN void attn_bwd_dq_body(const gstvd_attn_t& a, const int bx, const int h, const int b, char* smem) {
  constexpr bool BF = Img<T, D>::BF;
  constexpr int TP = D <= 64 ? 2 : 1;                         // 16-key tiles per inner iteration
  char* sKr = smem;                                           // row image of K
  char* sKt = BF ? smem + Img<T, D>::BYTES : smem;            // transposed-read image of K
  char* sVr = smem + (BF ? 2 : 1) * Img<T, D>::BYTES;         // row image of V
  float* smask = (float*)(smem + (BF ? 3 : 2) * Img<T, D>::BYTES);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int q = bx * 64 + wave * 16 + li;
  const bool qv = q < a.Lq;
  const HeadBase<T, D, GROUPED> hp(a, b, h);
  RowFrag<T, D> qf, dof;
  qf.load(hp.Q + (int64_t)q * a.ldq, qv, g);
  dof.load(hp.dO(a, q), qv, g);
  float delta = rows_sum(dof.dot(hp.O(a, q), qv, g));
  const int64_t stat = ((int64_t)b * a.nh + h) * a.Lq + q;
  if (qv && g == 0) a.delta[stat] = delta;
  const float lse = qv ? a.LSE[stat] : INFINITY;              // +inf => p = 0 for padded query rows
  const DropKey dk = make_drop(a.dropout_p, a.site, a.rng);
  const int Lkp = round4(a.Lk);
  const uint64_t ebase = ((uint64_t)(b * a.nh + h) * a.Lq + (uint64_t)(qv ? q : 0)) * (uint64_t)Lkp + (uint64_t)(4 * g);

  f32x4 acc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  KVStage<T, D> st;
  st.load(a, hp.K, hp.V, hp.bk, 0, tid);
  for (int c0 = 0; c0 < a.Lk; c0 += 64) {
    __syncthreads();
    st.store(sKr, BF ? sKt : nullptr, sVr, nullptr, smask, tid);
    __syncthreads();
    if (c0 + 64 < a.Lk) st.load(a, hp.K, hp.V, hp.bk, c0 + 64, tid);
    const int ntile = (a.Lk - c0 + 15) / 16 < 4 ? (a.Lk - c0 + 15) / 16 : 4;
    // TP tiles at a time.  d <= 64: two (32 keys) -- enough to pair them on the 16x16x32 second product and to halve the
    // per-tile bookkeeping, few enough live values for three waves per SIMD (a whole chunk at once needed 296 registers in the
    // merged kernel: one wave per SIMD, 105 us instead of 61 for the text shape).  d = 128: one -- the accumulators, operand
    // fragments and prefetch registers of that width leave no room for a second tile at two waves per SIMD.
    // FULL: all TP tiles present, no causal mask -- a body without control flow (see attn_fwd_body)
    auto tiles = [&](auto full_tag, const int pr, const int nt) {
      constexpr bool FULL = decltype(full_tag)::value;
      f32x4 s[TP], dp[TP];
      float ds[TP][4];
#pragma unroll
      for (int tt = 0; tt < TP; ++tt) {
        if (FULL || tt < nt) {
          s[tt] = first_product<T, D>(sKr, 16 * TP * pr + tt * 16, qf, lane);
          dp[tt] = first_product<T, D>(sVr, 16 * TP * pr + tt * 16, dof, lane);
        }
      }
#pragma unroll
      for (int tt = 0; tt < TP; ++tt) {
        if (FULL || tt < nt) {
          const int k0 = 16 * TP * pr + tt * 16;
          const f32x4 fac = drop_factor4e<E32>(dk, ebase + (uint64_t)(c0 + k0));
          f32x4 madd = *(const f32x4*)(smask + k0 + 4 * g);
          if (!FULL && a.causal) {
#pragma unroll
            for (int r = 0; r < 4; ++r) madd[r] = causal_add(a, madd[r], c0 + k0 + 4 * g + r, q);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = __expf(s[tt][r] * a.scale + madd[r] - lse);
            ds[tt][r] = p * (dp[tt][r] * fac[r] - delta) * a.scale;
          }
        }
      }
      if (TP > 1 && (FULL || nt > 1)) second_product_pair<T, D>(acc, sKt, 16 * TP * pr, ds[0], ds[TP - 1], lane);
      else second_product<T, D>(acc, sKt, 16 * TP * pr, ds[0], lane);
    };
#pragma unroll 1
    for (int pr = 0; pr < 4 / TP; ++pr) {
      const int nt = ntile - TP * pr;
      if (nt <= 0) break;
      if (TP > 1 && nt >= TP && !a.causal) tiles(std::true_type{}, pr, TP);      // (TP = 1: the generic body has no tile tests)
      else tiles(std::false_type{}, pr, nt);
    }
  }
  if (qv) {
    T* dQp = (T*)a.dQ + ((int64_t)b * a.Lq + q) * a.lddq + h * D;
#pragma unroll
    for (int i = 0; i < D / 16; ++i) st4(dQp + i * 16 + 4 * g, acc[i]);
  }
}

// =====================================================================================================
// backward, part 2: dK and dV; one wave owns 16 keys, queries stream through LDS
// =====================================================================================================
// dK / dV rows of this lane's key from the accumulators (dK^T, dV^T: rows d = 16 i + 4g + r, column = key li)
template <typename T, int D>
DEVFN void store_dkv(const gstvd_attn_t& a, int b, int h, int key, int g, const f32x4 (&accK)[D / 16], const f32x4 (&accV)[D / 16]) {
  if (key >= a.Lk) return;
  T* dKp = (T*)a.dK + ((int64_t)b * a.Lk + key) * a.lddk + h * D;
  T* dVp = (T*)a.dV + ((int64_t)b * a.Lk + key) * a.lddv + h * D;
#pragma unroll
  for (int i = 0; i < D / 16; ++i) {
    st4(dKp + i * 16 + 4 * g, accK[i]);
    st4(dVp + i * 16 + 4 * g, accV[i]);
  }
}

// GROUPED: b is a K / V row and the block walks the query chunks of ALL its kv_group query rows b * G .. b * G + G - 1, in
// ascending order, into the one set of accumulators: dK / dV of row b are the sums over the group, stored once -- no atomics, the
// same order of additions every run.  Q, O, dO, LSE and the draw indices are those of the query row (`member`); the chunk loop
// and its one-chunk-ahead prefetch run on across the members.
template <typename T, int D, bool E32, bool GROUPED = false>
DEVFN void attn_bwd_dkv_body(const gstvd_attn_t& a, const int bx, const int h, const int b, char* smem) {
  constexpr bool BF = Img<T, D>::BF;
  constexpr int IB = Img<T, D>::BYTES;
  constexpr int TP = D <= 64 ? 2 : 1;                         // 16-query tiles per inner iteration
  char* sQr = smem;
  char* sQt = BF ? smem + IB : smem;
  char* sOr = smem + (BF ? 2 : 1) * IB;                       // dO row image
  char* sOt = BF ? smem + 3 * IB : sOr;                       // dO transposed-read image
  float* sLse = (float*)(smem + (BF ? 4 : 2) * IB);
  float* sDel = sLse + 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int key = bx * 64 + wave * 16 + li;
  const bool kv = key < a.Lk;
  const HeadBase<T, D, false> hp(a, b, h);                    // K, V (and the mask) of row b
  // O, Q, dO, the statistics' base and the draw indices of the query row being walked: constants without the group
  typedef typename std::conditional<GROUPED, const T*, const T* const>::type RowPtr;
  typedef typename std::conditional<GROUPED, int64_t, const int64_t>::type StatBase;
  typedef typename std::conditional<GROUPED, PairDraw, const PairDraw>::type Draws;
  const int bq0 = GROUPED ? b * a.kv_group : b;               // the (first) query row
  const HeadBase<T, D, false> hq(a, bq0, h);
  const HeadBase<T, D, false>& h0 = GROUPED ? hq : hp;
  RowPtr Ob = h0.O(a, 0), Qb = h0.Q, dOb = h0.dO(a, 0);
  RowFrag<T, D> kf, vf;
  kf.load(hp.K + (int64_t)key * a.ldk, kv, g);
  vf.load(hp.V + (int64_t)key * a.ldv, kv, g);
  const float kadd = key_add(a, b, key);                      // additive term of this lane's key
  const DropKey dk = make_drop(a.dropout_p, a.site, a.rng);
  StatBase stat0 = ((int64_t)bq0 * a.nh + h) * a.Lq;
  Draws pw(stat0, a.Lk, g, key);

  f32x4 accK[D / 16], accV[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) accK[i] = accV[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // delta[q] = rowsum(dO * O) is recomputed here for every query chunk (four threads per query row, a quarter of the head
  // dimension each) instead of being read from the dQ half: the two halves of the backward then share no data and run as ONE
  // launch, side by side (they used to be two dependent launches).
  // (The one-pass kernel's row sum adds in another order -- two 8-wide halves per thread, not ld4 groups of four -- so the two
  // are not one helper: either order in the other kernel would change the bits of dQ / dK.)
  Stage64<T, D> pq, po;
  float plse = INFINITY, pdel = 0.f;
  auto prefetch = [&](int c0) {
    pq.load(Qb, a.ldq, c0, a.Lq, tid);
    po.load(dOb, a.lddo, c0, a.Lq, tid);
    const int qq = c0 + (tid >> 2), part = tid & 3;
    float dsum = 0.f;
    if (qq < a.Lq) {
      const T* dr = dOb + (int64_t)qq * a.lddo + part * (D / 4);
      const T* orow = Ob + (int64_t)qq * a.ldo + part * (D / 4);
#pragma unroll
      for (int e = 0; e < D / 4; e += 4) {
        const f32x4 x = ld4(dr + e), y = ld4(orow + e);
        dsum += x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
      }
    }
    dsum += __shfl_xor(dsum, 1, 64);
    dsum += __shfl_xor(dsum, 2, 64);
    pdel = dsum;                                              // valid in the lanes with part == 0
    if (tid < 64) {
      const int q1 = c0 + tid;
      plse = q1 < a.Lq ? a.LSE[stat0 + q1] : INFINITY;        // +inf => p = 0 for padded query rows
    }
  };
  prefetch(0);
  int m = 0;                                                  // GROUPED: the member of the group whose chunks are being consumed
  for (int c0 = 0; c0 < a.Lq; c0 += 64) {
    __syncthreads();
    pq.store(sQr, BF ? sQt : nullptr, tid);
    po.store(sOr, BF ? sOt : nullptr, tid);
    if (tid < 64) sLse[tid] = plse;
    if ((tid & 3) == 0) sDel[tid >> 2] = pdel;
    __syncthreads();
    if (c0 + 64 < a.Lq) prefetch(c0 + 64);
    bool next_member = false;
    if constexpr (GROUPED) {
      next_member = c0 + 64 >= a.Lq && m + 1 < a.kv_group;
      if (next_member) {                                      // the last chunk of member m: prefetch the next member's first
        const HeadBase<T, D, false> hn(a, bq0 + m + 1, h);
        Ob = hn.O(a, 0); Qb = hn.Q; dOb = hn.dO(a, 0);
        stat0 = ((int64_t)(bq0 + m + 1) * a.nh + h) * a.Lq;
        prefetch(0);
      }
    }
    const int ntile = (a.Lq - c0 + 15) / 16 < 4 ? (a.Lq - c0 + 15) / 16 : 4;
    const uint64_t e2chunk = pw.chunk(c0);
    auto tiles = [&](auto full_tag, const int pr, const int nt) {
      constexpr bool FULL = decltype(full_tag)::value;
      f32x4 s[TP], dp[TP];
      float pd[TP][4], ds[TP][4];
#pragma unroll
      for (int tt = 0; tt < TP; ++tt) {
        if (FULL || tt < nt) {
          s[tt] = first_product<T, D>(sQr, 16 * TP * pr + tt * 16, kf, lane);     // [q = 4g+r][key = li]
          dp[tt] = first_product<T, D>(sOr, 16 * TP * pr + tt * 16, vf, lane);
        }
      }
#pragma unroll
      for (int tt = 0; tt < TP; ++tt) {
        if (FULL || tt < nt) {
          const int q0 = 16 * TP * pr + tt * 16;
          const f32x4 lse4 = *(const f32x4*)(sLse + q0 + 4 * g);
          const f32x4 del4 = *(const f32x4*)(sDel + q0 + 4 * g);
          float f[4] = {1.f, 1.f, 1.f, 1.f};
          pair_drop_factors<E32>(dk, e2chunk, q0, pw.half, pw.odd, f);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float add = kadd;
            if (!FULL && a.causal) add = causal_add(a, add, key, c0 + q0 + 4 * g + r);
            const float p = __expf(s[tt][r] * a.scale + add - lse4[r]);
            pd[tt][r] = p * f[r];
            ds[tt][r] = p * (dp[tt][r] * f[r] - del4[r]) * a.scale;
          }
        }
      }
      if (TP > 1 && (FULL || nt > 1)) {
        second_product_pair<T, D>(accV, sOt, 16 * TP * pr, pd[0], pd[TP - 1], lane);
        second_product_pair<T, D>(accK, sQt, 16 * TP * pr, ds[0], ds[TP - 1], lane);
      } else {
        second_product<T, D>(accV, sOt, 16 * TP * pr, pd[0], lane);
        second_product<T, D>(accK, sQt, 16 * TP * pr, ds[0], lane);
      }
    };
#pragma unroll 1
    for (int pr = 0; pr < 4 / TP; ++pr) {
      const int nt = ntile - TP * pr;
      if (nt <= 0) break;
      if (TP > 1 && nt >= TP && !a.causal) tiles(std::true_type{}, pr, TP);      // (TP = 1: the generic body has no tile tests)
      else tiles(std::false_type{}, pr, nt);
    }
    if constexpr (GROUPED) {
      if (next_member) {                                      // on to member m + 1: its draw indices, its chunk 0 (c0 += 64 follows)
        ++m;
        pw = PairDraw(stat0, a.Lk, g, key);
        c0 = -64;
      }
    }
  }
  store_dkv<T, D>(a, b, h, key, g, accK, accV);
}
