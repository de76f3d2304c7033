// Fused dropout + residual + LayerNorm (forward/backward) and the two embedding front ends of the
// ViLBERT-dialog encoder / BERT-generation decoder.  HBM-bound: one wave64 per row, 4-element (8/16 B)
// vector accesses, row statistics by wave shuffles, dropout masks regenerated from the counter hash.
// Reference arithmetic: models/vilbert_dialog.py:283-296 (TF-style LN), :324-352 (BertEmbeddingsDialog),
// :1420-1427 (BertImageEmbeddings), :416-420 / :458-462 / :735-742 (dense -> dropout -> LN(x + residual)).
// The row arithmetic itself is in ln_row.h, shared with the fused prologues of gemm_rows.hip.
#include <stdio.h>
#include <type_traits>

#include "ln_row.h"

// rows per wave in backward: 2 (both rows' loads in flight before any reduction) for large M; 1 for small M, where the
// grid cannot fill the chip anyway and the shorter per-wave chain is what counts (decoder / vision rows)
static inline int ln_bwd_rw(int64_t M) { return M <= 8192 ? 1 : 2; }
// waves per block in backward.  Every block writes one [3][H] slab of column partials; with 4 one-row waves per block that
// was 9.4 MB of partials for a 4096x768 LayerNorm -- more than any one of its operands -- read again by the column-sum launch
// (0.34 ms per step).  From 2048 rows up a block has 16 waves (one block per CU, 147 KB of LDS for the per-wave slabs, same
// number of rows in flight on the chip): a quarter of the partial bytes.  The LayerNorm kernel itself takes the same time.
static inline int ln_bwd_nw(int64_t M, int mode, int64_t H) { return (M >= 2048 && mode != GSTVD_LN_EMBED && H <= 768) ? 16 : 4; }

// h = pre-LayerNorm row, 4 elements starting at column c
template <typename T, int MODE>
DEVFN f32x4 ln_prologue(const gstvd_ln_t& f, int64_t row, int c, const DropKey& dpre,
                        int64_t id, int64_t tpos, int64_t seg, const float* locrow) {
  f32x4 h;
  if (MODE == GSTVD_LN_RESID) {
    h = ld4((const T*)f.x + row * f.ldx + c);
    ln_resid(h, ln_drop(dpre, row, f.H, c), f.res != nullptr, [&] { return ld4((const T*)f.res + row * f.ldres + c); });
  } else if (MODE == GSTVD_LN_EMBED) {
    h = *(const f32x4*)(f.word + id * f.H + c) + *(const f32x4*)(f.pos + tpos * f.H + c);
    const float* trow = (seg < f.type_vocab) ? f.tt + seg * f.H : f.tt_ext + (seg - f.type_vocab) * f.H;
    h += *(const f32x4*)(trow + c);
  } else {
    h = ld4((const T*)f.x + row * f.ldx + c);
    f32x4 l = *(const f32x4*)(f.b_loc + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float* w = f.w_loc + (int64_t)(c + e) * 5;
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < 5; ++j) a += locrow[j] * w[j];
      l[e] += a;
    }
    h += l;
  }
  return h;
}

template <typename T, int MODE, int NV>
__global__ __launch_bounds__(256) void ln_fwd_kernel(gstvd_ln_t f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= f.M) return;
  const int H = (int)f.H;
  const DropKey dpre = make_drop(MODE == GSTVD_LN_RESID ? f.p_pre : 0.f, f.site_pre, f.rng);
  const DropKey dpost = make_drop(f.p_post, f.site_post, f.rng);
  int64_t id = 0, tpos = 0, seg = 0;
  float locrow[5] = {0, 0, 0, 0, 0};
  if (MODE == GSTVD_LN_EMBED) { id = f.ids[row]; tpos = row % f.T + f.pos_offset; seg = f.segs ? f.segs[row] : 0; }
  if (MODE == GSTVD_LN_IMAGE) {
#pragma unroll
    for (int j = 0; j < 5; ++j) locrow[j] = f.loc[row * 5 + j];
  }
  f32x4 h[NV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const auto [c, in] = ln_col(lane, i, H);
    h[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (in) {
      h[i] = ln_prologue<T, MODE>(f, row, c, dpre, id, tpos, seg, locrow);
      s += ln_sum4(h[i]);
    }
  }
  const float mean = ln_row_mean(s, H);
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (ln_col(lane, i, H).in) v += ln_var_term(h[i], mean, NV == 1);
  const float rstd = ln_rstd(v, H, f.eps);
  if (lane == 0) { f.mean[row] = mean; f.rstd[row] = rstd; }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const auto [c, in] = ln_col(lane, i, H);
    if (in) {
      f32x4 y = ln_y(h[i], mean, rstd, *(const f32x4*)(f.gamma + c), *(const f32x4*)(f.beta + c));
      y *= ln_drop(dpost, row, f.H, c);
      st4((T*)f.y + row * f.ldy + c, y);
    }
  }
}

// LDS of the backward in vectors of H floats per wave, read by the kernel's carve-up and by the launcher's size alike.  NVP: the
// column partials that go to HBM; embedding mode with H <= 1024 (EXT) adds the block's position row (NVL = 5) and, behind all
// waves' slabs, one word strip per wave.
constexpr bool ln_bwd_ext(int mode, int nv) { return mode == GSTVD_LN_EMBED && nv <= 4; }
constexpr int ln_bwd_nvp(int mode) { return mode == GSTVD_LN_EMBED ? 4 : 3; }
constexpr int ln_bwd_nvl(int mode, int nv) { return ln_bwd_ext(mode, nv) ? 5 : ln_bwd_nvp(mode); }
constexpr int ln_bwd_lds(int mode, int nv, int nw, int64_t H) {
  return (int)(nw * (ln_bwd_nvl(mode, nv) + (ln_bwd_ext(mode, nv) ? 1 : 0)) * H * sizeof(float));
}

// Backward: a block owns 4*RW consecutive rows, each wave RW of them (RW = 1 up to 8192 rows: measured 17.1 -> 13.0 us
// at 4096x768 and 13.4 -> 8.0 us at 400x768; RW = 2 beyond).  With RW = 2 both rows' loads are issued
// before any reduction (memory-level parallelism), column partial sums stay in registers and are combined
// across the 4 waves through LDS with plain stores (no LDS atomics), one [3][H] slab per block goes to HBM.
template <typename T, int MODE, int NV, int RW, int NW = 4>
__global__ __launch_bounds__(NW * 64) void ln_bwd_kernel(gstvd_ln_bwd_t p) {
  constexpr int LN_BWD_RPB = NW * RW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = (float*)smem;                   // [NW waves][NVL][H], then (EXT) [NW waves][H] word strips
  const gstvd_ln_t& f = p.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = (int)f.H;
  const DropKey dpre = make_drop(MODE == GSTVD_LN_RESID ? f.p_pre : 0.f, f.site_pre, f.rng);
  const DropKey dpost = make_drop(f.p_post, f.site_post, f.rng);
  constexpr int NVP = ln_bwd_nvp(MODE), NVL = ln_bwd_nvl(MODE, NV);
  constexpr bool EXT = ln_bwd_ext(MODE, NV);
  f32x4 ag[NV], ab[NV], ax[NV], a4[NV], ap[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) ag[i] = ab[i] = ax[i] = a4[i] = ap[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Embedding mode, whole batches of rows per block (M = B * T, B a multiple of the block's rows): a block takes rows of ONE
  // position t -- batch rows b0 .. b0 + RPB - 1 -- so their position-embedding gradients are summed in the block and reach
  // dpos[t] as one atomic add per element and block instead of one per row (B-way contention on every address of a table of
  // T rows: the kernel is the last one of backward, 0.1 ms for 4096 rows).
  const int64_t nbat = (MODE == GSTVD_LN_EMBED && f.T > 0) ? f.M / f.T : 0;
  const bool pos_block = EXT && nbat > 0 && nbat * f.T == f.M && nbat % LN_BWD_RPB == 0;
  const int64_t bpt = pos_block ? nbat / LN_BWD_RPB : 1;     // blocks per position
  const int64_t row0 = pos_block ? ((int64_t)(blockIdx.x % bpt) * LN_BWD_RPB + wave * RW) * f.T + blockIdx.x / bpt
                                 : (int64_t)blockIdx.x * LN_BWD_RPB + wave * RW;
  const int64_t rstep = pos_block ? f.T : 1;                 // distance between a wave's consecutive rows
  float* wstrip = red + (int64_t)NW * NVL * H + (int64_t)wave * H;          // embedding mode: one row of dh per wave
  f32x4 xh[RW][NV], gy[RW][NV], dyv[RW][NV];
  float s1[RW] = {}, s2[RW] = {}, rstd[RW] = {};
  int64_t id[RW] = {}, tpos[RW] = {}, seg[RW] = {};
  bool rv[RW];
#pragma unroll
  for (int j = 0; j < RW; ++j) {
    const int64_t row = row0 + j * rstep;
    rv[j] = row < f.M;
    float locrow[5] = {0, 0, 0, 0, 0};
    float mean = 0.f;
    if (rv[j]) {
      if (MODE == GSTVD_LN_EMBED) { id[j] = f.ids[row]; tpos[j] = row % f.T + f.pos_offset; seg[j] = f.segs ? f.segs[row] : 0; }
      if (MODE == GSTVD_LN_IMAGE) {
#pragma unroll
        for (int q = 0; q < 5; ++q) locrow[q] = f.loc[row * 5 + q];
      }
      mean = f.mean[row];
      rstd[j] = f.rstd[row];
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const auto [c, in] = ln_col(lane, i, H);
      xh[j][i] = gy[j][i] = dyv[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (rv[j] && in) {
        const f32x4 h = ln_prologue<T, MODE>(f, row, c, dpre, id[j], tpos[j], seg[j], locrow);
        xh[j][i] = ln_xhat(h, mean, rstd[j]);
        dyv[j][i] = ld4((const T*)p.dy + row * p.lddy + c) * ln_drop(dpost, row, f.H, c);
        ln_bwd_sums(dyv[j][i], *(const f32x4*)(f.gamma + c), xh[j][i], gy[j][i], s1[j], s2[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < RW; ++j) {
    const int64_t row = row0 + j * rstep;
    const float c1 = ln_row_mean(s1[j], H), c2 = ln_row_mean(s2[j], H);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const auto [c, in] = ln_col(lane, i, H);
      if (rv[j] && in) {
        const f32x4 dh = ln_bwd_dh(gy[j][i], xh[j][i], c1, c2, rstd[j]);
        ag[i] += dyv[j][i] * xh[j][i];
        ab[i] += dyv[j][i];
        if (MODE == GSTVD_LN_RESID) {
          if (p.dres) st4((T*)p.dres + row * p.lddres + c, dh);
          const f32x4 dx = dh * ln_drop(dpre, row, f.H, c);
          if (p.dx && (p.dx != p.dres || dpre.on)) st4((T*)p.dx + row * p.lddx + c, dx);
          ax[i] += dx;
        } else if (MODE == GSTVD_LN_IMAGE) {
          st4((T*)p.dres + row * p.lddres + c, dh);
          ax[i] += dh;
        } else {
          // token-type rows 0 / 1 receive a contribution from (almost) every token: reduce them through the block
          // partials instead of ~M*H atomics onto two rows; rarer segment ids keep the atomic path
          if (seg[j] == 0) ax[i] += dh;
          else if (seg[j] == 1 && f.type_vocab > 1) a4[i] += dh;
          else {
            float* tg = (seg[j] < f.type_vocab) ? p.dtt + seg[j] * f.H : p.dtt_ext + (seg[j] - f.type_vocab) * f.H;
#pragma unroll
            for (int e = 0; e < 4; ++e) atomicAdd(tg + c + e, dh[e]);
          }
          // padded positions have an exactly-zero gradient (their keys are masked everywhere): skip their atomics,
          // which would all hit the [PAD] word row
          if (dh[0] != 0.f || dh[1] != 0.f || dh[2] != 0.f || dh[3] != 0.f) {
            if (!pos_block) {
#pragma unroll
              for (int e = 0; e < 4; ++e) atomicAdd(p.dpos + tpos[j] * f.H + c + e, dh[e]);
            } else {
              ap[i] += dh;
            }
          }
          // word-embedding row: through the wave's LDS strip, so that one atomic instruction covers 64 CONSECUTIVE columns
          // (two full 128-byte lines) instead of every fourth dword of a 1 KB span (eight lines a quarter used each)
          if (EXT) {
            *(f32x4*)(wstrip + c) = dh;
          } else if (dh[0] != 0.f || dh[1] != 0.f || dh[2] != 0.f || dh[3] != 0.f) {
#pragma unroll
            for (int e = 0; e < 4; ++e) atomicAdd(p.dword + id[j] * f.H + c + e, dh[e]);
          }
        }
      }
    }
    if (EXT && rv[j]) {
      // (same wave wrote the strip: LDS operations of one wave complete in order)
      float* wrow = p.dword + id[j] * f.H;
      for (int c = lane; c < H; c += 64) {
        const float v = wstrip[c];
        if (v != 0.f) atomicAdd(wrow + c, v);
      }
    }
  }
  float* mine = red + (int64_t)wave * NVL * H;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const auto [c, in] = ln_col(lane, i, H);
    if (in) {
      *(f32x4*)(mine + c) = ag[i];
      *(f32x4*)(mine + H + c) = ab[i];
      *(f32x4*)(mine + 2 * H + c) = ax[i];
      if (NVP == 4) *(f32x4*)(mine + 3 * H + c) = a4[i];
      if (NVL == 5) *(f32x4*)(mine + 4 * H + c) = ap[i];
    }
  }
  __syncthreads();
  float* out = p.partial + (int64_t)blockIdx.x * NVP * H;
  for (int i = threadIdx.x * 4; i < NVP * H; i += NW * 256) {
    f32x4 a = *(const f32x4*)(red + i);
#pragma unroll
    for (int w = 1; w < NW; ++w) a += *(const f32x4*)(red + w * NVL * H + i);
    *(f32x4*)(out + i) = a;
  }
  if (NVL == 5 && pos_block) {                               // the block's position row: one atomic add per element
    const int64_t t = (int64_t)(blockIdx.x / bpt) + f.pos_offset;
    for (int i = threadIdx.x * 4; i < H; i += NW * 256) {
      f32x4 a = *(const f32x4*)(red + 4 * H + i);
#pragma unroll
      for (int w = 1; w < NW; ++w) a += *(const f32x4*)(red + w * NVL * H + 4 * H + i);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (a[e] != 0.f) atomicAdd(p.dpos + t * f.H + i + e, a[e]);
    }
  }
}

// ---- column reductions -------------------------------------------------------------------------------
// the table entry that owns block b: the last one whose first block blk0 is <= b
template <typename E> DEVFN int table_entry(const E* tab, int nent, int b) {
  int lo = 0, hi = nent - 1;
  while (lo < hi) { int mid = (lo + hi + 1) >> 1; if (tab[mid].blk0 <= b) lo = mid; else hi = mid - 1; }
  return lo;
}

// out_j[c] (+)= sum_k partial[k * stride + j * H + c] for the 64-column slice `local` of the entry's nvec * H wide row;
// block = 64 columns x 4 row groups
DEVFN void colsum_entry(const gstvd_colsum_entry_t e, int local) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int64_t col = (int64_t)local * 64 + cl, W = (int64_t)e.nvec * e.H;
  float a = 0.f;
  if (col < W) {
    // eight independent loads in flight per thread: the embedding LayerNorm's 1024 partial rows used to be 256 dependent
    // load -> add rounds per thread (118 us for a 48-block launch at the very end of backward)
    const float* src = e.partial + col;
    float p8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t k = rg;
    for (; k + 28 < e.nblk; k += 32) {
#pragma unroll
      for (int u = 0; u < 8; ++u) p8[u] += src[(k + 4 * u) * e.stride];
    }
    for (; k < e.nblk; k += 4) a += src[k * e.stride];
    a += ((p8[0] + p8[1]) + (p8[2] + p8[3])) + ((p8[4] + p8[5]) + (p8[6] + p8[7]));
  }
  red[rg][cl] = a;
  __syncthreads();
  if (rg == 0 && col < W) {
    a = red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl];
    const int64_t j = col / e.H, c = col % e.H;
    // (selects, not e.out[j]: a dynamically indexed member put the whole entry on the stack -- 88 B/lane of scratch)
    float* o = j == 0 ? e.out[0] : (j == 1 ? e.out[1] : e.out[2]);
    const int acc = j == 0 ? e.accumulate[0] : (j == 1 ? e.accumulate[1] : e.accumulate[2]);
    if (o) o[c] = acc ? o[c] + a : a;
  }
}
// one entry as the kernel's argument (gstvd_colsum_partials, stage 2 of gstvd_colsum): block b = slice b
__global__ __launch_bounds__(256) void colsum_entry_kernel(gstvd_colsum_entry_t e) { colsum_entry(e, blockIdx.x); }
// All pending column reductions of a backward pass in ONE launch: block b serves the 64-column slice
// (b - blk0) of the entry that contains it (binary search over the entries' first-block offsets).
__global__ __launch_bounds__(256) void colsum_batched_kernel(const gstvd_colsum_entry_t* tab, int nent) {
  const gstvd_colsum_entry_t e = tab[table_entry(tab, nent, blockIdx.x)];
  colsum_entry(e, blockIdx.x - e.blk0);
}

// stage 1 of a plain column sum: block = 64-row slab x 256 columns (column block cb) -> scratch[slab][N]
template <typename T>
DEVFN void colsum_slab(const T* x, int64_t ldx, int64_t M, int64_t N, float* scratch, int cb, int64_t slab) {
  __shared__ f32x4 red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c = (int64_t)cb * 256 + lane * 4, r0 = slab * 64;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (c < N) {
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      int64_t r = r0 + wave + 4 * i;
      if (r < M) a += ld4(x + r * ldx + c);
    }
  }
  red[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && c < N) {
    a = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
    *(f32x4*)(scratch + slab * N + c) = a;
  }
}
template <typename T>
__global__ __launch_bounds__(256) void colsum_slab_kernel(const T* x, int64_t ldx, int64_t M, int64_t N, float* scratch) {
  colsum_slab(x, ldx, M, N, scratch, blockIdx.x, blockIdx.y);
}
// table-driven form of the slab stage: every pending bias-gradient column sum of a backward pass in one launch
template <typename T>
__global__ __launch_bounds__(256) void colsum_slab_batched_kernel(const gstvd_slab_entry_t* tab, int nent) {
  const gstvd_slab_entry_t e = tab[table_entry(tab, nent, blockIdx.x)];
  const int ncb = (int)((e.N + 255) / 256), local = blockIdx.x - e.blk0;
  colsum_slab((const T*)e.x, e.ldx, e.M, e.N, e.scratch, local % ncb, local / ncb);
}

// dW_loc[h][j] += sum_m dh[m][h] loc[m][j]; grid (ceil(H/256), MS) with atomics
template <typename T>
__global__ __launch_bounds__(256) void locgrad_kernel(const T* dh, int64_t lddh, const float* loc, int64_t M, int64_t H, float* dw) {
  const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (h >= H) return;
  const int64_t per = (M + gridDim.y - 1) / gridDim.y;
  const int64_t m0 = blockIdx.y * per, m1 = (m0 + per < M) ? m0 + per : M;
  float a[5] = {0, 0, 0, 0, 0};
  for (int64_t m = m0; m < m1; ++m) {
    const float d = to_f(dh[m * lddh + h]);
#pragma unroll
    for (int j = 0; j < 5; ++j) a[j] += d * loc[m * 5 + j];
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) atomicAdd(dw + h * 5 + j, a[j]);
}

// ---- host side -------------------------------------------------------------------------------------
static int ln_check(const gstvd_ln_t* p) {
  if (!p) return GSTVD_E_NULL;
  if (p->dtype != GSTVD_F32 && p->dtype != GSTVD_BF16) return GSTVD_E_DTYPE;
  if (p->M <= 0 || p->H <= 0 || (p->H % 4) || p->H > 2048) return GSTVD_E_SHAPE;
  if (!p->gamma || !p->beta || !p->mean || !p->rstd) return GSTVD_E_NULL;
  if (p->mode == GSTVD_LN_RESID) { if (!p->x) return GSTVD_E_NULL; }
  else if (p->mode == GSTVD_LN_EMBED) { if (!p->ids || !p->word || !p->pos || !p->tt || !p->tt_ext || p->T <= 0) return GSTVD_E_NULL; }
  else if (p->mode == GSTVD_LN_IMAGE) { if (!p->x || !p->loc || !p->w_loc || !p->b_loc) return GSTVD_E_NULL; }
  else return GSTVD_E_UNSUPPORTED;
  return 0;
}

// The route of a launch: ONE decision -- mode, type, NV (256-column vectors per lane), RW (rows per wave), NW (waves per block) and
// the grid -- taken here; the launchers below act on it and gstvd_ln_kernel_name reports it.
struct LnRoute { int mode, bf, nv, rw, nw; int64_t nblk; };
static inline int ln_nv(int64_t H) { return H <= 256 ? 1 : (H <= 768 ? 3 : (H <= 1024 ? 4 : 8)); }

static LnRoute ln_fwd_route(const gstvd_ln_t& f) {
  return {f.mode, f.dtype == GSTVD_BF16, ln_nv(f.H), 1, 4, (f.M + 3) / 4};
}

extern "C" int64_t gstvd_ln_bwd_blocks(int64_t M) { const int rpb = 4 * ln_bwd_rw(M); return (M + rpb - 1) / rpb; }
extern "C" int64_t gstvd_ln_bwd_blocks_for(int64_t M, int64_t H, int32_t mode) {
  if (ln_bwd_nw(M, mode, H) == 16 && ln_bwd_rw(M) == 1) return (M + 15) / 16;
  return gstvd_ln_bwd_blocks(M);
}

// nblk = 0 or gstvd_ln_bwd_blocks(M): 4 waves per block; nblk = gstvd_ln_bwd_blocks_for(M, H, mode) where that differs: the
// caller sized `partial` for the 16-wave geometry; any other count is refused
static int ln_bwd_route(const gstvd_ln_bwd_t& b, LnRoute* r) {
  const gstvd_ln_t& f = b.f;
  const int64_t narrow = gstvd_ln_bwd_blocks(f.M), wide = gstvd_ln_bwd_blocks_for(f.M, f.H, f.mode);
  if (b.nblk > 0 && b.nblk != wide && b.nblk != narrow) return GSTVD_E_SHAPE;
  const bool w = b.nblk > 0 && b.nblk == wide && wide != narrow;
  *r = {f.mode, f.dtype == GSTVD_BF16, ln_nv(f.H), w ? 1 : ln_bwd_rw(f.M), w ? 16 : 4, w ? wide : narrow};
  return 0;
}

// The route's type, mode and NV as template arguments: go(T{}, mode, nv) with T the element type and two std::integral_constant
// -- the one ladder of each kind, for forward and backward alike.
template <typename F> static int by_ln_mode(int mode, F f) {
  if (mode == GSTVD_LN_RESID) return f(std::integral_constant<int, GSTVD_LN_RESID>{});
  if (mode == GSTVD_LN_EMBED) return f(std::integral_constant<int, GSTVD_LN_EMBED>{});
  return f(std::integral_constant<int, GSTVD_LN_IMAGE>{});
}
template <typename F> static int by_ln_nv(int nv, F f) {
  if (nv == 1) return f(std::integral_constant<int, 1>{});
  if (nv == 3) return f(std::integral_constant<int, 3>{});
  if (nv == 4) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 8>{});
}
template <typename F> static int by_ln_route(const LnRoute& r, F go) {
  return by_ln_mode(r.mode, [&](auto mode) {
    return by_ln_nv(r.nv, [&](auto nv) { return r.bf ? go(bf16{}, mode, nv) : go(float{}, mode, nv); });
  });
}

// plan-only mode (gstvd_ln_kernel_name): the launch site records the kernel handle it WOULD have launched and launches nothing
template <typename T, int MODE, int NV>
static int ln_fwd_go(const gstvd_ln_t& f, const LnRoute& r, hipStream_t s, const void** plan) {
  if (plan) { *plan = (const void*)ln_fwd_kernel<T, MODE, NV>; return 0; }
  hipLaunchKernelGGL((ln_fwd_kernel<T, MODE, NV>), dim3((unsigned)r.nblk), dim3(256), 0, s, f);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
static int ln_fwd_entry(const gstvd_ln_t* p, hipStream_t s, const void** plan) {
  int rc = ln_check(p);
  if (rc) return rc;
  if (!p->y) return GSTVD_E_NULL;
  const LnRoute r = ln_fwd_route(*p);
  return by_ln_route(r, [&](auto t, auto mode, auto nv) { return ln_fwd_go<decltype(t), mode.value, nv.value>(*p, r, s, plan); });
}
extern "C" int gstvd_ln_fwd(const gstvd_ln_t* p, gstvd_stream_t stream) { return ln_fwd_entry(p, (hipStream_t)stream, nullptr); }

template <typename T, int MODE, int NV, int RW, int NW>
static int ln_bwd_go(const gstvd_ln_bwd_t& p, const LnRoute& r, hipStream_t s, const void** plan) {
  auto k = ln_bwd_kernel<T, MODE, NV, RW, NW>;
  if (plan) { *plan = (const void*)k; return 0; }
  static int attr_rc = ensure_lds(k, ln_bwd_lds(MODE, NV, NW, NV * 256));      // once, for this instantiation's widest row
  if (attr_rc) return attr_rc;
  hipLaunchKernelGGL(k, dim3((unsigned)r.nblk), dim3(NW * 64), ln_bwd_lds(MODE, NV, NW, p.f.H), s, p);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
template <typename T, int MODE, int NV>
static int ln_bwd_geo(const gstvd_ln_bwd_t& p, const LnRoute& r, hipStream_t s, const void** plan) {
  // the 16-wave block exists for one-row waves, H <= 768, outside embedding mode: what ln_bwd_nw / gstvd_ln_bwd_blocks_for name;
  // should the two ever drift apart, the launch fails here instead of taking another kernel than the one reported
  if constexpr (MODE != GSTVD_LN_EMBED && NV <= 3) {
    if (r.nw == 16 && r.rw == 1) return ln_bwd_go<T, MODE, NV, 1, 16>(p, r, s, plan);
  }
  if (r.nw != 4) return GSTVD_E_UNSUPPORTED;
  return r.rw == 1 ? ln_bwd_go<T, MODE, NV, 1, 4>(p, r, s, plan) : ln_bwd_go<T, MODE, NV, 2, 4>(p, r, s, plan);
}
static int ln_bwd_entry(const gstvd_ln_bwd_t* b, hipStream_t s, const void** plan) {
  if (!b) return GSTVD_E_NULL;
  int rc = ln_check(&b->f);
  if (rc) return rc;
  if (!b->dy || !b->partial) return GSTVD_E_NULL;
  if (b->f.mode == GSTVD_LN_EMBED && (!b->dword || !b->dpos || !b->dtt || !b->dtt_ext)) return GSTVD_E_NULL;
  if (b->f.mode == GSTVD_LN_IMAGE && !b->dres) return GSTVD_E_NULL;
  LnRoute r;
  rc = ln_bwd_route(*b, &r);
  if (rc) return rc;
  return by_ln_route(r, [&](auto t, auto mode, auto nv) { return ln_bwd_geo<decltype(t), mode.value, nv.value>(*b, r, s, plan); });
}
extern "C" int gstvd_ln_bwd(const gstvd_ln_bwd_t* b, gstvd_stream_t stream) { return ln_bwd_entry(b, (hipStream_t)stream, nullptr); }

// Which kernel would gstvd_ln_fwd (bwd == 0: desc is a gstvd_ln_t) / gstvd_ln_bwd (bwd != 0: desc is a gstvd_ln_bwd_t) launch?  The
// entry point runs exactly as for a launch -- same checks, same route -- in plan-only mode: nothing is launched, no memory is
// touched.  Writes the device function's (mangled) symbol into buf; a buffer too small for it is GSTVD_E_SHAPE.
extern "C" int gstvd_ln_kernel_name(const void* desc, int32_t bwd, char* buf, int32_t buf_len) {
  if (!desc || !buf || buf_len <= 1) return GSTVD_E_NULL;
  const void* fn = nullptr;
  const int rc = bwd ? ln_bwd_entry((const gstvd_ln_bwd_t*)desc, nullptr, &fn) : ln_fwd_entry((const gstvd_ln_t*)desc, nullptr, &fn);
  if (rc) return rc;
  const char* name = fn ? hipKernelNameRefByPtr(fn, nullptr) : nullptr;
  if (!name) return GSTVD_E_UNSUPPORTED;
  const int n = snprintf(buf, (size_t)buf_len, "%s", name);
  return n >= 0 && n < buf_len ? 0 : GSTVD_E_SHAPE;
}

// one column sum described by an entry: a block per 64 of its nvec * H output columns
static int colsum_entry_launch(const gstvd_colsum_entry_t& e, hipStream_t s) {
  hipLaunchKernelGGL(colsum_entry_kernel, dim3((unsigned)((e.nvec * e.H + 63) / 64)), dim3(256), 0, s, e);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
extern "C" int gstvd_colsum_partials(const float* partial, int64_t nblk, int64_t nvec, int64_t H,
                                     float* out0, float* out1, float* out2, int32_t accumulate, gstvd_stream_t stream) {
  if (!partial) return GSTVD_E_NULL;
  if (nblk <= 0 || nvec <= 0 || nvec > 3 || H <= 0) return GSTVD_E_SHAPE;
  return colsum_entry_launch({partial, {out0, out1, out2}, nblk, 3 * H, H, (int32_t)nvec, {accumulate, accumulate, accumulate}, 0},
                             (hipStream_t)stream);
}

extern "C" int gstvd_colsum_batched(const gstvd_colsum_entry_t* table_dev, int64_t nent, int64_t total_blocks, gstvd_stream_t stream) {
  if (!table_dev) return GSTVD_E_NULL;
  if (nent <= 0 || total_blocks <= 0) return GSTVD_E_SHAPE;
  hipLaunchKernelGGL(colsum_batched_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev, (int)nent);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

// the slab stage of a plain column sum: scratch[slab][N] (slab = 64 rows)
static int colsum_slabs_launch(const void* x, int64_t ldx, int64_t M, int64_t N, int32_t dtype, float* scratch, int64_t scratch_elems,
                               hipStream_t s) {
  if (!x || !scratch) return GSTVD_E_NULL;
  if (M <= 0 || N <= 0 || (N % 4)) return GSTVD_E_SHAPE;
  const int64_t nslab = (M + 63) / 64;
  if (scratch_elems < nslab * N) return GSTVD_E_SHAPE;
  dim3 grid((unsigned)((N + 255) / 256), (unsigned)nslab);
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(colsum_slab_kernel<T>, grid, dim3(256), 0, s, (const T*)x, ldx, M, N, scratch));
  GSTVD_LAUNCH_CHECK();
  return 0;
}
// stage 1 only; finish with gstvd_colsum_batched / _partials
extern "C" int gstvd_colsum_slabs(const void* x, int64_t ldx, int64_t M, int64_t N, int32_t dtype, float* scratch,
                                  int64_t scratch_elems, gstvd_stream_t stream) {
  return colsum_slabs_launch(x, ldx, M, N, dtype, scratch, scratch_elems, (hipStream_t)stream);
}

extern "C" int gstvd_colsum_slabs_batched(const gstvd_slab_entry_t* table_dev, int64_t nent, int64_t total_blocks, int32_t dtype,
                                          gstvd_stream_t stream) {
  if (!table_dev) return GSTVD_E_NULL;
  if (nent <= 0 || total_blocks <= 0) return GSTVD_E_SHAPE;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(colsum_slab_batched_kernel<T>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev, (int)nent));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

// both stages: the slab stage, then out[c] (+)= sum_s scratch[s][c]
extern "C" int gstvd_colsum(const void* x, int64_t ldx, int64_t M, int64_t N, int32_t dtype, float* out,
                            float* scratch, int64_t scratch_elems, int32_t accumulate, gstvd_stream_t stream) {
  if (!out) return GSTVD_E_NULL;
  const int rc = colsum_slabs_launch(x, ldx, M, N, dtype, scratch, scratch_elems, (hipStream_t)stream);
  if (rc) return rc;
  return colsum_entry_launch({scratch, {out, nullptr, nullptr}, (M + 63) / 64, N, N, 1, {accumulate, 0, 0}, 0}, (hipStream_t)stream);
}

extern "C" int gstvd_locgrad(const void* dh, int64_t lddh, const float* loc, int64_t M, int64_t H, int32_t dtype,
                             float* dw_loc, int32_t accumulate, gstvd_stream_t stream) {
  if (!dh || !loc || !dw_loc) return GSTVD_E_NULL;
  if (M <= 0 || H <= 0) return GSTVD_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (!accumulate) {
    hipError_t e = hipMemsetAsync(dw_loc, 0, (size_t)H * 5 * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
  }
  dim3 grid((unsigned)((H + 255) / 256), 16);
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(locgrad_kernel<T>, grid, dim3(256), 0, s, (const T*)dh, lddh, loc, M, H, dw_loc));
  GSTVD_LAUNCH_CHECK();
  return 0;
}
