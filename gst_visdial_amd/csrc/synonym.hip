// Nearest neighbours by cosine for the coreference attack's synonym table (utils/text_attack.py:103-116 reads
// argsort(-cos_sim[row])[1:11] with a 0.5 cut out of a V x V matrix that comp_cos_sim_mat.py stores).  gstvd_cos_topk yields the K
// best per source row straight from the table of unit rows Ehat [V, D] fp32: the product runs on the f32-input MFMA (16x16x4, exact
// fp32) and each row's running K best is kept next to it, so the V x V matrix never exists.
//
// One kernel body serves both shapes.  A wave owns ONE block of 16 source rows (staged once in LDS) and walks a range of targets 64
// at a time (four 16x16 accumulators, the targets' fragments straight from global memory, two batches of loads in flight).  After a
// 64-target step each lane compares its 16 products against its rows' current K-th entry; the few that pass are inserted one by
// one into the row's sorted list in LDS (the rare path: once the lists have filled almost every candidate fails that comparison).
//   many sources: 2 waves = 2 source blocks, every wave walks all V targets, the lists are the result (written once, no workspace;
//                 32 rows of D = 300 take 40 KB of LDS, so three workgroups share a CU);
//   few sources : 4 waves = 1 source block, the targets split over the waves and over blockIdx.y; every (split, wave) leaves a
//                 partial list in the workspace and a second launch merges a row's partial lists.
// A pair's D products are added in one fixed order in both (k = 16 s + 4 g + e: s ascending, then e, then g inside the MFMA), so
// the two routes return the same bits.  No atomics; every output element is written once; the order (larger value first, then the
// smaller index: select.h's) is strict over distinct targets, so nothing depends on which workgroup finishes first.
#include "gemm_common.h"
#include "select.h"

namespace {

constexpr int TJ = 4;                     // 16-target tiles per wave step
constexpr int UB = 4;                     // 16-wide k steps per batch of loads
constexpr int STEP = TJ * 16;             // targets per wave step
constexpr int MAX_D = 512;                // a workgroup's source rows live in LDS: 32 x (D + 4) floats, 66 KB here (300 must fit: 40 KB)
constexpr int MANY_MIN_ROWS = 64 * 256;   // from here on the 32-row workgroups alone fill the 256 CUs twice over

typedef Sel Ent;                          // i == SEL_NONE: an unused slot while lists are built (stored as -1)

struct TopkP {
  const float* E; const int32_t* src; int64_t ld;
  int V, D, n, K; float thr;
  int chunk;                              // targets per workgroup (a multiple of 4 * STEP)
  int P;                                  // partial lists per source row in ws; 0: the lists go to idx / val
  Ent* ws; int32_t* idx; float* val;
};

// Sorted insert of (v, t) into a list of K entries, all 64 lanes of the wave calling; lanes 0..15 hold one entry each.  Entries
// better than the candidate form a prefix (the list is sorted), the rest moves down one slot, the last one falls out.
DEVFN void list_insert(volatile float* lv, volatile int* lx, int K, float v, int t, int lane) {
  const int k = lane & 15;
  const bool in = lane < 16 && k < K;
  const float ov = in ? lv[k] : 0.f;
  const int ox = in ? lx[k] : SEL_NONE;
  const float pv = (in && k > 0) ? lv[k - 1] : 0.f;
  const int px = (in && k > 0) ? lx[k - 1] : SEL_NONE;
  const int pos = __popcll(__ballot(in && sel_before(ov, ox, v, t)));
  if (in && k >= pos) {                   // (every read above is issued before any of these writes: LDS is in order per wave)
    lv[k] = k == pos ? v : pv;
    lx[k] = k == pos ? t : px;
  }
}

template <int SB, int NW>
__global__ __launch_bounds__(NW * 64) void cos_topk_kernel(TopkP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int WPB = NW / SB;            // waves per source block
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int Dp = (p.D + 15) & ~15, S = Dp + 4, NS = Dp / 16, NB = (NS + UB - 1) / UB, K = p.K;
  float* As = (float*)smem;               // [SB * 16][S], zero beyond D and for rows without a source
  float* lv = As + SB * 16 * S;           // [NW waves][16 rows][K]
  int* lx = (int*)(lv + NW * 16 * K);
  int* srow = lx + NW * 16 * K;                // [SB * 16] source index, -1: none
  const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int row0 = blockIdx.x * (SB * 16);
  for (int r = wave; r < SB * 16; r += NW) {
    const int gr = row0 + r;
    int s = -1;
    if (gr < p.n) {
      s = p.src ? p.src[gr] : gr;
      if (s < 0 || s >= p.V) s = -1;      // outside the table: no memory is read, the row stays empty
    }
    if (lane == 0) srow[r] = s;
    for (int k = lane * 4; k < S; k += 256)
      *(f32x4*)(As + r * S + k) = (s >= 0 && k < p.D) ? *(const f32x4*)(p.E + (int64_t)s * p.ld + k) : zero;
  }
  for (int i = tid; i < NW * 16 * K; i += NW * 64) { lv[i] = -__builtin_inff(); lx[i] = SEL_NONE; }
  __syncthreads();                        // the last one: from here on the waves do not meet

  const int blk = wave % SB, sl = wave / SB;
  const float* Aw = As + blk * 16 * S + li * S + 4 * g;
  volatile float* wv = lv + wave * 16 * K;
  volatile int* wx = lx + wave * 16 * K;
  int sidx[4], ki[4];
  float kv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { sidx[e] = srow[blk * 16 + 4 * g + e]; kv[e] = -__builtin_inff(); ki[e] = SEL_NONE; }
  const int sub = p.chunk / WPB;
  const int64_t tb = (int64_t)blockIdx.y * p.chunk + (int64_t)sl * sub;
  const int tbeg = (int)(tb < p.V ? tb : p.V), tend = (int)(tb + sub < p.V ? tb + sub : p.V);
  const int n_iter = (row0 + blk * 16 < p.n) ? (tend - tbeg + STEP - 1) / STEP : 0;
  const int Q = n_iter * NB;

  f32x4 acc[TJ];
#pragma unroll
  for (int j = 0; j < TJ; ++j) acc[j] = zero;

  auto load = [&](int q, f32x4 (&dst)[UB][TJ]) {
    const int it = q / NB, b = q - it * NB;
    const int t0 = tbeg + it * STEP;
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int k0 = (b * UB + u) * 16 + 4 * g;
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const int t = t0 + 16 * j + li;   // rows at or beyond V and columns at or beyond D are never read
        dst[u][j] = (q < Q && k0 < p.D && t < tend) ? *(const f32x4*)(p.E + (int64_t)t * p.ld + k0) : zero;
      }
    }
  };

  auto epilogue = [&](int t0) {
    bool pass[TJ][4];
    bool any = false;
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int t = t0 + 16 * j + li;
#pragma unroll
      for (int e = 0; e < 4; ++e) {       // lane holds dot(source 4 g + e, target t0 + 16 j + li)
        const float v = acc[j][e];
        pass[j][e] = sidx[e] >= 0 && t < tend && t != sidx[e] && v >= p.thr && sel_before(v, t, kv[e], ki[e]);
        any |= pass[j][e];
      }
    }
    if (__ballot(any) == 0) return;
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        unsigned long long m = __ballot(pass[j][e]);
        while (m) {
          const int L = __ffsll((long long)m) - 1;
          m &= m - 1;
          const float cv = __shfl(acc[j][e], L, 64);
          const int row = 4 * (L >> 4) + e;
          list_insert(wv + row * K, wx + row * K, K, cv, t0 + 16 * j + (L & 15), lane);
        }
      }
#pragma unroll
    for (int e = 0; e < 4; ++e) { kv[e] = wv[(4 * g + e) * K + K - 1]; ki[e] = wx[(4 * g + e) * K + K - 1]; }
  };

  auto mma = [&](int q, const f32x4 (&bf)[UB][TJ]) {
    const int it = q / NB, b = q - it * NB;
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int s = b * UB + u;
      if (s < NS) {
        const f32x4 a = *(const f32x4*)(Aw + 16 * s);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < TJ; ++j) acc[j] = mfma_f32_k4(a[e], bf[u][j][e], acc[j]);
      }
    }
    if (b == NB - 1) {
      epilogue(tbeg + it * STEP);
#pragma unroll
      for (int j = 0; j < TJ; ++j) acc[j] = zero;
    }
  };

  f32x4 b0[UB][TJ], b1[UB][TJ];
  load(0, b0);
  for (int q = 0; q < Q; q += 2) {
    load(q + 1, b1);
    mma(q, b0);
    load(q + 2, b0);
    if (q + 1 < Q) mma(q + 1, b1);
  }

  for (int i = lane; i < 16 * K; i += 64) {
    const int r = i / K, k = i - r * K, gr = row0 + blk * 16 + r;
    if (gr >= p.n) continue;
    const float v = wv[i];
    const int x = wx[i];
    if (p.P == 0) {
      p.idx[(int64_t)gr * K + k] = x == SEL_NONE ? -1 : x;
      p.val[(int64_t)gr * K + k] = x == SEL_NONE ? 0.f : v;
    } else {
      p.ws[((int64_t)gr * p.P + blockIdx.y * WPB + sl) * K + k] = Ent{v, x};
    }
  }
}

// Second launch of the few-sources route: one wave per source row over its P sorted partial lists; K passes, each taking the best
// entry that is worse than the one taken before (the order is strict: a target sits in exactly one partial list).
__global__ __launch_bounds__(64) void cos_topk_merge_kernel(const Ent* __restrict__ ws, int P, int K, int32_t* __restrict__ idx,
                                                            float* __restrict__ val) {
  const Ent* row = ws + (int64_t)blockIdx.x * P * K;
  const int lane = threadIdx.x;
  float lastv = __builtin_inff();
  int lasti = -1;
  for (int k = 0; k < K; ++k) {
    Sel b{-__builtin_inff(), SEL_NONE};
    for (int l = lane; l < P; l += 64) {              // a list is sorted: its first entry worse than the last one taken is its best left
      const Ent* list = row + (int64_t)l * K;
      for (int j = 0; j < K; ++j) {
        const Ent e = list[j];
        if (e.i == SEL_NONE) break;
        if (sel_before(lastv, lasti, e.v, e.i)) {
          b = sel_take(b, e.v, e.i);
          break;
        }
      }
    }
    b = sel_wave_best(b);
    const float bv = b.v;
    const int bi = b.i;
    if (lane == 0) {
      idx[(int64_t)blockIdx.x * K + k] = bi == SEL_NONE ? -1 : bi;
      val[(int64_t)blockIdx.x * K + k] = bi == SEL_NONE ? 0.f : bv;
    }
    if (bi == SEL_NONE) { lastv = -__builtin_inff(); lasti = SEL_NONE; }      // nothing is worse than this: the rest stays unused
    else { lastv = bv; lasti = bi; }
  }
}

struct Plan { int route; int splits; int chunk; int P; };

int auto_route(int64_t n) { return n >= MANY_MIN_ROWS ? GSTVD_COS_TOPK_MANY : GSTVD_COS_TOPK_FEW; }

Plan make_plan(int64_t n, int64_t V, int route) {
  Plan pl;
  pl.route = route == GSTVD_COS_TOPK_AUTO ? auto_route(n) : route;
  if (pl.route == GSTVD_COS_TOPK_MANY) {
    pl.splits = 1;
    pl.chunk = (int)((V + STEP - 1) / STEP * STEP);
    pl.P = 0;
  } else {                                 // enough (source block, target split) workgroups for four per CU
    const int64_t unit = 4 * STEP, blocks = (n + 15) / 16, units = (V + unit - 1) / unit;
    int64_t splits = 1024 / blocks;
    splits = splits < 1 ? 1 : (splits > units ? units : splits);
    pl.chunk = (int)(((V + splits - 1) / splits + unit - 1) / unit * unit);
    pl.splits = (int)((V + pl.chunk - 1) / pl.chunk);
    pl.P = pl.splits * 4;
  }
  return pl;
}

constexpr int lds_bytes(int SB, int NW, int D, int K) {
  return SB * 16 * (((D + 15) & ~15) + 4) * (int)sizeof(float) + NW * 16 * K * (int)sizeof(Ent) + SB * 16 * (int)sizeof(int);
}

template <int SB, int NW> int launch_topk(const TopkP& p, int splits, hipStream_t s) {
  static int attr_rc = ensure_lds((cos_topk_kernel<SB, NW>), lds_bytes(SB, NW, MAX_D, 16));
  if (attr_rc) return attr_rc;
  const dim3 grid((unsigned)((p.n + SB * 16 - 1) / (SB * 16)), (unsigned)splits);
  hipLaunchKernelGGL((cos_topk_kernel<SB, NW>), grid, dim3(NW * 64), lds_bytes(SB, NW, p.D, p.K), s, p);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int32_t gstvd_cos_topk_route(int64_t n, int64_t V) {
  (void)V;
  return n < 1 ? 0 : auto_route(n);
}

extern "C" int64_t gstvd_cos_topk_ws_bytes(int64_t n, int64_t V, int32_t K) {
  if (n < 1 || V < 1 || K < 1 || K > 16) return 0;
  return n * make_plan(n, V, GSTVD_COS_TOPK_FEW).P * K * (int64_t)sizeof(Ent);
}

extern "C" int gstvd_cos_topk(const float* Ehat, int64_t ld, int64_t V, int64_t D, const int32_t* src, int64_t n, int32_t K,
                              float threshold, int32_t route, void* ws, int64_t ws_bytes, int32_t* idx, float* val,
                              gstvd_stream_t s) {
  if (!Ehat || !idx || !val) return GSTVD_E_NULL;
  if (n < 1 || V < 1 || D < 1 || ld < D || K < 1 || K > 16 || (!src && n != V) || threshold != threshold) return GSTVD_E_SHAPE;
  if (route != GSTVD_COS_TOPK_AUTO && route != GSTVD_COS_TOPK_MANY && route != GSTVD_COS_TOPK_FEW) return GSTVD_E_SHAPE;
  if (D > MAX_D || V > (1 << 30) || n > (1 << 30)) return GSTVD_E_UNSUPPORTED;
  if ((D % 4) || (ld % 4) || ((uintptr_t)Ehat & 15)) return GSTVD_E_ALIGN;
  const Plan pl = make_plan(n, V, route);
  if (pl.P) {
    if (!ws) return GSTVD_E_NULL;
    if ((uintptr_t)ws & 7) return GSTVD_E_ALIGN;
    if (ws_bytes < n * pl.P * K * (int64_t)sizeof(Ent)) return GSTVD_E_SHAPE;
  }
  TopkP p{Ehat, src, ld, (int)V, (int)D, (int)n, K, threshold, pl.chunk, pl.P, (Ent*)ws, idx, val};
  hipStream_t st = (hipStream_t)s;
  if (pl.route == GSTVD_COS_TOPK_MANY) return launch_topk<2, 2>(p, 1, st);
  const int rc = launch_topk<1, 4>(p, pl.splits, st);
  if (rc) return rc;
  hipLaunchKernelGGL(cos_topk_merge_kernel, dim3((unsigned)n), dim3(64), 0, st, (const Ent*)ws, pl.P, (int)K, idx, val);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
