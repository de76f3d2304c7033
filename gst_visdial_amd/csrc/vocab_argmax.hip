// Arg-max over the vocabulary for the masked-LM fill-in (utils/text_attack.py:30-56: torch.argmax of BertForMaskedLM's logits at
// the [MASK] positions).  Two entry points:
//   gstvd_rows_argmax : logits [n, ld] already in memory -> per row the largest of columns 0..V-1 and its column;
//   gstvd_vocab_argmax: the decoder product fused in -- z[r, v] = sum_k x[r, k] * w[v, k] (bf16 operands, fp32 accumulate) + bias[v]
//                       -- so the [n, V] logits never exist.  MFMA tiles over (64-row block, 64-column vocabulary tile); a tile's
//                       epilogue reduces each of its rows to one (value, column) pair in a workspace [n, n_tiles]; a second, small
//                       launch reduces a row's pairs.  No atomics: the result does not depend on the order workgroups finish in.
// One total order everywhere, select.h's: larger value first, then the SMALLER column.  Inputs are assumed finite.
#include "gemm_common.h"
#include "select.h"

namespace {

typedef Sel Best;                                 // (value, column): one workspace entry

template <int CTRL> DEVFN void dpp_take(Best& b) {
  const float v = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, b.v), CTRL, 0xf, 0xf, true));
  const int c = __builtin_amdgcn_mov_dpp(b.i, CTRL, 0xf, 0xf, true);
  b = sel_take(b, v, c);
}
// Best over the 16 lanes of a DPP row (lanes with equal lane >> 4), result in every lane of the row: the moves of wave_sum.
DEVFN void row16_best(Best& b) {
  dpp_take<0xB1>(b);      // quad_perm [1,0,3,2]
  dpp_take<0x4E>(b);      // quad_perm [2,3,0,1]
  dpp_take<0x141>(b);     // row_half_mirror
  dpp_take<0x140>(b);     // row_mirror
}

// ---- rows_argmax: one workgroup per row, columns dealt to the threads in ascending order -------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rows_argmax_kernel(const T* __restrict__ z, int64_t ld, int V, int64_t* __restrict__ idx,
                                                          float* __restrict__ val) {
  __shared__ float smv[4];
  __shared__ int smi[4];
  const T* row = z + (int64_t)blockIdx.x * ld;
  Best b{-__builtin_inff(), SEL_NONE};
  for (int c = threadIdx.x; c < V; c += 256) {
    const float v = to_f(row[c]);
    if (v > b.v) { b.v = v; b.i = c; }          // a thread's columns ascend: strict > keeps the smaller one
  }
  b = sel_block_best<4>(b, smv, smi);
  if (threadIdx.x == 0) { idx[blockIdx.x] = b.i == SEL_NONE ? 0 : b.i; val[blockIdx.x] = b.v; }
}

// ---- second launch of the fused form: one wave per row over its n_tiles pairs -------------------------------------------------
__global__ __launch_bounds__(64) void pairs_argmax_kernel(const Best* __restrict__ ws, int n_tiles, int64_t* __restrict__ idx,
                                                          float* __restrict__ val) {
  const Best* row = ws + (int64_t)blockIdx.x * n_tiles;
  Best b{-__builtin_inff(), SEL_NONE};
  for (int t = threadIdx.x; t < n_tiles; t += 64) b = sel_take(b, row[t].v, row[t].i);
  b = sel_wave_best(b);
  if (threadIdx.x == 0) { idx[blockIdx.x] = b.i == SEL_NONE ? 0 : b.i; val[blockIdx.x] = b.v; }
}

// ---- fused product + per-tile reduction ---------------------------------------------------------------------------------------
// Workgroup = 4 waves on a tile of MI * 16 rows x 64 vocabulary columns.  The waves split K (contiguous quarters, so a wave walks
// whole cache lines of a table row) and every wave holds the full MI x 4 grid of 16x16 accumulators; operands go straight from
// global memory into MFMA fragments (a table element is used once per row block, the few X rows stay in L2).  The four partial
// grids are added through LDS in wave order 0, 1, 2, 3 -- a fixed order -- with wave w summing row block w, which it then reduces:
// in the 16x16x32 result a lane holds rows 4g..4g+3 of column lane & 15, so a row's 16 columns sit in the 16 lanes of one DPP row.
struct VocabP {
  const bf16* X; const bf16* W; const float* bias; Best* ws;
  int64_t ldx, ldw; int n, V, H, n_tiles;
};

constexpr int VT = 64, NI = VT / 16, NW = 4;

template <int MI>
__global__ __launch_bounds__(NW * 64) void vocab_argmax_kernel(VocabP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  f32x4* red = (f32x4*)smem;                       // [NW][MI * NI][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int tile = blockIdx.x, v0 = tile * VT, r0 = blockIdx.y * (MI * 16);
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const bf16x8 zero = __builtin_bit_cast(bf16x8, (s16x8){0, 0, 0, 0, 0, 0, 0, 0});
  const bf16* xrow[MI]; bool xin[MI];
  const bf16* wrow[NI]; bool win[NI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int r = r0 + i * 16 + li;
    xin[i] = r < p.n;
    xrow[i] = p.X + (int64_t)(xin[i] ? r : 0) * p.ldx + 8 * g;
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int v = v0 + j * 16 + li;
    win[j] = v < p.V;                              // rows of the table at or beyond V are never read
    wrow[j] = p.W + (int64_t)(win[j] ? v : 0) * p.ldw + 8 * g;
  }
  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nk = p.H / 32, per = (nk + NW - 1) / NW;
  const int s_end = min(nk, (wave + 1) * per);
  constexpr int UNR = MI >= 3 ? 2 : 4;
  for (int s0 = wave * per; s0 < s_end; s0 += UNR) {
    bf16x8 fa[UNR][MI], fb[UNR][NI];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {                // every load of the batch in flight before its first MFMA
      const bool kin = s0 + u < s_end;
      const int64_t k = (int64_t)(s0 + u) * 32;
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[u][i] = (kin && xin[i]) ? *(const bf16x8*)(xrow[i] + k) : zero;
#pragma unroll
      for (int j = 0; j < NI; ++j) fb[u][j] = (kin && win[j]) ? *(const bf16x8*)(wrow[j] + k) : zero;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = mfma_bf16_k32(fa[u][i], fb[u][j], acc[i][j]);
  }
  // lane holds z[r0 + 16 i + 4 g + e][v0 + 16 j + li], e = 0..3
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) red[(wave * MI * NI + i * NI + j) * 64 + lane] = acc[i][j];
  __syncthreads();
  if (wave >= MI) return;
  Best best[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) best[e] = Best{-__builtin_inff(), SEL_NONE};
#pragma unroll
  for (int j = 0; j < NI; ++j) {                   // columns ascend with j: strict > keeps the smaller one
    const int v = v0 + j * 16 + li;
    f32x4 t = red[(0 * MI * NI + wave * NI + j) * 64 + lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) t += red[(w * MI * NI + wave * NI + j) * 64 + lane];
    if (v < p.V) {
      const float b = p.bias[v];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float z = t[e] + b;
        if (z > best[e].v) { best[e].v = z; best[e].i = v; }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    row16_best(best[e]);
    const int r = r0 + wave * 16 + 4 * g + e;
    if (li == 0 && r < p.n) p.ws[(int64_t)r * p.n_tiles + tile] = best[e];
  }
}

template <int MI> int launch_vocab(const VocabP& p, hipStream_t s) {
  const int lds = NW * MI * NI * 64 * (int)sizeof(f32x4);
  static int attr_rc = ensure_lds(vocab_argmax_kernel<MI>, lds);
  if (attr_rc) return attr_rc;
  const dim3 grid((unsigned)p.n_tiles, (unsigned)((p.n + MI * 16 - 1) / (MI * 16)));
  hipLaunchKernelGGL(vocab_argmax_kernel<MI>, grid, dim3(NW * 64), lds, s, p);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int gstvd_rows_argmax(const void* logits, int64_t ld, int64_t n, int64_t V, int32_t dtype, int64_t* idx, float* val,
                                 gstvd_stream_t s) {
  if (!logits || !idx || !val) return GSTVD_E_NULL;
  if (n < 1 || V < 1 || V > 0x7fffffff || ld < V || n > 0x7fffffff) return GSTVD_E_SHAPE;
  GSTVD_FOR_DTYPE(dtype, T, hipLaunchKernelGGL(rows_argmax_kernel<T>, dim3((unsigned)n), dim3(256), 0, (hipStream_t)s,
                                               (const T*)logits, ld, (int)V, idx, val));
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t gstvd_vocab_argmax_ws_bytes(int64_t n, int64_t V) {
  if (n < 1 || V < 1) return 0;
  return n * ((V + VT - 1) / VT) * (int64_t)sizeof(Best);
}

extern "C" int gstvd_vocab_argmax(const void* X, int64_t ldx, const void* W, int64_t ldw, const float* bias, int64_t n, int64_t V,
                                  int64_t H, int32_t dtype, void* ws, int64_t ws_bytes, int64_t* idx, float* val, gstvd_stream_t s) {
  if (!X || !W || !bias || !ws || !idx || !val) return GSTVD_E_NULL;
  if (n < 1 || V < 1 || H < 1 || ldx < H || ldw < H) return GSTVD_E_SHAPE;
  if (dtype != GSTVD_BF16 || H % 32 || V > (1 << 30) || n > (1 << 20)) return GSTVD_E_UNSUPPORTED;
  if ((ldx % 8) || (ldw % 8) || ((uintptr_t)X & 15) || ((uintptr_t)W & 15) || ((uintptr_t)ws & 7)) return GSTVD_E_ALIGN;
  if (ws_bytes < gstvd_vocab_argmax_ws_bytes(n, V)) return GSTVD_E_SHAPE;
  VocabP p{(const bf16*)X, (const bf16*)W, bias, (Best*)ws, ldx, ldw, (int)n, (int)V, (int)H, (int)((V + VT - 1) / VT)};
  hipStream_t st = (hipStream_t)s;
  int rc;
  if (n <= 16) rc = launch_vocab<1>(p, st);
  else if (n <= 32) rc = launch_vocab<2>(p, st);
  else if (n <= 48) rc = launch_vocab<3>(p, st);
  else rc = launch_vocab<4>(p, st);
  if (rc) return rc;
  hipLaunchKernelGGL(pairs_argmax_kernel, dim3((unsigned)n), dim3(64), 0, st, (const Best*)p.ws, p.n_tiles, idx, val);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
