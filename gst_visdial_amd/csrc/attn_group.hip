// Backward of a grouped cross-attention launch (gstvd_attn_group_bwd): kv_group = G consecutive query rows share the K, V and
// key mask of ONE row -- the decoder's cross-attention when the G answer candidates of a dialog round are scored against one
// encoder pass (gstvd_attn_fwd with kv_group > 1).  gstvd_attn_bwd refuses such a descriptor; this entry takes it.
//
//   * the two bodies are those of the two-part backward (attn_common.h), instantiated with GROUPED: a dQ block owns 64 queries
//     of one (query row, head) and reads the keys of row b / G; a dK/dV block owns 64 keys of one (K/V row e, head) and walks the
//     query chunks of rows e * G .. e * G + G - 1 in ascending order into ONE set of accumulators, then stores once.  dK and dV
//     are therefore written, not accumulated: no float atomics, no reduction launch, the same order of additions every run;
//   * dropout: no keep bits exist for a grouped forward; both bodies hash the draws again, element index
//     ((b * nh + h) * Lq + q) * round4(Lk) + k with b the QUERY row -- the index the forward used;
//   * one launch, a 1-D grid with all key-owning blocks first: they run G times as many chunk rounds as without the group and
//     are the long pole (E * nh * ceil(Lk / 64) of them); the query-owning blocks (B * nh * ceil(Lq / 64)) fill in behind.
#include "common.h"
#include "attn_common.h"

// Two waves per SIMD for every head size: the key-owning blocks are few (fewer than the chip has CUs at the training shape) and
// long, so what counts is that their body -- the two-part backward's plus the group walk -- keeps its values in registers (at
// three waves per SIMD the d = 64 instantiations spill).
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void xgroup_bwd(gstvd_attn_t a, int nkb, int nqb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int G = a.kv_group;
  int id = blockIdx.x;
  const int nfirst = nkb * a.nh * (a.B / G);                  // key-owning blocks
  const bool is_dq = id >= nfirst;
  if (is_dq) id -= nfirst;
  const int per = is_dq ? nqb : nkb;
  const int bx = id % per, bh = id / per, h = bh % a.nh, b = bh / a.nh;      // b: a query row (dQ) or a K / V row (dK, dV)
  if constexpr (sizeof(T) == 2) {
    if (attn_small_index_space(a)) {
      if (!is_dq) attn_bwd_dkv_body<T, D, true, true>(a, bx, h, b, smem);
      else attn_bwd_dq_body<T, D, true, true>(a, bx, h, b, smem);
      return;
    }
  }
  if (!is_dq) attn_bwd_dkv_body<T, D, false, true>(a, bx, h, b, smem);
  else attn_bwd_dq_body<T, D, false, true>(a, bx, h, b, smem);
}

template <typename T, int D> static int xgroup_launch(const gstvd_attn_t& a, hipStream_t s) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int lds1 = (BF ? 3 : 2) * Img<T, D>::BYTES + 64 * 4;
  constexpr int lds2 = (BF ? 4 : 2) * Img<T, D>::BYTES + 128 * 4;
  constexpr int lds = lds1 > lds2 ? lds1 : lds2;
  static int rc = [] {
    if (lds <= 48 * 1024) return 0;
    hipError_t e = hipFuncSetAttribute((const void*)xgroup_bwd<T, D>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e == hipSuccess ? 0 : (int)e;
  }();
  if (rc) return rc;
  const int nkb = (a.Lk + 63) / 64, nqb = (a.Lq + 63) / 64;
  const int64_t nblk = (int64_t)nkb * a.nh * (a.B / a.kv_group) + (int64_t)nqb * a.nh * a.B;
  if (nblk > 0x7fffffffLL) return GSTVD_E_SHAPE;
  hipLaunchKernelGGL((xgroup_bwd<T, D>), dim3((unsigned)nblk), dim3(256), lds, s, a, nkb, nqb);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
template <typename T> static int xgroup_d(const gstvd_attn_t& a, hipStream_t s) {
  if (a.d == 32) return xgroup_launch<T, 32>(a, s);
  if (a.d == 64) return xgroup_launch<T, 64>(a, s);
  return xgroup_launch<T, 128>(a, s);
}

extern "C" int gstvd_attn_group_bwd(const gstvd_attn_t* a, gstvd_stream_t stream) {
  if (!a || !a->Q || !a->K || !a->V || !a->O) return GSTVD_E_NULL;
  if (a->dtype != GSTVD_F32 && a->dtype != GSTVD_BF16) return GSTVD_E_DTYPE;
  if (a->d != 32 && a->d != 64 && a->d != 128) return GSTVD_E_UNSUPPORTED;
  if (a->B <= 0 || a->nh <= 0 || a->Lq <= 0 || a->Lk <= 0) return GSTVD_E_SHAPE;
  if (a->causal || a->q_bstride != 0 || a->kv_bstride != 0 || a->kv_group < 0 || (a->kv_group > 1 && a->B % a->kv_group)) return GSTVD_E_UNSUPPORTED;
  const int ve = a->dtype == GSTVD_BF16 ? 8 : 4;
  if ((a->ldq % ve) || (a->ldk % ve) || (a->ldv % ve) || (a->ldo % 4)) return GSTVD_E_ALIGN;
  if (((uintptr_t)a->Q | (uintptr_t)a->K | (uintptr_t)a->V | (uintptr_t)a->O) & 15) return GSTVD_E_ALIGN;
  if (!a->dO || !a->dQ || !a->dK || !a->dV || !a->LSE || !a->delta) return GSTVD_E_NULL;
  if ((a->lddo % ve) || (a->lddq % 4) || (a->lddk % 4) || (a->lddv % 4)) return GSTVD_E_ALIGN;
  gstvd_attn_t g = *a;
  if (g.kv_group == 0) g.kv_group = 1;                        // (0 and 1 both mean one K / V row per query row)
  return g.dtype == GSTVD_BF16 ? xgroup_d<bf16>(g, (hipStream_t)stream) : xgroup_d<float>(g, (hipStream_t)stream);
}
