// LDS-DMA ring pieces shared by the bf16 tiles of gemm_dma.hip, gemm_dma256.hip and gemm_rows.hip: the DMA issue, the zero page, the
// per-thread unit table, the tile order, the consumers' K-step and the epilogue tail of a wave.
#pragma once
#include "gemm_common.h"

// LDS-DMA issue in inline asm.  The compiler's waitcnt pass treats a *builtin* global_load_lds as a pending LDS write and
// puts `s_waitcnt vmcnt(0)` in front of every ds_read_b64_tr_b16 that follows (it cannot see that the ring slot being
// read is not the one being filled) -- which serialises the ring for k-major operands.  Issued from asm the DMA is
// invisible to that pass; ordering is ours: a counted `s_waitcnt vmcnt(N)` + s_barrier before a slot is read, and
// `s_waitcnt vmcnt(0)` before the epilogue.  m0 (the LDS destination base) is saved/restored around the instruction.
DEVFN void glds16_asm(const char* gsrc, unsigned lds_dst_uniform) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst_uniform) : "memory");
}
DEVFN unsigned lds_addr(const char* p) { return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)p; }
// one 16-byte unit per lane into the 1 KB of LDS at the (wave-uniform) address lds_wave_base
DEVFN void glds16(const char* src, char* lds_wave_base) {
  glds16_asm(src, __builtin_amdgcn_readfirstlane(lds_addr(lds_wave_base)));
}

// What an out-of-range unit reads instead (tails never mask lanes).  One per translation unit: nothing outside these files uses it.
static __device__ __attribute__((aligned(256))) char g_zero_page[256];

// Per-thread description of the 16-byte units this thread feeds into one operand image, fixed over the K loop.  KD = K depth of a
// stage (64 or 32 elements); the images are those of gemm_common.h (rm_off<KD> / km_off_bf16): the LDS side of the DMA is
// lane-linear, so the read swizzle is applied to the per-lane SOURCE address.
template <int BX, bool KM, int NP, int NT, int KD = 64>
struct DmaUnits {
  const char* ptr[NP];   // address of the unit in K-tile 0 (meaningless when !okx)
  int kofs[NP];          // k index of the unit inside a K-tile
  bool okx[NP];
  int64_t kstep;         // byte advance per K-tile

  DEVFN void init(const char* g, int64_t ld, int64_t x0, int64_t X, int tid) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int u = i * NT + tid;
      int64_t x;
      if (!KM) {
        constexpr int LG = KD == 64 ? 3 : 2;               // 2^LG 16-byte slots per row
        const int r = u >> LG, ls = rm_slot<KD>(r, u & ((1 << LG) - 1));
        x = x0 + r;
        kofs[i] = ls * 8;
        ptr[i] = g + (x * ld + ls * 8) * 2;
      } else {
        constexpr int VPR = BX / 8, NB = BX / 16;
        const int kr = u / VPR, cu = u % VPR;
        const int f = (kr & 3) | (((kr >> 3) & 1) << 2);
        const int lb = ((cu >> 1) ^ f) & (NB - 1);
        x = x0 + lb * 16 + (cu & 1) * 8;
        kofs[i] = kr;
        ptr[i] = g + ((int64_t)kr * ld + x) * 2;
      }
      okx[i] = x < X;
    }
    kstep = KM ? KD * ld * 2 : KD * 2;
  }
  DEVFN void issue(int64_t kt, int64_t K, char* img, int wave) const {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const bool ok = okx[i] && (kt * KD + kofs[i] < K);
      glds16(ok ? ptr[i] + kt * kstep : (const char*)g_zero_page, img + (i * NT + wave * 64) * 16);
    }
  }
};

// XCD-aware block order: blocks b and b+8 share an XCD (private 4 MiB L2); give each XCD a contiguous run of ids
DEVFN int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// Tile order: tiles are numbered in column strips STRIP n-tiles wide, row-major inside a strip (the last strip may be narrower), so
// the ~32 consecutive ids an XCD runs concurrently form a compact block that shares A rows and B columns in its L2 (STRIP = 4: an
// (8 m) x (4 n) block).  wg = the tile's id, ntn = n-tiles of the problem, nwg = all its tiles; BM x BNU = the tile's extent.
template <int BM, int BNU, int STRIP>
DEVFN void tile_origin(int wg, int ntn, int nwg, int64_t& m0, int64_t& n0) {
  const int ntm = nwg / ntn;
  const int strip = wg / (STRIP * ntm), sw = (ntn - strip * STRIP) < STRIP ? (ntn - strip * STRIP) : STRIP;
  const int within = wg - strip * STRIP * ntm;
  m0 = (int64_t)(within / sw) * BM;
  n0 = (int64_t)(strip * STRIP + within % sw) * BNU;
}

// One 32-deep K-step of a wave's MI x NI accumulator tiles: read_b(j) / read_a(i) return the bf16x8 fragment of column / row block
// j / i.  PRELOAD_A: all A fragments up front, then the MFMAs (96 accumulator registers leave room for them at 168 VGPRs);
// otherwise one row block at a time in front of the MFMAs that use it (128 accumulator registers: the compiler then takes the
// fragments two at a time).
template <int MI, int NI, bool PRELOAD_A, typename RA, typename RB>
DEVFN void mma_step(f32x4 (&acc)[MI][NI], RA read_a, RB read_b) {
  bf16x8 fb[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) fb[j] = read_b(j);
  if constexpr (PRELOAD_A) {
    bf16x8 fa[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) fa[i] = read_a(i);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) acc[i][j] = mfma_bf16_k32(fb[j], fa[i], acc[i][j]);
  } else {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const bf16x8 fa = read_a(i);
#pragma unroll
      for (int j = 0; j < NI; ++j) acc[i][j] = mfma_bf16_k32(fb[j], fa, acc[i][j]);
    }
  }
}

DEVFN int opaque_lane(int lane) { asm volatile("" : "+v"(lane)); return lane; }

// Epilogue of a producer / consumer tile's consumer wave, MI x NI accumulator tiles at (mw, nw): bf16 outputs whose operand rows are
// 16-byte aligned go row-wise through the wave's parking space `park` in the idle ring (gemm_epilogue_rows, EPI_HB row blocks per
// pass), everything else tile-wise.  The caller has a barrier in front (nobody reads the ring any more).  The 8-wave tiles
// (dma_tile, dma_tile256) keep their tail -- no opaque lanes, the barrier behind the epilogue_rows_ok test -- written out (measured).
// The per-lane addresses are derived from an OPAQUE copy of the lane id: derived from `lane` the compiler computes them in front of
//   the K loop and, at the 168-VGPR cap of three waves per SIMD, spills them across it (8-28 B of scratch per lane, which also makes
//   the dispatch set up scratch memory) -- VERDICT r5 item 1b.  (The row-wise bf16 epilogue is better off without it.)  In the
//   tile-wise fallback, fresh opaque lane values per row block keep its 64-bit row / column indices from being computed up front
//   and spilled at that cap.
constexpr int EPI_HB = 4;
template <typename OT, int MI, int NI, bool LATE>
DEVFN void gemm_epilogue_wave(const GemmP& p, const f32x4 (&acc)[MI][NI], int64_t z, int64_t mw, int64_t nw, char* park, int lane) {
  const int lane_e = sizeof(OT) == 4 ? opaque_lane(lane) : lane;
  const int g = lane_e >> 4, li = lane_e & 15;
  const DropKey dk = make_drop((p.epi & GSTVD_EPI_DROPOUT) ? p.p : 0.f, p.site, p.rng);
  if constexpr (sizeof(OT) == 2) {
    if (epilogue_rows_ok(p)) {
      gemm_epilogue_rows<MI, NI, EPI_HB, LATE>(p, dk, acc, z, mw, nw, park, lane_e);
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int li_i = opaque_lane(li), g_i = opaque_lane(g);
#pragma unroll
    for (int j = 0; j < NI; ++j) gemm_epilogue_tile<bf16, OT>(p, dk, acc[i][j], z, mw + i * 16 + li_i, nw + j * 16 + 4 * g_i);
  }
}
