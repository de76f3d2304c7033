// 256x256x32 bf16 MFMA GEMM tile, 8 waves (each 128x64), LDS-DMA ring of NS256 stages (3 since round 3; 5 = the whole 160 KB LDS
// of a CU in rounds 1-2).
//
// Measured on MI355X (profiles/r01_pmc_gemm_l2_fetch.json): with 128x128x64 tiles the main loop is bound by the rate
// at which a CU can fill LDS (~35-50 GB/s per CU, L2 hit 70-82 %), i.e. by bytes staged per FLOP (1 B / 64 FLOP).
// This tile stages the same 32 KB per K-step but does 4x the MFMA work per step over half the K depth:
// 1 B / 128 FLOP.  Same ring / counted-vmcnt / one-barrier structure and the same zero-page tails as gemm_dma.hip.
//
// LDS images for a 32-deep K step (gemm_common.h: rm_off<32>, km_off_bf16; unit table: DmaUnits<.., 32> of gemm_ring.h):
//   row-major operand  : 256 rows x 64 B; 16-byte slot s of row r lives at slot s ^ (2*((r>>3)&1))
//   k-major operand    : 32 k-rows x 512 B; 32-byte block b of k-row r lives at block b ^ ((r&3) | ((r>>3)&1)<<2)
#include "gemm_ring.h"

static constexpr int g_strip_w = 8;      // column-strip width of the tile order (measured 2 / 4 / 8: 31.3 / 30.7 / 30.5 us at 4096x3072x768)
// Ring depth.  Rounds 1-2 used 5 stages (the whole 160 KB LDS of a CU).  Round 3 measured the K-step slope at 5 / 4 / 3 stages
// (tools/nt_study.py on three builds): 0.669 / 0.686 / 0.684 us (producer / consumer form), 0.775 / 0.736 / 0.778 us (8-wave form)
// -- the K loop is bound by the RATE at which a CU takes operands in, not by bytes in flight -- while every stage less takes
// ~0.8 us off the fill in front of the first MFMA: 29.0 -> 27.8 us at 4096x3072x768, step +0.8 % (1190 vs 1181 rounds/s, three
// A/B pairs).  The LDS allocation is the larger of the ring and the epilogue's parking space.
constexpr int NS256 = 3;

// NIU = 16-column accumulator tiles per wave actually used (4: the full 256-wide tile; 3: a 192-wide tile inside the same
// 256-wide LDS image -- N = 3072 then gives 16 x 16 = 256 tiles, one per CU, instead of 192 tiles on 256 CUs).
// K-step schedule: the DMA issue, then fragment reads two A fragments at a time in front of the MFMAs that use them (the
// compiler's own order).  The schedule variants and timing ablations rounds 2-4 measured against it are in DESIGN_HISTORY.md
// and profiles/.
template <typename OT, bool AKM, bool BKM, int NIU = 4>
DEVFN void dma_tile256(const GemmP& p, int64_t z, int wg, int ntn, int nwg, char* smem) {
  constexpr int BM = 256, BN = 256, WM = 2, WN = 4, NS = NS256, NT = 512;
  constexpr int WTM = BM / WM, WTN = NIU * 16, MI = WTM / 16, NI = NIU, BNU = WN * WTN;   // 8 x NIU accumulator tiles per wave
  constexpr int A_BYTES = BM * 64, B_BYTES = BN * 64, STAGE = A_BYTES + B_BYTES;
  constexpr int NPA = A_BYTES / (NT * 16), NPB = B_BYTES / (NT * 16), LPS = NPA + NPB;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  int64_t m0, n0;
  tile_origin<BM, BNU, g_strip_w>(wg, ntn, nwg, m0, n0);

  DmaUnits<BM, AKM, NPA, NT, 32> ua;
  DmaUnits<BN, BKM, NPB, NT, 32> ub;
  ua.init(p.A + z * p.sA * 2, p.lda, m0, p.M, tid);
  ub.init(p.B + z * p.sB * 2, p.ldb, n0, (n0 + BNU < p.N) ? n0 + BNU : p.N, tid);     // columns past the tile read the zero page

  f32x4 acc[MI][NI];
  zero_acc(acc);

  const int64_t nkt = (p.K + 31) / 32;
#pragma unroll
  for (int s = 0; s < NS - 1; ++s) {
    ua.issue(s, p.K, smem + s * STAGE, wave);
    ub.issue(s, p.K, smem + s * STAGE + A_BYTES, wave);
  }
  int slot = 0, fill = NS - 1;
  for (int64_t t = 0; t < nkt; ++t) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * LPS) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    ua.issue(t + NS - 1, p.K, smem + fill * STAGE, wave);
    ub.issue(t + NS - 1, p.K, smem + fill * STAGE + A_BYTES, wave);
    const char* cA = smem + slot * STAGE;
    const char* cB = cA + A_BYTES;
    mma_step<MI, NI, false>(acc, [&](int i) { return frag_bf16<BM, AKM, 32>(cA, wm * WTM + i * 16, 0, lane); },
                            [&](int j) { return frag_bf16<BN, BKM, 32>(cB, wn * WTN + j * 16, 0, lane); });
    slot = (slot + 1 == NS) ? 0 : slot + 1;
    fill = (fill + 1 == NS) ? 0 : fill + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // (the tail of gemm_epilogue_wave with a barrier in front of the parking stores, written out: behind the helper the 8-wave tile ran
  // 2 % slower at 4688 x 18432 x 768, profiles/gemm_refactor_resources.txt, tried and not kept)
  const int g = lane >> 4, li = lane & 15;
  const DropKey dk = make_drop((p.epi & GSTVD_EPI_DROPOUT) ? p.p : 0.f, p.site, p.rng);
  if constexpr (sizeof(OT) == 2) {
    if (epilogue_rows_ok(p)) {
      __builtin_amdgcn_s_barrier();            // every wave is done reading the ring: its LDS is free for the row-wise epilogue
      gemm_epilogue_rows<MI, NI, 4>(p, dk, acc, z, m0 + wm * WTM, n0 + wn * WTN, smem + wave * epi_wave_bytes<NI, 4>(), lane);
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
      gemm_epilogue_tile<bf16, OT>(p, dk, acc[i][j], z, m0 + wm * WTM + i * 16 + li, n0 + wn * WTN + j * 16 + 4 * g);
}

// ---- weight-gradient tile whose epilogue IS the optimizer step (gstvd_gemm_grouped_adamw) --------------------------------------
// The consumer waves hold 128 accumulator registers each and have nothing to spare for a stream of optimizer state (every
// in-consumer form of this epilogue spilled 100+ registers per lane); the four PRODUCER waves are idle after the K-loop and own
// nearly all of their 168 registers.  So: the consumers park their accumulators -- 4 x NI tiles = 64 rows at a time -- in their
// slices of the idle ring, exactly as gemm_epilogue_rows does, and after a barrier each producer wave runs AdamW on the parked
// rows of two consumer waves: a lane owns 4 consecutive columns of one row (16 lanes = one 256-byte row segment, whole lines per
// instruction), 16-byte loads of param / m / v, the update of common.h, 16-byte stores of param / m / v and 8 bytes of bf16
// shadow.  The state rows are fetched D row groups ahead of their use, IN PROGRAM ORDER in front of the stores of the groups in
// between (the compiler may not move a load across a store it cannot tell apart from it): 3 D 16-byte loads in flight per lane.
// Rows / columns outside the matrix: loads are clamped onto a valid element (no branch around a load), stores are masked.
// Addresses: wave-uniform 64-bit bases + one 32-bit lane offset per row group.
constexpr int ADAMW_PARK_DEPTH = 5;
template <int NI, int ROWS, int D>
DEVFN void adamw_rows_pass(const gstvd_adamw_fuse_t& af, float alpha, float lr, float wd, float bc, const float* park, int64_t flat0,
                           int rows_left, int cols_left, unsigned ldc, int lane) {
  static_assert(NI == 4, "16 lanes x 4 columns = the wave tile's 64 columns");
  constexpr int S = epi_row_floats<NI>(), RPI = 4, R = ROWS / RPI;
  if (rows_left <= 0 || cols_left <= 0) return;           // wave-uniform: the rows lie below / beside the matrix
  const int rl = lane >> 4, c4 = (lane & 15) * 4;
  const bool n_ok = c4 < cols_left;                       // N % 4 == 0: a 4-column piece is all in or all out
  float* Pt = af.param + flat0; float* Mt = af.m + flat0; float* Vt = af.v + flat0;
  bf16* St = (bf16*)af.shadow_bf16 + flat0;
  float* Gt = const_cast<float*>(af.grad_base) + flat0;
  const unsigned cofs = n_ok ? (unsigned)c4 : 0u;
  const int last = rows_left - 1;
  f32x4 bm[D + 1], bv[D + 1], bp[D + 1];
  auto fetch = [&](int rr, int b) {
    const int row = rr * RPI + rl;
    const unsigned o = (unsigned)(row < last ? row : last) * ldc + cofs;
    bm[b] = __builtin_nontemporal_load((const f32x4*)(Mt + o)); bv[b] = __builtin_nontemporal_load((const f32x4*)(Vt + o));
    bp[b] = __builtin_nontemporal_load((const f32x4*)(Pt + o));
  };
#pragma unroll
  for (int k = 0; k < D; ++k) fetch(k, k);
#pragma unroll
  for (int rr = 0; rr < R; ++rr) {
    if (rr + D < R) fetch(rr + D, (rr + D) % (D + 1));
    const int b = rr % (D + 1);
    const int row = rr * RPI + rl;
    f32x4 g4 = *(const f32x4*)(park + row * S + c4);
    g4 = g4 * alpha;                                     // what the plain epilogue stores as dW
    f32x4 p4 = bp[b], m4 = bm[b], v4 = bv[b];
    adamw_update4(p4, m4, v4, g4, af.grad_scale, lr, wd, bc, af.beta1, af.beta2, af.eps);
    if (row < rows_left && n_ok) {
      const unsigned o = (unsigned)row * ldc + (unsigned)c4;
      if (af.write_grad) st4(Gt + o, g4);
      __builtin_nontemporal_store(m4, (f32x4*)(Mt + o));
      __builtin_nontemporal_store(v4, (f32x4*)(Vt + o));
      __builtin_nontemporal_store(p4, (f32x4*)(Pt + o));
      if (af.shadow_bf16) st4(St + o, p4);
    }
  }
}

// Producer / consumer form of the same tile (grids of up to two rounds of tiles, and every grouped launch): 12 waves.  Waves 0-7 are the MFMA consumers of dma_tile256 (128x64 each)
// and never touch the memory pipeline; waves 8-11 are LDS-DMA producers (8 pieces of 1 KB per wave and stage) and never touch
// the matrix pipe.  One s_barrier per K-step still orders everything: before barrier t every producer has waited for its pieces
// of stage t (counted vmcnt) and every consumer has retired its fragment reads of slot t-1, so after it the consumers read slot t
// and the producers refill slot t-1 with stage t+NS-1.  Why: in the 8-wave kernel every wave spends ~260 cycles of each K-step
// issuing DMA and both waves of a SIMD do so at the same time (section 5 of DESIGN.md: 1358 cycles per step without any DMA
// instruction, 1725 with); here the consumers' step IS that DMA-free loop and the DMA issue runs beside it on a third wave of
// the SIMD.  Needs <= 168 VGPRs (three waves per SIMD).
template <typename OT, bool AKM, bool BKM, int NIU = 4, bool CS = false, bool ADAM = false>
DEVFN void pc_tile256(const GemmP& p, int64_t z, int wg, int ntn, int nwg, char* smem, const gstvd_adamw_fuse_t af = gstvd_adamw_fuse_t{}) {
  constexpr int BM = 256, BN = 256, WN = 4, NS = NS256, NTP = 256;
  constexpr int WTM = 128, WTN = NIU * 16, MI = 8, NI = NIU, BNU = WN * WTN;
  constexpr int A_BYTES = BM * 64, B_BYTES = BN * 64, STAGE = A_BYTES + B_BYTES;
  constexpr int NPA = A_BYTES / (NTP * 16), NPB = B_BYTES / (NTP * 16), LPS = NPA + NPB;      // 4 + 4 pieces per producer wave
  static_assert((NS - 2) * LPS <= 63, "vmcnt immediate out of range");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool producer = wave >= 8;
  int64_t m0, n0;
  tile_origin<BM, BNU, g_strip_w>(wg, ntn, nwg, m0, n0);
  const int64_t nkt = (p.K + 31) / 32;

  if (producer) {
    const int ptid = tid - 512, pw = wave - 8;
    DmaUnits<BM, AKM, NPA, NTP, 32> ua;
    DmaUnits<BN, BKM, NPB, NTP, 32> ub;
    ua.init(p.A + z * p.sA * 2, p.lda, m0, p.M, ptid);
    ub.init(p.B + z * p.sB * 2, p.ldb, n0, (n0 + BNU < p.N) ? n0 + BNU : p.N, ptid);
#pragma unroll
    for (int s = 0; s < NS - 1; ++s) {
      ua.issue(s, p.K, smem + s * STAGE, pw);
      ub.issue(s, p.K, smem + s * STAGE + A_BYTES, pw);
    }
    int fill = NS - 1, slot = 0;
    // CS (grouped weight gradients, k-major A = dY): the producers of the tiles in column block 0 also sum the A image over k
    // while it sits in the ring -- bias[m] = sum over the batch rows of dY[row][m], the bias gradient -- instead of a separate
    // pass over dY (colsum_slab_batched: 0.25 ms per step, a 0.7 GB re-read).  Lane = (row group rg = lane >> 3, column group
    // cg = 8 * wave + (lane & 7)): thread reads the 16-byte unit of columns 8cg..8cg+7 in k-rows 4rg..4rg+3 of every stage;
    // the eight row groups of a column group sit in one wave, so the final reduction is three shuffles, no LDS, no barrier.
    const bool do_cs = CS && AKM && (p.epi & GSTVD_EPI_COLSUM) && n0 == 0 && p.bias != nullptr;
    const int rg = lane >> 3, cg = pw * 8 + (lane & 7);
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t t = 0; t < nkt; ++t) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * LPS) : "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      ua.issue(t + NS - 1, p.K, smem + fill * STAGE, pw);
      ub.issue(t + NS - 1, p.K, smem + fill * STAGE + A_BYTES, pw);
      if (CS && do_cs) {
        const char* cA = smem + slot * STAGE;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bf16x8 v = *(const bf16x8*)(cA + km_off_bf16<BM>(rg * 4 + r, cg * 8));
#pragma unroll
          for (int e = 0; e < 8; ++e) cs[e] += (float)v[e];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads are done before this wave releases the slot at the next barrier
      }
      fill = (fill + 1 == NS) ? 0 : fill + 1;
      slot = (slot + 1 == NS) ? 0 : slot + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the ring's trailing (zero page) pieces
    __builtin_amdgcn_s_barrier();                          // pairs with the consumers' barrier in front of the epilogue
    if (CS && do_cs) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = cs[e];
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        cs[e] = v;
      }
      if (rg == 0) {
        const bool accb = (p.epi & GSTVD_EPI_COLSUM_ACC) != 0;
        float* out = const_cast<float*>(p.bias);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int64_t m = m0 + cg * 8 + e;
          if (m < p.M) out[m] = accb ? out[m] + cs[e] : cs[e];
        }
      }
    }
    if constexpr (ADAM) {
      if (p.epi & GSTVD_EPI_ADAMW) {
        // the tile's optimizer constants: uniform -> scalar loads.  addend = this weight's (lr, wd) pair in the device table
        const float* hp2 = (const float*)p.addend;
        const float ad_lr = hp2[0], ad_wd = hp2[1];
        const float ad_bc = adamw_bias_correction(af.beta1, af.beta2, af.step[0]);
        constexpr int HB = MI / 2, ROWS = HB * 16;
        const int64_t cflat = (const float*)p.C - af.grad_base;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          __builtin_amdgcn_s_barrier();                    // the consumers have parked half h (they waited lgkmcnt(0) before arriving)
          asm volatile("" ::: "memory");                   // no park read may be scheduled above the barrier
          if (ad_lr != 0.f) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {                  // this producer wave serves consumer waves 2 pw and 2 pw + 1
              const int cw = pw * 2 + c, cwm = cw / WN, cwn = cw % WN;
              const int64_t mw = m0 + cwm * WTM + h * ROWS, nw = n0 + cwn * WTN;
              const int rows_left = (int)(p.M - mw < ROWS ? p.M - mw : ROWS), cols_left = (int)(p.N - nw < WTN ? p.N - nw : WTN);
              adamw_rows_pass<NI, ROWS, ADAMW_PARK_DEPTH>(af, p.alpha, ad_lr, ad_wd, ad_bc, (const float*)(smem + cw * epi_wave_bytes<NI, HB>()),
                                           cflat + mw * p.ldc + nw, rows_left, cols_left, (unsigned)p.ldc, lane);
            }
          }
          if (h == 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every park read of this wave has returned
            __builtin_amdgcn_s_barrier();                  // the parks may be overwritten
          }
        }
      }
    }
    return;
  }

  const int wm = wave / WN, wn = wave % WN;
  f32x4 acc[MI][NI];
  zero_acc(acc);
  int slot = 0;
  for (int64_t t = 0; t < nkt; ++t) {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const char* cA = smem + slot * STAGE;
    const char* cB = cA + A_BYTES;
    // NIU <= 3: 96 accumulator registers, room for all eight A fragments up front (no spill at 168 VGPRs); 4: as dma_tile256
    mma_step<MI, NI, (NIU <= 3)>(acc, [&](int i) { return frag_bf16<BM, AKM, 32>(cA, wm * WTM + i * 16, 0, lane); },
                                 [&](int j) { return frag_bf16<BN, BKM, 32>(cB, wn * WTN + j * 16, 0, lane); });
    slot = (slot + 1 == NS) ? 0 : slot + 1;
  }
  __builtin_amdgcn_s_barrier();       // every producer has drained its DMAs, every consumer is done with the ring: LDS is free
  if constexpr (ADAM) {
    if (p.epi & GSTVD_EPI_ADAMW) {
      // park 64 rows, let the producer waves update them (adamw_rows_pass), twice
      const int lane_e = opaque_lane(lane);          // (why: see gemm_epilogue_wave)
      const int g = lane_e >> 4, li = lane_e & 15;
      constexpr int S = epi_row_floats<NI>(), HB = MI / 2;
      float* park = (float*)(smem + wave * epi_wave_bytes<NI, HB>());
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h) {
          __builtin_amdgcn_s_barrier();                    // the producers are done with the first half
          asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int i = 0; i < HB; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j) *(f32x4*)(park + (i * 16 + li) * S + j * 16 + 4 * g) = acc[h * HB + i][j];
        // The park crosses waves (the producers read it), and s_barrier on gfx950 waits for no counter: the LDS writes must
        // have retired before this wave arrives, and the compiler may not move them across the barrier either.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                      // parked
        asm volatile("" ::: "memory");
      }
      return;
    }
  }
  gemm_epilogue_wave<OT, MI, NI, (NIU >= 4)>(p, acc, z, m0 + wm * WTM, n0 + wn * WTN, smem + wave * epi_wave_bytes<NI, EPI_HB>(), lane);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Row-major A and B (the forward Linears with N >= 2304: QKV, FFN-up, cross-K/V, LM head), FULL-LINE staging (round 4).
// The 32-deep stages above fetch 64 bytes of every operand row per K-step: half of a 128-byte line, whose other half is fetched
// again one step later -- by then the 32 KB L1 has long turned over.  The LDS-DMA-only loop of such operands runs at 0.57 us per
// 32 KB against 0.46 us for k-major operands, whose rows are whole lines (round 2), and the producer / consumer K-step is
// producer bound.  Here an operand is filled 64 deep -- 128 bytes = one line per row and fill, 8 rows per wave instruction --
// and the fills ALTERNATE: an odd 32-deep step issues A(j) (K range [64j, 64j+64), used in steps 2j, 2j+1; slot j % 3), an even
// step B(j) (slot j % 2): still 32 KB of LDS-DMA per step, every byte of a fetched line used.  A(j) is issued in step 2j - 3 and
// B(j) in step 2j - 2, i.e. three resp. two steps ahead of their first use; a slot is refilled two resp. one barrier after its
// last read.  LDS: 3 x 32 KB + 2 x (32 | 24) KB.
//   image of a fill: row r at 128 r, 16-byte slot s of the row at slot s ^ ((r >> 1) & 7) -- conflict-free for the b128 lane
//   groups with the 16x16x32 fragment pattern (checked exhaustively); the swizzle is applied to the
//   per-lane SOURCE address, the LDS side of the DMA stays lane-linear.
// Requires K % 64 == 0 (every K of the step); other shapes take pc_tile256.
// Measured (round 4, tools/r04_nt64_check.sh): K-step slope 0.702 -> 0.630 us at 4096 x 3072, 0.552 -> 0.498 at 4096 x 2304 (vendor
// BLAS 0.495 / 0.399), fixed part +0.7 .. 1.0 us (three fills in front of the first MFMA); 4096x3072x768 30.4 -> 29.6 us.
// An L2 PREFETCH of the lines of fill j + 2 .. 6 (consumer waves 0 / 1 touching this workgroup's share of the rows it shares with
// the 8 resp. 4 workgroups of its XCD, one dword per line) changed nothing: slope 0.647 / 0.644 / 0.641 / 0.638 us for 0 / 2 / 4 / 6
// fills ahead -- the ring is not waiting on beyond-L2 latency (removed again, with its sweep script).
DEVFN int rm64_off(int row, int slot) { return row * 128 + ((slot ^ ((row >> 1) & 7)) << 4); }

template <int ROWS, int NP>            // NP = 1 KB pieces per producer wave and fill (ROWS / 32)
struct Dma64 {
  const char* ptr[NP];
  bool okx[NP];
  DEVFN void init(const char* g, int64_t ld, int64_t x0, int64_t X, int ptid) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int u = i * 256 + ptid, r = u >> 3, ls = (u & 7) ^ ((r >> 1) & 7);
      const int64_t x = x0 + r;
      okx[i] = x < X;
      ptr[i] = g + (x * ld + ls * 8) * 2;
    }
  }
  DEVFN void issue(int64_t j, int64_t J, char* img, int pw) const {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      glds16((okx[i] && j < J) ? ptr[i] + j * 128 : (const char*)g_zero_page, img + (i * 256 + pw * 64) * 16);
    }
  }
};

template <typename OT, int NIU>
DEVFN void pc_tile256_nt64(const GemmP& p, int64_t z, int wg, int ntn, int nwg, char* smem) {
  constexpr int BM = 256, WN = 4, WTM = 128, WTN = NIU * 16, MI = 8, NI = NIU, BNU = WN * WTN;
  constexpr int A_SLOT = BM * 128, B_SLOT = BNU * 128, B_BASE = 3 * A_SLOT;
  constexpr int NPA = BM / 32, NPB = BNU / 32;
  static_assert(NPA + NPB <= 63, "vmcnt immediate out of range");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int64_t m0, n0;
  tile_origin<BM, BNU, g_strip_w>(wg, ntn, nwg, m0, n0);
  const int64_t nkt = p.K / 32, J = p.K / 64;

  if (wave >= 8) {                     // ---- producers
    const int ptid = tid - 512, pw = wave - 8;
    Dma64<BM, NPA> ua;
    Dma64<BNU, NPB> ub;
    ua.init(p.A + z * p.sA * 2, p.lda, m0, p.M, ptid);
    ub.init(p.B + z * p.sB * 2, p.ldb, n0, p.N, ptid);
    ua.issue(0, J, smem, pw);
    ub.issue(0, J, smem + B_BASE, pw);
    ua.issue(1, J, smem + A_SLOT, pw);
    int sa = 2, sb = 1;                // slots of the next A / B fill
    int64_t ja = 2, jb = 1;
    for (int64_t t = 0; t < nkt; t += 2) {
      // even step t = 2j: A(j) and B(j) must have landed; the youngest fill in flight is A(j+1)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPA) : "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      ub.issue(jb, J, smem + B_BASE + sb * B_SLOT, pw);          // B(j+1): its slot held B(j-1), last read in step t - 1
      ++jb; sb ^= 1;
      // odd step: nothing new is needed (A(j), B(j) are in use); in flight: A(j+1), B(j+1)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPA + NPB) : "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      ua.issue(ja, J, smem + sa * A_SLOT, pw);                   // A(j+2): its slot held A(j-1), last read in step t - 1
      ++ja; sa = (sa + 1 == 3) ? 0 : sa + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the trailing (zero page) fills
    __builtin_amdgcn_s_barrier();                                 // pairs with the consumers' barrier in front of the epilogue
    return;
  }

  const int wm = wave / WN, wn = wave % WN;                        // ---- consumers
  f32x4 acc[MI][NI];
  zero_acc(acc);
  int sa = 0, sb = 0;
  const int g = lane >> 4, li = lane & 15;
  for (int64_t t = 0; t < nkt; t += 2) {
    const char* cA = smem + sa * A_SLOT;
    const char* cB = smem + B_BASE + sb * B_SLOT;
#pragma unroll
    for (int h = 0; h < 2; ++h) {          // the two 32-deep halves of the 64-deep images
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      mma_step<MI, NI, (NIU <= 3)>(acc, [&](int i) { return *(const bf16x8*)(cA + rm64_off(wm * WTM + i * 16 + li, h * 4 + g)); },
                                   [&](int j) { return *(const bf16x8*)(cB + rm64_off(wn * WTN + j * 16 + li, h * 4 + g)); });
    }
    sa = (sa + 1 == 3) ? 0 : sa + 1;
    sb ^= 1;
  }
  __builtin_amdgcn_s_barrier();        // every producer has drained its DMAs, every consumer is done with the ring: LDS is free
  gemm_epilogue_wave<OT, MI, NI, (NIU >= 4)>(p, acc, z, m0 + wm * WTM, n0 + wn * WTN, smem + wave * epi_wave_bytes<NI, EPI_HB>(), lane);
}

template <typename OT, bool AKM, bool BKM, int NIU = 4>
__global__ __launch_bounds__(512) void gemm_dma256_kernel(GemmP p, int ntn, int nwg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  dma_tile256<OT, AKM, BKM, NIU>(p, blockIdx.y, xcd_remap(blockIdx.x, nwg), ntn, nwg, smem);
}

template <typename OT, bool AKM, bool BKM, int NIU = 4>
__global__ __launch_bounds__(768) void gemm_pc256_kernel(GemmP p, int ntn, int nwg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  pc_tile256<OT, AKM, BKM, NIU>(p, blockIdx.y, xcd_remap(blockIdx.x, nwg), ntn, nwg, smem);
}

template <typename OT, int NIU>
__global__ __launch_bounds__(768) void gemm_pc256_nt64_kernel(GemmP p, int ntn, int nwg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  pc_tile256_nt64<OT, NIU>(p, blockIdx.y, xcd_remap(blockIdx.x, nwg), ntn, nwg, smem);
}

// Which tile of the table a workgroup of a grouped launch runs.
//   bmap != nullptr (the host's order, ops.GemmGroup: gstvd_gemm_grouped*'s `block_map_dev`): block b runs tile bmap[b], or
//     nothing when that is negative (padding of the shorter XCD queues).  Blocks are dealt to the XCDs round-robin (observed, speed
//     only), so entries b = x, x + 8, x + 16, ... are XCD x's queue: the host puts whole problems -- tiles that share operand
//     panels and run for the same time -- back to back into ONE queue, so that the ~32 tiles an XCD runs at a time stream the
//     same few panels through its L2 in step.
//   bmap == nullptr: XCD x walks chunks x, x+8, x+16, ... of 2^chs consecutive tiles (rounds 1-4).
// A map entry's tile id is its bits 0-20; the bits above are ignored (reserved).  (Round 5 tried a START BARRIER in them -- position of
// the tile in its unit and the unit's size, the workgroups of a unit waiting for each other before their K loops: 7.5 % fewer operand
// fetches, 2.3 % slower, and the call cost the fused kernel 256 B/lane of scratch; removed, profiles/r05_group_sync_ab.txt.)
// A tile id >= total names no tile of the table: the host checks the map it builds, the kernels skip such an entry so that a bad
// map cannot write.
constexpr int GROUP_TILE_MASK = 0x1fffff;
DEVFN int grouped_tile_id(const int* bmap, int total, int chs) {
  const int bid = blockIdx.x;
  if (bmap) return bmap[bid];
  const int full = total - total % (8 << chs);
  return bid < full ? (((bid >> 3) >> chs) * 8 + (bid & 7)) * (1 << chs) + ((bid >> 3) & ((1 << chs) - 1)) : bid;
}

// The grouped kernels' prologue.  False: this workgroup's entry names no tile of the table.  Otherwise the problem's GemmP, the
// tile's index inside the problem and the problem's tile grid (ntn columns, nwg tiles).
DEVFN bool grouped_tile(const gstvd_gemm_t* tab, const int* tile_off, int nprob, int total, int chs, const int* bmap, GemmP& p, int& tile,
                        int& ntn, int& nwg) {
  const int entry = grouped_tile_id(bmap, total, chs), gid = entry & GROUP_TILE_MASK;
  if (entry < 0 || gid >= total) return false;
  int lo = 0, hi = nprob - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tile_off[mid] <= gid) lo = mid; else hi = mid - 1; }
  p = gemm_p_from(tab[lo]);
  p.sA = p.sB = p.sC = p.sAdd = p.sAux = 0;
  ntn = (int)((p.N + 255) / 256);
  nwg = (int)((p.M + 255) / 256) * ntn;
  tile = gid - tile_off[lo];
  return true;
}

template <typename OT, bool AKM, bool BKM>
__global__ __launch_bounds__(768) void gemm_pc256_grouped_kernel(const gstvd_gemm_t* tab, const int* tile_off, int nprob, int total, int chs,
                                                                 const int* bmap) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  GemmP p;
  int tile, ntn, nwg;
  if (!grouped_tile(tab, tile_off, nprob, total, chs, bmap, p, tile, ntn, nwg)) return;
  pc_tile256<OT, AKM, BKM, 4, true>(p, 0, tile, ntn, nwg, smem);
}

__global__ __launch_bounds__(768) void gemm_pc256_grouped_adamw_kernel(const gstvd_gemm_t* tab, const int* tile_off, int nprob, int total, int chs,
                                                                       const int* bmap, gstvd_adamw_fuse_t af) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  GemmP p;
  int tile, ntn, nwg;
  if (!grouped_tile(tab, tile_off, nprob, total, chs, bmap, p, tile, ntn, nwg)) return;
  pc_tile256<float, true, true, 4, true, true>(p, 0, tile, ntn, nwg, smem, af);
}

constexpr int RING256 = NS256 * (256 + 256) * 64;
constexpr int PARK256 = 8 * epi_wave_bytes<4, 4>();        // eight waves park 4 x 4 accumulator tiles each (row-wise epilogue)
constexpr int LDS256 = RING256 > PARK256 ? RING256 : PARK256;
// Producer / consumer form up to this many tiles per launch: measured -7 % per launch on single-round grids (4096x3072x768 33.8
// -> 31.3 us, per K-step 0.82 -> 0.76 us), +7 % on the 1368-tile cross-K/V projection (its extra ~1.5 us of fixed cost is paid
// 5.3 times): up to 2 rounds of tiles.  Larger grids take the 8-wave dma_tile256.
constexpr int64_t PC256_MAX_TILES = 512;
// Single-problem policy: the big tile only pays when its (4x smaller) grid still covers most of the chip.
constexpr int64_t GEMM256_MIN_TILES = 120;
// Tiles per XCD chunk of a grouped launch without a block map = 2^GROUP_CHUNK_LOG2 (8: measured best of 1..128 inside the step).
constexpr int GROUP_CHUNK_LOG2 = 3;

// The (NIU = 4, NIU = 3) instantiations of one kernel: both get their LDS size once, `narrow` (192-wide tiles) picks K3.
using Kern256 = void (*)(GemmP, int, int);
template <Kern256 K4, Kern256 K3, int THREADS, int LDS4, int LDS3 = LDS4>
static int launch_pair256(bool narrow, const dim3& grid, const GemmP& p, int ntn, hipStream_t s) {
  static int attr_rc = ensure_lds(K4, LDS4) | ensure_lds(K3, LDS3);
  if (attr_rc) return attr_rc;
  GSTVD_LAUNCH(narrow ? K3 : K4, grid, dim3(THREADS), narrow ? LDS3 : LDS4, s, p, ntn, (int)grid.x);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

template <typename OT, bool AKM, bool BKM>
static int launch256(const GemmP& p, int64_t batch, int niu, hipStream_t s) {
  const int bnu = niu == 3 ? 192 : 256;
  const int ntm = (int)((p.M + 255) / 256), ntn = (int)((p.N + bnu - 1) / bnu);
  const dim3 grid((unsigned)(ntm * ntn), (unsigned)batch);
  if ((int64_t)ntm * ntn * batch > PC256_MAX_TILES)
    return launch_pair256<gemm_dma256_kernel<OT, AKM, BKM, 4>, gemm_dma256_kernel<OT, AKM, BKM, 3>, 512, LDS256>(niu == 3, grid, p, ntn, s);
  if constexpr (!AKM && !BKM) {
    // full-line (64-deep, alternating) staging of two row-major operands
    if (p.K % 64 == 0 && p.K >= 128) {
      constexpr int L4 = 3 * 256 * 128 + 2 * 256 * 128, L3 = 3 * 256 * 128 + 2 * 192 * 128;
      constexpr int P4 = 8 * epi_wave_bytes<4, 4>(), P3 = 8 * epi_wave_bytes<3, 4>();
      constexpr int lds4 = L4 > P4 ? L4 : P4, lds3 = L3 > P3 ? L3 : P3;
      static_assert(lds4 <= 160 * 1024 && lds3 <= 160 * 1024, "LDS budget");
      return launch_pair256<gemm_pc256_nt64_kernel<OT, 4>, gemm_pc256_nt64_kernel<OT, 3>, 768, lds4, lds3>(niu == 3, grid, p, ntn, s);
    }
  }
  return launch_pair256<gemm_pc256_kernel<OT, AKM, BKM, 4>, gemm_pc256_kernel<OT, AKM, BKM, 3>, 768, LDS256>(niu == 3, grid, p, ntn, s);
}

// Tile width: 256 columns, or 192 when that needs fewer rounds of 256 CUs for the work it does.  Cost model from the
// measured kernel: ~14 us fixed + 0.95 us per 32-deep K step for the full tile, ~0.9x that per step for the 192 one.
static int pick_niu(const GemmP& p, int64_t batch) {
  const double nkt = (double)((p.K + 31) / 32), ntm = (double)((p.M + 255) / 256);
  const double t4 = ntm * (double)((p.N + 255) / 256) * batch, t3 = ntm * (double)((p.N + 191) / 192) * batch;
  const double r4 = (double)(int64_t)((t4 + 255) / 256), r3 = (double)(int64_t)((t3 + 255) / 256);
  return r3 * (14.0 + 0.84 * nkt) < r4 * (14.0 + 0.95 * nkt) ? 3 : 4;     // measured 0.73 vs 0.82 us per step at K = 768
}

int gemm_dma256_dispatch(const GemmP& p, int64_t batch, int akm, int bkm, int out_f32, hipStream_t s) {
  const int64_t tiles = ((p.M + 255) / 256) * ((p.N + 255) / 256) * batch;
  if (p.M < 256 || p.N < 256 || tiles < GEMM256_MIN_TILES) return GSTVD_E_UNSUPPORTED;
  const int niu = pick_niu(p, batch);
  return by_out_layout<NO_TT>(out_f32, akm, bkm, [&](auto t, auto a, auto b) {      // k-major A with row-major B: gemm_dma.hip
    return launch256<typename decltype(t)::type, a.value, b.value>(p, batch, niu, s);
  });
}

// Weight gradients are long-K problems (K = rows of the batch): the producer / consumer tile gains ~0.08 us on every one of
// their ~128 K-steps (18432x768x4688: 160 -> 143 us).
template <typename OT, bool AKM, bool BKM>
static int grouped256(const gstvd_gemm_t* tab, const int* off, int nprob, int total, const int* bmap, int nblocks, hipStream_t s) {
  auto kp = gemm_pc256_grouped_kernel<OT, AKM, BKM>;
  static int pc_rc = ensure_lds(kp, LDS256);
  if (pc_rc) return pc_rc;
  GSTVD_LAUNCH(kp, dim3((unsigned)(bmap ? nblocks : total)), dim3(768), LDS256, s, tab, off, nprob, total, GROUP_CHUNK_LOG2, bmap);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_gemm_group_tile(void) { return 256; }

extern "C" int32_t gstvd_gemm_group_caps(void) { return 1; }

// symbol of the grouped kernel for a (dtype, layout) combination -- same plan-only mechanism as gstvd_gemm_kernel_name
extern "C" int gstvd_gemm_grouped_kernel_name(int32_t dtype_in, int32_t dtype_out, int32_t a_kmajor, int32_t b_kmajor, char* buf,
                                              int32_t buf_len) {
  if (!buf || buf_len <= 1) return GSTVD_E_NULL;
  const void* fn = nullptr;
  static gstvd_gemm_t dummy_tab;
  static int32_t dummy_off;
  gstvd_plan_capture = &fn;
  const int rc = gstvd_gemm_grouped(&dummy_tab, &dummy_off, 1, 1, dtype_in, dtype_out, a_kmajor, b_kmajor, nullptr, 0, nullptr);
  gstvd_plan_capture = nullptr;
  if (rc) return rc;
  return copy_kernel_name(fn, buf, buf_len);
}

extern "C" int gstvd_gemm_grouped_adamw_kernel_name(char* buf, int32_t buf_len) {
  if (!buf || buf_len <= 1) return GSTVD_E_NULL;
  return copy_kernel_name((const void*)gemm_pc256_grouped_adamw_kernel, buf, buf_len);
}

// argument checks shared by the two grouped entry points
static int grouped_check(const gstvd_gemm_t* table_dev, const int32_t* tile_off_dev, int64_t nprob, int64_t total_tiles,
                         const int32_t* block_map_dev, int64_t nblocks) {
  if (!table_dev || !tile_off_dev) return GSTVD_E_NULL;
  if (nprob <= 0 || total_tiles <= 0) return GSTVD_E_SHAPE;
  if (block_map_dev && (nblocks < total_tiles || total_tiles > GROUP_TILE_MASK)) return GSTVD_E_SHAPE;     // a map that cannot name every tile
  return 0;
}

extern "C" int gstvd_gemm_grouped_adamw(const gstvd_gemm_t* table_dev, const int32_t* tile_off_dev, int64_t nprob, int64_t total_tiles,
                                        const gstvd_adamw_fuse_t* f, const int32_t* block_map_dev, int64_t nblocks, gstvd_stream_t stream) {
  if (!f || !f->grad_base || !f->param || !f->m || !f->v || !f->step) return GSTVD_E_NULL;
  if (const int crc = grouped_check(table_dev, tile_off_dev, nprob, total_tiles, block_map_dev, nblocks)) return crc;
  if (((uintptr_t)f->grad_base | (uintptr_t)f->param | (uintptr_t)f->m | (uintptr_t)f->v | (uintptr_t)f->shadow_bf16) & 15) return GSTVD_E_ALIGN;
  auto kp = gemm_pc256_grouped_adamw_kernel;
  static int rc = ensure_lds(kp, LDS256);
  if (rc) return rc;
  GSTVD_LAUNCH(kp, dim3((unsigned)(block_map_dev ? nblocks : total_tiles)), dim3(768), LDS256, (hipStream_t)stream, table_dev, tile_off_dev,
               (int)nprob, (int)total_tiles, GROUP_CHUNK_LOG2, block_map_dev, *f);
  GSTVD_LAUNCH_CHECK();
  return 0;
}

extern "C" int gstvd_gemm_grouped(const gstvd_gemm_t* table_dev, const int32_t* tile_off_dev, int64_t nprob, int64_t total_tiles,
                                  int32_t dtype_in, int32_t dtype_out, int32_t a_kmajor, int32_t b_kmajor,
                                  const int32_t* block_map_dev, int64_t nblocks, gstvd_stream_t stream) {
  if (const int crc = grouped_check(table_dev, tile_off_dev, nprob, total_tiles, block_map_dev, nblocks)) return crc;
  if (dtype_in != GSTVD_BF16 || (dtype_out != GSTVD_F32 && dtype_out != GSTVD_BF16)) return GSTVD_E_UNSUPPORTED;
  return by_out_layout<NO_TT>(dtype_out == GSTVD_F32, a_kmajor, b_kmajor, [&](auto t, auto a, auto b) {      // the 256 tile's layouts
    return grouped256<typename decltype(t)::type, a.value, b.value>(table_dev, tile_off_dev, (int)nprob, (int)total_tiles, block_map_dev,
                                                                   (int)nblocks, (hipStream_t)stream);
  });
}
