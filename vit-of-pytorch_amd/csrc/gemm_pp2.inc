// Included by gemm.hip (inside its anonymous namespace): the half-tile scheduled ping-pong kernel.
//
// Same 256 x 256 x 64 tile and two alternating wave groups as gemm_pp_kernel, but every LDS-DMA is
// issued by the group that is in its LDS-read slot, never by the group about to multiply: measured
// with s_memtime stamps (tools/gemm_diag.hip), the 8 buffer_load...lds per wave issued at the start
// of a multiply slot cost ~500 cycles of issue and delayed that slot's MFMAs. Operand tiles are kept
// as 128-row half images so that buffers free up at half granularity: group g reads A half g and
// both B halves of k-tile t in slot 2t+g. LDS (160 KiB): A0 x2, A1 x2 (16 KiB each), B x3 (32 KiB).
//   slot 2j   (group 0 reads k-tile j):  group 0 issues A1(j+1) and B half 0 of k-tile j+2
//   slot 2j+1 (group 1 reads k-tile j):  group 1 issues A0(j+2) and B half 1 of k-tile j+2
// Every DMA has >= 2 slots of flight; each group waits at the end of its read slot (counted vmcnt)
// for the DMAs it issued two slots earlier, then joins the barrier that lets their readers in.
// Generalised ring (diagnostic configs): NA buffers per A half and NB = NA + 1 B buffers; in slot 2j group 0
// issues A1(j + NA - 1) and B half 0 of k-tile j + NB - 1, in slot 2j + 1 group 1 issues A0(j + NA) and B half 1
// of k-tile j + NB - 1, and each group leaves the DMAs of its last NA - 1 read slots in flight at its wait
// (NA = 2, NB = 3: the schedule above).
// one 256 x 256 output tile (tile row tm, column tn, batch z, K-split split_idx) of the GEMM p by the calling
// 512-thread workgroup; `orig` is its launch index (diagnostics only)
template <bool AK, bool BKC, int EPI, int BK = 64, int NA = 2>
__device__ __forceinline__ void pp2_tile(const GemmDev& p, const int tm, const int tn, const int z,
                                         const int split_idx, const int orig) {
  constexpr int BM = 256, BN = 256, KK = BK / 32;
  constexpr int NB = NA + 1;
  constexpr int TN = BN / 4, FM = 8, FN = TN / 16;
  constexpr int HALF = 128 * BK * 2;  // one half image (16 KiB at BK = 64)
  constexpr int A0_OFF = 0, A1_OFF = NA * HALF, B_OFF = 2 * NA * HALF;
  constexpr int LDS = (2 * NA + 2 * NB) * HALF;  // 160 KiB at BK = 64, NA = 2
  constexpr int I = BK / 16;                     // DMA instructions per wave per half image
  constexpr int LDW = TN + 4;
  constexpr int PR = 32;
  constexpr int WST = PR * LDW * 4;
  static_assert(8 * WST <= LDS && LDS <= 160 * 1024, "LDS budget / epilogue staging");
  static_assert(2 * I * (NA - 1) <= 32 && (2 * NA - 1) * I <= 62 && 2 * (NB - 1) * I <= 62, "vmcnt range");
  __shared__ __attribute__((aligned(16))) char smem[LDS];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wave >> 2, wn = wave & 3;
  const int m0 = tm * BM, n0 = tn * BN;
  if (p.diag >= 100 && ((orig >> 3) & 1) && (orig >> 3) < 32) {
    // diagnostic (VIT_GEMM_DIAG = 100 + us): delay every other first-wave workgroup of each XCD,
    // so the CUs of one XCD reach their epilogue stores out of phase
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)(p.diag - 100) * 100ull)
      __builtin_amdgcn_s_sleep(8);
  }

  const char* Ab = p.A + (long)z * p.a_bs * 2;
  const char* Bb = p.B + (long)z * p.b_bs * 2;
  const long a_shift = AK ? (long)m0 * p.lda * 2 : (long)m0 * 2;
  const long b_shift = BKC ? (long)n0 * p.ldb * 2 : (long)n0 * 2;
  const uint32_t a_rec = (long)p.a_bytes > a_shift ? (uint32_t)(p.a_bytes - a_shift) : 0u;
  const uint32_t b_rec = (long)p.b_bytes > b_shift ? (uint32_t)(p.b_bytes - b_shift) : 0u;
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(Ab + a_shift, a_rec);
  const __amdgpu_buffer_rsrc_t rsB = make_rsrc(Bb + b_shift, b_rec);
  // byte offset of row / column 128 of the tile in the global operand (the second half image)
  const int a_h1 = AK ? (int)(128 * p.lda * 2) : 256;
  const int b_h1 = BKC ? (int)(128 * p.ldb * 2) : 256;

  const int nkt = p.K / BK;
  const int kt0 = (int)((long)nkt * split_idx / p.split_k);
  const int kt1 = (int)((long)nkt * (split_idx + 1) / p.split_k);
  const int nk = kt1 - kt0;

  v4f acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
  v8s af[KK][FM], bfr[KK][FN];
  const int w4 = wave & 3;
#ifdef VIT_PP2_STAMPS
  // diagnostic build, VIT_GEMM_DIAG = 4: s_memtime at 8 points of k-tile nk / 2's read slot and multiply slot, waves 0
  // and 4 of the launch-index-0 workgroup, kept in SGPRs and written out after the loop
  const bool stw = p.diag == 4 && p.stamps && orig == 0 && split_idx == 0 && z == 0 && w4 == 0;
  unsigned long long stv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define PP2_ST(k)                                          \
  do {                                                     \
    if (stw && j == nk / 2) {                              \
      __builtin_amdgcn_sched_barrier(0);                   \
      stv[k] = __builtin_amdgcn_s_memtime();               \
      __builtin_amdgcn_sched_barrier(0);                   \
    }                                                      \
  } while (0)
#else
#define PP2_ST(k) \
  do {            \
  } while (0)
#endif

  // one 16 KiB half image = 4 DMA instructions per wave of the issuing group
  auto ld_a = [&](int h, int t) {
    stage_tile<128, BK, AK, 4>(smem, (h ? A1_OFF : A0_OFF) + (t % NA) * HALF, rsA, p.lda, kt0 + t, w4, lane,
                               h ? a_h1 : 0);
  };
  auto ld_b = [&](int h, int t) {
    stage_tile<128, BK, BKC, 4>(smem, B_OFF + (t % NB) * 2 * HALF + h * HALF, rsB, p.ldb, kt0 + t, w4, lane,
                                h ? b_h1 : 0);
  };
  // M/N-contiguous operands: transposed fragment reads by inline asm (read_frag_tr_asm), so hipcc's waitcnt pass
  // does not put a vmcnt(0) in front of them for the LDS-DMA in flight into the other buffers (the round-3 finding
  // of gemm_pp_kernel); per-lane offsets within a half image, the buffer base added as a wave-uniform value
  uint32_t a_lane[AK ? 1 : FM], b_lane[BKC ? 1 : FN];
  if constexpr (!AK) {
#pragma unroll
    for (int i = 0; i < FM; ++i) a_lane[i] = frag_tr_lane_off<128>(i * 16, lane);
  }
  if constexpr (!BKC) {
#pragma unroll
    for (int jn = 0; jn < FN; ++jn) b_lane[jn] = frag_tr_lane_off<128>((wn & 1) * 64 + jn * 16, lane);
  }
  const uint32_t s0 = (uint32_t)(uintptr_t)LDS_PTR(char, smem);
  // fragment reads of k-tile t; the caller issues its DMA behind them and then waits lgkmcnt(0)
  auto mem = [&](int t) {
    const int aoff = (grp ? A1_OFF : A0_OFF) + (t % NA) * HALF;
    const int boff = B_OFF + (t % NB) * 2 * HALF + (wn >> 1) * HALF;
    const uint32_t ab = __builtin_amdgcn_readfirstlane(s0 + aoff), bb = __builtin_amdgcn_readfirstlane(s0 + boff);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
      for (int jn = 0; jn < FN; ++jn) {
        if constexpr (BKC)
          bfr[kk][jn] = read_frag<128, BK, BKC>(smem, boff, (wn & 1) * 64 + jn * 16, kk, lane);
        else
          bfr[kk][jn] = kk == 0 ? read_frag_tr_asm<128, 0>(b_lane[jn] + bb) : read_frag_tr_asm<128, 1>(b_lane[jn] + bb);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        if constexpr (AK)
          af[kk][i] = read_frag<128, BK, AK>(smem, aoff, i * 16, kk, lane);
        else
          af[kk][i] = kk == 0 ? read_frag_tr_asm<128, 0>(a_lane[i] + ab) : read_frag_tr_asm<128, 1>(a_lane[i] + ab);
      }
    }
  };
  // Interleaved read slot (both operands M/N-contiguous: the split-K weight gradients): one stream, the slot's 2 I DMA
  // pieces (the A half first, then the B half) one after every (KK (FN + FM)) / (2 I) fragments instead of all behind
  // the reads. Stamps (profiles/r06/gemm_pp2_stamps*.txt): the weight gradient's read slot (48 transposed 8-B reads +
  // 8 pieces, ≈1 450 cycles) is longer than the partner's 64 MFMAs (≈1 130), and the interleaved order shortens the
  // partner's wait at the slot barrier (540 -> 420 cycles); 2-6% per weight-gradient GEMM, bit-identical
  // (gemm_ilv_ab.txt). The K-contiguous slots (24 16-B reads, balanced against the MFMAs) keep reads-then-DMA.
  // Diagnostic builds: VIT_GEMM_ILV = 0 / 1 forces it off / on for every layout.
#ifdef VIT_DIAG_KNOBS
  const bool ilv = p.ilv < 0 ? (!AK && !BKC) : p.ilv > 0;
#else
  constexpr bool ilv = !AK && !BKC;
#endif
  auto frag = [&](int t, int f) {
    constexpr int NF = FN + FM;
    const int kk = f / NF, r = f % NF;
    const int aoff = (grp ? A1_OFF : A0_OFF) + (t % NA) * HALF;
    const int boff = B_OFF + (t % NB) * 2 * HALF + (wn >> 1) * HALF;
    const uint32_t ab = __builtin_amdgcn_readfirstlane(s0 + aoff), bb = __builtin_amdgcn_readfirstlane(s0 + boff);
    if (r < FN) {
      if constexpr (BKC)
        bfr[kk][r] = read_frag<128, BK, BKC>(smem, boff, (wn & 1) * 64 + r * 16, kk, lane);
      else
        bfr[kk][r] = kk == 0 ? read_frag_tr_asm<128, 0>(b_lane[r] + bb) : read_frag_tr_asm<128, 1>(b_lane[r] + bb);
    } else {
      const int i = r - FN;
      if constexpr (AK)
        af[kk][i] = read_frag<128, BK, AK>(smem, aoff, i * 16, kk, lane);
      else
        af[kk][i] = kk == 0 ? read_frag_tr_asm<128, 0>(a_lane[i] + ab) : read_frag_tr_asm<128, 1>(a_lane[i] + ab);
    }
  };
  auto piece = [&](int q, int j, bool g1) {
    __builtin_amdgcn_sched_barrier(0);
    if (q < I) {  // group 0: A1(j + NA - 1); group 1: A0(j + NA)
      const int t = g1 ? j + NA : j + NA - 1;
      if (t < nk)
        stage_piece<128, BK, AK, 4>(smem, (g1 ? A0_OFF : A1_OFF) + (t % NA) * HALF, rsA, p.lda, kt0 + t, w4, lane,
                                    g1 ? 0 : a_h1, q);
    } else {  // B half (g1) of k-tile j + NB - 1
      const int t = j + NB - 1;
      if (t < nk)
        stage_piece<128, BK, BKC, 4>(smem, B_OFF + (t % NB) * 2 * HALF + (g1 ? HALF : 0), rsB, p.ldb, kt0 + t, w4,
                                     lane, g1 ? b_h1 : 0, q - I);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto slot_ilv = [&](int j, bool g1) {
    constexpr int NFR = KK * (FN + FM), NP = 2 * I, PER = NFR / NP;
    static_assert(PER * NP == NFR, "whole fragments between pieces");
#pragma unroll
    for (int f = 0; f < NFR; ++f) {
      frag(j, f);
      if (f % PER == PER - 1) piece(f / PER, j, g1);
    }
  };
  auto reads_done = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  auto compute = [&]() {
    if (p.prio == 1) __builtin_amdgcn_s_setprio(1);  // the MFMA cluster ahead of the partner group's issue
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int jn = 0; jn < FN; ++jn)
          acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, af[kk][i]),
                                                               __builtin_bit_cast(v8bf, bfr[kk][jn]), acc[i][jn], 0, 0, 0);
    if (p.prio == 1) __builtin_amdgcn_s_setprio(0);
  };
  // prio 2 (diagnostic): the reading group's fragment reads and DMA issue ahead of the partner's MFMAs instead
  auto read_prio = [&](bool hi) {
    if (p.prio == 2) {
      if (hi) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
  };
  auto barrier = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  // wait until at most `younger` (a multiple of I, <= 2 I (NA - 1)) of this wave's DMAs are still outstanding
  auto wait_younger = [&](int younger) {
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NA == 2 && I == 4) {
      if (younger >= 8)
        wait_vm<8>();
      else if (younger >= 4)
        wait_vm<4>();
      else
        wait_vm<0>();
    } else {
      switch (younger / I) {
        case 0: wait_vm<0>(); break;
        case 1: wait_vm<I>(); break;
        case 2: wait_vm<2 * I>(); break;
        case 3: wait_vm<3 * I>(); break;
        case 4: wait_vm<4 * I>(); break;
        case 5: wait_vm<5 * I>(); break;
        case 6: wait_vm<6 * I>(); break;
        case 7: wait_vm<7 * I>(); break;
        default: wait_vm<8 * I>(); break;
      }
    }
  };
  // DMA instructions group 0 / group 1 issue in their read slot of k-tile j (0 outside [0, nk))
  auto dma0 = [&](int j) { return j < 0 ? 0 : I * ((j + NA - 1 < nk) + (j + NB - 1 < nk)); };
  auto dma1 = [&](int j) { return j < 0 ? 0 : I * ((j + NA < nk) + (j + NB - 1 < nk)); };
  auto in_flight = [&](int j, bool g1) {  // the DMAs of read slots j - NA + 2 .. j may stay outstanding
    int n = 0;
#pragma unroll
    for (int d = 0; d < NA - 1; ++d) n += g1 ? dma1(j - d) : dma0(j - d);
    return n;
  };

  // prologue: group 0 every A0 k-tile up to NA - 1 and A1 up to NA - 2, group 1 both B halves up to NB - 2
  // (NA = 2: k-tile 0 whole, A0 and B of k-tile 1)
  if (grp == 0) {
#pragma unroll
    for (int t = 0; t < NA; ++t)
      if (t < nk) ld_a(0, t);
#pragma unroll
    for (int t = 0; t < NA - 1; ++t)
      if (t < nk) ld_a(1, t);
  } else {
#pragma unroll
    for (int t = 0; t < NB - 1; ++t)
      if (t < nk) {
        ld_b(0, t);
        ld_b(1, t);
      }
  }
  wait_vm<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // 2nk barriers per group; group 1's multiply of the last k-tile (slot 2nk) is followed by none.
  // In its read slot a group issues its fragment reads first and its DMA half behind them (the buffers
  // it refills were last read before the barrier that opened the slot): issued ahead of the reads, the
  // 8 DMA instructions per wave held the reads back (the weight-gradient kernel's measurement,
  // profiles/r03/wgrad_slots_summary.txt).
  if (grp == 0) {
    for (int j = 0; j < nk; ++j) {
      // slot 2j: read k-tile j, issue A1(j + NA - 1) and B half 0 of k-tile j + NB - 1
      PP2_ST(0);
      read_prio(true);
      if (ilv) {
        slot_ilv(j, false);
        PP2_ST(1);
      } else {
        mem(j);
        PP2_ST(1);
        if (j + NA - 1 < nk) ld_a(1, j + NA - 1);
        if (j + NB - 1 < nk) ld_b(0, j + NB - 1);
      }
      read_prio(false);
      PP2_ST(2);
      reads_done();
      PP2_ST(3);
      wait_younger(in_flight(j, false));
      PP2_ST(4);
      barrier();
      PP2_ST(5);
      compute();  // slot 2j+1
      PP2_ST(6);
      barrier();
      PP2_ST(7);
    }
  } else if (nk > 0) {
    barrier();  // slot 0
    for (int j = 0; j < nk; ++j) {
      // slot 2j+1: read k-tile j, issue A0(j + NA) and B half 1 of k-tile j + NB - 1
      PP2_ST(0);
      read_prio(true);
      if (ilv) {
        slot_ilv(j, true);
        PP2_ST(1);
      } else {
        mem(j);
        PP2_ST(1);
        if (j + NA < nk) ld_a(0, j + NA);
        if (j + NB - 1 < nk) ld_b(1, j + NB - 1);
      }
      read_prio(false);
      PP2_ST(2);
      reads_done();
      PP2_ST(3);
      wait_younger(in_flight(j, true));
      PP2_ST(4);
      barrier();
      PP2_ST(5);
      compute();  // slot 2j+2
      PP2_ST(6);
      if (j + 1 < nk) barrier();
      PP2_ST(7);
    }
  }
#ifdef VIT_PP2_STAMPS
  if (stw && lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) p.stamps[grp * 8 + k] = stv[k];
  }
#endif
#undef PP2_ST

  // ---- epilogue (as gemm_pp_kernel): wave-private staging, 32 rows per pass. Group 0 starts while
  // group 1 multiplies its last k-tile from registers; no DMA is outstanding (every group drained
  // its vmcnt in its last read slots) and no LDS read is pending.
  if (p.diag == 2) {  // diagnostic: mainloop only (keep the accumulators alive)
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int jn = 0; jn < FN; ++jn) t += acc[i][jn][0] + acc[i][jn][1] + acc[i][jn][2] + acc[i][jn][3];
    if (t == 1234.5f) ((float*)p.C)[threadIdx.x] = t;
    return;
  }
  const int wm0 = grp * 128, wn0 = wn * TN;
  const int g = lane >> 4, c = lane & 15;
  float* ws = reinterpret_cast<float*>(smem + wave * WST);
  constexpr int CPR = TN / 8;
  float csum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  constexpr int IT = PR * CPR / 64;  // 8-column chunks per lane and pass
  static_assert(IT * 64 == PR * CPR, "whole chunks per pass");
  // (the accumulating table launch prefetches its old destination values on the whole-tile path only; on this
  // generic path, the edge tiles and unaligned destinations, epi_store8 reads them at store time: the 16 words of
  // prefetch registers per lane beside the live accumulators would spill)
  constexpr int GW = (EPI & EPI_ACC) ? 0 : AuxPre<EPI>::W;
  constexpr int AW = GW > 0 ? GW : 1;
  uint4 axc[IT][AW], axn[IT][AW];  // aux chunks of this pass / the next one
  auto fetch_pass = [&](uint4 (*ax)[AW], int pass) {
    if constexpr (GW > 0) {
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int e = lane + it * 64, row = e / CPR, ch = e % CPR;
        const int m = m0 + wm0 + pass * PR + row, n = n0 + wn0 + ch * 8;
        if (p.vec && m < p.M && n + 8 <= p.N) AuxPre<EPI>::fetch(p, m, n, ax[it], z);
      }
    }
  };
  if (EpiOut<EPI>::FAST && p.vec && p.diag == 0 && m0 + BM <= p.M && n0 + BN <= p.N) {
    epilogue_fast<EPI, FN, LDW, CPR>(p, acc, ws, lane, m0 + wm0, n0 + wn0, z, split_idx, csum);
  } else {
  fetch_pass(axc, 0);
#pragma unroll
  for (int pass = 0; pass < 128 / PR; ++pass) {
    if (pass + 1 < 128 / PR) fetch_pass(axn, pass + 1);
#pragma unroll
    for (int i = 0; i < PR / 16; ++i)
#pragma unroll
      for (int jn = 0; jn < FN; ++jn)
#pragma unroll
        for (int r = 0; r < 4; ++r) ws[(i * 16 + 4 * g + r) * LDW + jn * 16 + c] = acc[pass * (PR / 16) + i][jn][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int e = lane + it * 64, row = e / CPR, ch = e % CPR;
      const int m = m0 + wm0 + pass * PR + row, n = n0 + wn0 + ch * 8;
      float v[8];
      ld8f(ws + row * LDW + ch * 8, v);
      if (m >= p.M || n >= p.N || p.diag == 1 || (p.diag == 3 && (blockIdx.x & 1))) continue;
      if constexpr ((EPI & EPI_PATH) != 0) {  // stochastic depth (GW > 0: a BIAS_RESID_F32 variant): one multiplier
        const float ps = path_mult(p, m);      // load per row chunk, for either store path
        if (p.vec && n + 8 <= p.N) {
          float u[8];
          AuxPre<EPI>::unpack(axc[it], u);
          epi_store8<EPI>(p, z, split_idx, m, n, v, u, ps);
          if (p.col_partial) {
#pragma unroll
            for (int k = 0; k < 8; ++k) csum[k] += v[k];
          }
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) epi_store<EPI>(p, z, split_idx, m, n + k, v[k], ps);
        }
      } else
      if (p.vec && n + 8 <= p.N) {
        if constexpr (GW > 0) {
          float u[8];
          AuxPre<EPI>::unpack(axc[it], u);
          epi_store8<EPI>(p, z, split_idx, m, n, v, u);
        } else {
          epi_store8<EPI>(p, z, split_idx, m, n, v);
        }
        if (p.col_partial) {
#pragma unroll
          for (int k = 0; k < 8; ++k) csum[k] += v[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) epi_store<EPI>(p, z, split_idx, m, n + k, v[k]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if constexpr (GW > 0) {
#pragma unroll
      for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int w = 0; w < AW; ++w) axc[it][w] = axn[it][w];
    }
  }
  }
  if (p.col_partial) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int o = CPR; o < 64; o <<= 1) csum[k] += __shfl_xor(csum[k], o, 64);
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
    if (lane < CPR) {
#pragma unroll
      for (int k = 0; k < 8; ++k) red[grp * BN + wn0 + lane * 8 + k] = csum[k];
    }
    __syncthreads();
    for (int col = threadIdx.x; col < BN; col += 512)
      if (n0 + col < p.N) p.col_partial[(long)tm * p.N + n0 + col] = red[col] + red[BN + col];
  }
}

// (tile, split, batch) of split-K workgroup w of a GEMM with nwg tiles (tile fastest)
__device__ __forceinline__ void splitk_coords(const GemmDev& p, int w, int nwg, int tiles_m, int tiles_n, int& tm, int& tn,
                                              int& z, int& split_idx) {
  const int zs = w / nwg;
  z = zs / p.split_k;
  split_idx = zs % p.split_k;
  tile_coords(w % nwg, tiles_m, tiles_n, p.group_m, tm, tn);
}

// XCD-major position of launch index `lin` in a space of `total` workgroups (bijective): the dispatcher deals
// consecutive launch indices to the 8 XCDs in turn; each XCD gets a contiguous run of positions
__device__ __forceinline__ int xcd_major(int lin, int total) {
  const int xcd = lin & 7, q8 = total >> 3, r8 = total & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (lin >> 3);
}

template <bool AK, bool BKC, int EPI, int BK = 64, int NA = 2>
__global__ void __launch_bounds__(512) gemm_pp2_kernel(const GemmDev p) {
  const int tiles_m = (p.M + 255) / 256, tiles_n = (p.N + 255) / 256;
  const int nwg = tiles_m * tiles_n;
  const int orig = blockIdx.x;
  int tm, tn, z, split_idx;
  if (p.split_k > 1 && p.split_xcd) {
    // split-K (weight gradients): the (tile, split, batch) space XCD-major, as gemm_pp_kernel
    const int total = nwg * p.split_k * (int)gridDim.z;
    const int lin = blockIdx.x + nwg * (blockIdx.y + p.split_k * blockIdx.z);
    splitk_coords(p, xcd_major(lin, total), nwg, tiles_m, tiles_n, tm, tn, z, split_idx);
  } else {
    tile_coords(xcd_major(orig, nwg), tiles_m, tiles_n, p.group_m, tm, tn);
    z = blockIdx.z;
    split_idx = blockIdx.y;
  }
  pp2_tile<AK, BKC, EPI, BK, NA>(p, tm, tn, z, split_idx, orig);
}

// Several split-K weight-gradient GEMMs (same operand layouts) in one launch: the concatenation of their
// (tile, split, batch) spaces, XCD-major as a whole; workgroup positions [start[i], start[i + 1]) belong to
// member i. Fills the CUs with one grid where the members alone would leave a wave partly empty (the
// out-projection's 9 tiles and q|k|v's 27 at B/16).
template <bool AK, bool BKC>
__global__ void __launch_bounds__(512) gemm_pp2_group_kernel(const GemmGroup G) {
  const int orig = blockIdx.x;
  const int w = xcd_major(orig, G.start[G.n]);
  int gi = 0;
#pragma unroll
  for (int k = 1; k < GEMM_GROUP_MAX; ++k)
    if (k < G.n && w >= G.start[k]) gi = k;
  gi = __builtin_amdgcn_readfirstlane(gi);
  const GemmDev& p = G.g[gi];
  const int tiles_m = (p.M + 255) / 256, tiles_n = (p.N + 255) / 256;
  int tm, tn, z, split_idx;
  splitk_coords(p, w - G.start[gi], tiles_m * tiles_n, tiles_m, tiles_n, tm, tn, z, split_idx);
  pp2_tile<AK, BKC, VIT_EPI_SPLITK>(p, tm, tn, z, split_idx, orig);
}

// The group with its members in a device-memory table (any member count; vit_gemm_group_launch): the weight
// gradients of a whole backward as one grid. Members may differ in K and in split: a member at split 1 whose
// descriptor carries its output's own strides (c_bs, ldc) writes its gradient directly, one accumulation chain over
// all of K and no slab. The whole space is XCD-major, members in the caller's order, so one member's tiles (which
// share its operand panels) are adjacent positions of one XCD. Assumed about dispatch, for speed only: launch
// indices are dealt to the 8 XCDs in turn and start in order, so in every round an XCD's CUs hold a run of
// neighbouring positions. No workgroup waits for another; a different dispatch order costs L2 hits, not results.
// ACC = EPI_ACC: the instantiation whose direct members with GemmDev::acc set add into their destination (each
// output element belongs to one workgroup at split 1, so the read-modify-write needs no atomics and is deterministic);
// its slab members and plain direct members store as in the ACC = 0 instantiation.
template <bool AK, bool BKC, int ACC = 0>
__global__ void __launch_bounds__(512) gemm_pp2_table_kernel(const GemmDev* __restrict__ tab,
                                                             const int* __restrict__ start, const int n) {
  const int orig = blockIdx.x;
  const int w = xcd_major(orig, (int)gridDim.x);
  // wave-uniform binary search (blockIdx only: scalar loads): the last member with start[gi] <= w
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (w >= start[mid])
      lo = mid;
    else
      hi = mid;
  }
  const int gi = __builtin_amdgcn_readfirstlane(lo);
  const GemmDev p = tab[gi];  // a copy in registers: the main loop's "memory" clobbers reload nothing
  const int tiles_m = (p.M + 255) / 256, tiles_n = (p.N + 255) / 256;
  int tm, tn, z, split_idx;
  splitk_coords(p, w - start[gi], tiles_m * tiles_n, tiles_m, tiles_n, tm, tn, z, split_idx);
  pp2_tile<AK, BKC, VIT_EPI_SPLITK | ACC>(p, tm, tn, z, split_idx, orig);
}

template <bool AK, bool BKC, int EPI, int BK = 64, int NA = 2>
hipError_t launch_pp2(const GemmDev& d, int batch, int split, hipStream_t s) {
  const int tiles = ((d.M + 255) / 256) * ((d.N + 255) / 256);
  dim3 grid(tiles, split, batch);
  hipLaunchKernelGGL((gemm_pp2_kernel<AK, BKC, EPI, BK, NA>), grid, dim3(512), 0, s, d);
  return hipGetLastError();
}

// the split-K group (M/N-contiguous operands: the weight gradients' layout)
inline hipError_t launch_pp2_group(const GemmGroup& g, hipStream_t s) {
  hipLaunchKernelGGL((gemm_pp2_group_kernel<false, false>), dim3(g.start[g.n]), dim3(512), 0, s, g);
  return hipGetLastError();
}

// ... with the members in a device table of n descriptors and n + 1 starts (total = start[n] workgroups)
template <int ACC>
hipError_t launch_pp2_table(const void* table, int n, int total, hipStream_t s) {
  const GemmDev* tab = (const GemmDev*)table;
  const int* start = (const int*)((const char*)table + vitg::group_table_start_off(n));
  hipLaunchKernelGGL((gemm_pp2_table_kernel<false, false, ACC>), dim3(total), dim3(512), 0, s, tab, start, n);
  return hipGetLastError();
}
