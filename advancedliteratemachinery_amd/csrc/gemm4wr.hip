// gemm_4w_r<TOut>: 256x256 output tiles on four waves with the WEIGHT operand streamed global -> registers (selectors 16 .. 18; a unit of
// its own; round 4, the follow-up its ablation asked for: DESIGN.md section 10).
//
// The hypothesis it was built on (profiles/r04l_gemm4w_ablation_big_k.txt): the operand path of gemm_4w / gemm_256 alone (no MFMA) took
// 1.3x the matrix-core time at 21 B/clk and CU of a 64 B/clk path -- bounded, it seemed, by the bytes in flight (48-64 KB of the 160 KB
// ring per CU) times 1.1 us of L2 -> LDS latency.  LDS cannot hold more; the register file can.  RESULT (DESIGN.md section 10,
// profiles/r04p_*, r04w_*): with 160 KB per CU requested the kernel is bit-exact and 3-8 % SLOWER than gemm_256 -- what is in flight is
// bounded below the software, by the L1's request queue towards L2 (54-72 lines outstanding per CU at 460-570 cycles each).  The kernel
// stays as the base of gemm_4w_p (gemm4wp.hip) and as the carrier of the no-MFMA ablation (17) and the phase trace (18).  The four
// waves split the tile's FEATURES (wave w: all 256 tokens x features 64 w .. 64 w + 63), so
//   * a wave's weight rows are its own: the 8 W fragments of a 64-deep K stage go straight from global memory into registers (the
//     MFMA A operand of gemm_dma: lane = (feature l & 15, 16-byte k chunk l >> 4); the two fragments of a row's 128-byte line are
//     requested back to back), FOUR stages of them live (128 registers), requested three stages ahead;
//   * only X goes through LDS: DMA tiles of 256 tokens x 64 k (32 KB, full-line rows, source-side swizzle as gemm_4w) through a
//     ring of 5 = four stages ahead; every wave reads every X fragment (16 per 32 of K), just in time through 8 fragment registers,
//     each feeding 4 MFMAs -- the same 32 ds_read_b128 per 128 MFMAs as gemm_4w, half its DMA instructions;
//   * per wave and stage: 128 MFMAs, 32 fragment reads, 8 global loads, 8 DMA instructions, one barrier (three quarters into the
//     stage: certifies the next X tile, frees the slot of the previous one), ~40 KB per wave requested and not yet consumed
//     (160 KB per CU in flight instead of 48-64);
//   * accumulators a[0..255] addressed literally, zero fill / MFMAs / epilogue reads in asm exactly as gemm_4w (same build audit:
//     the kernel's name contains gemm_4w); the same MFMA, operand orientation and ascending-k order as every other GEMM kernel of the
//     library: results are bit-identical (tests/gpu_checks.py::check_gemm_4w);
//   * epilogue through LDS in four 64-token passes per wave (wave-private 64 x 68 fp32 regions over the drained ring), geometry and
//     arithmetic of gemm_256's.
// bf16 operands, bf16 / fp32 / split-bf16 row-major destination, K % 256 == 0, N % 8 == 0.
#include "gemm_common.h"

namespace omp_gemm {
namespace {

template <typename TOut, bool SPLIT, int ABL = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_4w_r(GemmP p) {
  typedef bf16_t T;
  constexpr bool F32O = sizeof(TOut) == 4;
  static_assert(!(SPLIT && F32O), "split rows: bf16 storage");
  typedef bf16x8 frag;
  constexpr int NS = 5;                 // X tiles in the ring
  constexpr int ROWB = 128;             // bytes of K per LDS row (64 bf16 = one cache line)
  constexpr int OPT = 256 * ROWB;       // one X tile: 32 KB
  constexpr int ES = 68;                // epilogue row pitch (floats)
  constexpr int EWAVE = 64 * ES * 4;    // epilogue bytes per wave (64 token rows x 64 features)
  extern __shared__ __attribute__((aligned(16))) char smem[];   // NS * OPT (the epilogue regions, 4 * EWAVE, alias the drained ring)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = p.tiles_m * p.tiles_n;
  const int lid = xcd_remap(blockIdx.x, nwg);
  const int tm = __builtin_amdgcn_readfirstlane(lid / p.tiles_n);   // the division runs on the vector ALU: back to scalar registers,
  const int tn = __builtin_amdgcn_readfirstlane(lid - tm * p.tiles_n);   // or the tile origin occupies vector registers through the main loop
  const int64_t m0 = (int64_t)tm * 256;
  const int n0 = tn * 256;
  const int nst = p.K / 64;             // stages = X tiles (a multiple of 4)

  // ABL == 4 (selector 18, development): wave 0 stamps s_memtime at the phase boundaries into p.trace[blockIdx][8]
  unsigned long long tr[5] = {0, 0, 0, 0, 0};
  auto stamp = [&](auto I) {
    if constexpr (ABL == 4) tr[decltype(I)::value] = __builtin_amdgcn_s_memtime();
  };
  stamp(std::integral_constant<int, 0>());

  // ---- X by DMA: pieces 8 * wave .. 8 * wave + 7 (8 rows each) of every tile; scalar tile base + 32-bit lane byte offset ------
  const int lr = lane >> 3, lc = (lane & 7) ^ lr;   // row inside the piece; the source chunk that lands in slot lane & 7
  const T* Xt = reinterpret_cast<const T*>(p.A) + m0 * p.lda;
  unsigned xoff[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int64_t gm = m0 + (wave * 8 + j) * 8 + lr; if (gm > p.M - 1) gm = p.M - 1;
    xoff[j] = (unsigned)(((gm - m0) * p.lda + lc * 8) * 2);
  }
  auto uniform_ptr = [](const void* q) -> const char* {
    const uint64_t bs = reinterpret_cast<uint64_t>(q);
    const uint64_t sb = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(bs >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)bs);
    return reinterpret_cast<const char*>(sb);
  };
  auto issue_x = [&](int t, auto PC) {
    constexpr int pc = decltype(PC)::value;
    const bool live = t < nst;   // beyond K: every lane reads the first 16 bytes of the tile's first row (see `stage`)
    int ka = (live ? t : 0) * 64;
    if (p.a_wrap > 0 && ka >= p.a_wrap) ka -= p.a_wrap;   // bf16x3: K tiles beyond [hi | lo] re-read the hi plane
    char* dst = smem + (t % NS) * OPT + (wave * 8 + pc) * 1024;
    const char* src = uniform_ptr(Xt + ka) + (size_t)(live ? xoff[pc] : 0u);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  };

  // ---- W straight into registers: feature rows n0 + 64 wave + 16 a + (lane & 15), 16-byte chunk lane >> 4 of each 32-deep k step ----
  const int lrow = lane & 15, lg = lane >> 4;
  const T* Wt = reinterpret_cast<const T*>(p.W) + (int64_t)n0 * p.ldw;
  unsigned woff[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int gn = n0 + wave * 64 + a * 16 + lrow; if (gn > p.N - 1) gn = p.N - 1;
    woff[a] = (unsigned)(((int64_t)(gn - n0) * p.ldw + lg * 8) * 2);
  }
  frag fwr[4][8];   // [ring slot = stage & 3][k step * 4 + feature block]
  // fragment idx (0..7) of stage t: feature block idx >> 1, k step idx & 1 (the two halves of a row's cache line back to back)
  auto load_w = [&](int t, auto SL, auto IDX) {
    constexpr int sl = decltype(SL)::value, idx = decltype(IDX)::value, a = idx >> 1, k = idx & 1;
    // asm: hipcc's own vmcnt bookkeeping gives up on loads that stay in flight across a loop back edge next to LDS DMA (it put
    // s_waitcnt vmcnt(0) in front of their first use, i.e. drained the whole pipeline twice per four stages); the waits are counted
    // by hand below.  The compiler believes the value is there when the statement ends: the build audit checks that it never
    // copies or spills a fragment register (no v_mov / scratch on them inside the loop).
    frag& dst = fwr[sl][k * 4 + a];
    const bool live = t < nst;
    const unsigned vo = live ? woff[a] : 0u;
    const char* sb = uniform_ptr(Wt + (live ? t : 0) * 64);
    if constexpr (ABL != 1) asm volatile("global_load_dwordx4 %0, %1, %2 offset:%c3" : "=v"(dst) : "v"(vo), "s"(sb), "i"(k * 64) : "memory");
  };

  typedef std::integral_constant<int, 0> I0;
  typedef std::integral_constant<int, 1> I1;
  typedef std::integral_constant<int, 2> I2;
  typedef std::integral_constant<int, 3> I3;

  // ---- prologue in the order of the steady pattern (stage s requests W(s + 3), then X(s + 4)): X0 | W0 X1 | W1 X2 | W2 X3 -------
  static_for<8>([&](auto PC) { issue_x(0, PC); });
  static_for<8>([&](auto IDX) { load_w(0, I0(), IDX); });
  static_for<8>([&](auto PC) { issue_x(1, PC); });
  static_for<8>([&](auto IDX) { load_w(1, I1(), IDX); });
  static_for<8>([&](auto PC) { issue_x(2, PC); });
  static_for<8>([&](auto IDX) { load_w(2, I2(), IDX); });
  static_for<8>([&](auto PC) { issue_x(3, PC); });

  // Accumulators: block (a = feature block of 16, b = token block of 16) lives in a[(16 a + b) * 4 .. + 3].  Contract as gemm_4w: this
  // statement names every AGPR as a clobber; the build audit demands no spill, no scratch, no compiler-generated v_accvgpr_*.
  static_for<256>([&](auto I) { asm volatile("v_accvgpr_write_b32 a[%c0], 0" ::"i"(decltype(I)::value)); });
  asm volatile("s_nop 4" ::: OMP_ALL_AGPRS);

  // X fragment (k step, token block b) of a tile: row 16 b + lrow, chunk 4 k + lg -> (16 b + lrow) * 128 + (((4 k + lg) ^ (lrow & 7)) << 4)
  const int xl0 = lrow * ROWB + ((lg ^ (lrow & 7)) << 4), xl1 = lrow * ROWB + (((4 + lg) ^ (lrow & 7)) << 4);
  frag fxr[8];   // block q = 16 k + b of a stage lives in fxr[q & 7]; requested 6 blocks ahead
  // asm for the same reason as the W loads: hipcc waits for them with lgkmcnt(0) (every outstanding read, the youngest 4 MFMAs old)
  // where the ring needs lgkmcnt(5).  `tile` = LDS byte address of the X tile
  auto ld_x = [&](unsigned tile, auto Q) {
    constexpr int q = decltype(Q)::value, k = q >> 4, b = q & 15;
    frag& dst = fxr[q & 7];
    const unsigned ad = tile + (unsigned)(k ? xl1 : xl0);
    if constexpr (ABL != 2) asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=v"(dst) : "v"(ad), "i"(b * 16 * ROWB) : "memory");
  };
  const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  // X tile 0 has landed everywhere (behind it in request order: W0 X1 W1 X2 W2 X3 = 48 instructions) -> the first six fragments
  asm volatile("s_waitcnt vmcnt(48)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  stamp(I1());   // X tile 0 landed everywhere
  static_for<6>([&](auto Q) { ld_x(smem_lds, Q); });
  __builtin_amdgcn_sched_barrier(0);

  // Stage s: 128 MFMAs = blocks q = 0..31 (k step q >> 4, token block q & 15) x 4 feature blocks.  Requests: W(s + 3) under blocks
  // 2,3 6,7 10,11 14,15; X(s + 4) under blocks 24..31, behind the barrier in front of block 24 -- its slot held X(s - 1).  At that
  // barrier X(s + 1) must have landed (its fragments are read from block 26 on); requested after it: W(s+1) X(s+2) W(s+2) X(s+3)
  // W(s+3) = 40 instructions may still be out; at the top of a stage W(s) must be there: X(s+1) W(s+1) X(s+2) W(s+2) X(s+3) = 40 again.
  // EVERY stage is this one piece of straight-line code, the last ones included: a request for a tile beyond K keeps its place in
  // the count and degenerates to one 16-byte read for the whole wave (lane offset 0 from a valid row: `issue_x` / `load_w`), what
  // it delivers is never consumed.  (A separately guarded tail -- a loop over a switch of slot-specialised stages -- made hipcc
  // copy the fragment registers between its cases while their loads were in flight, and park registers in a0..a9.)
  auto stage = [&](int s, auto SL) {
    constexpr int sl = decltype(SL)::value;
    const unsigned xt = smem_lds + (unsigned)((s % NS) * OPT);
    const unsigned xn = smem_lds + (unsigned)(((s + 1) % NS) * OPT);
    asm volatile("s_waitcnt vmcnt(40)" ::: "memory");
    static_for<128>([&](auto I) {
      constexpr int i = decltype(I)::value, q = i >> 2, a = i & 3, k = q >> 4, b = q & 15, r0 = (a * 16 + b) * 4;
      if constexpr (i == 96) {
        asm volatile("s_waitcnt vmcnt(40)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      // X fragment of block q: requested 6 blocks ago, the 5 younger requests may still be out
      if constexpr (a == 0) asm volatile("s_waitcnt lgkmcnt(5)" ::: "memory");
      if constexpr (ABL != 3) asm volatile("v_mfma_f32_16x16x32_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(fwr[sl][k * 4 + a]), "v"(fxr[q & 7]), "i"(r0), "i"(r0 + 3) : "memory");
      else asm volatile("" ::"v"(fwr[sl][k * 4 + a]), "v"(fxr[q & 7]) : "memory");
      if constexpr (a == 0) {
        if constexpr (q + 6 < 32) ld_x(xt, std::integral_constant<int, (q + 6) & 31>());
        else ld_x(xn, std::integral_constant<int, (q + 6) & 31>());   // behind the last stage: whatever the slot holds, never consumed
      }
      if constexpr (a == 2 && q < 16 && (q & 3) >= 2) load_w(s + 3, std::integral_constant<int, ((sl + 3) & 3)>(), std::integral_constant<int, ((q >> 2) * 2 + (q & 1))>());
      if constexpr (a == 2 && q >= 24) issue_x(s + 4, std::integral_constant<int, (q - 24)>());
    });
    __builtin_amdgcn_sched_barrier(0);
  };
  for (int s = 0; s < nst; s += 4) {   // K % 256 == 0
    stage(s, I0());
    stage(s + 1, I1());
    stage(s + 2, I2());
    stage(s + 3, I3());
  }
  stamp(I2());   // main loop done (this wave)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the degenerate requests of the last stages
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // the last MFMAs' results are read by compiler code below
  __builtin_amdgcn_s_barrier();   // every wave is done with the ring: the epilogue regions alias it
  __builtin_amdgcn_sched_barrier(0);
  stamp(I3());   // ... every wave

  // ---- epilogue: four 64-token passes per wave through a wave-private LDS region --------------------------------------------
  // role: 16-byte column chunk (lane & 7) of rows (lane >> 3) + 8 * it (the register file is full until the main loop ends: nothing
  // of the epilogue is computed or requested before this point)
  // the lane id is re-derived (mbcnt) so that no lane-dependent value of the prologue stays live through the loop for the epilogue's sake
  const int el = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int elrow = el & 15, elg = el >> 4;
  const int ncol = n0 + wave * 64 + (el & 7) * 8;
  const float* bias = p.bias;
  if (bias != nullptr && p.bias_row != nullptr) bias += (int64_t)(*p.bias_row) * p.bias_row_stride;
  const bool bias_vec = bias != nullptr && ncol + 8 <= p.N && (reinterpret_cast<uintptr_t>(bias) & 15) == 0;
  float bcol[8];
  {
    const float* bsrc = bias_vec ? bias + ncol : reinterpret_cast<const float*>(p.W);
    const f32x4 braw0 = *reinterpret_cast<const f32x4*>(bsrc);
    const f32x4 braw1 = *reinterpret_cast<const f32x4*>(bsrc + 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) { bcol[q] = bias_vec ? braw0[q] : 0.f; bcol[q + 4] = bias_vec ? braw1[q] : 0.f; }
  }
  if (bias != nullptr && !bias_vec) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (ncol + q < p.N) bcol[q] = bias[ncol + q];
  }
  const TOut* res = reinterpret_cast<const TOut*>(p.residual);
  TOut* C = reinterpret_cast<TOut*>(p.C);
  float* E = reinterpret_cast<float*>(smem + wave * EWAVE);
  const int erow = el >> 3, ecol = (el & 7) * 8;
  const bool col_ok = ncol + 8 <= p.N;
  auto pass = [&](auto P_, auto ACT) {
    constexpr int ps = decltype(P_)::value;
    const int64_t mrow0 = m0 + ps * 64;
    u32x4 rres[8][F32O ? 2 : 1];   // 8 residual values per row chunk: 16 B (bf16) / 32 B (fp32)
    if (res != nullptr && col_ok) {
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        int64_t m = mrow0 + it * 8 + erow; if (m > p.M - 1) m = p.M - 1;
        rres[it][0] = *reinterpret_cast<const u32x4*>(res + m * p.ldr + ncol);
        if constexpr (F32O) rres[it][1] = *reinterpret_cast<const u32x4*>(res + m * p.ldr + ncol + 4);
      }
    }
    // accumulators of token blocks 4 ps .. 4 ps + 3 (64 tokens) x the 4 feature blocks: E[token][feature]
    static_for<16>([&](auto I) {
      constexpr int a = decltype(I)::value >> 2, bl = decltype(I)::value & 3, r0 = (a * 16 + ps * 4 + bl) * 4;
      f32x4 v;
      asm volatile("v_accvgpr_read_b32 %0, a[%c4]\n\tv_accvgpr_read_b32 %1, a[%c5]\n\tv_accvgpr_read_b32 %2, a[%c6]\n\tv_accvgpr_read_b32 %3, a[%c7]"
                   : "=v"(v[0]), "=v"(v[1]), "=v"(v[2]), "=v"(v[3])
                   : "i"(r0), "i"(r0 + 1), "i"(r0 + 2), "i"(r0 + 3));
      *reinterpret_cast<f32x4*>(E + (bl * 16 + elrow) * ES + a * 16 + elg * 4) = v;
    });
    // the region is private to this wave: LDS operations of one wave complete in order
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int r = it * 8 + erow;
      const int64_t m = mrow0 + r;
      const f32x4 t0 = *reinterpret_cast<const f32x4*>(E + r * ES + ecol);
      const f32x4 t1 = *reinterpret_cast<const f32x4*>(E + r * ES + ecol + 4);
      float v[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        v[q] += bcol[q];
        if constexpr (decltype(ACT)::value == OMP_ACT_RELU) v[q] = fmaxf(v[q], 0.0f);
      }
      if constexpr (decltype(ACT)::value == OMP_ACT_GELU) {
        if constexpr (F32O) {   // fp32 destinations keep the < 1 ulp erf form; bf16 and split pairs take the packed GELU
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = gelu_erf(v[q]);
        } else {
          gelu_fast_n<8>(v);
        }
      }
      auto put8 = [&](TOut* dst, const float* w) {
        if constexpr (F32O) {
          *reinterpret_cast<f32x4*>(dst) = f32x4{w[0], w[1], w[2], w[3]};
          *reinterpret_cast<f32x4*>(dst + 4) = f32x4{w[4], w[5], w[6], w[7]};
        } else {
          bf16x8 o;
          pack16(w, o);
          *reinterpret_cast<bf16x8*>(dst) = o;
        }
      };
      if (res != nullptr) {
        if (p.C2 != nullptr && m < p.M && col_ok) put8(reinterpret_cast<TOut*>(p.C2) + m * p.ldc2 + ncol, v);
        float rv[8];
        if constexpr (F32O) {
          unpack16(__builtin_bit_cast(f32x4, rres[it][0]), rv);
          unpack16(__builtin_bit_cast(f32x4, rres[it][1]), rv + 4);
        } else {
          unpack16(__builtin_bit_cast(bf16x8, rres[it][0]), rv);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] += rv[q];
      }
      if (m < p.M && col_ok) {
        if constexpr (SPLIT) {
          bf16x8 hi, lo;
#pragma unroll
          for (int q = 0; q < 8; ++q) { hi[q] = (bf16_t)v[q]; lo[q] = (bf16_t)(v[q] - (float)hi[q]); }
          *reinterpret_cast<bf16x8*>(C + m * p.ldc + ncol) = hi;
          *reinterpret_cast<bf16x8*>(C + m * p.ldc + p.N + ncol) = lo;
        } else {
          put8(C + m * p.ldc + ncol, v);
        }
      }
    }
  };
  auto all4 = [&](auto ACT) { pass(I0(), ACT); pass(I1(), ACT); pass(I2(), ACT); pass(I3(), ACT); };
  if (p.act == OMP_ACT_GELU) all4(std::integral_constant<int, OMP_ACT_GELU>());
  else if (p.act == OMP_ACT_RELU) all4(std::integral_constant<int, OMP_ACT_RELU>());
  else all4(std::integral_constant<int, OMP_ACT_NONE>());
  if constexpr (ABL == 4) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // stores retired
    stamp(std::integral_constant<int, 4>());
    if (tid == 0 && p.trace != nullptr) {
      unsigned long long* t = p.trace + (long long)blockIdx.x * 8;
      t[0] = tr[0]; t[1] = tr[1]; t[2] = tr[2]; t[3] = tr[3]; t[4] = tr[4];
      t[5] = (unsigned long long)__builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20);   // XCC_ID (HW_REG 20), low 4 bits
    }
  }
}

template <typename TOut, bool SPLIT, int ABL = 0>
int launch_4wr_t(GemmP& p, hipStream_t st) {
  constexpr size_t smem = 5 * 32768;   // the X ring; the epilogue regions (4 x 17 KB) alias it
  constexpr auto kern = gemm_4w_r<TOut, SPLIT, ABL>;
  if (const int rc = omp_raise_lds<kern>("omp_gemm_bias_act")) return rc;
  p.tiles_m = (int)ceil_div64(p.M, 256); p.tiles_n = (int)ceil_div64(p.N, 256);
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n), dim3(256), smem, st, p);
  return OMP_OK;
}

template <typename TOut>
int launch_4wr(GemmP& p, hipStream_t st) {
  if constexpr (sizeof(TOut) == 2) {
    if (p.split_out) return launch_4wr_t<TOut, true>(p, st);
  }
  return launch_4wr_t<TOut, false>(p, st);
}

}  // namespace

int gemm4wr_launch(GemmP& p, bool f32_out, hipStream_t st) { return f32_out ? launch_4wr<float>(p, st) : launch_4wr<bf16_t>(p, st); }

int gemm4wr_launch_dev(GemmP& p, bool f32_out, hipStream_t st, int abl) {
  if (abl == 4) return f32_out ? launch_4wr_t<float, false, 4>(p, st) : launch_4wr_t<bf16_t, false, 4>(p, st);
  if (abl == 3 && !f32_out) return launch_4wr_t<bf16_t, false, 3>(p, st);
  return gemm_not_built(14 + abl);
}

}  // namespace omp_gemm
