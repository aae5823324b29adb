// gemm_4w<TOut>: 256x256 output tiles on FOUR waves (one per SIMD), 256 accumulator registers each (selectors 10 .. 14; a unit of
// its own; round 4).
//
// gemm_256 (gemm256.hip) keeps a 256x256 tile on EIGHT waves of 128x64: per 64-deep K tile every wave reads 24 operand fragments
// for 64 matrix-core instructions (192 KB of ds_read per K tile and CU) and synchronises the workgroup eight times per K tile.  Here a
// wave owns 128x128 (8 x 8 blocks of 16x16, 64 accumulator quads = the whole accumulator file; one wave per SIMD), so a 32-deep K
// stage costs 16 fragment reads for 64 MFMAs (128 KB per 64 of K) and ONE barrier:
//   * operands global -> LDS by DMA in OPERAND TILES of K = 64: 256 rows x 128 B = 32 KB (a row = one full 128-byte cache line; the
//     first version staged K = 32, i.e. 64-byte rows, and every line crossed L2 -> CU twice: profiles/r04e_gemm4w_ablation.txt),
//     alternating X(T), W(T), X(T+1), ... through a ring of 5 slots (160 KB); a wave instruction fills 8 rows x 128 B
//     lane-linearly, the conflict-free swizzle (slot = chunk ^ (row & 7)) is applied to the per-lane SOURCE address, and the
//     address is a scalar base + a 32-bit lane offset (no 64-bit vector arithmetic between the MFMAs of a SIMD's only wave);
//   * a stage s = 2 T + h is the K half h of tile T: 64 MFMAs as four quadrants (W half x X half, 16 MFMAs) in an order that frees
//     half a fragment set early enough to prefetch the next stage into it (below), 4 ds_read_b128 and 2 DMA instructions issued in
//     the shadow of the first MFMAs of every quadrant, one counted vmcnt + s_barrier in the middle of the stage;
//   * the accumulators are addressed LITERALLY (a[0..255]) from asm statements: hipcc's allocator cannot keep 64 live accumulator
//     quads in place (it copied ~120 registers per 32 MFMAs between the register files and spilled ~300, builtin and "+a" asm
//     alike), so the MFMAs, the zero fill and the epilogue's reads are asm; advancedliteratemachinery_amd/audit.py (run by build.py) proves per build
//     that the compiler neither spilled nor touched the accumulator file itself;
//   * the same MFMA (16x16x32), operand orientation and ascending-k accumulation order as gemm_dma / gemm_256: a row's result does
//     not depend on which of the kernels produced it (tests/gpu_checks.py::check_gemm_4w demands equality bit for bit);
//   * epilogue through LDS in two 64-token passes per wave (wave-private 64 x 132 fp32 regions over the drained ring), bias /
//     activation / residual / 16-byte row-contiguous stores exactly as gemm_256.
// bf16 operands, bf16 / fp32 / split-bf16 row-major destination or the blocked K / V^T slabs, K % 64 == 0, N % 8 == 0.

// ABL (development, selectors 12..14: wrong results, valid timing): 1 = no DMA in the main loop, 2 = no fragment reads, 3 = no MFMAs --
// which resource paces the loop (profiles/r04e_gemm4w_ablation.txt)
#include "gemm_common.h"

namespace omp_gemm {
namespace {

template <typename TOut, int SM, bool SPLIT, int NS, int ABL = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_4w(GemmP p) {
  typedef bf16_t T;
  constexpr bool F32O = sizeof(TOut) == 4;
  static_assert(!(F32O && SM != OMP_STORE_PLAIN), "fp32 K / V^T slabs stay on gemm_dma");
  static_assert(!(SPLIT && F32O), "split rows / split-plane slabs: bf16 storage");
  static_assert(NS == 5, "ring of 5 operand-tile slots (160 KB)");
  typedef bf16x8 frag;
  constexpr int ROWB = 128;             // bytes of K per LDS row (64 bf16 = one cache line)
  constexpr int OPT = 256 * ROWB;       // one operand tile: 32 KB
  constexpr int IPO = 8;                // DMA instructions per wave and operand tile (8 pieces of 8 rows)
  constexpr int ES = 132;               // epilogue row pitch (floats)
  constexpr int EWAVE = 64 * ES * 4;    // epilogue bytes per wave (64 token rows x 128 features)
  extern __shared__ __attribute__((aligned(16))) char smem[];   // NS * OPT (the epilogue regions, 4 * EWAVE, alias the drained ring)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nwg = p.tiles_m * p.tiles_n;
  const int lid = xcd_remap(blockIdx.x, nwg);
  const int tm = lid / p.tiles_n, tn = lid % p.tiles_n;
  const int64_t m0 = (int64_t)tm * 256;
  const int n0 = tn * 256;
  const int nj = 2 * (p.K / 64);        // operand tiles: j even = X(j / 2), odd = W(j / 2); also the number of stages

  // ---- DMA roles: pieces 8 * wave .. 8 * wave + 7 (8 rows each) of every operand tile -----------------------------------
  // source address = wave-uniform tile base (scalar registers, advanced by the K offset) + a 32-bit per-lane offset inside the tile
  const int lr = lane >> 3, lc = (lane & 7) ^ lr;   // row inside the piece; the source chunk that lands in slot lane & 7
  const T* Xt = reinterpret_cast<const T*>(p.A) + m0 * p.lda;
  const T* Wt = reinterpret_cast<const T*>(p.W) + (int64_t)n0 * p.ldw;
  unsigned xoff[8], woff[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int64_t gm = m0 + (wave * 8 + j) * 8 + lr; if (gm > p.M - 1) gm = p.M - 1;
    int gn = n0 + (wave * 8 + j) * 8 + lr; if (gn > p.N - 1) gn = p.N - 1;
    xoff[j] = (unsigned)((gm - m0) * p.lda + lc * 8);
    woff[j] = (unsigned)((int64_t)(gn - n0) * p.ldw + lc * 8);
  }
  // piece `pc` (0..7, a compile-time constant) of operand tile j
  auto issue_one = [&](int j, auto PC) {
    constexpr int pc = decltype(PC)::value;
    const int Tk = j >> 1;
    int ka = Tk * 64;
    const bool isw = (j & 1) != 0;
    if (!isw && p.a_wrap > 0 && ka >= p.a_wrap) ka -= p.a_wrap;   // bf16x3: K tiles beyond [hi | lo] re-read the hi plane
    char* dst = smem + (j % NS) * OPT + (wave * 8 + pc) * 1024;
    const uint64_t bs = reinterpret_cast<uint64_t>(isw ? Wt + ka : Xt + ka);
    const uint64_t sb = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(bs >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)bs);
    const char* src = reinterpret_cast<const char*>(sb) + (size_t)((isw ? woff[pc] : xoff[pc]) * 2u);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  };

  // epilogue role: 16-byte column chunk (lane & 15) of rows (lane >> 4) + 4 * it; its bias is requested now
  const int ncol = n0 + wn * 128 + (lane & 15) * 8;
  const float* bias = (SM == OMP_STORE_VBLK) ? nullptr : p.bias;   // V^T slabs: rows are features, the bias follows m
  if (bias != nullptr && p.bias_row != nullptr) bias += (int64_t)(*p.bias_row) * p.bias_row_stride;
  const bool bias_vec = bias != nullptr && ncol + 8 <= p.N && (reinterpret_cast<uintptr_t>(bias) & 15) == 0;
  const float* bsrc = bias_vec ? bias + ncol : reinterpret_cast<const float*>(p.W);
  const f32x4 braw0 = *reinterpret_cast<const f32x4*>(bsrc);
  const f32x4 braw1 = *reinterpret_cast<const f32x4*>(bsrc + 4);

  // ---- prologue: operand tiles 0, 1, 2 and the first half of tile 3 (the steady pattern continues from there) ------------
  int pro = 0;   // DMA instructions of this wave requested behind tile 1
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nj) {
      static_for<8>([&](auto PC) {
        if (j < 3 || decltype(PC)::value < 4) issue_one(j, PC);
      });
      if (j >= 2) pro += j == 2 ? 8 : 4;
    }

  // Accumulators: block (a = W block of 16 features, b = X block of 16 tokens) lives in a[(8 a + b) * 4 .. + 3], ALL 256 registers of
  // the accumulator file.  Contract (cdna_hip_programming.md 5.7 item 4): this statement names every AGPR as a clobber, so the kernel
  // descriptor allocates them; the build audit demands no spill, no scratch and no compiler-generated v_accvgpr_* in this kernel.
  static_for<256>([&](auto I) { asm volatile("v_accvgpr_write_b32 a[%c0], 0" ::"i"(decltype(I)::value)); });
  asm volatile("s_nop 4" ::: OMP_ALL_AGPRS);

  const int lrow = lane & 15, lg = lane >> 4;
  // fragment byte offsets inside an operand tile: row r (16-row aligned + lrow), K half h, chunk 4 h + lg -> r * 128 + (((4 h + lg) ^ (r & 7)) << 4)
  const int fsw0 = (lg ^ (lrow & 7)) << 4, fsw1 = ((4 + lg) ^ (lrow & 7)) << 4;
  const int xrow = (wm * 128 + lrow) * ROWB;   // + b * 16 * ROWB
  const int wrow = (wn * 128 + lrow) * ROWB;   // + a * 16 * ROWB
  // ONE fragment set (16 fragments = 64 registers), refilled quadrant by quadrant.  Quadrant orders:
  //   order A (even stages; holds W-lo, X-lo on entry): (lo,lo) [read X-hi]  (lo,hi) [read W-hi]  | barrier |
  //                                                      (hi,hi) [read next W-lo]  (hi,lo) [read next X-hi]
  //   order B (odd stages;  holds W-lo, X-hi on entry): (lo,hi) [read X-lo]  (lo,lo) [read W-hi]  | barrier |
  //                                                      (hi,lo) [read next W-lo]  (hi,hi) [read next X-lo]
  // every accumulator still receives exactly one MFMA per stage, in ascending k order.
  frag fw[8], fx[8];
  // fragment loads of one operand half (4 fragments) of stage s, in two pairs (`pr` = 0 / 1; 2 = all four)
  auto ld_w = [&](int st, auto H, int pr = 2) {
    constexpr int h = decltype(H)::value;
    const char* base = smem + ((2 * (st >> 1) + 1) % NS) * OPT + wrow + ((st & 1) ? fsw1 : fsw0);
#pragma unroll
    for (int a = h * 4; a < h * 4 + 4; ++a)
      if (pr == 2 || ((a & 3) >> 1) == pr) fw[a] = *reinterpret_cast<const frag*>(base + a * 16 * ROWB);
  };
  auto ld_x = [&](int st, auto H, int pr = 2) {
    constexpr int h = decltype(H)::value;
    const char* base = smem + ((2 * (st >> 1)) % NS) * OPT + xrow + ((st & 1) ? fsw1 : fsw0);
#pragma unroll
    for (int b = h * 4; b < h * 4 + 4; ++b)
      if (pr == 2 || ((b & 3) >> 1) == pr) fx[b] = *reinterpret_cast<const frag*>(base + b * 16 * ROWB);
  };
  // What the asm MFMA costs (cdna_hip_programming.md 5.7): the compiler neither schedules around it nor pads its hazards -- the
  // operand fragments are compiler-issued ds_reads (their lgkmcnt waits are the compiler's), an accumulator is only re-read by the
  // MFMA that accumulates into it 64 MFMAs later (no wait states needed), and the epilogue's reads sit behind explicit nops.
  // a quadrant: 16 MFMAs; hook(I) runs after the I-th
  auto quad = [&](auto AH, auto BH, auto hook) {
    constexpr int ah = decltype(AH)::value, bh = decltype(BH)::value;
    static_for<16>([&](auto I) {
      constexpr int i = decltype(I)::value, a = ah * 4 + (i >> 2), b = bh * 4 + (i & 3), r0 = (a * 8 + b) * 4;
      // "memory": the compiler may not move the fragment loads of the hooks across an MFMA -- hoisted to the top of the quadrant
      // they sat in front of a compiler-inserted lgkmcnt(0) (the operands of the first MFMA), i.e. their latency was exposed
      if constexpr (ABL != 3) asm volatile("v_mfma_f32_16x16x32_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(fw[a]), "v"(fx[b]), "i"(r0), "i"(r0 + 3) : "memory");
      else asm volatile("" ::"v"(fw[a]), "v"(fx[b]) : "memory");
      hook(I);
    });
  };
  typedef std::integral_constant<int, 0> I0;
  typedef std::integral_constant<int, 1> I1;

  // operand tiles 0 and 1 have landed everywhere -> the fragments order A starts from
  {
    wait_dma_tiles<4>(pro >> 2);
    __builtin_amdgcn_s_barrier();
    ld_w(0, I0());
    ld_x(0, I0());
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  }

  // Stage s reads operand tiles 2 T and 2 T + 1 (T = s / 2); their slots are free again after the barrier of stage 2 T + 1.  DMA
  // schedule: quadrants 1, 2 request pieces 4..7 of operand tile s + 3, quadrants 3, 4 (behind the barrier) pieces 0..3 of tile
  // s + 4, whose slot held tile s - 1 (read for the last time before this stage's barrier).  At the barrier of stage s the tiles up
  // to s + 2 must have landed (the next stage's fragments are read right behind it): only tile s + 3 (8 instructions) may be out.
  // STEADY = 1: the caller guarantees s + 4 < nj: no branch inside the stage; STEADY = 0: the last stages, checked at run time
  auto stage = [&](int s, auto ORDER, auto STEADY) {
    constexpr int ord = decltype(ORDER)::value;           // 0 = A, 1 = B
    constexpr bool steady = decltype(STEADY)::value != 0;
    typedef std::integral_constant<int, ord> XH0;          // X half the stage enters with
    typedef std::integral_constant<int, 1 - ord> XH1;      // ... and the one it reads first
    const bool next = steady ? true : s + 1 < nj;          // a next stage exists
    const bool d3 = ABL == 1 ? false : (steady ? true : s + 3 < nj);
    const bool d4 = ABL == 1 ? false : (steady ? true : s + 4 < nj);
    // every quadrant: fragment pair loads after MFMAs 0 and 1, DMA instructions after MFMAs 4 and 6
    // quadrant 1: (W-lo, entry X half); the other X half of this stage arrives under it
    quad(I0(), XH0(), [&](auto I) {
      constexpr int i = decltype(I)::value;
      if constexpr (i < 2 && ABL != 2) ld_x(s, XH1(), i);
      if constexpr (i == 4 || i == 6) { if (d3) issue_one(s + 3, std::integral_constant<int, (4 + ((i - 4) >> 1))>()); }
    });
    __builtin_amdgcn_sched_barrier(0);
    // quadrant 2: (W-lo, other X half); W-hi of this stage arrives under it
    quad(I0(), XH1(), [&](auto I) {
      constexpr int i = decltype(I)::value;
      if constexpr (i < 2 && ABL != 2) ld_w(s, I1(), i);
      if constexpr (i == 4 || i == 6) { if (d3) issue_one(s + 3, std::integral_constant<int, (6 + ((i - 4) >> 1))>()); }
    });
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // every read of this stage has returned
    if (next) {
      if (d3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPO) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                        // operand tiles <= s + 2 have landed everywhere; tile s - 1's slot is free
    }
    __builtin_amdgcn_sched_barrier(0);
    // quadrant 3: (W-hi, other X half); W-lo of the NEXT stage arrives under it
    quad(I1(), XH1(), [&](auto I) {
      constexpr int i = decltype(I)::value;
      if constexpr (i < 2 && ABL != 2) { if (next) ld_w(s + 1, I0(), i); }
      if constexpr (i == 4 || i == 6) { if (d4) issue_one(s + 4, std::integral_constant<int, ((i - 4) >> 1)>()); }
    });
    __builtin_amdgcn_sched_barrier(0);
    // quadrant 4: (W-hi, entry X half); the next stage's entry X half (= this stage's OTHER half index) arrives under it
    quad(I1(), XH0(), [&](auto I) {
      constexpr int i = decltype(I)::value;
      if constexpr (i < 2 && ABL != 2) { if (next) ld_x(s + 1, XH1(), i); }
      if constexpr (i == 4 || i == 6) { if (d4) issue_one(s + 4, std::integral_constant<int, (2 + ((i - 4) >> 1))>()); }
    });
    __builtin_amdgcn_sched_barrier(0);
  };
  int s = 0;
  for (; s + 1 + 4 < nj; s += 2) {
    stage(s, I0(), I1());
    stage(s + 1, I1(), I1());
  }
  for (; s < nj; ++s) {
    if (s & 1) stage(s, I1(), I0());
    else stage(s, I0(), I0());
  }
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // the last MFMAs' results are read by compiler code below (5.7 item 2)
  __builtin_amdgcn_s_barrier();   // every wave is done with the ring: the epilogue regions alias it
  __builtin_amdgcn_sched_barrier(0);

  // ---- epilogue: two 64-token passes per wave through a wave-private LDS region -----------------------------------------
  float bcol[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) { bcol[q] = bias_vec ? braw0[q] : 0.f; bcol[q + 4] = bias_vec ? braw1[q] : 0.f; }
  if (bias != nullptr && !bias_vec) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (ncol + q < p.N) bcol[q] = bias[ncol + q];
  }
  const TOut* res = reinterpret_cast<const TOut*>(p.residual);
  TOut* C = reinterpret_cast<TOut*>(p.C);
  float* E = reinterpret_cast<float*>(smem + wave * EWAVE);
  const int erow = lane >> 4, ecol = (lane & 15) * 8, esw = ((lane >> 2) & 1) * 4;
  const bool col_ok = ncol + 8 <= p.N;
  auto pass = [&](auto P_, auto ACT) {
    constexpr int ps = decltype(P_)::value;
    const int64_t mrow0 = m0 + wm * 128 + ps * 64;
    // accumulators of X blocks 4 ps .. 4 ps + 3 (64 tokens) x all 8 W blocks: E[token][feature]
    static_for<32>([&](auto I) {
      constexpr int a = decltype(I)::value >> 2, b = decltype(I)::value & 3, r0 = (a * 8 + ps * 4 + b) * 4;
      f32x4 v;
      asm volatile("v_accvgpr_read_b32 %0, a[%c4]\n\tv_accvgpr_read_b32 %1, a[%c5]\n\tv_accvgpr_read_b32 %2, a[%c6]\n\tv_accvgpr_read_b32 %3, a[%c7]"
                   : "=v"(v[0]), "=v"(v[1]), "=v"(v[2]), "=v"(v[3])
                   : "i"(r0), "i"(r0 + 1), "i"(r0 + 2), "i"(r0 + 3));
      *reinterpret_cast<f32x4*>(E + (b * 16 + lrow) * ES + a * 16 + lg * 4) = v;
    });
    // the region is private to this wave: LDS operations of one wave complete in order
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      u32x4 rres[8][F32O ? 2 : 1];   // residual of 8 row chunks: 16 B (bf16) / 32 B (fp32) each
      if (res != nullptr && col_ok) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          int64_t m = mrow0 + (half * 8 + it) * 4 + erow; if (m > p.M - 1) m = p.M - 1;
          rres[it][0] = *reinterpret_cast<const u32x4*>(res + m * p.ldr + ncol);
          if constexpr (F32O) rres[it][1] = *reinterpret_cast<const u32x4*>(res + m * p.ldr + ncol + 4);
        }
      }
      float brow[8];
      if constexpr (SM == OMP_STORE_VBLK) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          int64_t m = mrow0 + (half * 8 + it) * 4 + erow; if (m > p.M - 1) m = p.M - 1;
          brow[it] = p.bias != nullptr ? p.bias[m] : 0.f;
        }
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int r = (half * 8 + it) * 4 + erow;
        const int64_t m = mrow0 + r;
        // lanes 4..7 of every 8-lane group read their upper quad first: the eight 16-byte reads of a ds_read_b128 group then
        // cover 8 different 4-bank columns (8 k and 8 k + 4 mod 32 for k = 0..3) instead of colliding two by two
        const f32x4 ta = *reinterpret_cast<const f32x4*>(E + r * ES + ecol + esw);
        const f32x4 tb = *reinterpret_cast<const f32x4*>(E + r * ES + ecol + 4 - esw);
        const f32x4 t0 = esw ? tb : ta, t1 = esw ? ta : tb;
        float v[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          if constexpr (SM == OMP_STORE_VBLK) v[q] += brow[it]; else v[q] += bcol[q];
          if constexpr (decltype(ACT)::value == OMP_ACT_RELU) v[q] = fmaxf(v[q], 0.0f);
        }
        if constexpr (decltype(ACT)::value == OMP_ACT_GELU) {
          if constexpr (F32O) {   // fp32 destinations keep the < 1 ulp erf form; split pairs (16 mantissa bits) take the packed GELU like bf16: 3.2e-7 abs error is below their resolution
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = gelu_erf(v[q]);
          } else {
            gelu_fast_n<8>(v);
          }
        }
        if constexpr (SM == OMP_STORE_KBLK) {
          if (m < p.M && col_ok) {
            const int d = p.kv_nH * 64;
            const int b = (int)(m / p.kv_tok), ml = (int)(m - (int64_t)b * p.kv_tok);
            const int nl = ncol / d, h = (ncol - nl * d) >> 6, dd = ncol & 63;
            if constexpr (SPLIT) {
              bf16x8 hi, lo;
#pragma unroll
              for (int q = 0; q < 8; ++q) { hi[q] = (bf16_t)v[q]; lo[q] = (bf16_t)(v[q] - (float)hi[q]); }
              TOut* dst = C + (((((int64_t)nl * p.kv_B + b) * p.kv_nH + h) * (p.kv_mpad >> 5) + (ml >> 5)) * 2) * 2048 + (ml & 31) * 64 + dd;
              *reinterpret_cast<bf16x8*>(dst) = hi;
              *reinterpret_cast<bf16x8*>(dst + 2048) = lo;
            } else {
              bf16x8 o;
              pack16(v, o);
              *reinterpret_cast<bf16x8*>(C + ((((int64_t)nl * p.kv_B + b) * p.kv_nH + h) * p.kv_mpad + ml) * 64 + dd) = o;
            }
          }
          continue;
        }
        if constexpr (SM == OMP_STORE_VBLK) {
          if (m < p.M && col_ok) {
            const int d = p.kv_nH * 64;
            const int nl = (int)(m / d), h = ((int)(m - (int64_t)nl * d)) >> 6, dd = (int)m & 63;
            const int b = ncol / p.kv_tok, ml = ncol - b * p.kv_tok;
            const int blk = ml >> 5, j = (ml & 31) >> 3;
            const int64_t at = ((((int64_t)nl * p.kv_B + b) * p.kv_nH + h) * (p.kv_mpad >> 5) + blk) * (SPLIT ? 4096 : 2048) + dd * 32 + (j & 1) * 16 + (j >> 1) * 4;
            if constexpr (SPLIT) {
              bf16x4 h0, h1, l0, l1;
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                h0[q] = (bf16_t)v[q]; l0[q] = (bf16_t)(v[q] - (float)h0[q]);
                h1[q] = (bf16_t)v[4 + q]; l1[q] = (bf16_t)(v[4 + q] - (float)h1[q]);
              }
              *reinterpret_cast<bf16x4*>(C + at) = h0;
              *reinterpret_cast<bf16x4*>(C + at + 8) = h1;
              *reinterpret_cast<bf16x4*>(C + at + 2048) = l0;
              *reinterpret_cast<bf16x4*>(C + at + 2048 + 8) = l1;
            } else {
              *reinterpret_cast<bf16x4*>(C + at) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
              *reinterpret_cast<bf16x4*>(C + at + 8) = bf16x4{(bf16_t)v[4], (bf16_t)v[5], (bf16_t)v[6], (bf16_t)v[7]};
            }
          }
          continue;
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
    }
  };
  auto both = [&](auto ACT) { pass(I0(), ACT); pass(I1(), ACT); };
  if (p.act == OMP_ACT_GELU) both(std::integral_constant<int, OMP_ACT_GELU>());
  else if (p.act == OMP_ACT_RELU) both(std::integral_constant<int, OMP_ACT_RELU>());
  else both(std::integral_constant<int, OMP_ACT_NONE>());
}

template <typename TOut, int SM, bool SPLIT, int NS, int ABL = 0>
int launch_4w_sm(GemmP& p, hipStream_t st) {
  constexpr size_t ring = (size_t)NS * 32768, epi = 4 * 64 * 132 * 4;   // 5 operand-tile slots; the epilogue regions alias them
  constexpr size_t smem = ring > epi ? ring : epi;
  constexpr auto kern = gemm_4w<TOut, SM, SPLIT, NS, ABL>;
  if (const int rc = omp_raise_lds<kern>("omp_gemm_bias_act")) return rc;
  p.tiles_m = (int)ceil_div64(p.M, 256); p.tiles_n = (int)ceil_div64(p.N, 256);
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n), dim3(256), smem, st, p);
  return OMP_OK;
}

template <typename TOut, int NS>
int launch_4w(GemmP& p, hipStream_t st) {
  if constexpr (sizeof(TOut) == 2) {
    if (p.store_mode == OMP_STORE_KBLK) return p.split_out ? launch_4w_sm<TOut, OMP_STORE_KBLK, true, NS>(p, st) : launch_4w_sm<TOut, OMP_STORE_KBLK, false, NS>(p, st);
    if (p.store_mode == OMP_STORE_VBLK) return p.split_out ? launch_4w_sm<TOut, OMP_STORE_VBLK, true, NS>(p, st) : launch_4w_sm<TOut, OMP_STORE_VBLK, false, NS>(p, st);
    if (p.split_out) return launch_4w_sm<TOut, OMP_STORE_PLAIN, true, NS>(p, st);
  }
  return launch_4w_sm<TOut, OMP_STORE_PLAIN, false, NS>(p, st);
}

}  // namespace

int gemm4w_launch(GemmP& p, bool f32_out, hipStream_t st) { return f32_out ? launch_4w<float, 5>(p, st) : launch_4w<bf16_t, 5>(p, st); }

int gemm4w_launch_ablation(GemmP& p, bool f32_out, hipStream_t st, int abl) {
  if (!f32_out) {
    if (abl == 1) return launch_4w_sm<bf16_t, OMP_STORE_PLAIN, false, 5, 1>(p, st);
    if (abl == 2) return launch_4w_sm<bf16_t, OMP_STORE_PLAIN, false, 5, 2>(p, st);
    if (abl == 3) return launch_4w_sm<bf16_t, OMP_STORE_PLAIN, false, 5, 3>(p, st);
  }
  return gemm_not_built(11 + abl);
}

}  // namespace omp_gemm
