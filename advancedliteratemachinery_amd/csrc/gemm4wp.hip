// gemm_4w_p<TOut>: gemm_4w_r made PERSISTENT (gemm4wr.hip; selectors 20 .. 22; a unit of its own; round 4).
//
// tools/gemm4wr_trace.py (profiles/r04r_gemm4wr_trace.txt) timed the phases of a 256x256 tile with one workgroup per CU, K = 512, bf16
// destination: 13.9 k cycles from the first instruction to "X tile 0 landed", 20.7 k in the main loop (16.4 k of MFMAs), 12.6 k in the
// LDS-staged epilogue; with an fp32 destination + fp32 residual the epilogue is 44 k.  Nothing overlaps the prologue or the epilogue,
// because the CU holds ONE workgroup -- that, not the main loop, is where the time was.  Here
//   * a workgroup walks over tiles (ordinal k -> tile xcd_remap(blockIdx.x + k * gridDim.x): the workgroups of an XCD stay on
//     neighbouring tiles) and its stages form ONE stream across them: stage g requests W of stage g + 3 and X of stage g + 4 whichever
//     tile those belong to, so the next tile's first operands are requested under the last stages of this one and land during its
//     epilogue -- there is no prologue after the first tile;
//   * the epilogue uses registers only (the ring keeps receiving the next tile): an accumulator block is (16 features of this wave,
//     16 tokens) with lane = (token, 4 consecutive features), so it leaves as one 8-byte (bf16) / 16-byte (fp32) store per lane;
//     the four feature blocks of a token row are stored back to back (128 / 256 contiguous bytes per row); the accumulators are
//     zeroed as they are read;
//   * the main loop is gemm_4w_r's (W fragments global -> registers three stages ahead, X by DMA through a ring of five, one barrier per
//     64-deep stage, accumulators a[0..255] addressed literally; same build audit, same bits).
// Counted waits with the epilogue's stores in flight: vmcnt counts loads and stores, loads retire in order among loads.  "At most n
// operations out" therefore still implies "every load with n younger LOADS behind it has landed", whatever the stores do: the waits of
// the main loop stay correct, they only may wait for some stores as well.
// RESULT (profiles/r04s_*, r04v_*): bit-exact; +9-30 % over gemm_256 behind a GELU epilogue and +7 % at K = 768 (dispatched there),
// equal or a few per cent behind on long K -- the cycles saved per tile reappear as waiting inside the main loop: the operand stream
// from L2 paces every tile kernel of this library (counters in profiles/r04w_*).
// bf16 operands, bf16 / fp32 / split-bf16 row-major destination, M % 256 == 0, N % 256 == 0, K % 256 == 0, 16-byte aligned bias.
// X3 (selector 22): the three products of a bf16x3 GEMM fused over SHARED operand tiles.  A rows are [hi | lo] (K0 each), W rows
// [w_hi | w_hi | w_lo]; the other kernels walk K' = 3 K0 as three passes (hi w_hi, lo w_hi, hi w_lo) and fetch every hi tile twice.  Here a
// 64-deep chunk c of K0 is three sub-stages over two X tiles and two W fragment sets: (W_hi, X_hi), (W_hi, X_lo), (W_lo, X_hi) -- 2/3 of
// the operand bytes, 2/3 of the requests, two barriers per three sub-stages.  The summation order differs from the three-pass kernels
// (chunk by chunk instead of plane by plane): equal to them within fp32 rounding, not bit for bit.  K0 % 128 == 0.
#include "gemm_common.h"

namespace omp_gemm {
namespace {

template <typename TOut, bool SPLIT, int ABL = 0, bool X3 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_4w_p(GemmP p) {
  typedef bf16_t T;
  constexpr bool F32O = sizeof(TOut) == 4;
  static_assert(!(SPLIT && F32O), "split rows: bf16 storage");
  typedef bf16x8 frag;
  constexpr int NS = 5;                 // X tiles in the ring
  constexpr int ROWB = 128;             // bytes of K per LDS row (64 bf16 = one cache line)
  constexpr int OPT = 256 * ROWB;       // one X tile: 32 KB
  extern __shared__ __attribute__((aligned(16))) char smem[];   // NS * OPT: the X ring and nothing else

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntile = p.tiles_m * p.tiles_n;
  const int G = (int)gridDim.x;
  const int nk = (ntile - (int)blockIdx.x + G - 1) / G;   // tiles of this workgroup (>= 1: the grid never exceeds the tile count)
  const int K0 = p.K / 3;                                 // X3: width of one operand plane
  const int nst = X3 ? K0 / 64 : p.K / 64;                // stages per tile (a multiple of 4); X3: chunks per tile (even)

  auto uniform_ptr = [](const void* q) -> const char* {
    const uint64_t bs = reinterpret_cast<uint64_t>(q);
    const uint64_t sb = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(bs >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)bs);
    return reinterpret_cast<const char*>(sb);
  };
  // tile ordinal k of this workgroup -> origin (row m0, column n0); the division runs on the vector ALU: back to scalar registers
  auto origin = [&](int k, int64_t& m0, int& n0) {
    const int lid = xcd_remap((int)blockIdx.x + k * G, ntile);
    const int tm = __builtin_amdgcn_readfirstlane(lid / p.tiles_n);
    const int tn = __builtin_amdgcn_readfirstlane(lid - tm * p.tiles_n);
    m0 = (int64_t)tm * 256; n0 = tn * 256;
  };

  // ---- X by DMA: pieces 8 * wave .. 8 * wave + 7 (8 rows each) of every tile; scalar tile base + 32-bit lane byte offset ------
  const int lr = lane >> 3, lc = (lane & 7) ^ lr;   // row inside the piece; the source chunk that lands in slot lane & 7
  // one lane offset for all 8 pieces (the piece's 8 rows go into the scalar base: the register file is full in this kernel)
  const unsigned xoff = (unsigned)(((wave * 64 + lr) * p.lda + lc * 8) * 2);
  const int64_t xpiece = 8 * p.lda * 2;   // bytes between pieces
  // `src` = uniform address of (tile row 0, k offset of the stage), `g` = position of the stage in this workgroup's stream
  auto issue_x = [&](const char* src, int slot, auto PC, bool thin = false) {
    constexpr int pc = decltype(PC)::value;
    char* dst = smem + slot * OPT + (wave * 8 + pc) * 1024;
    // thin: ABL == 5 (selector 21, development; wrong results, valid timing): the requests of every third stage degenerate to one
    // 16-byte line per instruction -> 2/3 of the operand bytes under the same instruction stream (the estimate that X3 was built on)
    const char* s2 = thin ? src : src + pc * xpiece + (size_t)xoff;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)s2,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  };
  auto x_src = [&](const char* xb, int ks) -> const char* {   // X base of a tile, stage ks -> uniform source address
    int ka = ks * 64;
    if (p.a_wrap > 0 && ka >= p.a_wrap) ka -= p.a_wrap;   // bf16x3: K tiles beyond [hi | lo] re-read the hi plane
    return uniform_ptr(xb + (int64_t)ka * 2);
  };

  // ---- W straight into registers: feature rows n0 + 64 wave + 16 a + (lane & 15), 16-byte chunk lane >> 4 of each 32-deep k step ----
  const int lrow = lane & 15, lg = lane >> 4;
  const unsigned woff = (unsigned)((((int64_t)(wave * 64 + lrow)) * p.ldw + lg * 8) * 2);   // feature block a: + 16 a rows in the scalar base
  const int64_t wblock = 16 * p.ldw * 2;
  frag fwr[4][8];   // [ring slot = stage & 3][k step * 4 + feature block]
  // asm loads, waits counted by hand (gemm4wr.hip: hipcc drains the pipeline in front of loads that stay in flight across a back edge)
  auto load_w = [&](const char* src, auto SL, auto IDX, bool thin = false) {
    constexpr int sl = decltype(SL)::value, idx = decltype(IDX)::value, a = idx >> 1, k = idx & 1;
    frag& dst = fwr[sl][k * 4 + a];
    const unsigned vo = thin ? 0u : woff;
    const char* sa = thin ? src : src + a * wblock;
    if constexpr (ABL != 1) asm volatile("global_load_dwordx4 %0, %1, %2 offset:%c3" : "=v"(dst) : "v"(vo), "s"(sa), "i"(k * 64) : "memory");
  };

  typedef std::integral_constant<int, 0> I0;
  typedef std::integral_constant<int, 1> I1;
  typedef std::integral_constant<int, 2> I2;
  typedef std::integral_constant<int, 3> I3;

  // ---- first tile: prologue in the order of the steady pattern: X0 | W0 X1 | W1 X2 | W2 X3 ----------------------------------------
  int64_t m0; int n0;
  origin(0, m0, n0);
  const char* Xcur = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.A) + m0 * p.lda);
  const char* Wcur = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.W) + (int64_t)n0 * p.ldw);
  // X3: sources of plane pl (0 hi, 1 lo) of chunk c of a tile (X rows [hi | lo], W rows [w_hi | w_hi | w_lo])
  auto x3_src = [&](const char* xb, int c, int pl) -> const char* { return uniform_ptr(xb + ((int64_t)pl * K0 + (int64_t)c * 64) * 2); };
  auto w3_src = [&](const char* wb, int c, int pl) -> const char* { return uniform_ptr(wb + ((int64_t)pl * 2 * K0 + (int64_t)c * 64) * 2); };
  if constexpr (X3) {   // chunk 0 in the order every later chunk is requested in: W_hi | X_hi | X_lo | W_lo
    const char* wh = w3_src(Wcur, 0, 0); const char* wl = w3_src(Wcur, 0, 1);
    const char* xh = x3_src(Xcur, 0, 0); const char* xl = x3_src(Xcur, 0, 1);
    static_for<8>([&](auto IDX) { load_w(wh, I0(), IDX); });
    static_for<8>([&](auto PC) { issue_x(xh, 0, PC); });
    static_for<8>([&](auto PC) { issue_x(xl, 1, PC); });
    static_for<8>([&](auto IDX) { load_w(wl, I1(), IDX); });
  } else {
    const char* x0 = x_src(Xcur, 0); const char* x1 = x_src(Xcur, 1); const char* x2 = x_src(Xcur, 2); const char* x3 = x_src(Xcur, 3);
    const char* w0 = uniform_ptr(Wcur); const char* w1 = uniform_ptr(Wcur + 128); const char* w2 = uniform_ptr(Wcur + 256);
    static_for<8>([&](auto PC) { issue_x(x0, 0, PC); });
    static_for<8>([&](auto IDX) { load_w(w0, I0(), IDX); });
    static_for<8>([&](auto PC) { issue_x(x1, 1, PC); });
    static_for<8>([&](auto IDX) { load_w(w1, I1(), IDX); });
    static_for<8>([&](auto PC) { issue_x(x2, 2, PC); });
    static_for<8>([&](auto IDX) { load_w(w2, I2(), IDX); });
    static_for<8>([&](auto PC) { issue_x(x3, 3, PC); });
  }

  // Accumulators: block (a = feature block of 16, b = token block of 16) lives in a[(16 a + b) * 4 .. + 3].  Contract as gemm_4w: this
  // statement names every AGPR as a clobber; the build audit demands no spill, no scratch, no compiler-generated v_accvgpr_*.
  static_for<256>([&](auto I) { asm volatile("v_accvgpr_write_b32 a[%c0], 0" ::"i"(decltype(I)::value)); });
  asm volatile("s_nop 4" ::: OMP_ALL_AGPRS);

  // X fragment (k step, token block b) of a tile: row 16 b + lrow, chunk 4 k + lg -> (16 b + lrow) * 128 + (((4 k + lg) ^ (lrow & 7)) << 4)
  const int xl0 = lrow * ROWB + ((lg ^ (lrow & 7)) << 4), xl1 = lrow * ROWB + (((4 + lg) ^ (lrow & 7)) << 4);
  frag fxr[8];   // block q = 16 k + b of a stage lives in fxr[q & 7]; requested 6 blocks ahead
  auto ld_x = [&](unsigned tile, auto Q) {
    constexpr int q = decltype(Q)::value, k = q >> 4, b = q & 15;
    frag& dst = fxr[q & 7];
    const unsigned ad = tile + (unsigned)(k ? xl1 : xl0);
    if constexpr (ABL != 2) asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=v"(dst) : "v"(ad), "i"(b * 16 * ROWB) : "memory");
  };
  const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  // X tile 0 has landed everywhere (behind it in request order: W0 X1 W1 X2 W2 X3 = 48 instructions; X3: both X planes of chunk 0, W_lo
  // = 8 behind them) -> the first six fragments
  if constexpr (X3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(48)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  static_for<6>([&](auto Q) { ld_x(smem_lds, Q); });
  __builtin_amdgcn_sched_barrier(0);

  // Stage (s of the current tile, g of the stream): 128 MFMAs = blocks q = 0..31 (k step q >> 4, token block q & 15) x 4 feature
  // blocks.  Requests: W of stage g + 3 under blocks 2,3 6,7 10,11 14,15; X of stage g + 4 under blocks 24..31, behind the barrier in
  // front of block 24 -- its slot held X(g - 1).  At that barrier X(g + 1) must have landed (its fragments are read from block 26
  // on); requested after it: W(g+1) X(g+2) W(g+2) X(g+3) W(g+3) = 40 loads may still be out; at the top of a stage W(g) must be there:
  // X(g+1) W(g+1) X(g+2) W(g+2) X(g+3) = 40 again.  Requests past this tile's K go to the NEXT tile's first stages (Xnxt / Wnxt); behind
  // the last tile they repeat this tile's first stages (valid addresses, never consumed).
  const char* Xnxt = Xcur;
  const char* Wnxt = Wcur;
  auto stage = [&](int s, int g, auto SL) {
    constexpr int sl = decltype(SL)::value;
    const unsigned xt = smem_lds + (unsigned)((g % NS) * OPT);
    const unsigned xn = smem_lds + (unsigned)(((g + 1) % NS) * OPT);
    const int s3 = s + 3, s4 = s + 4;
    const char* wsrc = uniform_ptr(s3 < nst ? Wcur + (int64_t)s3 * 128 : Wnxt + (int64_t)(s3 - nst) * 128);
    const char* xsrc = s4 < nst ? x_src(Xcur, s4) : x_src(Xnxt, s4 - nst);
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
        else ld_x(xn, std::integral_constant<int, (q + 6) & 31>());   // the next stage's (next tile's) first blocks
      }
      if constexpr (a == 2 && q < 16 && (q & 3) >= 2) load_w(wsrc, std::integral_constant<int, ((sl + 3) & 3)>(), std::integral_constant<int, ((q >> 2) * 2 + (q & 1))>(), ABL == 5 && ((g + 3) % 3) == 2);
      if constexpr (a == 2 && q >= 24) issue_x(xsrc, (g + 4) % NS, std::integral_constant<int, (q - 24)>(), ABL == 5 && ((g + 4) % 3) == 2);
    });
    __builtin_amdgcn_sched_barrier(0);
  };

  // X3 sub-stage `part` of chunk c (parity par = c & 1) of the current tile.  Operands: W registers fwr[2 par + (part == 2)], X slot
  // 2 par + (part == 1).  Requests of a chunk, all for chunk c + 1 (parity 1 - par; of the next tile when past this one's K0), in this order:
  //   part 0: W_hi' under blocks 2,3 6,7 10,11 14,15 | barrier B0 in front of block 24: every wave is done with chunk c - 1, its X slots are
  //           free | X_hi' under blocks 24..31;   part 1: X_lo' under blocks 0..7, W_lo' under blocks 8..15;   part 2: none, barrier B2 in
  //           front of block 24: X_hi' and X_lo' have landed everywhere (behind X_lo' in request order: W_lo' = 8 loads).
  // Waits: top of part 0 needs W_hi (requested a chunk ago; behind it X_hi X_lo W_lo = 24), top of part 2 needs W_lo (behind it the four
  // requests of this chunk = 32); part 1 re-uses W_hi and reads X_lo, certified by the previous chunk's B2.
  auto stage3 = [&](int c, auto PAR, auto PART) {
    constexpr int par = decltype(PAR)::value, part = decltype(PART)::value, npar = 1 - par;
    constexpr int wsl = 2 * par + (part == 2 ? 1 : 0);
    constexpr int xsl = 2 * par + (part == 1 ? 1 : 0);
    constexpr int xnl = part == 0 ? 2 * par + 1 : (part == 1 ? 2 * par : 2 * npar);   // the X slot the NEXT sub-stage reads
    const unsigned xt = smem_lds + (unsigned)(xsl * OPT), xn = smem_lds + (unsigned)(xnl * OPT);
    const bool nextt = c + 1 >= nst;
    const char* xb = nextt ? Xnxt : Xcur;
    const char* wb = nextt ? Wnxt : Wcur;
    const int cc = nextt ? c + 1 - nst : c + 1;
    const char* wsrc = part == 2 ? nullptr : w3_src(wb, cc, part);   // part 0: W_hi', part 1: W_lo'
    const char* xsrc = part == 2 ? nullptr : x3_src(xb, cc, part);   // part 0: X_hi', part 1: X_lo'
    if constexpr (part == 0) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    if constexpr (part == 2) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
    static_for<128>([&](auto I) {
      constexpr int i = decltype(I)::value, q = i >> 2, a = i & 3, k = q >> 4, b = q & 15, r0 = (a * 16 + b) * 4;
      if constexpr (i == 96 && part == 0) __builtin_amdgcn_s_barrier();
      if constexpr (i == 96 && part == 2) {
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      if constexpr (a == 0) asm volatile("s_waitcnt lgkmcnt(5)" ::: "memory");
      asm volatile("v_mfma_f32_16x16x32_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(fwr[wsl][k * 4 + a]), "v"(fxr[q & 7]), "i"(r0), "i"(r0 + 3) : "memory");
      if constexpr (a == 0) {
        if constexpr (q + 6 < 32) ld_x(xt, std::integral_constant<int, (q + 6) & 31>());
        else ld_x(xn, std::integral_constant<int, (q + 6) & 31>());
      }
      if constexpr (part == 0 && a == 2 && q < 16 && (q & 3) >= 2) load_w(wsrc, std::integral_constant<int, (2 * npar)>(), std::integral_constant<int, ((q >> 2) * 2 + (q & 1))>());
      if constexpr (part == 0 && a == 2 && q >= 24) issue_x(xsrc, 2 * npar, std::integral_constant<int, (q - 24)>());
      if constexpr (part == 1 && a == 2 && q < 8) issue_x(xsrc, 2 * npar + 1, std::integral_constant<int, q>());
      if constexpr (part == 1 && a == 2 && q >= 8 && q < 16) load_w(wsrc, std::integral_constant<int, (2 * npar + 1)>(), std::integral_constant<int, (q - 8)>());
    });
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---- epilogue of the tile at (m0, n0): registers only ------------------------------------------------------------------------
  const float* bias = p.bias;
  if (bias != nullptr && p.bias_row != nullptr) bias += (int64_t)(*p.bias_row) * p.bias_row_stride;
  const TOut* res = reinterpret_cast<const TOut*>(p.residual);
  TOut* C = reinterpret_cast<TOut*>(p.C);
  TOut* C2 = reinterpret_cast<TOut*>(p.C2);
  // The tile's bias (features 64 wave + 16 a + 4 lg ..+3) is requested when the tile starts, by asm like the W fragments (a load the
  // compiler knows of would make it wait for everything in flight when the epilogue first touches the value).  It has landed long
  // before the epilogue: loads retire in order and every stage waits until at most 40 are out, with 16 younger ones per stage.
  f32x4 bv[4];
  const unsigned boff = (unsigned)(lg * 16);
  auto load_bias = [&](int bn0) {
    if (bias != nullptr) {
      const char* bsrc = uniform_ptr(bias + bn0 + wave * 64);
      static_for<4>([&](auto A_) {
        constexpr int a = decltype(A_)::value;
        f32x4& dst = bv[a];
        const unsigned bo = boff;
        const char* bs = bsrc;
        asm volatile("global_load_dwordx4 %0, %1, %2 offset:%c3" : "=v"(dst) : "v"(bo), "s"(bs), "i"(a * 64) : "memory");
      });
    }
  };
#pragma unroll
  for (int a = 0; a < 4; ++a) bv[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  load_bias(n0);
  // RES (compile time): a residual is added.  Its loads are asm as well: a load the compiler tracks is waited for with vmcnt(0) once
  // stores are in flight (loads and stores share the counter and retire out of order with respect to each other), i.e. every block
  // would wait for the previous block's store to be acknowledged.  Groups of 8 blocks (2 token blocks x 4 feature blocks), group
  // q + 1 requested before group q is consumed; the wait in front of group q is vmcnt(8): "at most the 8 younger LOADS are out" --
  // it drains the previous group's stores too (they may retire before or after the loads), once per group instead of once per block.
  const unsigned roff = (unsigned)((lrow * p.ldr + lg * 4) * (int64_t)sizeof(TOut));
  auto epilogue = [&](int64_t em0, int en0, auto ACT, auto RES) {
    constexpr bool has_res = decltype(RES)::value != 0;
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // the last MFMAs' results are read below
    const int ncol = en0 + wave * 64 + lg * 4;            // + 16 a
    const int64_t mrow = em0 + lrow;                      // + 16 b
    typedef typename std::conditional<F32O, f32x4, bf16x4>::type rvec;
    rvec rr[2][8];
    const char* rbase = has_res ? uniform_ptr(res + em0 * p.ldr + en0 + wave * 64) : nullptr;
    const int64_t rstep_b = 16 * p.ldr * (int64_t)sizeof(TOut);   // bytes between token blocks
    auto req = [&](auto GRP) {
      constexpr int grp = decltype(GRP)::value;
      static_for<8>([&](auto J) {
        constexpr int j = decltype(J)::value, b = grp * 2 + (j >> 2), a = j & 3;
        rvec& dst = rr[grp & 1][j];
        const unsigned ro = roff;
        const char* sa = rbase + b * rstep_b + a * 16 * (int)sizeof(TOut);
        if constexpr (F32O) asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(ro), "s"(sa) : "memory");
        else asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(dst) : "v"(ro), "s"(sa) : "memory");
      });
    };
    if constexpr (has_res) req(I0());
    static_for<8>([&](auto GRP) {
      constexpr int grp = decltype(GRP)::value;
      if constexpr (has_res) {
        if constexpr (grp < 7) {
          req(std::integral_constant<int, (grp + 1) & 7>());
          asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      }
      static_for<8>([&](auto J) {
        constexpr int j = decltype(J)::value, b = grp * 2 + (j >> 2), a = j & 3, r0 = (a * 16 + b) * 4;
        float v[4];
        asm volatile("v_accvgpr_read_b32 %0, a[%c4]\n\tv_accvgpr_read_b32 %1, a[%c5]\n\tv_accvgpr_read_b32 %2, a[%c6]\n\tv_accvgpr_read_b32 %3, a[%c7]\n\t"
                     "v_accvgpr_write_b32 a[%c4], 0\n\tv_accvgpr_write_b32 a[%c5], 0\n\tv_accvgpr_write_b32 a[%c6], 0\n\tv_accvgpr_write_b32 a[%c7], 0"
                     : "=v"(v[0]), "=v"(v[1]), "=v"(v[2]), "=v"(v[3])
                     : "i"(r0), "i"(r0 + 1), "i"(r0 + 2), "i"(r0 + 3));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] += bv[a][e];
          if constexpr (decltype(ACT)::value == OMP_ACT_RELU) v[e] = fmaxf(v[e], 0.0f);
        }
        if constexpr (decltype(ACT)::value == OMP_ACT_GELU) {
          if constexpr (F32O) {   // fp32 destinations keep the < 1 ulp erf form; bf16 and split pairs take the packed GELU
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
          } else {
            gelu_fast_n<4>(v);
          }
        }
        const int64_t m = mrow + b * 16;
        const int n = ncol + a * 16;
        auto put4 = [&](TOut* dst, const float* w) {
          if constexpr (F32O) *reinterpret_cast<f32x4*>(dst) = f32x4{w[0], w[1], w[2], w[3]};
          else *reinterpret_cast<bf16x4*>(dst) = bf16x4{(bf16_t)w[0], (bf16_t)w[1], (bf16_t)w[2], (bf16_t)w[3]};
        };
        if constexpr (has_res) {
          if (C2 != nullptr) put4(C2 + m * p.ldc2 + n, v);
          const rvec r = rr[grp & 1][j];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (float)r[e];
        }
        if constexpr (SPLIT) {
          bf16x4 hi, lo;
#pragma unroll
          for (int e = 0; e < 4; ++e) { hi[e] = (bf16_t)v[e]; lo[e] = (bf16_t)(v[e] - (float)hi[e]); }
          *reinterpret_cast<bf16x4*>(C + m * p.ldc + n) = hi;
          *reinterpret_cast<bf16x4*>(C + m * p.ldc + p.N + n) = lo;
        } else {
          put4(C + m * p.ldc + n, v);
        }
      });
    });
    asm volatile("s_nop 4" ::: "memory");   // accumulator writes above -> the next tile's first MFMAs
  };
  auto epilogue_act = [&](int64_t em0, int en0, auto RES) {
    if (p.act == OMP_ACT_GELU) epilogue(em0, en0, std::integral_constant<int, OMP_ACT_GELU>(), RES);
    else if (p.act == OMP_ACT_RELU) epilogue(em0, en0, std::integral_constant<int, OMP_ACT_RELU>(), RES);
    else epilogue(em0, en0, std::integral_constant<int, OMP_ACT_NONE>(), RES);
  };

  int g = 0;
  for (int k = 0; k < nk; ++k) {
    if (k + 1 < nk) {
      int64_t m1; int n1;
      origin(k + 1, m1, n1);
      Xnxt = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.A) + m1 * p.lda);
      Wnxt = reinterpret_cast<const char*>(reinterpret_cast<const T*>(p.W) + (int64_t)n1 * p.ldw);
    } else {
      Xnxt = Xcur; Wnxt = Wcur;
    }
    if constexpr (X3) {
      for (int c = 0; c < nst; c += 2) {         // K0 % 128 == 0
        stage3(c, I0(), I0()); stage3(c, I0(), I1()); stage3(c, I0(), I2());
        stage3(c + 1, I1(), I0()); stage3(c + 1, I1(), I1()); stage3(c + 1, I1(), I2());
      }
    } else {
      for (int s = 0; s < nst; s += 4, g += 4) {   // K % 256 == 0
        stage(s, g, I0());
        stage(s + 1, g + 1, I1());
        stage(s + 2, g + 2, I2());
        stage(s + 3, g + 3, I3());
      }
    }
    if (res != nullptr) epilogue_act(m0, n0, I1());
    else epilogue_act(m0, n0, I0());
    if (k + 1 < nk) {
      origin(k + 1, m0, n0);
      load_bias(n0);
    }
    Xcur = Xnxt; Wcur = Wnxt;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the requests behind the last tile
}

template <typename TOut, bool SPLIT, int ABL = 0, bool X3 = false>
int launch_4wp_t(GemmP& p, hipStream_t st) {
  constexpr size_t smem = 5 * 32768;   // the X ring (X3: four of the five slots)
  constexpr auto kern = gemm_4w_p<TOut, SPLIT, ABL, X3>;
  if (const int rc = omp_raise_lds<kern>("omp_gemm_bias_act")) return rc;
  p.tiles_m = (int)ceil_div64(p.M, 256); p.tiles_n = (int)ceil_div64(p.N, 256);
  const int ntile = p.tiles_m * p.tiles_n;
  int grid = omp_device_cus() & ~7;    // a multiple of 8: a workgroup's tiles stay on its XCD's share of the tile list
  if (grid < 8) grid = 8;
  if (grid > ntile) grid = ntile;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, p);
  return OMP_OK;
}

template <typename TOut>
int launch_4wp(GemmP& p, hipStream_t st) {
  if constexpr (sizeof(TOut) == 2) {
    if (p.split_out) return launch_4wp_t<TOut, true>(p, st);
  }
  return launch_4wp_t<TOut, false>(p, st);
}

template <typename TOut>
int launch_4wx3(GemmP& p, hipStream_t st) {
  if constexpr (sizeof(TOut) == 2) return launch_4wp_t<TOut, true, 0, true>(p, st);
  else return launch_4wp_t<TOut, false, 0, true>(p, st);
}

}  // namespace

int gemm4wp_launch(GemmP& p, bool f32_out, hipStream_t st) { return f32_out ? launch_4wp<float>(p, st) : launch_4wp<bf16_t>(p, st); }

int gemm4wp_launch_ablation(GemmP& p, bool f32_out, hipStream_t st, int abl) {
  if (abl == 5 && f32_out) return launch_4wp_t<float, false, 5>(p, st);
  return gemm_not_built(21);
}

int gemm4wx3_launch(GemmP& p, bool f32_out, hipStream_t st) { return f32_out ? launch_4wx3<float>(p, st) : launch_4wx3<bf16_t>(p, st); }

}  // namespace omp_gemm
