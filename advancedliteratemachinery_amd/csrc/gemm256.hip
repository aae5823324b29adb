// gemm_256<TOut>: the large-N Swin GEMMs (qkv, fc1, fc2) on 256x256x64 tiles (selector 9; a unit of its own).
//
// The 128x128 kernel (gemm_dma, gemm.hip) tops out near 30 % of the bf16 matrix-core peak on these shapes: two co-resident
// workgroups hide each other's DMA round trips, but every K tile still costs a full barrier + fragment-read
// restart, and a 128x128 tile moves twice the operand bytes per flop through L2 -> LDS.  This kernel follows the
// phase-interleaved schedule of the CDNA4 playbook (cdna_hip_programming.md, "256^2 8-phase template"), restated for
// this library's operand orientation and swizzle:
//   * 8 waves = 2 (M) x 4 (N); a wave owns 128 x 64 of the tile as 2 x 2 quadrants of 64 x 32 (4 x 2 fragments);
//   * a K tile (64) is FOUR phases, one quadrant x K = 64 each (16 MFMAs); a phase is a LOAD segment (fragment
//     ds_reads for the phases ahead, one 16 KB half tile of DMA) and a COMPUTE segment (the 16 MFMAs, s_setprio 1),
//     each closed by a raw s_barrier;
//   * the two wave groups (M halves) run ONE SEGMENT APART (group 1 passes one extra barrier first): on every SIMD
//     the matrix pipe of one wave runs under the LDS / DMA traffic of its partner;
//   * operands: global -> LDS by DMA in half tiles (128 rows x 128 B), two 64 KB buffers, swizzle on the source
//     address exactly as gemm_dma; a half tile is re-requested two K tiles ahead as soon as its last fragment read
//     is two phases old, ONE counted `s_waitcnt vmcnt(4)` per K tile (two half tiles stay in flight across the
//     barriers), data is read one phase after the wait that retires it (one barrier more than the wait, because
//     of the stagger);
//   * per K tile a wave reads 24 fragments (both W sub-blocks + X sub-block 0 in phase 0, X sub-block 1 in phase 2)
//     for 64 MFMAs;
//   * epilogue through LDS in two 64-row halves per wave (wave-private regions: no workgroup barrier), bias /
//     activation / residual / 16-byte row-contiguous stores exactly as gemm_dma (same arithmetic order: a row's
//     result does not depend on which kernel produced it).
// bf16 operands, bf16 / fp32 / split-bf16 row-major destination, K % 64 == 0, K >= 128, N % 8 == 0.

// TOut = bf16 or float (fp32 residual streams / fp32 consumers); SPLIT (TOut = bf16, plain store): the result leaves as a
// split-bf16 pair row [hi | lo] (OMP_BF16X2: hi at column n, lo at column N + n), the storage format of the bf16x3 engine.
#include "gemm_common.h"

namespace omp_gemm {
namespace {

template <typename TOut, int SM, bool SPLIT = false>   // SM: OMP_STORE_PLAIN, or the blocked K / V^T slabs of the cross-attention memory
__global__ __launch_bounds__(512, 2) void gemm_256(GemmP p) {
  typedef bf16_t T;
  constexpr bool F32O = sizeof(TOut) == 4;
  static_assert(!(F32O && SM != OMP_STORE_PLAIN), "fp32 K / V^T slabs stay on gemm_dma");
  static_assert(!(SPLIT && F32O), "split rows / split-plane slabs: bf16 storage");
  typedef bf16x8 frag;
  constexpr int ROWB = 128;            // bytes of K per LDS row
  constexpr int HALF = 128 * ROWB;     // one DMA half tile: 128 rows
  constexpr int BUF = 4 * HALF;        // X-lo | X-hi | W-lo | W-hi
  constexpr int ES = 68;               // epilogue row pitch (floats)
  constexpr int EWAVE = 64 * ES * 4;   // epilogue bytes per wave (64 rows)
  extern __shared__ __attribute__((aligned(16))) char smem[];   // max(2 * BUF, 8 * EWAVE)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int nwg = p.tiles_m * p.tiles_n;
  const int lid = xcd_remap(blockIdx.x, nwg);
  const int tm = lid / p.tiles_n, tn = lid % p.tiles_n;
  const int64_t m0 = (int64_t)tm * 256;
  const int n0 = tn * 256;
  const int nk = p.K / 64;

  // ---- DMA: a half tile = 16 wave instructions of 8 rows x 128 B; every wave issues 2 of each half tile ----------
  const int lr = lane >> 3, lc = (lane & 7) ^ lr;
  const T* Xb = reinterpret_cast<const T*>(p.A);
  const T* Wb = reinterpret_cast<const T*>(p.W);
  int64_t xoff[2][2], woff[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int64_t gm = m0 + h * 128 + wave * 16 + j * 8 + lr; if (gm > p.M - 1) gm = p.M - 1;
      int gn = n0 + h * 128 + wave * 16 + j * 8 + lr; if (gn > p.N - 1) gn = p.N - 1;
      xoff[h][j] = gm * p.lda + lc * 8;
      woff[h][j] = (int64_t)gn * p.ldw + lc * 8;
    }
  auto issue_x = [&](int kt, int h) {
    char* dst = smem + (kt & 1) * BUF + h * HALF + wave * 16 * ROWB;
    int ka = kt * 64;
    if (p.a_wrap > 0 && ka >= p.a_wrap) ka -= p.a_wrap;   // bf16x3: K tiles beyond [hi | lo] re-read the hi plane
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Xb + xoff[h][j] + ka),
                                       (__attribute__((address_space(3))) void*)(dst + j * 8 * ROWB), 16, 0, 0);
  };
  auto issue_w = [&](int kt, int h) {
    char* dst = smem + (kt & 1) * BUF + (2 + h) * HALF + wave * 16 * ROWB;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Wb + woff[h][j] + kt * 64),
                                       (__attribute__((address_space(3))) void*)(dst + j * 8 * ROWB), 16, 0, 0);
  };

  // epilogue role: 16-byte column chunk (lane & 7) of rows (lane >> 3) + 8 * it; its bias is requested now
  const int ncol = n0 + wn * 64 + (lane & 7) * 8;
  const float* bias = (SM == OMP_STORE_VBLK) ? nullptr : p.bias;   // V^T slabs: rows are features, the bias follows m
  // per-position bias table of the decoders' q / k projections (row *bias_row, a device scalar: hipGraph-replayable)
  if (bias != nullptr && p.bias_row != nullptr) bias += (int64_t)(*p.bias_row) * p.bias_row_stride;
  const bool bias_vec = bias != nullptr && ncol + 8 <= p.N && (reinterpret_cast<uintptr_t>(bias) & 15) == 0;
  const float* bsrc = bias_vec ? bias + ncol : reinterpret_cast<const float*>(p.W);
  const f32x4 braw0 = *reinterpret_cast<const f32x4*>(bsrc);
  const f32x4 braw1 = *reinterpret_cast<const f32x4*>(bsrc + 4);

  // ---- prologue: K tile 0 whole, W halves of K tile 1 (its X halves are requested in phases 0 and 1) ----------------
  issue_x(0, 0); issue_x(0, 1); issue_w(0, 0); issue_w(0, 1);
  if (nk > 1) { issue_w(1, 0); issue_w(1, 1); }

  f32x4 acc[2][2][4][2];   // [X sub-block a][W sub-block b][row fragment i][column fragment j]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lrow = lane & 15, lg = lane >> 4;
  // fragment addresses inside a buffer: row r of a half tile, 16-byte chunk c -> r * 128 + ((c ^ (r & 7)) << 4);
  // all fragment rows are 16-row aligned + lrow, so (r & 7) == (lrow & 7)
  const int sw0 = ((0 * 4 + lg) ^ (lrow & 7)) << 4, sw1 = ((1 * 4 + lg) ^ (lrow & 7)) << 4;
  const int xbase = wm * HALF + lrow * ROWB;                                  // + (a * 64 + i * 16) * ROWB
  const int wbase = (2 + (wn >> 1)) * HALF + ((wn & 1) * 64 + lrow) * ROWB;   // + (b * 32 + j * 16) * ROWB
  frag fx[4][2], fw[2][2][2];   // X sub-block in use: [i][k-step]; both W sub-blocks: [b][j][k-step]

  if (nk > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                 // K tile 0 has landed everywhere
  if (wm == 1) __builtin_amdgcn_s_barrier();    // stagger: group 1 runs one segment behind group 0
  __builtin_amdgcn_sched_barrier(0);

  auto load_x = [&](const char* buf, int a) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const char* r = buf + xbase + (a * 64 + i * 16) * ROWB;
      fx[i][0] = *reinterpret_cast<const frag*>(r + sw0);
      fx[i][1] = *reinterpret_cast<const frag*>(r + sw1);
    }
  };
  auto load_w = [&](const char* buf) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const char* r = buf + wbase + (b * 32 + j * 16) * ROWB;
        fw[b][j][0] = *reinterpret_cast<const frag*>(r + sw0);
        fw[b][j][1] = *reinterpret_cast<const frag*>(r + sw1);
      }
  };
  auto quad = [&](auto A_, auto B_) {
    constexpr int a = decltype(A_)::value, b = decltype(B_)::value;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[a][b][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[b][j][s], fx[i][s], acc[a][b][i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  typedef std::integral_constant<int, 0> I0;
  typedef std::integral_constant<int, 1> I1;

  for (int t = 0; t < nk; ++t) {
    const char* buf = smem + (t & 1) * BUF;
    // phase 0: fragments of both W sub-blocks and X sub-block 0; request X-lo of K tile t+1; quadrant (0, 0)
    load_w(buf);
    load_x(buf, 0);
    if (t + 1 < nk) issue_x(t + 1, 0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    quad(I0(), I0());
    __builtin_amdgcn_s_barrier();
    // phase 1: request X-hi of K tile t+1; quadrant (0, 1)
    if (t + 1 < nk) issue_x(t + 1, 1);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    quad(I0(), I1());
    __builtin_amdgcn_s_barrier();
    // phase 2: fragments of X sub-block 1; request W-lo of K tile t+2 (the W fragments of K tile t were read two
    // phases ago); quadrant (1, 1)
    load_x(buf, 1);
    if (t + 2 < nk) issue_w(t + 2, 0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    quad(I1(), I1());
    __builtin_amdgcn_s_barrier();
    // phase 3: request W-hi of K tile t+2; retire K tile t+1 (everything but the two W halves just requested);
    // quadrant (1, 0)
    if (t + 2 < nk) {
      issue_w(t + 2, 1);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    quad(I1(), I0());
    __builtin_amdgcn_s_barrier();
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();    // balance the stagger: every wave has passed the same number of barriers
  __builtin_amdgcn_sched_barrier(0);

  // ---- epilogue: two 64-row halves per wave through a wave-private LDS region ----------------------------------------
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
  const int erow = lane >> 3, ecol = (lane & 7) * 8;
  const bool col_ok = ncol + 8 <= p.N;
  auto half = [&](auto A_, auto ACT) {
    constexpr int a = decltype(A_)::value;
    const int64_t mrow0 = m0 + wm * 128 + a * 64;
    u32x4 rres[8][F32O ? 2 : 1];   // 8 residual values per row chunk: 16 B (bf16) / 32 B (fp32)
    if (res != nullptr && col_ok) {
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        int64_t m = mrow0 + it * 8 + erow; if (m > p.M - 1) m = p.M - 1;
        rres[it][0] = *reinterpret_cast<const u32x4*>(res + m * p.ldr + ncol);
        if constexpr (F32O) rres[it][1] = *reinterpret_cast<const u32x4*>(res + m * p.ldr + ncol + 4);
      }
    }
    float brow[8];
    if constexpr (SM == OMP_STORE_VBLK) {
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        int64_t m = mrow0 + it * 8 + erow; if (m > p.M - 1) m = p.M - 1;
        brow[it] = p.bias != nullptr ? p.bias[m] : 0.f;
      }
    }
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          *reinterpret_cast<f32x4*>(E + (i * 16 + lrow) * ES + b * 32 + j * 16 + lg * 4) = acc[a][b][i][j];
    // the region is private to this wave: LDS operations of one wave complete in order, the compiler's own
    // lgkmcnt waits cover the read-after-write below
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int r = it * 8 + erow;
      const int64_t m = mrow0 + r;
      const f32x4 t0 = *reinterpret_cast<const f32x4*>(E + r * ES + ecol);
      const f32x4 t1 = *reinterpret_cast<const f32x4*>(E + r * ES + ecol + 4);
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
        // K slab [nl][b][h][Mpad][64]: row m = memory token (image b, key ml); the 8 columns are 8 dims of one head
        if (m < p.M && col_ok) {
          const int d = p.kv_nH * 64;
          const int b = (int)(m / p.kv_tok), ml = (int)(m - (int64_t)b * p.kv_tok);
          const int nl = ncol / d, h = (ncol - nl * d) >> 6, dd = ncol & 63;
          if constexpr (SPLIT) {   // split planes: block ml / 32 = [hi plane 32 x 64 | lo plane] (the parity engine's slabs)
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
        // V^T slab [nl][b][h][Mpad/32][64][32] (swapped operands: row m = value feature, the 8 columns are 8 memory
        // tokens of one image, kv_tok % 8 == 0): inside a 32-key block slot 8g + 4 half + r <-> key 16 half + 4g + r,
        // so keys 8j .. 8j+3 and 8j+4 .. 8j+7 are two runs of 4 slots, 8 slots apart
        if (m < p.M && col_ok) {
          const int d = p.kv_nH * 64;
          const int nl = (int)(m / d), h = ((int)(m - (int64_t)nl * d)) >> 6, dd = (int)m & 63;
          const int b = ncol / p.kv_tok, ml = ncol - b * p.kv_tok;
          const int blk = ml >> 5, j = (ml & 31) >> 3;
          if constexpr (SPLIT) {
            TOut* dst = C + (((((int64_t)nl * p.kv_B + b) * p.kv_nH + h) * (p.kv_mpad >> 5) + blk) * 2) * 2048 + dd * 32 + (j & 1) * 16 + (j >> 1) * 4;
            bf16x4 h0, h1, l0, l1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              h0[q] = (bf16_t)v[q]; l0[q] = (bf16_t)(v[q] - (float)h0[q]);
              h1[q] = (bf16_t)v[4 + q]; l1[q] = (bf16_t)(v[4 + q] - (float)h1[q]);
            }
            *reinterpret_cast<bf16x4*>(dst) = h0;
            *reinterpret_cast<bf16x4*>(dst + 8) = h1;
            *reinterpret_cast<bf16x4*>(dst + 2048) = l0;
            *reinterpret_cast<bf16x4*>(dst + 2048 + 8) = l1;
          } else {
            TOut* dst = C + ((((int64_t)nl * p.kv_B + b) * p.kv_nH + h) * (p.kv_mpad >> 5) + blk) * 2048 + dd * 32 + (j & 1) * 16 + (j >> 1) * 4;
            *reinterpret_cast<bf16x4*>(dst) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
            *reinterpret_cast<bf16x4*>(dst + 8) = bf16x4{(bf16_t)v[4], (bf16_t)v[5], (bf16_t)v[6], (bf16_t)v[7]};
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
  };
  auto both = [&](auto ACT) { half(I0(), ACT); half(I1(), ACT); };
  if (p.act == OMP_ACT_GELU) both(std::integral_constant<int, OMP_ACT_GELU>());
  else if (p.act == OMP_ACT_RELU) both(std::integral_constant<int, OMP_ACT_RELU>());
  else both(std::integral_constant<int, OMP_ACT_NONE>());
}

template <typename TOut, int SM, bool SPLIT = false>
int launch_256_sm(GemmP& p, hipStream_t st) {
  constexpr size_t smem = 8 * 64 * 68 * 4;   // 139264 B: the epilogue regions; the two operand buffers take 131072 B
  constexpr auto kern = gemm_256<TOut, SM, SPLIT>;
  if (const int rc = omp_raise_lds<kern>("omp_gemm_bias_act")) return rc;
  p.tiles_m = (int)ceil_div64(p.M, 256); p.tiles_n = (int)ceil_div64(p.N, 256);
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n), dim3(512), smem, st, p);
  return OMP_OK;
}

template <typename TOut>
int launch_256(GemmP& p, hipStream_t st) {
  if constexpr (sizeof(TOut) == 2) {
    if (p.store_mode == OMP_STORE_KBLK) return p.split_out ? launch_256_sm<TOut, OMP_STORE_KBLK, true>(p, st) : launch_256_sm<TOut, OMP_STORE_KBLK>(p, st);
    if (p.store_mode == OMP_STORE_VBLK) return p.split_out ? launch_256_sm<TOut, OMP_STORE_VBLK, true>(p, st) : launch_256_sm<TOut, OMP_STORE_VBLK>(p, st);
    if (p.split_out) return launch_256_sm<TOut, OMP_STORE_PLAIN, true>(p, st);
  }
  return launch_256_sm<TOut, OMP_STORE_PLAIN>(p, st);
}

}  // namespace

int gemm256_launch(GemmP& p, bool f32_out, hipStream_t st) { return f32_out ? launch_256<float>(p, st) : launch_256<bf16_t>(p, st); }

}  // namespace omp_gemm
