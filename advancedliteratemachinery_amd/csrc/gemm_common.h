// What more than one GEMM unit needs (internal: gemm.hip and the tile-kernel units gemm256.hip, gemm4w.hip, gemm4wr.hip, gemm4wp.hip):
// the parameter block, the shared device helpers, the host predicates of the tile kernels and the launch entry points of their units.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace omp_gemm {

struct GemmP {
  const void* A; int64_t lda;
  const void* W; int64_t ldw;
  const float* bias; const int32_t* bias_row; int64_t bias_row_stride;
  int bias_row_mod, bias_row_off;                       // > 0: the table's per-row form -- row m takes table row (bias_row_off + m) % bias_row_mod (gemm_dma, gemm_small)
  const void* residual; int64_t ldr;
  void* C; int64_t ldc;
  int64_t M; int N; int K;
  int act; int trans_out; int64_t trans_rows, trans_ld;
  int tiles_m, tiles_n; int small_hint;
  const float* ln_g; const float* ln_b; float ln_eps;   // optional LayerNorm prologue (A is fp32)
  int store_mode; int bias_m;                           // OMP_STORE_*; bias indexed by m instead of n
  int kv_B, kv_tok, kv_mpad, kv_nH, kv_kb;              // blocked K / V^T destination geometry
  void* C2; int64_t ldc2;                               // optional second destination without the residual
  int a_wrap;                                           // > 0: A rows are split-bf16 pairs [hi | lo] of a_wrap elements, K columns beyond wrap back (bf16x3)
  int split_out;                                        // bf16 destination written as split pairs: hi at column n, lo at column N + n
  unsigned long long* trace;                            // debug: per-workgroup phase timestamps (gemm_dma<..., TRACE>)
};

// bf16 destinations take the bf16 engine's GELU everywhere (vectorised or not: a value must not depend on which
// kernel or epilogue path produced it), fp32 destinations the < 1 ulp erf form
template <typename TOut>
__device__ __forceinline__ float apply_act(float v, int act, bool precise = false) {
  if (act == OMP_ACT_GELU) {
    if constexpr (std::is_same<TOut, bf16_t>::value) return precise ? gelu_erf(v) : gelu_fast2(f32x2{v, 0.0f})[0];
    else return gelu_erf(v);
  }
  if (act == OMP_ACT_RELU) return fmaxf(v, 0.0f);
  return v;
}

// Store 4 consecutive-n values v (bias and activation already applied) of token m: adds the residual and
// honours the destination layout (plain / transposed / blocked K / blocked V^T).
template <typename TOut>
__device__ __forceinline__ void store4(const GemmP& p, int64_t m, int n, const float* vin) {
  if (m >= p.M || n >= p.N) return;
  const TOut* res = reinterpret_cast<const TOut*>(p.residual);
  TOut* C = reinterpret_cast<TOut*>(p.C);
  float v[4] = {vin[0], vin[1], vin[2], vin[3]};
  if (p.store_mode == OMP_STORE_KBLK) {
    // m = memory token (image b, key ml), n..n+3 = 4 dims of one head of one (decoder, layer) slab:
    // K slab [nl][b][h][Mpad][64]
    const int d = p.kv_nH * 64;
    const int b = (int)(m / p.kv_tok), ml = (int)(m % p.kv_tok);
    const int nl = n / d, h = (n % d) >> 6, dd = n & 63;
    if constexpr (sizeof(TOut) == 2) {
      if (p.split_out) {   // split planes: block ml / 32 = [hi plane 32 x 64 | lo plane]
        TOut* dst = C + (((((int64_t)nl * p.kv_B + b) * p.kv_nH + h) * (p.kv_mpad >> 5) + (ml >> 5)) * 2) * 2048 + (ml & 31) * 64 + dd;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < p.N) {
            const bf16_t hi = (bf16_t)v[r];
            dst[r] = hi;
            dst[2048 + r] = (bf16_t)(v[r] - (float)hi);
          }
        return;
      }
    }
    TOut* dst = C + ((((int64_t)nl * p.kv_B + b) * p.kv_nH + h) * p.kv_mpad + ml) * 64 + dd;
    if (n + 3 < p.N) {
      if constexpr (sizeof(TOut) == 4) *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
      else *reinterpret_cast<bf16x4*>(dst) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < p.N) dst[r] = from_f32<TOut>(v[r]);
    }
    return;
  }
  if (p.store_mode == OMP_STORE_VBLK) {
    // swapped operands: m = value feature (decoder-layer nl, head h, dim dd), n..n+3 = 4 memory tokens.
    // V^T slab [nl][b][h][Mpad/KB][64][KB]; inside a block the KB keys sit in the order the PV matrix-core
    // product consumes them (bf16: slot 8g + 4*half + r <-> key 16*half + 4g + r; f32: natural order).
    const int d = p.kv_nH * 64, KB = p.kv_kb;
    const int nl = (int)(m / d), h = (int)(m % d) >> 6, dd = (int)m & 63;
    const int PLN = (sizeof(TOut) == 2 && p.split_out) ? 2 : 1;   // split planes: a block is [hi plane 64 x KB | lo plane]
    auto slot = [&](int tok, int& b) -> int64_t {
      b = tok / p.kv_tok;
      const int ml = tok - b * p.kv_tok;
      const int blk = ml / KB, kl = ml - blk * KB;
      const int pos = (KB == 32) ? (((kl & 15) >> 2) * 8 + (kl >> 4) * 4 + (kl & 3)) : kl;
      return ((((int64_t)nl * p.kv_B + b) * p.kv_nH + h) * (p.kv_mpad / KB) + blk) * (64 * KB * PLN) + dd * KB + pos;
    };
    // element by element (split planes; tokens per image not a multiple of 4: MGP-STR's 257): ONE division for the 4 tokens -- (image, key) of the
    // first, then walked -- instead of three per element (round 6: the V^T projection of a ViT block spent 540 us here against 200 for the product)
    auto walk = [&](auto&& put) {
      int b = n / p.kv_tok, ml = n - b * p.kv_tok;
      const int64_t per_head = (int64_t)(p.kv_mpad / KB) * (64 * KB * PLN);
      int64_t base = (((int64_t)nl * p.kv_B + b) * p.kv_nH + h) * per_head + dd * KB;
      const int sh = KB == 32 ? 5 : 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (n + r < p.N) {
          const int blk = ml >> sh, kl = ml & (KB - 1);
          const int pos = (KB == 32) ? (((kl & 15) >> 2) * 8 + (kl >> 4) * 4 + (kl & 3)) : kl;
          put(base + (int64_t)blk * (64 * KB * PLN) + pos, r);
        }
        if (++ml == p.kv_tok) { ml = 0; base += (int64_t)p.kv_nH * per_head; }
      }
    };
    if constexpr (sizeof(TOut) == 2) {
      if (p.split_out) {
        walk([&](int64_t i, int r) {
          const bf16_t hi = (bf16_t)v[r];
          C[i] = hi;
          C[i + 64 * KB] = (bf16_t)(v[r] - (float)hi);
        });
        return;
      }
    }
    if (n + 3 < p.N && (p.kv_tok & 3) == 0) {   // 4 tokens of one image, contiguous slots
      int b0;
      const int64_t i0 = slot(n, b0);
      if constexpr (sizeof(TOut) == 4) *reinterpret_cast<f32x4*>(C + i0) = f32x4{v[0], v[1], v[2], v[3]};
      else *reinterpret_cast<bf16x4*>(C + i0) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    } else {
      walk([&](int64_t i, int r) { C[i] = from_f32<TOut>(v[r]); });
    }
    return;
  }
  if (p.trans_out) {
    int64_t bidx = m / p.trans_rows, mi = m % p.trans_rows;
    TOut* base = C + bidx * (int64_t)p.N * p.trans_ld + mi;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < p.N) base[(int64_t)(n + r) * p.trans_ld] = from_f32<TOut>(v[r]);
    return;
  }
  if constexpr (sizeof(TOut) == 2) {
    if (p.split_out) {   // split-bf16 pair rows (no residual: checked on the host)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < p.N) {
          const bf16_t hi = (bf16_t)v[r];
          C[m * p.ldc + n + r] = hi;
          C[m * p.ldc + p.N + n + r] = (bf16_t)(v[r] - (float)hi);
        }
      return;
    }
  }
  const bool full = (n + 3 < p.N) && ((p.ldc & 3) == 0) && (res == nullptr || (p.ldr & 3) == 0);
  if (full) {
    if (res != nullptr) {
      if constexpr (sizeof(TOut) == 4) {
        f32x4 rv = *reinterpret_cast<const f32x4*>(res + m * p.ldr + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += rv[r];
      } else {
        bf16x4 rv = *reinterpret_cast<const bf16x4*>(res + m * p.ldr + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
      }
    }
    if constexpr (sizeof(TOut) == 4) {
      f32x4 o = {v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(C + m * p.ldc + n) = o;
    } else {
      bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
      *reinterpret_cast<bf16x4*>(C + m * p.ldc + n) = o;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (n + r < p.N) {
        float o = v[r];
        if (res != nullptr) o += to_f32(res[m * p.ldr + n + r]);
        C[m * p.ldc + n + r] = from_f32<TOut>(o);
      }
    }
  }
}

// bias + activation of the 4 consecutive-n values a lane holds for token m, then store4.
template <typename TOut>
__device__ __forceinline__ void epilogue_store(const GemmP& p, const float* bias, int64_t m, int n,
                                               f32x4 acc) {
  if (m >= p.M || n >= p.N) return;
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float b = 0.0f;
    if (bias != nullptr) b = p.bias_m ? bias[m] : (n + r < p.N ? bias[n + r] : 0.0f);
    v[r] = apply_act<TOut>(acc[r] + b, p.act);
  }
  store4<TOut>(p, m, n, v);
}

// bijective XCD remap: consecutive logical tile ids land on the same XCD (block b runs on XCD b%8)
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  const int start = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return start + idx;
}

// wait until at most `tiles` of this wave's most recently issued K tiles (IPT DMA instructions each) are
// still in flight; the count must be an immediate, hence the switch (wave-uniform, so one scalar branch)
template <int IPT>
__device__ __forceinline__ void wait_dma_tiles(int tiles) {
  static_assert(IPT * 7 <= 63, "vmcnt immediate out of range");
  switch (tiles) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPT * 1) : "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPT * 2) : "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPT * 3) : "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPT * 4) : "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPT * 5) : "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPT * 6) : "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPT * 7) : "memory"); break;
  }
}

// compile-time loops: f(std::integral_constant<int, 0>()), f(<1>), ... (the four-wave kernels name registers and DMA pieces by number)
template <int... I, class F>
__device__ __forceinline__ void static_for_seq(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>()), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_seq(std::make_integer_sequence<int, N>(), f); }

// the 256 accumulator registers by name (asm clobber list: the kernel descriptor then allocates them and the compiler keeps out)
#define OMP_A4(n) "a" #n "0", "a" #n "1", "a" #n "2", "a" #n "3", "a" #n "4", "a" #n "5", "a" #n "6", "a" #n "7", "a" #n "8", "a" #n "9"
#define OMP_ALL_AGPRS                                                                                                                   \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", OMP_A4(1), OMP_A4(2), OMP_A4(3), OMP_A4(4), OMP_A4(5), OMP_A4(6), OMP_A4(7),   \
      OMP_A4(8), OMP_A4(9), OMP_A4(10), OMP_A4(11), OMP_A4(12), OMP_A4(13), OMP_A4(14), OMP_A4(15), OMP_A4(16), OMP_A4(17), OMP_A4(18), \
      OMP_A4(19), OMP_A4(20), OMP_A4(21), OMP_A4(22), OMP_A4(23), OMP_A4(24), "a250", "a251", "a252", "a253", "a254", "a255"

// ---------------------------------------------------------------------------------------------
// Host side: the products each tile kernel takes (gemm_accepts and gemm_auto_select in gemm.hip ask here) ...
// ---------------------------------------------------------------------------------------------
// shapes gemm_256 (gemm256.hip) takes (everything else stays on gemm_dma)
inline bool gemm256_ok(const GemmP& p, bool bf16_in, bool bf16_out) {
  if (!(bf16_in && !p.trans_out && (p.bias_row == nullptr || (p.bias_row_stride % 4) == 0) && p.ln_g == nullptr && p.K % 64 == 0 && p.K >= 128 && p.N % 8 == 0 &&
        (p.a_wrap == 0 || p.a_wrap % 64 == 0)))
    return false;
  if (p.store_mode == OMP_STORE_PLAIN)
    return !p.bias_m && (p.ldc % 8) == 0 && (p.residual == nullptr || (p.ldr % 8) == 0) && (p.C2 == nullptr || (p.ldc2 % 8) == 0) &&
           (!p.split_out || (bf16_out && p.residual == nullptr));
  if (!bf16_out) return false;
  // blocked cross-attention memory (bf16 or split planes): 32-key blocks, whole 8-token chunks inside one image, no residual / activation
  if (p.kv_kb != 32 || p.residual != nullptr || p.act != OMP_ACT_NONE || p.C2 != nullptr) return false;
  if (p.store_mode == OMP_STORE_KBLK) return !p.bias_m && p.N % 64 == 0;
  if (p.store_mode == OMP_STORE_VBLK) return (p.bias == nullptr || p.bias_m) && p.kv_tok % 8 == 0;
  return false;
}

// shapes gemm_4w (gemm4w.hip) takes: those of gemm_256 (its stages are 32 deep, but the library's K granularity stays 64) and K = 64
inline bool gemm4w_ok(const GemmP& p, bool bf16_in, bool bf16_out) {
  if (p.K == 64) {   // two stages: fewer than the ring holds, handled by the prologue / tail guards
    GemmP q = p;
    q.K = 128;
    return gemm256_ok(q, bf16_in, bf16_out);
  }
  return gemm256_ok(p, bf16_in, bf16_out);
}

// shapes gemm_4w_r (gemm4wr.hip) takes: row-major destinations of gemm_256 with K a multiple of four 64-deep stages
inline bool gemm4wr_ok(const GemmP& p, bool bf16_in, bool bf16_out) {
  return p.store_mode == OMP_STORE_PLAIN && p.K % 256 == 0 && gemm256_ok(p, bf16_in, bf16_out);
}

// shapes gemm_4w_p (gemm4wp.hip) takes: gemm_4w_r's without ragged edges, bias readable as 16-byte vectors
inline bool gemm4wp_ok(const GemmP& p, bool bf16_in, bool bf16_out) {
  if (!gemm4wr_ok(p, bf16_in, bf16_out)) return false;
  if (p.M % 256 != 0 || p.N % 256 != 0) return false;
  if (p.bias != nullptr && ((reinterpret_cast<uintptr_t>(p.bias) & 15) != 0 || (p.bias_row != nullptr && p.bias_row_stride % 4 != 0))) return false;
  const int esz = bf16_out ? 2 : 4;
  if ((reinterpret_cast<uintptr_t>(p.C) % (4 * esz)) != 0 || (p.ldc * esz) % (4 * esz) != 0) return false;
  if (p.residual != nullptr && ((reinterpret_cast<uintptr_t>(p.residual) % (4 * esz)) != 0 || p.ldr % 4 != 0)) return false;
  if (p.C2 != nullptr && ((reinterpret_cast<uintptr_t>(p.C2) % (4 * esz)) != 0 || p.ldc2 % 4 != 0)) return false;
  return true;
}

// the fused three-product kernel (gemm_4w_p<..., X3>): bf16x3 operands of a shape gemm_4w_p takes (K = 3 K0 a multiple of 256, i.e. K0 % 256 == 0; the
// kernel itself needs an even number of 64-deep chunks, K0 % 128 == 0)
inline bool gemm4wx3_ok(const GemmP& p, bool bf16_in, bool bf16_out) {
  return p.a_wrap > 0 && (p.a_wrap % 2) == 0 && p.K == 3 * (p.a_wrap / 2) && (p.a_wrap / 2) % 128 == 0 && gemm4wp_ok(p, bf16_in, bf16_out) &&
         (bf16_out ? p.split_out != 0 : true);
}

// ... and the launch entry points of the tile-kernel units, one per selector group (gemm_launch_sel in gemm.hip; bf16 operands throughout).
// Each raises its kernel's LDS limit, sets p.tiles_m / p.tiles_n and launches on `st`; f32_out chooses the fp32 instantiations, p.store_mode and
// p.split_out the destination layout.  `abl` is the development variant of the kernel template (ABL); a selector that is not built for the
// destination type answers gemm_not_built().
inline int gemm_not_built(int which) {
  omp_set_error("omp_gemm_bias_act: kernel selector %d is not built for these types", which);   // gemm_accepts refuses them first
  return OMP_ERR_INVALID;
}
int gemm256_launch(GemmP& p, bool f32_out, hipStream_t st);                    // 9 (gemm256.hip)
int gemm4w_launch(GemmP& p, bool f32_out, hipStream_t st);                     // 10, 11 (gemm4w.hip)
int gemm4w_launch_ablation(GemmP& p, bool f32_out, hipStream_t st, int abl);   // 12..14: abl = 1..3, bf16 destinations
int gemm4wr_launch(GemmP& p, bool f32_out, hipStream_t st);                    // 16 (gemm4wr.hip)
int gemm4wr_launch_dev(GemmP& p, bool f32_out, hipStream_t st, int abl);       // 17: abl = 3 (no MFMAs, bf16 destinations); 18: abl = 4 (timestamps)
int gemm4wp_launch(GemmP& p, bool f32_out, hipStream_t st);                    // 20 (gemm4wp.hip)
int gemm4wp_launch_ablation(GemmP& p, bool f32_out, hipStream_t st, int abl);  // 21: abl = 5, fp32 destinations
int gemm4wx3_launch(GemmP& p, bool f32_out, hipStream_t st);                   // 22

}  // namespace omp_gemm
