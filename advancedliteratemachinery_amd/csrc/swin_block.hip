// Attention half of a Swin block in ONE kernel, for Swin-B stage 0 (C = 128, 4 heads of 32) and stage 1 (C = 256, 8 heads):
//     x <- x + proj(window_attention(qkv(LayerNorm(x))))        (reference swin_transformer.py:196-253, first residual)
// The unfused chain moves 4.6 KB per token through HBM at C = 128 (LN 0.75 + qkv 1.0 + attention 1.0 + proj 1.25 ... of reads and
// writes); here a token's fp32 row is read once and written once, q / k / v / P / O never leave the CU.
//
// swin_block_kernel<S, TRACE> is one source for both stages; the policy S (Stage0 / Stage1) says what differs.  One persistent
// workgroup per CU, 8 waves = S::GROUPS windows in flight x S::HEADS heads.  Per window, the same for both:
//   * LayerNorm of its 49 tokens (fp32 rows fetched one window AHEAD; C / 16 lanes per token, DPP sums) -> bf16 tile [64][C] in
//     LDS, chunk-swizzled (16-byte chunk c of row r at slot c ^ (r & 15)) so that every MFMA fragment is one conflict-free
//     ds_read_b128 (rows of padding tokens and rows 49..63 are zero: the reference pads AFTER norm1, so their q / k / v are the bias)
//   * each wave produces its head's
//       k^T = Wk X^T,  q^T = Wq X^T   (accumulator layout [dim 4g+r][token li]  == the operand layout of S^T = K Q^T, up to a
//                                      permutation of the 32 dims that K and Q share)
//       v   = X Wv^T                  (accumulator layout [token 4g+r][dim li]  == the A operand of O^T = V^T P with the key
//                                      order the S^T accumulators give P)
//     so the whole attention (same arithmetic as swin_attn_mfma_kernel<bf16, EXPB>: expanded bias seeds, base-2 softmax,
//     SW-MSA regions only on edge windows) runs out of registers, no LDS round trip
//   * O (bf16) goes through the same LDS tile to become the proj operand; out^T = Wp O^T + b + x is stored as 16-byte
//     pieces straight into the residual stream (in place: a window touches only its own tokens)
//   * the four phase barriers per window order LDS traffic only (lds_barrier): the rows in flight for the next window and
//     the residual / proj-weight loads are never drained at a barrier
// Where the weights come from is the difference:
//   * Stage0: the qkv weights (384 x 128 bf16 = 96 KB) sit in LDS for the life of the workgroup, swizzled like the tile; a workgroup
//     takes two windows.  The proj weights of the wave's 32 output channels (8 fragments, L2-resident) are re-fetched per window
//     together with the residual rows -- held across windows they cost 32 of the 256 registers a wave has at two waves per SIMD, and
//     the kernel spilled
//   * Stage1: 393 KB of qkv weights + 128 KB of proj weights fit neither LDS nor registers: a workgroup is ONE window x 8 heads, and
//     every wave streams its head's operand fragments straight from the fragment-major image written by
//     model/packing.py::pack_attn_block (1 KB contiguous per fragment, L2-resident, one k-step ahead of the matrix cores).  The
//     products run k-step-outer so that only the four token fragments of one k-step are live.
// Biases and the norm1 vectors sit in LDS behind the tiles (6 C floats).
// Measured (profiles/r03o_kbench_swin_block.txt): 32 images of 256 x 256 tokens at C = 128, 2.26 ms for the four launches -> 1.11 ms;
// instruction-issue-bound (about 2 900 instructions per wave and window), HBM floor 0.36 ms.  Device code of both instantiations
// against the two separate kernels they replace: profiles/r12a_swin_block_isa.txt.

#include "common.h"
#include "swin_common.h"

namespace {

struct SwinGeo { int B, H, W, shift, nWy, nWx, n_win; };

struct SwinBlockP {                      // stage 0: the weights as the model holds them
  const float* x; float* out;
  const float* ln_g; const float* ln_b; float eps;
  const bf16_t* qkv_w; const float* qkv_b;
  const float* bias_exp;                 // [heads][64 queries][64 keys] (omp_swin_expand_bias)
  const bf16_t* proj_w; const float* proj_b;
  SwinGeo geo;
  unsigned long long* trace;             // development: per-workgroup phase cycle sums (TRACE instantiation)
};
struct SwinBlockPackedP {                // stage 1: qkv and proj weights as the fragment-major image of pack_attn_block
  const float* x; float* out;
  const float* ln_g; const float* ln_b; float eps;
  const bf16_t* wpack; const float* qkv_b;
  const float* bias_exp;
  const float* proj_b;
  SwinGeo geo;
  unsigned long long* trace;
};

// The two instantiations.  A tile row holds C bf16 (PITCH bytes); LayerNorm spreads a token's C fp32 over LN_LANES lanes of 16 values.
struct Stage0 {
  typedef SwinBlockP P;
  static constexpr int C = 128, HEADS = 4, GROUPS = 2, W_BYTES = 384 * 256;   // W_BYTES: the resident qkv image
  static constexpr const char* NAME = "omp_swin_attn_block";
  static constexpr const char* WEIGHTS = "qkv_w / proj_w";
};
struct Stage1 {
  typedef SwinBlockPackedP P;
  static constexpr int C = 256, HEADS = 8, GROUPS = 1, W_BYTES = 0;
  static constexpr const char* NAME = "omp_swin_attn_block_packed";
  static constexpr const char* WEIGHTS = "wpack";
};
template <class S> constexpr int PITCH = S::C * 2;
template <class S> constexpr int LN_LANES = S::C / 16;
template <class S> constexpr int KSTEPS = S::C / 32;
template <class S> constexpr int TILE_BYTES = 64 * PITCH<S>;
template <class S> constexpr int VEC_FLOATS = 6 * S::C;   // qkv bias | proj bias | norm1 gamma | norm1 beta, fp32 in LDS
template <class S> constexpr int LDS_BYTES = S::W_BYTES + S::GROUPS * TILE_BYTES<S> + VEC_FLOATS<S> * 4;

__device__ __forceinline__ int sw_off(int row, int chunk) { return row * 256 + ((chunk ^ (row & 15)) << 4); }

struct Win { int b, wy, wx; };
__device__ __forceinline__ Win win_decode(const SwinGeo& p, int widx) {
  Win w;
  w.wx = widx % p.nWx;
  const int r = widx / p.nWx;
  w.wy = r % p.nWy; w.b = r / p.nWy;
  return w;
}
// window-local token t (< 64; callers mask t >= 49) -> row of x (or -1: padding token); sy / sx = its place in the shifted grid
__device__ __forceinline__ int64_t win_token(const SwinGeo& p, const Win& w, int t, int& sy, int& sx) {
  const int Hp = p.nWy * WS, Wp = p.nWx * WS;
  const int ty = (t * 37) >> 8, tx = t - ty * WS;   // t / 7 for t < 64
  sy = w.wy * WS + ty; sx = w.wx * WS + tx;
  int py = sy + p.shift, px = sx + p.shift;
  if (py >= Hp) py -= Hp;
  if (px >= Wp) px -= Wp;
  return (py < p.H && px < p.W) ? ((int64_t)w.b * p.H + py) * p.W + px : (int64_t)-1;
}

// sum over groups of N = 8 / 16 consecutive lanes on the DPP path (two quad permutes, one half-row mirror, one row mirror): no LDS traffic
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <int N>
__device__ __forceinline__ float lane_sum(float v) {
  v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);   // row_half_mirror: the other quad of the 8
  if constexpr (N == 16) v += dpp_mov<0x140>(v);   // row_mirror: the other 8 of the 16-lane row
  return v;
}

// workgroup barrier that orders LDS traffic only: __syncthreads() also drains vmcnt, i.e. it would wait at every phase boundary for
// the next window's rows (HBM latency) and for the residual / proj-weight loads issued just before it
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ bf16x8 pack8(const f32x4& a, const f32x4& b) {
  bf16x8 f = {(bf16_t)a[0], (bf16_t)a[1], (bf16_t)a[2], (bf16_t)a[3], (bf16_t)b[0], (bf16_t)b[1], (bf16_t)b[2], (bf16_t)b[3]};
  return f;
}

__device__ __forceinline__ f32x4 sum4(const f32x4 a, const f32x4 b) { return f32x4{a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]}; }

template <class S, bool TRACE>
__global__ __launch_bounds__(512, 1) void swin_block_kernel(typename S::P p) {
  typedef Mma<bf16_t> MM;
  constexpr int C = S::C, PT = PITCH<S>, LL = LN_LANES<S>, KS = KSTEPS<S>;
  constexpr bool RESIDENT = S::W_BYTES > 0;
  unsigned long long tr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto now = [&]() -> unsigned long long { if constexpr (TRACE) return __builtin_amdgcn_s_memtime(); else return 0ull; };
  const unsigned long long t_start = now();
  extern __shared__ __attribute__((aligned(16))) char lds[];   // Wqkv image (Stage0) | one tile per window group | vectors
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: address terms built on it live in SGPRs
  int grp = 0, head = wave;
  if constexpr (S::GROUPS == 2) { grp = wave >> 2; head = wave & 3; }
  const int li = lane & 15, g = lane >> 4;
  char* tile = lds + S::W_BYTES + grp * TILE_BYTES<S>;
  const float* vec = reinterpret_cast<const float*>(lds + S::W_BYTES + S::GROUPS * TILE_BYTES<S>);
  const float* v_qb = vec; const float* v_pb = vec + 3 * C; const float* v_g = vec + 4 * C; const float* v_b = vec + 5 * C;

  if constexpr (RESIDENT) {
    for (int idx = tid; idx < 384 * 16; idx += 512) {
      const int row = idx >> 4, ch = idx & 15;
      *reinterpret_cast<bf16x8*>(lds + sw_off(row, ch)) = *reinterpret_cast<const bf16x8*>(p.qkv_w + row * C + ch * 8);
    }
  }
  for (int idx = tid; idx < VEC_FLOATS<S>; idx += 512) {
    float v;
    if (idx < 3 * C) v = p.qkv_b[idx];
    else if (idx < 4 * C) v = p.proj_b[idx - 3 * C];
    else if (idx < 5 * C) v = p.ln_g[idx - 4 * C];
    else v = p.ln_b[idx - 5 * C];
    const_cast<float*>(vec)[idx] = v;
  }
  // operand fragment of tile rows R + li (R a multiple of 16), k-step ks (channels ks*32 + g*8 .. +8): byte offset R * PT + cx[ks], the row
  // term an immediate.  Stage1 walks its k-steps in a rolled loop and forms the same offset as cx0 ^ (ks << 6).  (Each stage computes only
  // its own form: with both in the source the stage-0 instruction order changes, profiles/r12a_swin_block_isa.txt.)
  [[maybe_unused]] int cx[4], cx0 = 0;
  if constexpr (RESIDENT) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) cx[ks] = li * PT + (((ks * 4 + g) ^ li) << 4);
  } else {
    cx0 = li * PT + ((g ^ li) << 4);
  }
  // Stage0: this head's rows of the q block in the LDS image; k rows + 128 * 256, v rows + 256 * 256
  [[maybe_unused]] const char* wl = nullptr;
  if constexpr (RESIDENT) wl = lds + head * 32 * 256;
  // LayerNorm: LL lanes per token (lane j of them holds the 16-byte pieces j, j + LL, j + 2 LL, j + 3 LL of the fp32 row, so one wave
  // load covers 64 / LL tokens x 16 LL contiguous bytes); wave `head` normalises tokens it*32 + head * (64 / LL) + tk, it = 0, 1
  const int tk = lane / LL, lj = lane % LL;
  const int ln_row = head * (64 / LL) + tk;                       // + 32 it
  // bf16 piece of fp32 piece c = k*LL + lj: 16-byte chunk (c >> 1), half (lj & 1); chunk ^ (row & 15), k enters as ^ (k * (LL * 8))
  const int ln_off = ln_row * PT + (((lj >> 1) ^ (ln_row & 15)) << 4) + (lj & 1) * 8;
  // O^T accumulator piece (dims dt*16 + 4g .. +4 of query t4*16 + li) -> tile[query][head*32 + dim]
  const int o_off0 = li * PT + (((head * 4 + (g >> 1)) ^ li) << 4) + (g & 1) * 8;
  const int o_off1 = li * PT + (((head * 4 + 2 + (g >> 1)) ^ li) << 4) + (g & 1) * 8;
  // Stage1: fragment (ks*6 + sel*2 + dt) of this head | fragment (nt*KS + ks) of this wave's 32 output channels
  [[maybe_unused]] const bf16_t* wq = nullptr;
  [[maybe_unused]] const bf16_t* wpj = nullptr;
  if constexpr (!RESIDENT) {
    wq = p.wpack + (int64_t)head * (KS * 6 * 512) + lane * 8;
    wpj = p.wpack + 3 * C * C + (int64_t)head * (2 * KS * 512) + lane * 8;
  }

  f32x4 xr[2][4];   // rows that are not fetched keep whatever (finite) values the registers held: their LayerNorm is discarded
#pragma unroll
  for (int it = 0; it < 2; ++it)
#pragma unroll
    for (int k = 0; k < 4; ++k) xr[it][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  unsigned ok = 0;
  Win nxt;           // the window whose rows are in flight: decoded once, used again when it becomes the current one
  auto prefetch = [&](int widx) {
    ok = 0;
    const bool live = widx < p.geo.n_win;
    nxt = win_decode(p.geo, live ? widx : 0);
    const Win w = nxt;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int t = it * 32 + ln_row;
      int sy, sx;
      const int64_t tok = win_token(p.geo, w, t, sy, sx);
      const bool rd = live && t < WT && tok >= 0;
      if (rd) {
        const float* src = p.x + tok * C + lj * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) xr[it][k] = *reinterpret_cast<const f32x4*>(src + k * (LL * 4));
        ok |= 1u << it;
      }
    }
  };

  const int Hp = p.geo.nWy * WS, Wp = p.geo.nWx * WS;
  const float scale2 = 0.17677669529663687f * 1.4426950408889634f;   // 32^-0.5 * log2(e): base-2 softmax on (q.k + bias / scale)
  const float* be_head = p.bias_exp + head * 4096;   // uniform
  const int be_lane = li * 64 + g * 4;

  int w0 = blockIdx.x * S::GROUPS;
  prefetch(w0 + grp);
  __syncthreads();   // the weight image and the vectors are complete

  for (; w0 < p.geo.n_win; w0 += gridDim.x * S::GROUPS) {
    const bool valid = S::GROUPS == 1 || w0 + grp < p.geo.n_win;
    const unsigned long long c0 = now();
    const Win win = nxt;
    const int wx = win.wx, wy = win.wy;

    // ---- LayerNorm -> bf16 tile (two-pass statistics; a row's C channels sit in LL lanes x 16 values) ------------------------
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      float s1 = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) s1 += (xr[it][k][0] + xr[it][k][1]) + (xr[it][k][2] + xr[it][k][3]);
      const float mean = lane_sum<LL>(s1) * (1.0f / C);
      float s2 = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = xr[it][k][e] - mean; s2 += d * d; }
      const float rstd = 1.0f / sqrtf(lane_sum<LL>(s2) * (1.0f / C) + p.eps);
      const bool real = (ok >> it) & 1u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(v_g + k * (LL * 4) + lj * 4);
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(v_b + k * (LL * 4) + lj * 4);
        bf16x4 y = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
        if (real) {
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = (bf16_t)((xr[it][k][e] - mean) * rstd * g4[e] + b4[e]);
        }
        *reinterpret_cast<bf16x4*>(tile + it * 32 * PT + (ln_off ^ (k * (LL * 8)))) = y;
      }
    }
    prefetch(w0 + (int)gridDim.x * S::GROUPS + grp);   // the next window's rows land while this one is computed
    const unsigned long long c1 = now();
    lds_barrier();   // B1: tile = LayerNorm(x) of the window
    const unsigned long long c2 = now();

    // ---- k^T, v, q^T of this head as operand fragments ------------------------------------------------------------------------
    bf16x8 kf[4], qf[4], vf[2][2];
    [[maybe_unused]] bf16x8 xf[4][4];   // Stage0: operand fragments of the tile, xf[tt][ks] = rows tt*16 + li, channels ks*32 + g*8 .. +8
    if constexpr (RESIDENT) {   // weights from the LDS image, one product after the other over the 16 tile fragments held in registers
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) xf[tt][ks] = *reinterpret_cast<const bf16x8*>(tile + tt * (16 * PT) + cx[ks]);
      {  // k^T [dim][token]
        f32x4 acc[2][4];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) acc[dt][tt] = *reinterpret_cast<const f32x4*>(v_qb + C + head * 32 + dt * 16 + g * 4);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wl + (C + dt * 16) * 256 + cx[ks]);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) MM::mma(acc[dt][tt], wf, xf[tt][ks]);
          }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) kf[tt] = pack8(acc[0][tt], acc[1][tt]);
      }
      {  // v [token][dim]
        f32x4 acc[4][2];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) { const float bv = v_qb[2 * C + head * 32 + dt * 16 + li]; acc[tt][dt] = f32x4{bv, bv, bv, bv}; }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wl + (2 * C + dt * 16) * 256 + cx[ks]);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) MM::mma(acc[tt][dt], xf[tt][ks], wf);
          }
#pragma unroll
        for (int ps = 0; ps < 2; ++ps)
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) vf[ps][dt] = pack8(acc[2 * ps][dt], acc[2 * ps + 1][dt]);
      }
      {  // q^T [dim][token]
        f32x4 acc[2][4];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) acc[dt][tt] = *reinterpret_cast<const f32x4*>(v_qb + head * 32 + dt * 16 + g * 4);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wl + dt * 16 * 256 + cx[ks]);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) MM::mma(acc[dt][tt], wf, xf[tt][ks]);
          }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) qf[tt] = pack8(acc[0][tt], acc[1][tt]);
      }
    } else {   // weights streamed, k-step outer; the six weight fragments of the next k-step are in flight under the 24 products
      f32x4 ka[2][4], qa[2][4], va[4][2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          qa[dt][tt] = *reinterpret_cast<const f32x4*>(v_qb + head * 32 + dt * 16 + g * 4);
          ka[dt][tt] = *reinterpret_cast<const f32x4*>(v_qb + C + head * 32 + dt * 16 + g * 4);
          const float bv = v_qb[2 * C + head * 32 + dt * 16 + li];
          va[tt][dt] = f32x4{bv, bv, bv, bv};
        }
      bf16x8 wf[6];
#pragma unroll
      for (int f = 0; f < 6; ++f) wf[f] = *reinterpret_cast<const bf16x8*>(wq + f * 512);
#pragma unroll 1
      for (int ks = 0; ks < KS; ++ks) {   // rolled: the fully unrolled form hoists all 48 fragment loads and spills
        bf16x8 wn[6];
        if (ks + 1 < KS) {
#pragma unroll
          for (int f = 0; f < 6; ++f) wn[f] = *reinterpret_cast<const bf16x8*>(wq + ((ks + 1) * 6 + f) * 512);
        }
        bf16x8 xk[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) xk[tt] = *reinterpret_cast<const bf16x8*>(tile + tt * (16 * PT) + (cx0 ^ (ks << 6)));
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          MM::mma(qa[0][tt], wf[0], xk[tt]);
          MM::mma(qa[1][tt], wf[1], xk[tt]);
          MM::mma(ka[0][tt], wf[2], xk[tt]);
          MM::mma(ka[1][tt], wf[3], xk[tt]);
          MM::mma(va[tt][0], xk[tt], wf[4]);
          MM::mma(va[tt][1], xk[tt], wf[5]);
        }
        if (ks + 1 < KS) {
#pragma unroll
          for (int f = 0; f < 6; ++f) wf[f] = wn[f];
        }
      }
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) { kf[tt] = pack8(ka[0][tt], ka[1][tt]); qf[tt] = pack8(qa[0][tt], qa[1][tt]); }
#pragma unroll
      for (int ps = 0; ps < 2; ++ps)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) vf[ps][dt] = pack8(va[2 * ps][dt], va[2 * ps + 1][dt]);
    }

    const unsigned long long c3 = now();
    // ---- attention of this head, as swin_attn_mfma_kernel<bf16, EXPB> (swin_attn.hip) --------------------------------------
    // SW-MSA: only the last window row / column of the padded grid mixes regions (swin_transformer.py:369-387)
    const bool edge = p.geo.shift > 0 && (wy == p.geo.nWy - 1 || wx == p.geo.nWx - 1);
    unsigned long long krid = 0;   // region id (0..8) of this lane's 16 keys, 4 bits each
    if (edge) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = kt * 16 + g * 4 + r;
          const int ty = (j * 37) >> 8, tx = j - ty * WS;
          krid |= (unsigned long long)swin_region(wy * WS + ty, wx * WS + tx, Hp, Wp, p.geo.shift) << ((kt * 4 + r) * 4);
        }
    }
    f32x4 oacc[2][4];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4) oacc[dt][t4] = f32x4{0.f, 0.f, 0.f, 0.f};
    // per-iteration copy of the lane offset: keeps the 16 bias addresses of a window out of loop-invariant registers
    int be_l;
    asm volatile("v_mov_b32 %0, %1" : "=v"(be_l) : "v"(be_lane));
    const float* be = be_head + be_l;
    f32x4 bnext[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) bnext[kt] = *reinterpret_cast<const f32x4*>(be + kt * 16);
    int64_t qtok[4];
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      int i = t4 * 16 + li;
      const bool real_q = i < WT;
      if (i > WT - 1) i = WT - 1;            // clamped rows are never stored
      int sy, sx;
      const int64_t tok = win_token(p.geo, win, i, sy, sx);
      qtok[t4] = (real_q && valid) ? tok : (int64_t)-1;
      int rid_i = 0;
      if (edge) rid_i = swin_region(sy, sx, Hp, Wp, p.geo.shift);
      f32x4 bcur[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) bcur[kt] = bnext[kt];
      if (t4 < 3) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) bnext[kt] = *reinterpret_cast<const f32x4*>(be + (t4 + 1) * 16 * 64 + kt * 16);
      }
      float sc[16];
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        f32x4 st = bcur[kt];
        MM::mma(st, kf[kt], qf[t4]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float a = st[r] * scale2;   // (q.k + bias / scale) * scale * log2 e; padding keys are -inf through the seed
          if (edge && (int)((krid >> ((kt * 4 + r) * 4)) & 15) != rid_i) a += -100.0f * 1.4426950408889634f;
          sc[kt * 4 + r] = a;
          mx = fmaxf(mx, a);
        }
      }
      mx = quad_group_max(mx);
      float l = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        sc[k] = __builtin_amdgcn_exp2f(sc[k] - mx);
        l += sc[k];
      }
      l = quad_group_sum(l);
      const float inv = 1.0f / l;
#pragma unroll
      for (int k = 0; k < 16; ++k) sc[k] *= inv;
#pragma unroll
      for (int ps = 0; ps < 2; ++ps) {
        const bf16x8 pf = {(bf16_t)sc[ps * 8 + 0], (bf16_t)sc[ps * 8 + 1], (bf16_t)sc[ps * 8 + 2], (bf16_t)sc[ps * 8 + 3],
                           (bf16_t)sc[ps * 8 + 4], (bf16_t)sc[ps * 8 + 5], (bf16_t)sc[ps * 8 + 6], (bf16_t)sc[ps * 8 + 7]};
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) MM::mma(oacc[dt][t4], vf[ps][dt], pf);
      }
    }

    const unsigned long long c4 = now();
    lds_barrier();   // B2: every wave of the window has taken its tile fragments; the tile becomes O
    // O^T accumulators [dim dt*16 + 4g + r][query t4*16 + li] -> tile[query][head*32 + dim] (bf16)
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const f32x4 o = oacc[dt][t4];
        const bf16x4 ov = {(bf16_t)o[0], (bf16_t)o[1], (bf16_t)o[2], (bf16_t)o[3]};
        *reinterpret_cast<bf16x4*>(tile + t4 * (16 * PT) + (dt ? o_off1 : o_off0)) = ov;
      }
    // residual rows of this lane's output pieces (L2: the window's rows were fetched one iteration ago)
    f32x4 res[4][2];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        res[tt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (qtok[tt] >= 0) res[tt][nt] = *reinterpret_cast<const f32x4*>(p.x + qtok[tt] * C + head * 32 + nt * 16 + g * 4);
      }
    // ---- out^T = Wp O^T + b + x: this wave produces output channels [32 head, +32) of its window, accumulator
    //      [channel head*32 + nt*16 + 4g + r][token tt*16 + li] ------------------------------------------------------------------------
    unsigned long long c5;
    if constexpr (RESIDENT) {   // rows of Wp as A operands (L2-resident, 8 KB per wave); O is taken whole, then B4, then products + stores
      bf16x8 wp[2][4];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          wp[nt][ks] = *reinterpret_cast<const bf16x8*>(p.proj_w + (head * 32 + nt * 16 + li) * C + ks * 32 + g * 8);
      lds_barrier();   // B3: tile = O of the window, all heads
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) xf[tt][ks] = *reinterpret_cast<const bf16x8*>(tile + tt * (16 * PT) + cx[ks]);
      lds_barrier();   // B4: the tile may be overwritten by the next window's LayerNorm
      c5 = now();
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          f32x4 acc = *reinterpret_cast<const f32x4*>(v_pb + head * 32 + nt * 16 + g * 4);
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) MM::mma(acc, wp[nt][ks], xf[tt][ks]);
          if (qtok[tt] >= 0) *reinterpret_cast<f32x4*>(p.out + qtok[tt] * C + head * 32 + nt * 16 + g * 4) = sum4(res[tt][nt], acc);
        }
    } else {   // k-step outer over the streamed fragments, O read per k-step; B4 after the products, then the stores
      bf16x8 pw[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) pw[nt] = *reinterpret_cast<const bf16x8*>(wpj + (nt * KS) * 512);
      lds_barrier();   // B3: tile = O of the window, all heads
      f32x4 pa[2][4];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) pa[nt][tt] = *reinterpret_cast<const f32x4*>(v_pb + head * 32 + nt * 16 + g * 4);
#pragma unroll 1
      for (int ks = 0; ks < KS; ++ks) {
        bf16x8 pn[2];
        if (ks + 1 < KS) {
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) pn[nt] = *reinterpret_cast<const bf16x8*>(wpj + (nt * KS + ks + 1) * 512);
        }
        bf16x8 of[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) of[tt] = *reinterpret_cast<const bf16x8*>(tile + tt * (16 * PT) + (cx0 ^ (ks << 6)));
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) MM::mma(pa[nt][tt], pw[nt], of[tt]);
        if (ks + 1 < KS) { pw[0] = pn[0]; pw[1] = pn[1]; }
      }
      lds_barrier();   // B4: the tile may be overwritten by the next window's LayerNorm
      c5 = now();
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
          if (qtok[tt] >= 0) *reinterpret_cast<f32x4*>(p.out + qtok[tt] * C + head * 32 + nt * 16 + g * 4) = sum4(res[tt][nt], pa[nt][tt]);
    }
    if constexpr (TRACE) {
      const unsigned long long c6 = now();
      tr[1] += c1 - c0; tr[2] += c2 - c1; tr[3] += c3 - c2; tr[4] += c4 - c3; tr[5] += c5 - c4; tr[6] += c6 - c5;
    }
  }
  if constexpr (TRACE) {
    // wave 0: total | LayerNorm + prefetch issue | wait B1 | fragments + q k v | attention | B2, O, loads, B3, (fragments | proj,) B4 | (proj +) stores | start
    if (threadIdx.x == 0 && p.trace != nullptr) {
      unsigned long long* t = p.trace + (long long)blockIdx.x * 8;
      t[0] = now() - t_start; t[1] = tr[1]; t[2] = tr[2]; t[3] = tr[3]; t[4] = tr[4]; t[5] = tr[5]; t[6] = tr[6]; t[7] = t_start;
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Checks the shape, fills the geometry and launches swin_block_kernel<S> on min(ceil(windows / S::GROUPS), CUs) persistent workgroups.
// The caller has set p's pointers and says whether its weight pointers are 16-byte aligned.
template <class S>
int swin_block_launch(typename S::P& p, bool weights_aligned, int B, int H, int W, int C, int nH, int window, int shift, omp_stream_t s) {
  OMP_CHECK_ARG(C == S::C && nH == S::HEADS, "%s: built for C = %d with %d heads (got C=%d nH=%d)", S::NAME, S::C, S::HEADS, C, nH);
  OMP_CHECK_ARG(window == WS, "%s: only window 7 is built (got %d)", S::NAME, window);
  OMP_CHECK_ARG(shift >= 0 && shift < WS, "%s: bad shift %d", S::NAME, shift);
  OMP_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: bad shape", S::NAME);
  SwinGeo& geo = p.geo;
  geo.B = B; geo.H = H; geo.W = W; geo.shift = shift;
  geo.nWy = (H + WS - 1) / WS; geo.nWx = (W + WS - 1) / WS;
  const int64_t nw = (int64_t)B * geo.nWy * geo.nWx;
  OMP_CHECK_ARG(nw < (int64_t)1 << 30, "%s: too many windows", S::NAME);
  geo.n_win = (int)nw;
  OMP_CHECK_ARG(aligned16(p.x) && aligned16(p.out) && weights_aligned && aligned16(p.bias_exp),
                "%s: x / out / %s / bias_expanded must be 16-byte aligned (the kernel moves 16-byte vectors)", S::NAME, S::WEIGHTS);
  p.trace = omp_cur().mlp_trace;   // omp_debug_swin_mlp_trace: the development buffer also takes this kernel's phase sums
  if constexpr (LDS_BYTES<S> > 64 * 1024) {
    if (const int rc = p.trace == nullptr ? omp_raise_lds<swin_block_kernel<S, false>>(S::NAME) : omp_raise_lds<swin_block_kernel<S, true>>(S::NAME)) return rc;
  }
  const int n_cu = omp_device_cus();
  const int64_t groups = (nw + S::GROUPS - 1) / S::GROUPS;
  const int grid = (int)(groups < n_cu ? groups : n_cu);
  if (p.trace != nullptr) hipLaunchKernelGGL((swin_block_kernel<S, true>), dim3((unsigned)grid), dim3(512), LDS_BYTES<S>, (hipStream_t)s, p);
  else hipLaunchKernelGGL((swin_block_kernel<S, false>), dim3((unsigned)grid), dim3(512), LDS_BYTES<S>, (hipStream_t)s, p);
  OMP_CHECK_LAUNCH(S::NAME);
  return OMP_OK;
}

}  // namespace

// x (fp32 [B*H*W, 128]) -> out = x + proj(W-MSA / SW-MSA(LayerNorm(x))) for Swin-B stage-0 geometry (C = 128, 4 heads, window 7);
// out may be x.  Replaces LayerNorm + qkv GEMM + window attention + proj GEMM of the bf16 engine (swin_transformer.py:196-253).
extern "C" int omp_swin_attn_block(const void* x, void* out, const float* ln_g, const float* ln_b, float eps, const void* qkv_w,
                                   const float* qkv_b, const float* bias_expanded, const void* proj_w, const float* proj_b, int B, int H,
                                   int W, int C, int nH, int window, int shift, omp_stream_t s) {
  OMP_CHECK_ARG(x && out && ln_g && ln_b && qkv_w && qkv_b && bias_expanded && proj_w && proj_b, "omp_swin_attn_block: null pointer");
  SwinBlockP p;
  p.x = (const float*)x; p.out = (float*)out; p.ln_g = ln_g; p.ln_b = ln_b; p.eps = eps;
  p.qkv_w = (const bf16_t*)qkv_w; p.qkv_b = qkv_b; p.bias_exp = bias_expanded; p.proj_w = (const bf16_t*)proj_w; p.proj_b = proj_b;
  return swin_block_launch<Stage0>(p, aligned16(qkv_w) && aligned16(proj_w), B, H, W, C, nH, window, shift, s);
}

// The same block for C = 256 with 8 heads (Swin-B stage 1); wpack = model/packing.py::pack_attn_block(qkv.weight, proj.weight, 8).
extern "C" int omp_swin_attn_block_packed(const void* x, void* out, const float* ln_g, const float* ln_b, float eps, const void* wpack,
                                          const float* qkv_b, const float* bias_expanded, const float* proj_b, int B, int H, int W, int C,
                                          int nH, int window, int shift, omp_stream_t s) {
  OMP_CHECK_ARG(x && out && ln_g && ln_b && wpack && qkv_b && bias_expanded && proj_b, "omp_swin_attn_block_packed: null pointer");
  SwinBlockPackedP p;
  p.x = (const float*)x; p.out = (float*)out; p.ln_g = ln_g; p.ln_b = ln_b; p.eps = eps;
  p.wpack = (const bf16_t*)wpack; p.qkv_b = qkv_b; p.bias_exp = bias_expanded; p.proj_b = proj_b;
  return swin_block_launch<Stage1>(p, aligned16(wpack), B, H, W, C, nH, window, shift, s);
}
