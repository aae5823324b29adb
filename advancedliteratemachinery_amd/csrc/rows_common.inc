// Shared pieces of the row-owner chain kernels (csrc/dec_rows.hip: the decoder / Swin chains over bf16 operands and over the split-bf16 operands
// of the parity engine; csrc/kv_rows.hip: the memory projection): the per-wave weight stream with its register ring of asm loads and
// hand-counted waits, the LDS-only barrier, row LayerNorm.
// Included inside each file's anonymous namespace.
constexpr int NW = 8;                  // waves per workgroup
constexpr int D = 512;                 // d_model

// XCD placement of a chain launch (omp_dec_rows_args.xcd_mask; speed only).  The dispatcher is observed to place block b on XCD b % 8
// (MI355X_MICROARCH.md, workgroup dispatch): a launch confined to the XCDs of `mask` has 8 blocks per group of popcount(mask) tiles, the blocks
// of the other XCDs retire at once (-1), the others take tile (b / 8) * popcount(mask) + rank of their XCD inside the mask.  If the dispatcher
// places blocks differently the same tiles are computed, only elsewhere.
__device__ __forceinline__ int xcd_tile(int mask) {
  const int b = (int)blockIdx.x;
  if (mask == 0) return b;
  const int xcd = b & 7;
  if (!((mask >> xcd) & 1)) return -1;
  return (b >> 3) * __builtin_popcount(mask) + __builtin_popcount(mask & ((1 << xcd) - 1));
}

template <int... I, class F>
__device__ __forceinline__ void sfor_seq(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>()), ...); }
template <int N, class F>
__device__ __forceinline__ void sfor(F&& f) { sfor_seq(std::make_integer_sequence<int, N>(), f); }

struct Stream {
  const char* base;   // wave-uniform: the next fragment to REQUEST (kept in scalar registers)
  unsigned voff;      // lane * 16
};
__device__ __forceinline__ Stream stream_of_wave(const char* wstream, int64_t wave_stride, int wave, int lane) {
  const uint64_t bs = reinterpret_cast<uint64_t>(wstream + (int64_t)wave * wave_stride);
  Stream st;
  st.base = reinterpret_cast<const char*>(((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(bs >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)bs));
  st.voff = lane * 16;
  return st;
}

// hipcc does not keep a register ring of loads in flight (it sinks the loads to their uses and drains vmcnt(0)): asm loads, hand-counted waits.
// Exactly PFN of these loads are outstanding at every take; loads return in order, so compiler-issued loads or stores in between only make the
// wait more conservative.  The comments in the asm text name the registers for the build audit (advancedliteratemachinery_amd/audit.py).
template <int U, int PFN>
__device__ __forceinline__ void ws_issue(u32x4 (&ring)[PFN], Stream& st) {
  asm volatile("global_load_dwordx4 %0, %1, %2 ; ring-load" : "=v"(ring[U]) : "v"(st.voff), "s"(st.base) : "memory");
  st.base += 1024;
}
template <int U, int PFN>
__device__ __forceinline__ bf16x8 ws_take(u32x4 (&ring)[PFN]) {
  asm volatile("s_waitcnt vmcnt(%1) ; ring-take %0" : "+v"(ring[U]) : "n"(PFN - 1) : "memory");
  bf16x8 f;
  __builtin_memcpy(&f, &ring[U], 16);
  return f;
}
// The ring runs PFN fragments ahead of the stream's end.  The compiler sees no further use of those registers and would hand them to the
// code that follows -- where the requests still in flight would land on live values (the build audit caught exactly that).  After a
// kernel's last product: wait for everything, with the ring registers as operands so that they stay allocated until then.
__device__ __forceinline__ void ws_drain(u32x4 (&ring)[8]) {
  asm volatile("s_waitcnt vmcnt(0) ; ring-drain" : "+v"(ring[0]), "+v"(ring[1]), "+v"(ring[2]), "+v"(ring[3]), "+v"(ring[4]), "+v"(ring[5]), "+v"(ring[6]), "+v"(ring[7])::"memory");
}
__device__ __forceinline__ void ws_drain(u32x4 (&ring)[16]) {
  asm volatile("s_waitcnt vmcnt(0) ; ring-drain" : "+v"(ring[0]), "+v"(ring[1]), "+v"(ring[2]), "+v"(ring[3]), "+v"(ring[4]), "+v"(ring[5]), "+v"(ring[6]), "+v"(ring[7]),
               "+v"(ring[8]), "+v"(ring[9]), "+v"(ring[10]), "+v"(ring[11]), "+v"(ring[12]), "+v"(ring[13]), "+v"(ring[14]), "+v"(ring[15])::"memory");
}
// A value the optimiser cannot trace back: epilogues index with opaque copies of the lane coordinates so that their address arithmetic is
// redone where it is used instead of being kept live (as 64-bit pointers, 40+ registers) across the product loops -- the kernels sit at
// the 256-register budget of two waves per SIMD.
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
// LDS-only barrier: the weight ring stays in flight across it (a __syncthreads() would drain vmcnt(0))
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int NFT, int RTT>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[NFT][RTT]) {
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft)
#pragma unroll
    for (int rt = 0; rt < RTT; ++rt) acc[ft][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// two-pass LayerNorm of one 512-wide row held 8 values per lane (the embedding prologue: a wave per row)
__device__ __forceinline__ void ln_row512(float* v, const float* __restrict__ g, const float* __restrict__ b, int lane, float eps) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += v[i];
  s = wave_sum(s);
  const float mean = s * (1.0f / D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) { const float d = v[i] - mean; q += d * d; }
  q = wave_sum(q);
  const float rstd = 1.0f / sqrtf(q * (1.0f / D) + eps);
  const f32x4 g0 = *reinterpret_cast<const f32x4*>(g + lane * 8), g1 = *reinterpret_cast<const f32x4*>(g + lane * 8 + 4);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(b + lane * 8), b1 = *reinterpret_cast<const f32x4*>(b + lane * 8 + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = (v[i] - mean) * rstd * g0[i] + b0[i];
    v[i + 4] = (v[i + 4] - mean) * rstd * g1[i] + b1[i];
  }
}

// the bias quads of this lane's NFT feature tiles (loaded BEFORE the product whose epilogue uses them: the load hides under the product)
template <int NFT>
__device__ __forceinline__ void load_bias(f32x4 (&bb)[NFT], const float* __restrict__ bias, int fwave, int flimit, int g) {
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) {
    const int f = fwave + ft * 16 + g * 4;
    bb[ft] = f < flimit ? *reinterpret_cast<const f32x4*>(bias + f) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

