// Posterior lexicon decoding: for every word crop the lexicon word MGP-STR's character head finds most likely, and the
// runner-up, on the device.  The head is non-autoregressive, so P(word) = prod_i p_i(word[i]) *
// p_len([s]) is exact under the reference's decoding rule (OCR/MGP-STR/test_final.py:172-181).  Floats end at the costs:
//
//   logprob_costs_kernel     a 256-thread workgroup = one query; a wave = one of its 26 scored positions at a time (position 0 of
//                            the 27 is dropped, as recognize does).  Lane c < 38 holds class c: wave maximum, sum of exp, log in
//                            fp32, cost = clip(floor(-logp * 1024 + 0.5), 0, 2^20 - 1) as int32.  The wave's least (cost, class)
//                            goes to LDS; after one barrier wave 0 walks the 26 minima: greedy[q] = (sum of the minima through the
//                            first [s], its position), on the quantised costs.
//   lexicon_posterior_kernel a 256-thread workgroup = one query x one slice of that query's range [lo, hi) of lexicon indices (the
//                            shape of lexicon_nearest_kernel).  The query's 26 x 38 int32 costs (3952 bytes) and the 256-byte
//                            class table go into LDS once; every thread walks whole lexicon words 256 apart, eight pool bytes per
//                            global load, one LDS byte and one LDS word per character plus the [s] term, and keeps its TWO least
//                            keys (score << 32) | index.  Wave and workgroup reductions of the pair; the pair goes to
//                            work[q][slice] with ordinary stores -- every slice writes, an empty one writes two all-ones keys.
//   lexicon_post_merge_kernel  a wave = one query: the two least keys over its slices' pairs -> best[q][0..1].
// The two least of a set do not depend on the order in which pairs are merged, so the output does not depend on scheduling;
// ties go to the lowest index because the index is the low half of the key.  Integers only after the costs, so
// utils/lexicon_post.py: score_cpu / greedy_cpu (the specification) and these kernels agree on every output.
// Nothing is allocated and nothing synchronises: logits, costs, lexicon, work and best are the caller's.
#include "common.h"

namespace {

constexpr int LXP_THREADS = 256;
constexpr int LXP_WAVES = LXP_THREADS / OMP_WAVE;
constexpr int LXP_POS = 26;       // scored positions
constexpr int LXP_CLS = 38;       // classes: [GO], [s], 36 characters
constexpr int LXP_EOS = 1;
constexpr int LXP_WMAX = 25;      // a word and its [s] fit the 26 positions
constexpr int LXP_CAP = (1 << 20) - 1;
constexpr int LXP_SLICES = 4096;  // the launch aims at this many workgroups: 16 per compute unit of an MI355X; work is sized by it
constexpr unsigned long long LXP_NONE = ~0ull;

__global__ __launch_bounds__(LXP_THREADS) void logprob_costs_kernel(const float* __restrict__ logits, int32_t* __restrict__ costs,
                                                                   int32_t* __restrict__ greedy) {
  __shared__ int32_t pos_min[LXP_POS];   // (cost << 6) | class of the position's least cost: cost < 2^20, class < 64
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* lg = logits + ((int64_t)q * (LXP_POS + 1) + 1) * LXP_CLS;
  int32_t* out = costs + (int64_t)q * LXP_POS * LXP_CLS;
  for (int p = wave; p < LXP_POS; p += LXP_WAVES) {
    const bool live = lane < LXP_CLS;
    const float x = live ? lg[p * LXP_CLS + lane] : -INFINITY;
    float m = x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = live ? expf(x - m) : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    // -logp = (m - x) + log(sum) >= 0; fmaxf / fminf also settle a NaN row (a NaN operand yields the other one)
    const float units = floorf(((m - x) + logf(sum)) * 1024.0f + 0.5f);
    const int32_t cost = (int32_t)fminf(fmaxf(units, 0.0f), (float)LXP_CAP);
    if (live) out[p * LXP_CLS + lane] = cost;
    int32_t key = live ? ((cost << 6) | lane) : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = min(key, __shfl_xor(key, o, 64));
    if (lane == 0) pos_min[p] = key;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t total = 0, len = LXP_POS;
    for (int p = 0; p < LXP_POS; ++p) {
      const int32_t key = pos_min[p];
      total += key >> 6;
      if ((key & 63) == LXP_EOS) { len = p; break; }
    }
    greedy[2 * (int64_t)q] = total;
    greedy[2 * (int64_t)q + 1] = len;
  }
}

// the 8 pool bytes from p on, little endian; bytes at or beyond pool_bytes read as 0 and are never fetched
__device__ __forceinline__ uint64_t lxp_load8(const uint8_t* __restrict__ pool, int64_t p, int64_t pool_bytes) {
  uint64_t v = 0;
  if (p + 8 <= pool_bytes) {
    __builtin_memcpy(&v, pool + p, 8);
  } else {
    for (int k = 0; k < 8 && p + k < pool_bytes; ++k) v |= (uint64_t)pool[p + k] << (8 * k);
  }
  return v;
}

// (a, b) = the two least of {a, b, k}; a <= b on entry and on exit
__device__ __forceinline__ void lxp_insert(unsigned long long& a, unsigned long long& b, unsigned long long k) {
  b = min(b, max(a, k));
  a = min(a, k);
}

__global__ __launch_bounds__(LXP_THREADS) void lexicon_posterior_kernel(const int32_t* __restrict__ costs, const int32_t* __restrict__ q_lo,
                                                                       const int32_t* __restrict__ q_hi, const uint8_t* __restrict__ pool,
                                                                       int64_t pool_bytes, const int32_t* __restrict__ offsets, int L,
                                                                       const uint8_t* __restrict__ class_table, int chunks,
                                                                       unsigned long long* __restrict__ work) {
  __shared__ int32_t cost[LXP_POS * LXP_CLS];
  __shared__ uint8_t cls_of[256];
  __shared__ unsigned long long wave_pair[LXP_WAVES][2];
  const int q = blockIdx.x / chunks, c = blockIdx.x - q * chunks;
  // the range is clamped to [0, L]; an empty range or an empty slice of it walks no word and writes two all-ones keys.
  // All of this is uniform over the workgroup.
  const int lo = q_lo ? max(q_lo[q], 0) : 0;
  const int hi = q_hi ? min(q_hi[q], L) : L;
  int64_t w0 = 0, w1 = 0;
  if (lo < hi) {
    const int64_t per = ((int64_t)(hi - lo) + chunks - 1) / chunks;
    w0 = lo + c * per;
    w1 = min(w0 + per, (int64_t)hi);
  }
  unsigned long long a = LXP_NONE, b = LXP_NONE;
  if (w0 < w1) {
    const int32_t* cq = costs + (int64_t)q * LXP_POS * LXP_CLS;
    for (int i = threadIdx.x; i < LXP_POS * LXP_CLS; i += LXP_THREADS) cost[i] = cq[i];
    cls_of[threadIdx.x] = class_table[threadIdx.x];
    __syncthreads();
    for (int64_t w = w0 + threadIdx.x; w < w1; w += LXP_THREADS) {
      // a word is offsets[w] .. offsets[w + 1], clamped into the pool: a damaged table reads nothing outside.  Longer than 25
      // characters: skipped, not truncated.
      const int64_t s = min(max((int64_t)offsets[w], (int64_t)0), pool_bytes);
      const int64_t e = min(max((int64_t)offsets[w + 1], s), pool_bytes);
      if (e - s > LXP_WMAX) continue;
      const int n = (int)(e - s);
      uint32_t score = (uint32_t)cost[n * LXP_CLS + LXP_EOS];
      bool ok = true;
      for (int j = 0; j < n; j += 8) {
        uint64_t chars = lxp_load8(pool, s + j, pool_bytes);
        const int kn = min(8, n - j);
        for (int k = 0; k < kn; ++k) {
          const int cls = cls_of[chars & 0xff];
          chars >>= 8;
          ok = ok && cls < LXP_CLS;                                   // 255 = unscorable; a table entry of 38..254 counts as such too
          score += (uint32_t)cost[(j + k) * LXP_CLS + min(cls, LXP_CLS - 1)];
        }
      }
      if (ok) lxp_insert(a, b, ((unsigned long long)score << 32) | (uint32_t)w);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long oa = __shfl_xor(a, o, 64), ob = __shfl_xor(b, o, 64);
    b = min(min(b, ob), max(a, oa));
    a = min(a, oa);
  }
  if ((threadIdx.x & 63) == 0) {
    wave_pair[threadIdx.x >> 6][0] = a;
    wave_pair[threadIdx.x >> 6][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < LXP_WAVES; ++i) {
      const unsigned long long oa = wave_pair[i][0], ob = wave_pair[i][1];
      b = min(min(b, ob), max(a, oa));
      a = min(a, oa);
    }
    work[2 * (int64_t)blockIdx.x] = a;
    work[2 * (int64_t)blockIdx.x + 1] = b;
  }
}

__global__ __launch_bounds__(LXP_THREADS) void lexicon_post_merge_kernel(const unsigned long long* __restrict__ work, int n, int chunks,
                                                                        unsigned long long* __restrict__ best) {
  const int lane = threadIdx.x & 63, q = blockIdx.x * LXP_WAVES + (threadIdx.x >> 6);
  if (q >= n) return;
  unsigned long long a = LXP_NONE, b = LXP_NONE;
  for (int c = lane; c < chunks; c += 64) {
    const unsigned long long oa = work[2 * ((int64_t)q * chunks + c)], ob = work[2 * ((int64_t)q * chunks + c) + 1];
    b = min(min(b, ob), max(a, oa));
    a = min(a, oa);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long oa = __shfl_xor(a, o, 64), ob = __shfl_xor(b, o, 64);
    b = min(min(b, ob), max(a, oa));
    a = min(a, oa);
  }
  if (lane == 0) {
    best[2 * (int64_t)q] = a;
    best[2 * (int64_t)q + 1] = b;
  }
}

}  // namespace

extern "C" int omp_logprob_costs(const float* logits, int n, int32_t* costs, int32_t* greedy, omp_stream_t s) {
  OMP_CHECK_ARG(logits && costs && greedy, "omp_logprob_costs: null pointer");
  OMP_CHECK_ARG(n > 0, "omp_logprob_costs: %d queries", n);
  hipLaunchKernelGGL(logprob_costs_kernel, dim3((unsigned)n), dim3(LXP_THREADS), 0, (hipStream_t)s, logits, costs, greedy);
  OMP_CHECK_LAUNCH("omp_logprob_costs");
  return OMP_OK;
}

extern "C" int omp_lexicon_posterior(const int32_t* costs, int n, const int32_t* q_lo, const int32_t* q_hi, const uint8_t* pool,
                                     int64_t pool_bytes, const int32_t* offsets, int L, const uint8_t* class_table, int range_hint,
                                     uint64_t* best, uint64_t* work, omp_stream_t s) {
  OMP_CHECK_ARG(costs && pool && offsets && class_table && best && work, "omp_lexicon_posterior: null pointer");
  OMP_CHECK_ARG((q_lo == nullptr) == (q_hi == nullptr), "omp_lexicon_posterior: q_lo and q_hi go together");
  OMP_CHECK_ARG(n > 0 && L > 0 && pool_bytes >= 0 && range_hint >= 0, "omp_lexicon_posterior: %d queries, %d words, %lld pool bytes, range hint %d",
                n, L, (long long)pool_bytes, range_hint);
  // Workgroups per query, as omp_lexicon_nearest cuts them: a thread should have a word to walk, so no more than
  // ceil(range / 256); and the launch should hold about LXP_SLICES workgroups.  n * chunks < n + LXP_SLICES: the size of work.
  const int64_t range = (q_lo && range_hint > 0) ? min((int64_t)range_hint, (int64_t)L) : (int64_t)L;
  const int64_t want = ceil_div64(LXP_SLICES, n);
  const int64_t chunks = max((int64_t)1, min(want, ceil_div64(range, LXP_THREADS)));
  OMP_CHECK_ARG(chunks * n <= (int64_t)0x7fffffff, "omp_lexicon_posterior: %d queries exceed one grid", n);
  hipLaunchKernelGGL(lexicon_posterior_kernel, dim3((unsigned)(chunks * n)), dim3(LXP_THREADS), 0, (hipStream_t)s, costs, q_lo, q_hi, pool,
                     pool_bytes, offsets, L, class_table, (int)chunks, reinterpret_cast<unsigned long long*>(work));
  OMP_CHECK_LAUNCH("omp_lexicon_posterior");
  hipLaunchKernelGGL(lexicon_post_merge_kernel, dim3((unsigned)((n + LXP_WAVES - 1) / LXP_WAVES)), dim3(LXP_THREADS), 0, (hipStream_t)s,
                     reinterpret_cast<const unsigned long long*>(work), n, (int)chunks, reinterpret_cast<unsigned long long*>(best));
  OMP_CHECK_LAUNCH("omp_lexicon_posterior (merge)");
  return OMP_OK;
}
