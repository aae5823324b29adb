// Lexicon correction: for every query word the nearest word of a lexicon under the Levenshtein distance, on the device
// (DESIGN.md section 15).  The distance is the one the reference's recogniser evaluation uses (OCR/MGP-STR/test_final.py:14,
// nltk.metrics.distance.edit_distance: insert / delete / substitute cost 1, no transpositions).
//
// Myers' bit-parallel recurrence (in Hyyro's formulation for the global distance): the query's m <= 64 characters are the
// bits of a 64-bit column, Peq[c] has bit i set where query[i] == c, and one lexicon character advances the column
// (Pv, Mv: the vertical +1 / -1 differences) and the score D[m][j] with a dozen integer operations.  Integers only, so
// utils/lexicon.py: nearest_cpu (the specification) and this kernel agree on every output.
//
//   lexicon_fill_kernel     best[q] = all ones ("no word") ahead of the search, on the same stream
//   lexicon_nearest_kernel  a 256-thread workgroup = one query x one slice of that query's range [lo, hi) of lexicon
//                           indices.  Every thread computes its own entry of the query's match table Peq (256 x 64 bits,
//                           2 KB of LDS, the only LDS besides four partial minima), then walks whole lexicon words, one
//                           per thread and 256 apart, eight characters per global load and one LDS read per character,
//                           keeping the least key (dist << 32) | index.  Wave minimum, workgroup minimum, one 64-bit
//                           atomicMin on best[q] per workgroup.  A minimum does not depend on the order of its operands,
//                           so the output does not depend on scheduling; ties go to the lowest index because the index
//                           is the low half of the key.
// Nothing is allocated and nothing synchronises: queries, lexicon and best are the caller's.
#include "common.h"

namespace {

constexpr int LEX_THREADS = 256;
constexpr int LEX_QMAX = 64;     // query characters: the bits of one column
constexpr int LEX_WMAX = 255;    // lexicon word characters
constexpr unsigned long long LEX_NONE = ~0ull;

__global__ __launch_bounds__(256) void lexicon_fill_kernel(unsigned long long* __restrict__ best, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) best[i] = LEX_NONE;
}

// the 8 pool bytes from p on, little endian; bytes at or beyond pool_bytes read as 0 and are never fetched
__device__ __forceinline__ uint64_t lex_load8(const uint8_t* __restrict__ pool, int64_t p, int64_t pool_bytes) {
  uint64_t v = 0;
  if (p + 8 <= pool_bytes) {
    __builtin_memcpy(&v, pool + p, 8);
  } else {
    for (int k = 0; k < 8 && p + k < pool_bytes; ++k) v |= (uint64_t)pool[p + k] << (8 * k);
  }
  return v;
}

__global__ __launch_bounds__(LEX_THREADS) void lexicon_nearest_kernel(const uint8_t* __restrict__ q_codes, const int32_t* __restrict__ q_len,
                                                                      const int32_t* __restrict__ q_lo, const int32_t* __restrict__ q_hi,
                                                                      const uint8_t* __restrict__ pool, int64_t pool_bytes,
                                                                      const int32_t* __restrict__ offsets, int L, int chunks,
                                                                      unsigned long long* __restrict__ best) {
  __shared__ uint64_t peq[256];
  __shared__ unsigned long long wave_min[LEX_THREADS / OMP_WAVE];
  const int q = blockIdx.x / chunks, c = blockIdx.x - q * chunks;
  // the descriptor is checked here, per query: a length outside [0, 64] is refused (best[q] stays all ones), a range is
  // clamped to [0, L]; an empty range or an empty slice of it has nothing to do.  All of this is uniform over the workgroup.
  const int m = q_len[q];
  if (m < 0 || m > LEX_QMAX) return;
  const int lo = q_lo ? max(q_lo[q], 0) : 0;
  const int hi = q_hi ? min(q_hi[q], L) : L;
  if (lo >= hi) return;
  const int64_t per = ((int64_t)(hi - lo) + chunks - 1) / chunks;
  const int64_t w0 = lo + c * per, w1 = min(w0 + per, (int64_t)hi);
  if (w0 >= w1) return;

  // Peq: thread t owns symbol t.  The query's 64 bytes are at a workgroup-uniform address.  Codes 254 and 255 are the
  // "unknown" symbols of queries and of lexicon words: they match nothing, so their entries stay 0.
  {
    const uint8_t* qc = q_codes + (int64_t)q * LEX_QMAX;
    uint64_t mask = 0;
    if (threadIdx.x < 254) {
      for (int i = 0; i < m; ++i) mask |= (uint64_t)(qc[i] == threadIdx.x) << i;
    }
    peq[threadIdx.x] = mask;
  }
  __syncthreads();

  unsigned long long mine = LEX_NONE;
  const int top = m - 1;   // the score follows bit m - 1 of the horizontal differences; m == 0 is handled apart
  for (int64_t w = w0 + threadIdx.x; w < w1; w += LEX_THREADS) {
    // a word is offsets[w] .. offsets[w + 1], clamped into the pool and to 255 characters: a damaged table reads nothing outside
    const int64_t s = min(max((int64_t)offsets[w], (int64_t)0), pool_bytes);
    const int64_t e = min(max((int64_t)offsets[w + 1], s), min(pool_bytes, s + LEX_WMAX));
    const int n = (int)(e - s);
    uint32_t score;
    if (m == 0) {
      score = (uint32_t)n;
    } else {
      uint64_t Pv = ~0ull, Mv = 0;
      score = (uint32_t)m;
      for (int j = 0; j < n; j += 8) {
        uint64_t chars = lex_load8(pool, s + j, pool_bytes);
        const int kn = min(8, n - j);
        for (int k = 0; k < kn; ++k) {
          const uint64_t Eq = peq[chars & 0xff];
          chars >>= 8;
          const uint64_t Xv = Eq | Mv;
          const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
          uint64_t Ph = Mv | ~(Xh | Pv);
          uint64_t Mh = Pv & Xh;
          score += (uint32_t)(Ph >> top) & 1u;
          score -= (uint32_t)(Mh >> top) & 1u;
          Ph = (Ph << 1) | 1;   // row 0 of the table is 0, 1, 2, ...: the whole word is aligned, not a substring
          Mh <<= 1;
          Pv = Mh | ~(Xv | Ph);
          Mv = Ph & Xv;
        }
      }
    }
    const unsigned long long key = ((unsigned long long)score << 32) | (uint32_t)w;
    mine = min(mine, key);
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(mine, o, 64);
    mine = min(mine, other);
  }
  if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long b = wave_min[0];
#pragma unroll
    for (int i = 1; i < LEX_THREADS / OMP_WAVE; ++i) b = min(b, wave_min[i]);
    if (b != LEX_NONE) atomicMin(best + q, b);
  }
}

}  // namespace

extern "C" int omp_lexicon_nearest(const uint8_t* q_codes, const int32_t* q_len, const int32_t* q_lo, const int32_t* q_hi, int n,
                                   const uint8_t* pool, int64_t pool_bytes, const int32_t* offsets, int L, int range_hint,
                                   uint64_t* best, omp_stream_t s) {
  OMP_CHECK_ARG(q_codes && q_len && pool && offsets && best, "omp_lexicon_nearest: null pointer");
  OMP_CHECK_ARG((q_lo == nullptr) == (q_hi == nullptr), "omp_lexicon_nearest: q_lo and q_hi go together");
  OMP_CHECK_ARG(n > 0 && L > 0 && pool_bytes >= 0, "omp_lexicon_nearest: %d queries, %d words, %lld pool bytes", n, L, (long long)pool_bytes);
  // Workgroups per query.  A thread should have a word to walk, so no more than ceil(range / 256); and the launch should
  // hold 16 workgroups per compute unit (two rounds of the 8 that fit one), so few queries against a long lexicon are cut
  // into many slices while many queries against short ranges get one workgroup each and fill the chip by their number.
  const int64_t range = (q_lo && range_hint > 0) ? min((int64_t)range_hint, (int64_t)L) : (int64_t)L;
  const int64_t want = ceil_div64(16 * (int64_t)omp_device_cus(), n);
  int64_t chunks = max((int64_t)1, min(want, ceil_div64(range, LEX_THREADS)));
  chunks = min(chunks, (int64_t)0x7fffffff / n);
  OMP_CHECK_ARG(chunks >= 1, "omp_lexicon_nearest: %d queries exceed one grid", n);
  hipLaunchKernelGGL(lexicon_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s,
                     reinterpret_cast<unsigned long long*>(best), n);
  OMP_CHECK_LAUNCH("omp_lexicon_nearest (fill)");
  hipLaunchKernelGGL(lexicon_nearest_kernel, dim3((unsigned)(chunks * n)), dim3(LEX_THREADS), 0, (hipStream_t)s, q_codes, q_len, q_lo, q_hi,
                     pool, pool_bytes, offsets, L, (int)chunks, reinterpret_cast<unsigned long long*>(best));
  OMP_CHECK_LAUNCH("omp_lexicon_nearest");
  return OMP_OK;
}
