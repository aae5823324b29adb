// Page patterns: where a SHAPE stands in the text of a read page -- a date, an amount, an id -- with up to k errors.
// utils/page_pattern.py (row_py / search_cpu: the specification) and this kernel agree on every integer.  A pattern is 1 .. 64 positions,
// each a character class, each mandatory or optional: D[0][j] = 0, D[i][0] = D[i-1][0] + skip_i,
// D[i][j] = min(D[i-1][j-1] + (t_j not in C_i), D[i-1][j] + skip_i, D[i][j-1] + 1), skip_i = 0 for an optional position, else 1;
// v_j = min(D[P][j], k + 1).
//
// The job frame is page_frame.h's (pg_window), which page_search.hip shares; PpStep holds the column:
//
//   page_pattern_kernel   one wave (a 64-thread workgroup) per job (page, pattern).
//     rows      Wu and Manber's R_0 .. R_k (1992), one 64-bit word each, in registers: bit i of R_d says that a prefix of i + 1 positions
//               ends at this column with at most d errors.  For a character with class word B
//                 R'_0 = cl(((R_0 << 1) | 1) & B)
//                 R'_d = cl((((R_d << 1) | 1) & B) | R_{d-1} | ((R_{d-1} << 1) | 1) | ((R'_{d-1} << 1) | 1))
//               and v_j is the least d whose R_d holds bit P - 1, else k + 1.  The body is instantiated on k + 1 = 1 .. 9 and the job's
//               (uniform) k picks one: nothing is indexed dynamically and nothing spills.
//     cl        the closure over optional positions (Navarro and Raffinot): bit i reaches i + 1 while position i + 1 is optional, and a
//               leading optional run is always set.  Three words per pattern -- A the optional bits, I the bit before each of their
//               runs (for a leading run its own first bit), F the last bit of each run -- give it in one subtraction: X |= lead;
//               Df = X | F; X |= A & (~(Df - I) ^ Df).  The borrow of a run stops at its F bit, so the runs do not disturb each other.
//     chunks    lane l owns the end columns cs + 1 .. cs + 128, cs = 128 (64 r + l) in round r.  A lane starts W = P + k <= 72 columns
//               before cs with the fresh column R_0 = cl(0), R_d = cl(R_{d-1} | ((R_{d-1} << 1) | 1)): an alignment of cost <= k covers
//               at most P + k characters, so v_cs and every later v equal those of the whole text.  A column below 1 is skipped.
//     text      the round's characters, 128 before its first chunk to 1 after its last, staged in LDS with 4 bytes of padding per 128.
//     mask      LDS, [sigma + 1] words copied from the pattern's table: bit i of mask[c] says that code c is in the class of position i.
//               Row sigma is 0: every code at or above sigma reads it, so a garbage byte matches nothing and indexes nothing.
//     best      per lane the least key (v << 32) | end over its own columns, then a wave min; column 0 is (k + 1, 0).
//     hits      as page search: per-lane lists in caller-owned scratch, an exclusive scan of the counts over the lanes, lane g resolves
//               the start of hit g.  The start is the LEAST s >= end - (P + dist) whose anchored cost equals dist (the longest match):
//               the same rows over t[end-1], t[end-2], ... with mask and opt bit-reversed within P.  The fresh column's empty prefix
//               feeds the first step's match and substitution; after that there is neither a `| 1` nor a leading run set outright
//               -- a match that ENDS in an inserted character costs more than dist at a hit, because v_end <= v_{end-1}.  The walk goes all min(end, P + dist) <= 72 characters, still in LDS, and keeps the LAST l whose
//               R_dist holds bit P - 1.
//   No atomics; the hits come out in ascending end whatever the scheduling.  Bits at or above P never reach a lower bit.
// A job out of range (a page or pattern that is not there, P outside 1 .. 64, opt bits at or above P, no mandatory position, k outside
// 0 .. min(Mand - 1, 8), a page above 65535 characters, a range outside the pool) is REFUSED on the device: n_hits = -1, best and hits -1,
// and nothing outside the pool is read.  Nothing is allocated and nothing synchronises.
#include "page_frame.h"

namespace {

constexpr int PP_K_MAX = 8;            // errors at the most
constexpr int PP_BEFORE = 128;         // characters staged before the round's first chunk

static_assert(PP_BEFORE >= PG_POS_MAX + PP_K_MAX, "page_pattern layout");

// the words of the closure over the optional positions `opt`
struct Closure {
  u64 lead, A, I, F;
  __device__ __forceinline__ explicit Closure(u64 opt) {
    lead = opt & ~(opt + 1);
    A = opt;
    I = ((opt >> 1) & ~opt) | (opt & 1ull);                // the leading run has no bit before it: its own first bit stands in
    F = opt & ~(opt >> 1);
  }
  // Lead: the empty prefix stands at this column (the search everywhere, the anchored walk in its fresh column only)
  template <bool Lead>
  __device__ __forceinline__ u64 close(u64 X) const {
    if (Lead) X |= lead;
    const u64 Df = X | F;
    return X | (A & (~(Df - I) ^ Df));
  }
};

template <int K>
__device__ __forceinline__ void pp_fresh(u64 (&R)[K], const Closure& cl) {
  R[0] = cl.close<true>(0);
#pragma unroll
  for (int d = 1; d < K; ++d) R[d] = cl.close<true>(R[d - 1] | ((R[d - 1] << 1) | 1ull));
}

// one column.  Search: the empty prefix stands at every column (`| 1` everywhere, the leading run set).  The anchored walk has it in
// its fresh column only: `in` = 1 in the first step, for the match and the substitution, which come from the column before.
template <int K, bool Search>
__device__ __forceinline__ void pp_step(u64 (&R)[K], u64 B, const Closure& cl, u64 in) {
  u64 old = R[0];
  u64 now = cl.close<Search>(((old << 1) | in) & B);
  R[0] = now;
#pragma unroll
  for (int d = 1; d < K; ++d) {
    const u64 mine = R[d];
    const u64 x = (((mine << 1) | in) & B) | old | ((old << 1) | in) | ((now << 1) | (Search ? 1ull : 0ull));
    old = mine;
    now = cl.close<Search>(x);
    R[d] = now;
  }
}

// the least d whose row holds bit `top`, else K
template <int K>
__device__ __forceinline__ int pp_value(const u64 (&R)[K], int top) {
  int v = K;
#pragma unroll
  for (int d = K - 1; d >= 0; --d)
    if ((R[d] >> top) & 1ull) v = d;
  return v;
}

// pg_window's Stepper under k = K - 1: the rows of one lane
template <int K>
struct PpStep {
  int P, top;
  Closure cl, rcl;                                         // of the pattern, and of the reversed pattern for the start walk
  u64 R[K];
  __device__ __forceinline__ PpStep(int P_, u64 opt) : P(P_), top(P_ - 1), cl(opt), rcl(__brevll(opt) >> (64 - P_)) {}
  __device__ __forceinline__ int warm() const { return P + K - 1; }
  __device__ __forceinline__ int stage_from() const { return 0; }
  __device__ __forceinline__ int none() const { return K; }   // k + 1: nothing within k
  __device__ __forceinline__ int tol() const { return K - 1; }
  __device__ __forceinline__ void fresh() { pp_fresh<K>(R, cl); }
  __device__ __forceinline__ int step(u64 B, int) {
    pp_step<K, true>(R, B, cl, 1ull);
    return pp_value<K>(R, top);
  }
  // the anchored rows of the reversed pattern over all min(end, P + dist) characters: the LAST l whose R_dist holds bit P - 1
  template <class At>
  __device__ __forceinline__ int start(int end, int dist, At at) const {
    u64 Q[K];
    pp_fresh<K>(Q, rcl);
    const int lmax = min(end, P + dist);
    int found = 0;
    for (int l = 1; l <= lmax; ++l) {
      const u64 B = __brevll(at(end - l)) >> (64 - P);
      pp_step<K, false>(Q, B, rcl, l == 1 ? 1ull : 0ull);
      u64 hit = 0;
#pragma unroll
      for (int d = 0; d < K; ++d)
        if (d == dist) hit = Q[d];
      if ((hit >> top) & 1ull) found = l;                  // the anchored cost is never below dist: the bit says it equals dist
    }
    return found ? end - found : -2;                       // -2 cannot happen: the start exists within P + dist characters
  }
};

template <int K>
__device__ __forceinline__ int pp_job(const uint8_t* __restrict__ t, int n, int P, u64 opt, int sigma, int H, const u64* mask, uint8_t* text, int2* slot,
                                      int2* list, int32_t* jhits, u64* key_out) {
  PpStep<K> st(P, opt);
  return pg_window<PP_BEFORE>(st, t, n, sigma, H, mask, text, slot, list, jhits, key_out);
}

__global__ __launch_bounds__(64) void page_pattern_kernel(const uint8_t* __restrict__ pool, int64_t pool_bytes, const int32_t* __restrict__ page_off,
                                                          const int32_t* __restrict__ page_len, int n_pages, const u64* __restrict__ masks,
                                                          const u64* __restrict__ opts, const int32_t* __restrict__ pat_len,
                                                          const int32_t* __restrict__ tol, int n_patterns, const int32_t* __restrict__ jobs, int sigma, int H,
                                                          int2* scratch, int32_t* __restrict__ best, int32_t* __restrict__ n_hits, int32_t* __restrict__ hits) {
  __shared__ __align__(16) u64 mask[PG_SIGMA_MAX + 2];
  __shared__ __align__(16) uint8_t text[PgText<PP_BEFORE>::BYTES];
  __shared__ int2 slot[PG_HITS_MAX];
  const int job = blockIdx.x, lane = threadIdx.x;
  int32_t* jhits = hits + (int64_t)job * H * 3;
  const int p = jobs[2 * job], qi = jobs[2 * job + 1];
  // all of this is uniform over the wave
  bool ok = p >= 0 && p < n_pages && qi >= 0 && qi < n_patterns;
  int n = 0, P = 0, k = 0;
  int64_t po = 0;
  u64 opt = 0;
  if (ok) {
    n = page_len[p];
    po = page_off[p];
    P = pat_len[qi];
    opt = opts[qi];
    k = tol[qi];
    ok = n >= 0 && n <= PG_LEN_MAX && P >= 1 && P <= PG_POS_MAX && po >= 0 && po + n <= pool_bytes;
    if (ok) {
      const int mand = P - __popcll(opt);
      ok = (P == 64 || (opt >> P) == 0) && mand >= 1 && k >= 0 && k <= min(mand - 1, PP_K_MAX);
    }
  }
  if (!ok) {
    pg_refuse(job, H, best, n_hits, jhits);
    return;
  }
  pg_classes(mask, masks, qi, sigma);
  __syncthreads();
  const uint8_t* __restrict__ t = pool + po;
  int2* list = scratch + ((int64_t)job * 64 + lane) * H;   // this lane's first H hits of the round: (end, dist)
  u64 key = 0;
  int base = 0;
  switch (k) {                                             // uniform
    case 0: base = pp_job<1>(t, n, P, opt, sigma, H, mask, text, slot, list, jhits, &key); break;
    case 1: base = pp_job<2>(t, n, P, opt, sigma, H, mask, text, slot, list, jhits, &key); break;
    case 2: base = pp_job<3>(t, n, P, opt, sigma, H, mask, text, slot, list, jhits, &key); break;
    case 3: base = pp_job<4>(t, n, P, opt, sigma, H, mask, text, slot, list, jhits, &key); break;
    case 4: base = pp_job<5>(t, n, P, opt, sigma, H, mask, text, slot, list, jhits, &key); break;
    case 5: base = pp_job<6>(t, n, P, opt, sigma, H, mask, text, slot, list, jhits, &key); break;
    case 6: base = pp_job<7>(t, n, P, opt, sigma, H, mask, text, slot, list, jhits, &key); break;
    case 7: base = pp_job<8>(t, n, P, opt, sigma, H, mask, text, slot, list, jhits, &key); break;
    default: base = pp_job<9>(t, n, P, opt, sigma, H, mask, text, slot, list, jhits, &key); break;
  }
  pg_tail(jhits, base, H);
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 other = __shfl_xor(key, d, 64);
    if (other < key) key = other;
  }
  if (lane == 0) {
    n_hits[job] = base;
    best[2 * job] = (int)(key >> 32);
    best[2 * job + 1] = (int)(key & 0xffffffffull);
  }
}

}  // namespace

extern "C" int omp_page_pattern_search(const uint8_t* pool, int64_t pool_bytes, const int32_t* page_off, const int32_t* page_len, int n_pages,
                                       const uint64_t* masks, const uint64_t* opt, const int32_t* pat_len, const int32_t* k, int n_patterns,
                                       const int32_t* jobs, int n_jobs, int sigma, int max_hits, void* scratch, int64_t scratch_bytes, int32_t* best,
                                       int32_t* n_hits, int32_t* hits, omp_stream_t s) {
  OMP_CHECK_ARG(pool && page_off && page_len && masks && opt && pat_len && k && jobs && scratch && best && n_hits && hits,
                "omp_page_pattern_search: null pointer");
  if (const int rc = pg_check_args("omp_page_pattern_search", "patterns", n_jobs, n_pages, n_patterns, pool_bytes, sigma, max_hits)) return rc;
  const int64_t need = (int64_t)n_jobs * 64 * max_hits * (int64_t)sizeof(int2);
  OMP_CHECK_ARG(scratch_bytes >= need, "omp_page_pattern_search: %lld bytes of scratch, %d jobs at max_hits %d need %lld", (long long)scratch_bytes,
                n_jobs, max_hits, (long long)need);
  OMP_CHECK_ARG(((uintptr_t)scratch & 7) == 0 && ((uintptr_t)masks & 7) == 0 && ((uintptr_t)opt & 7) == 0,
                "omp_page_pattern_search: scratch, masks and opt must be 8-byte aligned");
  hipLaunchKernelGGL(page_pattern_kernel, dim3((unsigned)n_jobs), dim3(64), 0, (hipStream_t)s, pool, pool_bytes, page_off, page_len, n_pages,
                     reinterpret_cast<const u64*>(masks), reinterpret_cast<const u64*>(opt), pat_len, k, n_patterns, jobs, sigma, max_hits,
                     reinterpret_cast<int2*>(scratch), best, n_hits, hits);
  OMP_CHECK_LAUNCH("omp_page_pattern_search");
  return OMP_OK;
}
