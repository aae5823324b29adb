// Page expressions: where a regular EXPRESSION -- groups, alternation, real loops over character classes -- stands in the text of a read
// page, exactly.  utils/page_regex.py (ends_cpu / search_cpu: the specification; ends_chunked: this kernel's split)
// and this kernel agree on every integer.  An expression is Glushkov's position automaton of 1 .. 64 positions: first and last (the
// positions a match can begin / end with) and follow[i] (the positions that can come after position i), one 64-bit word each.  Bit i of
// the state D says that a match prefix has just consumed a character at position i:
//   D_0 = 0, D_j = (Follow(D_{j-1}) | first) & B(t_j), Follow(D) = OR of follow[i] over the bits i of D; column j is an END iff D_j & last.
//
//   page_regex_kernel   one wave (a 64-thread workgroup) per job (page, expression).
//     tables    Follow(D) is one lookup per byte of D: T[b][v] = OR of follow[8 b + i] over the bits i of v, 8-byte words, b < NB =
//               ceil(P / 8), built in LDS by the wave from the expression's 64 follow words (16 KB at the most).  The body is instantiated
//               on NB = 1 .. 8 and the job's (uniform) P picks one.
//     chunks    lane l owns the columns cs + 1 .. cs + 128, cs = 128 (64 r + l) in round r.  A match has no length bound, so there is no
//               warm-up.  The step is linear over union, so:
//               1. the speculative pass: every lane runs its chunk from D = 0 (lane 0: from the exact exit state of the round before),
//                  first injected at every column, and keeps its end bits E (two words) and its exit state X;
//               2. carry rounds: every lane l >= 1 that holds text takes X of lane l - 1, keeps the bits it has not carried yet
//                  (new = in & ~carried), runs them through its chunk WITHOUT injection (C = Follow(C) & B), ORs C & last into E and C
//                  after its last column into X, and leaves the chunk as soon as C == 0;
//               3. until a ballot finds no lane with new bits.  carried only grows, so the rounds end; a bounded expression's carry dies
//                  within P characters (two rounds), a.*b degenerates to the serial run: slow and exact.
//     text      the round's 8192 characters staged in LDS with 4 bytes of padding per 128, as page_pattern.hip.
//     mask      LDS, [sigma + 1] words; row sigma is 0: every code at or above sigma reads it.
//     hits      a set bit of E whose next column is no end; the next column of a lane's bit 127 is the next lane's bit 0 (one lane
//               shift).  An exclusive scan of the counts over the lanes, then every lane writes its ends to the slots < H straight from
//               its registers: no per-lane lists, no scratch, no atomics, ascending ends whatever the scheduling.  The LAST column of a
//               round cannot be judged before the first column of the next round is known: one uniform pending flag, and that hit is
//               emitted before the next round's.
//     starts    after the last round the byte tables are rebuilt from pred in the same LDS, and lane g < min(n_hits, H) walks hit g back
//               over the text in global memory: R = last & B(t_end); while R: if R & first remember s; R = Pred(R) & B(t_{s-1}).  No cap.
// A job out of range (a page or expression that is not there, P outside 1 .. 64, bits of first, last, a follow or a pred row at or above
// P, a non-zero row at or above P, first == 0 or last == 0, a page above 65535 characters, a range outside the pool) is REFUSED on the
// device: n_hits = -1, best and hits -1, and nothing outside the pool is read.  Nothing is allocated and nothing synchronises.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int PR_LEN_MAX = 65535;      // characters a page
constexpr int PR_POS_MAX = 64;         // positions an expression
constexpr int PR_CHUNK = 128;          // columns per lane
constexpr int PR_HITS_MAX = 64;        // hits kept per job
constexpr int PR_SIGMA_MAX = 254;
constexpr int PR_JOBS_MAX = 1 << 20;
constexpr int PR_ROUND = 64 * PR_CHUNK;                    // columns per round of the wave
constexpr int PR_TEXT_BYTES = PR_ROUND + 4 * 64;           // 4 bytes of padding per chunk: the lanes' bytes fall in different banks
constexpr int PR_NO_END = 0x7fffffff;

static_assert(PR_HITS_MAX <= 64 && PR_POS_MAX == 64 && PR_CHUNK == 128, "page_regex layout");

// T[b][v] = OR of rows[8 b + i] over the bits i of v, b < NB
template <int NB>
__device__ __forceinline__ void pr_build(u64* T, const u64* rows) {
  for (int e = threadIdx.x; e < NB * 256; e += 64) {
    const int b = e >> 8, v = e & 255;
    u64 w = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if ((v >> i) & 1) w |= rows[8 * b + i];
    T[e] = w;
  }
}

template <int NB>
__device__ __forceinline__ u64 pr_move(const u64* T, u64 D) {
  u64 F = 0;
#pragma unroll
  for (int b = 0; b < NB; ++b) F |= T[b * 256 + (int)((D >> (8 * b)) & 255ull)];
  return F;
}

// The ends of one job, by the whole wave -> n_hits; slot[g] the end of hit g < H; *least_out this lane's least end
template <int NB>
__device__ __forceinline__ int pr_ends(const uint8_t* __restrict__ t, int n, u64 first, u64 last, int sigma, int H, const u64* mask, const u64* T,
                                       uint8_t* text, int* slot, int* least_out) {
  const int lane = threadIdx.x;
  u64 carry = 0;                                           // the exact state after the round before
  int pend = 0;                                            // the last column of the round before is an end, and not judged yet
  int base = 0;                                            // hits of the rounds before this one
  int least = PR_NO_END;
  for (int r0 = 0; r0 < n; r0 += PR_ROUND) {
    const int hi = min(PR_ROUND, n - r0);                  // characters of this round
    for (int rel = lane; rel < hi; rel += 64) text[rel + 4 * (rel / PR_CHUNK)] = t[r0 + rel];
    __syncthreads();
    const int cs = lane * PR_CHUNK;
    const int cnt = max(0, min(PR_CHUNK, hi - cs));        // characters of this lane
    const uint8_t* mine = text + cs + 4 * lane;
    auto class_of = [&](int i) -> u64 { return i < cnt ? mask[min((int)mine[i], sigma)] : 0ull; };
    // ---- the speculative pass, the lanes in step; a lane past its text runs on B = 0 ----
    const int imax = min(PR_CHUNK, hi);                    // lane 0 has the most columns
    u64 D = lane == 0 ? carry : 0ull, E0 = 0, E1 = 0;
    u64 bn = class_of(0);
    for (int i = 0; i < imax; ++i) {
      const u64 B = bn;
      bn = class_of(i + 1);                                // one column ahead: the two LDS reads do not depend on the recurrence
      D = (pr_move<NB>(T, D) | first) & B;
      const u64 e = (D & last) ? 1ull << (i & 63) : 0ull;
      if (i < 64) E0 |= e; else E1 |= e;
    }
    // ---- carry rounds ----
    u64 X = D, carried = 0;
    for (;;) {
      const u64 in = __shfl_up(X, 1, 64);
      const u64 nw = (lane > 0 && cnt > 0) ? in & ~carried : 0ull;
      if (__ballot(nw != 0) == 0) break;
      carried |= nw;
      u64 C = nw;
      for (int i = 0; i < cnt && C != 0; ++i) {
        C = pr_move<NB>(T, C) & mask[min((int)mine[i], sigma)];
        const u64 e = (C & last) ? 1ull << (i & 63) : 0ull;
        E0 |= i < 64 ? e : 0ull;
        E1 |= i < 64 ? 0ull : e;
      }
      X |= C;                                              // C != 0 here only after the last column
    }
    carry = __shfl(X, 63, 64);
    // ---- hits: an end whose next column is none ----
    u64 low = __shfl_down(E0 & 1ull, 1, 64);               // the next lane's first column
    if (lane == 63) low = 0;
    u64 H0 = E0 & ~((E0 >> 1) | (E1 << 63)), H1 = E1 & ~((E1 >> 1) | (low << 63));
    const bool more = n > r0 + PR_ROUND;                   // uniform: column r0 + 8192 has a next column, in the next round
    int pend_next = 0;
    if (more) {
      pend_next = (int)(__shfl(E1, 63, 64) >> 63);
      if (lane == 63) H1 &= ~(1ull << 63);
    }
    if (pend && !(__shfl(E0, 0, 64) & 1ull)) {             // the pending end of the round before is a hit: before this round's hits
      if (lane == 0 && base < H) slot[base] = r0;
      base += 1;
    }
    pend = pend_next;
    if (E0 | E1) least = min(least, r0 + cs + 1 + (E0 ? __ffsll((long long)E0) - 1 : 64 + __ffsll((long long)E1) - 1));
    const int mine_hits = __popcll(H0) + __popcll(H1);
    int incl = mine_hits;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    const int total = __shfl(incl, 63, 64);
    int at = base + incl - mine_hits;
    while (H0 != 0 && at < H) {
      slot[at++] = r0 + cs + __ffsll((long long)H0);
      H0 &= H0 - 1;
    }
    while (H1 != 0 && at < H) {
      slot[at++] = r0 + cs + 64 + __ffsll((long long)H1);
      H1 &= H1 - 1;
    }
    base += total;
    __syncthreads();                                       // the next round overwrites text; slot is read after the last round
  }
  *least_out = least;
  return base;
}

// the start of the hit that ends at column `end`: the least s with t[s, end) in the language.  T holds the tables of pred.
template <int NB>
__device__ __forceinline__ int pr_start(const uint8_t* __restrict__ t, int end, u64 first, u64 last, int sigma, const u64* mask, const u64* T) {
  int s = end - 1, found = -2;                             // -2 cannot happen: `end` is an end
  u64 R = last & mask[min((int)t[s], sigma)];
  while (R != 0) {
    if (R & first) found = s;
    if (s == 0) break;
    --s;
    R = pr_move<NB>(T, R) & mask[min((int)t[s], sigma)];
  }
  return found;
}

template <int NB>
__device__ __forceinline__ int pr_job(const uint8_t* __restrict__ t, int n, u64 first, u64 last, int sigma, int H, const u64* mask, u64* T, const u64* rows,
                                      uint8_t* text, int* slot, int32_t* jhits, int* least_out) {
  const int lane = threadIdx.x;
  pr_build<NB>(T, rows);                                   // follow
  __syncthreads();
  const int base = pr_ends<NB>(t, n, first, last, sigma, H, mask, T, text, slot, least_out);
  __syncthreads();
  pr_build<NB>(T, rows + PR_POS_MAX);                      // pred, in the same LDS
  __syncthreads();
  if (lane < min(base, H)) {
    const int end = slot[lane];
    jhits[3 * lane] = end;
    jhits[3 * lane + 1] = 0;
    jhits[3 * lane + 2] = pr_start<NB>(t, end, first, last, sigma, mask, T);
  }
  return base;
}

__global__ __launch_bounds__(64) void page_regex_kernel(const uint8_t* __restrict__ pool, int64_t pool_bytes, const int32_t* __restrict__ page_off,
                                                        const int32_t* __restrict__ page_len, int n_pages, const u64* __restrict__ masks,
                                                        const u64* __restrict__ firsts, const u64* __restrict__ lasts, const u64* __restrict__ follow,
                                                        const u64* __restrict__ pred, const int32_t* __restrict__ pat_len, int n_expr,
                                                        const int32_t* __restrict__ jobs, int sigma, int H, int32_t* __restrict__ best,
                                                        int32_t* __restrict__ n_hits, int32_t* __restrict__ hits) {
  __shared__ __align__(16) u64 T[8 * 256];
  __shared__ __align__(16) u64 mask[PR_SIGMA_MAX + 2];
  __shared__ __align__(16) u64 rows[2 * PR_POS_MAX];       // follow | pred
  __shared__ __align__(16) uint8_t text[PR_TEXT_BYTES];
  __shared__ int slot[PR_HITS_MAX];
  const int job = blockIdx.x, lane = threadIdx.x;
  int32_t* jhits = hits + (int64_t)job * H * 3;
  const int p = jobs[2 * job], qi = jobs[2 * job + 1];
  // all of this is uniform over the wave
  bool ok = p >= 0 && p < n_pages && qi >= 0 && qi < n_expr;
  int n = 0, P = 0;
  int64_t po = 0;
  u64 first = 0, last = 0;
  if (ok) {
    n = page_len[p];
    po = page_off[p];
    P = pat_len[qi];
    first = firsts[qi];
    last = lasts[qi];
    ok = n >= 0 && n <= PR_LEN_MAX && P >= 1 && P <= PR_POS_MAX && po >= 0 && po + n <= pool_bytes && first != 0 && last != 0 &&
         (P == 64 || ((first | last) >> P) == 0);
    if (ok) {                                              // lane i holds row i of follow and of pred
      const u64 f = follow[(int64_t)qi * PR_POS_MAX + lane], b = pred[(int64_t)qi * PR_POS_MAX + lane];
      const bool mine = lane < P ? (P == 64 || ((f | b) >> P) == 0) : (f | b) == 0;
      ok = __ballot(!mine) == 0;
      rows[lane] = f;
      rows[PR_POS_MAX + lane] = b;
    }
  }
  if (!ok) {
    if (lane == 0) {
      n_hits[job] = -1;
      best[2 * job] = -1;
      best[2 * job + 1] = -1;
    }
    for (int i = lane; i < 3 * H; i += 64) jhits[i] = -1;
    return;
  }
  const u64* __restrict__ row = masks + (int64_t)qi * (sigma + 1);
  for (int c = lane; c < sigma; c += 64) mask[c] = row[c];
  if (lane == 0) mask[sigma] = 0;                          // whatever the table holds there: a code at or above sigma is in no class
  __syncthreads();
  const uint8_t* __restrict__ t = pool + po;
  int least = PR_NO_END, base = 0;
  switch ((P + 7) >> 3) {                                  // uniform
    case 1: base = pr_job<1>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &least); break;
    case 2: base = pr_job<2>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &least); break;
    case 3: base = pr_job<3>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &least); break;
    case 4: base = pr_job<4>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &least); break;
    case 5: base = pr_job<5>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &least); break;
    case 6: base = pr_job<6>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &least); break;
    case 7: base = pr_job<7>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &least); break;
    default: base = pr_job<8>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &least); break;
  }
  for (int g = min(base, H) + lane; g < H; g += 64) {
    jhits[3 * g] = -1;
    jhits[3 * g + 1] = -1;
    jhits[3 * g + 2] = -1;
  }
  for (int d = 32; d >= 1; d >>= 1) least = min(least, __shfl_xor(least, d, 64));
  if (lane == 0) {
    n_hits[job] = base;
    best[2 * job] = least == PR_NO_END ? 1 : 0;
    best[2 * job + 1] = least == PR_NO_END ? 0 : least;
  }
}

}  // namespace

extern "C" int omp_page_regex_search(const uint8_t* pool, int64_t pool_bytes, const int32_t* page_off, const int32_t* page_len, int n_pages,
                                     const uint64_t* masks, const uint64_t* first, const uint64_t* last, const uint64_t* follow, const uint64_t* pred,
                                     const int32_t* pat_len, int n_expressions, const int32_t* jobs, int n_jobs, int sigma, int max_hits, int32_t* best,
                                     int32_t* n_hits, int32_t* hits, omp_stream_t s) {
  OMP_CHECK_ARG(pool && page_off && page_len && masks && first && last && follow && pred && pat_len && jobs && best && n_hits && hits,
                "omp_page_regex_search: null pointer");
  OMP_CHECK_ARG(n_jobs > 0 && n_jobs <= PR_JOBS_MAX && n_pages > 0 && n_expressions > 0 && pool_bytes >= 0 && pool_bytes <= 0x7fffffffll,
                "omp_page_regex_search: %d jobs (1 .. %d), %d pages, %d expressions, %lld pool bytes", n_jobs, PR_JOBS_MAX, n_pages, n_expressions,
                (long long)pool_bytes);
  OMP_CHECK_ARG(sigma >= 0 && sigma <= PR_SIGMA_MAX, "omp_page_regex_search: sigma %d (0 .. %d)", sigma, PR_SIGMA_MAX);
  OMP_CHECK_ARG(max_hits >= 1 && max_hits <= PR_HITS_MAX, "omp_page_regex_search: max_hits %d (1 .. %d)", max_hits, PR_HITS_MAX);
  OMP_CHECK_ARG((((uintptr_t)masks | (uintptr_t)first | (uintptr_t)last | (uintptr_t)follow | (uintptr_t)pred) & 7) == 0,
                "omp_page_regex_search: masks, first, last, follow and pred must be 8-byte aligned");
  hipLaunchKernelGGL(page_regex_kernel, dim3((unsigned)n_jobs), dim3(64), 0, (hipStream_t)s, pool, pool_bytes, page_off, page_len, n_pages,
                     reinterpret_cast<const u64*>(masks), reinterpret_cast<const u64*>(first), reinterpret_cast<const u64*>(last),
                     reinterpret_cast<const u64*>(follow), reinterpret_cast<const u64*>(pred), pat_len, n_expressions, jobs, sigma, max_hits, best, n_hits,
                     hits);
  OMP_CHECK_LAUNCH("omp_page_regex_search");
  return OMP_OK;
}
