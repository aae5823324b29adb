// Page expressions: where a regular EXPRESSION -- groups, alternation, real loops over character classes -- stands in the text of a read
// page, exactly or within k <= 4 insertions, deletions and substitutions (section 31).  utils/page_regex.py
// (ends_cpu / search_cpu and dist_cpu / fuzzy_start / fuzzy_search_cpu: the specification; ends_chunked and dist_chunked: this kernel's
// split) and this kernel agree on every integer.  An expression is Glushkov's position automaton of 1 .. 64 positions: first and last (the
// positions a match can begin / end with) and follow[i] (the positions that can come after position i), one 64-bit word each.  Bit i of
// the state D says that a match prefix has just consumed a character at position i:
//   D_0 = 0, D_j = (Follow(D_{j-1}) | first) & B(t_j), Follow(D) = OR of follow[i] over the bits i of D; column j is an END iff D_j & last.
// With errors the rows are Wu and Manber's, as in page_pattern.hip, over Follow instead of a shift:
//   Fol(X) = Follow(X) | first;  before any text R_0 = 0, R_i = Fol(R_{i-1});  at a column with class word B
//     R'_0 = Fol(R_0) & B,  R'_i = (Fol(R_i) & B) | Fol(R_{i-1}) | R_{i-1} | Fol(R'_{i-1})      match, substitution, insertion, deletion
//   v_j = the least i with R'_i & last != 0, else k + 1.  2 k + 1 Follow lookups a column, k + 1 of them in a dependent chain.
// The exact search IS the search with errors at k = 0: one row, D = R_0, v_j = 0 at an end and 1 elsewhere.
//
//   page_regex_kernel<K1_MAX>   one wave (a 64-thread workgroup) per job (page, expression); the job frame (the refusal, the class table,
//                               the slot scan, the tail) is page_frame.h's.  The body is instantiated on NB = ceil(P / 8) and on
//                               K1 = k + 1 <= K1_MAX, so the rows, the planes and the carry words are registers, and the job's (uniform)
//                               P and k pick one.  omp_page_regex_search launches <1>: k is 0, no tolerance is read, and the kernel holds
//                               the one-row bodies only, so its register budget is that of one row.  omp_page_regex_fuzzy_search
//                               launches <5>.
//     tables    Follow(D) is one lookup per byte of D: T[b][v] = OR of follow[8 b + i] over the bits i of v, 8-byte words, b < NB,
//               built in LDS by the wave from the expression's 64 follow words (16 KB at the most).
//     chunks    lane l owns the columns cs + 1 .. cs + 128, cs = 128 (64 r + l) in round r.  A match has no length bound, so there is no
//               warm-up.  The step is R' = L(R) | constant with L linear over union, so:
//               1. the speculative pass: every lane runs its chunk from the deletion-only rows (at k = 0: from D = 0; lane 0: from the
//                  exact exit rows of the round before), first injected at every column, and keeps K1 END PLANES of two words (plane i
//                  holds a column iff R_i & last != 0 there) and its exit rows X;
//               2. carry rounds: every lane l >= 1 that holds text takes the K1 rows X of lane l - 1, keeps the bits it has not carried
//                  yet (new_i = in_i & ~carried_i), runs them through L WITHOUT any first, ORs the ends into the planes and the rows after
//                  its last column into X, and leaves the chunk as soon as every row is 0;
//               3. until a ballot finds no lane with a new bit in any row.  carried only grows, so the rounds end; a bounded expression's
//                  carry dies within about P + k characters (insertion moves a carried bit up one row a column), a.*b degenerates to the
//                  serial run: slow and exact.
//     text      the round's 8192 characters staged in LDS with 4 bytes of padding per 128: the lanes' bytes fall in different banks.
//     mask      LDS, [sigma + 1] words; row sigma is 0: every code at or above sigma reads it.
//     hits      v_j is the number of planes without column j, and hit_ends' rule (v_j <= k, v_j <= v_{j-1}, v_j < v_{j+1} or j == n) is
//               bitwise on the planes against themselves shifted by one column either way (at k = 0: a set bit whose next column is no
//               end); the neighbour columns of a lane's bits 0 and 127 come from the lane before and after by one lane shift.  The LAST
//               column of a round cannot be judged before the first column of the next round is known: its distance and whether it
//               passed the first two conditions are carried (uniform), and that hit is emitted before the next round's.
//     slots     a scan of the counts over the lanes, then every lane writes (end | dist << 16) to the slots < H straight from its
//               registers: no per-lane lists, no scratch, no atomics, ascending ends whatever the scheduling.
//     starts    after the last round the byte tables are rebuilt from pred in the same LDS, and lane g < min(n_hits, H) walks hit g back
//               over the text in global memory with the same step over pred, last injected into row i while fewer than i + 1 characters
//               are consumed; s is remembered whenever R_dist & first.  No cap.
// A job out of range (a page or expression that is not there, P outside 1 .. 64, bits of first, last, a follow or a pred row at or above
// P, a non-zero row at or above P, first == 0 or last == 0, a page above 65535 characters, a range outside the pool, and with errors k
// outside 0 .. 4) is REFUSED on the device: n_hits = -1, best and hits -1, and nothing outside the pool is read.  Nothing is allocated and
// nothing synchronises.
#include "page_frame.h"

namespace {

constexpr int PR_K_MAX = 4;            // errors at the most
constexpr int PR_TEXT_BYTES = PG_ROUND + 4 * 64;           // 4 bytes of padding per chunk
constexpr int PR_NO_KEY = 0x7fffffff;

static_assert(PR_K_MAX < 8, "page_regex layout");

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

// one column: inj_old[i] is ORed into Follow of the OLD row i, inj_new[i] into Follow of the NEW row i (the deletion term)
template <int NB, int K1>
__device__ __forceinline__ void pr_step(const u64* T, u64 (&R)[K1], const u64 (&inj_old)[K1], const u64 (&inj_new)[K1], u64 B) {
  u64 below = pr_move<NB>(T, R[0]) | inj_old[0];           // Fol of the old row i - 1
  u64 old = R[0];
  R[0] = below & B;
#pragma unroll
  for (int i = 1; i < K1; ++i) {
    const u64 self = pr_move<NB>(T, R[i]) | inj_old[i];
    const u64 nw = (self & B) | below | old | pr_move<NB>(T, R[i - 1]) | inj_new[i - 1];
    old = R[i];
    below = self;
    R[i] = nw;
  }
}

// the hits of one job, by the whole wave -> n_hits; slot[g] = end | dist << 16 of hit g < H; *key_out this lane's least (dist << 20 | end)
template <int NB, int K1>
__device__ __forceinline__ int pr_ends(const uint8_t* __restrict__ t, int n, u64 first, u64 last, int sigma, int H, const u64* mask, const u64* T,
                                       uint8_t* text, int* slot, int* key_out) {
  const int lane = threadIdx.x;
  u64 with_first[K1], without[K1], init[K1], carry[K1];
  init[0] = 0;
#pragma unroll
  for (int i = 0; i < K1; ++i) {
    with_first[i] = first;
    without[i] = 0;
    if (i > 0) init[i] = pr_move<NB>(T, init[i - 1]) | first;  // deletions only
  }
#pragma unroll
  for (int i = 0; i < K1; ++i) carry[i] = init[i];         // the exact rows after the round before
  int pv = K1;                                             // v of the last column of the round before; v_0 = k + 1
  int pend = 0;                                            // that column passed v <= k and v <= v_{j-1}, and is not judged yet
  int base = 0;                                            // hits of the rounds before this one
  int key = PR_NO_KEY;
  for (int r0 = 0; r0 < n; r0 += PG_ROUND) {
    const int hi = min(PG_ROUND, n - r0);                  // characters of this round
    for (int rel = lane; rel < hi; rel += 64) text[rel + 4 * (rel / PG_CHUNK)] = t[r0 + rel];
    __syncthreads();
    const int cs = lane * PG_CHUNK;
    const int cnt = max(0, min(PG_CHUNK, hi - cs));        // characters of this lane
    const uint8_t* mine = text + cs + 4 * lane;
    auto class_of = [&](int i) -> u64 { return i < cnt ? mask[min((int)mine[i], sigma)] : 0ull; };
    // ---- the speculative pass, the lanes in step ----
    const int imax = min(PG_CHUNK, hi);                    // lane 0 has the most columns
    u64 R[K1], E0[K1], E1[K1];
#pragma unroll
    for (int i = 0; i < K1; ++i) {
      R[i] = lane == 0 ? carry[i] : init[i];
      E0[i] = 0;
      E1[i] = 0;
    }
    u64 bn = class_of(0);
    for (int c = 0; c < imax; ++c) {
      const u64 B = bn;
      bn = class_of(c + 1);                                // one column ahead: the two LDS reads do not depend on the recurrence
      pr_step<NB, K1>(T, R, with_first, with_first, B);
      const u64 bit = 1ull << (c & 63);
#pragma unroll
      for (int i = 0; i < K1; ++i) {
        const u64 e = (R[i] & last) ? bit : 0ull;
        if (c < 64) E0[i] |= e; else E1[i] |= e;
      }
    }
    // a lane that holds fewer than imax columns ran past its text (errors keep rows alive on B = 0): its planes end with its text.  Its
    // exit rows are never read: no lane after it holds text, and the round is the last.
    const u64 m0 = cnt >= 64 ? ~0ull : (1ull << cnt) - 1ull, m1 = cnt >= 128 ? ~0ull : cnt <= 64 ? 0ull : (1ull << (cnt - 64)) - 1ull;
#pragma unroll
    for (int i = 0; i < K1; ++i) {
      E0[i] &= m0;
      E1[i] &= m1;
    }
    // ---- carry rounds ----
    u64 X[K1], carried[K1];
#pragma unroll
    for (int i = 0; i < K1; ++i) {
      X[i] = R[i];
      carried[i] = 0;
    }
    for (;;) {
      u64 C[K1], any = 0;
#pragma unroll
      for (int i = 0; i < K1; ++i) {
        const u64 in = __shfl_up(X[i], 1, 64);
        C[i] = (lane > 0 && cnt > 0) ? in & ~carried[i] : 0ull;
        any |= C[i];
      }
      if (__ballot(any != 0) == 0) break;
#pragma unroll
      for (int i = 0; i < K1; ++i) carried[i] |= C[i];
      for (int c = 0; c < cnt && any != 0; ++c) {
        pr_step<NB, K1>(T, C, without, without, mask[min((int)mine[c], sigma)]);
        const u64 bit = 1ull << (c & 63);
        any = 0;
#pragma unroll
        for (int i = 0; i < K1; ++i) {
          const u64 e = (C[i] & last) ? bit : 0ull;
          E0[i] |= c < 64 ? e : 0ull;
          E1[i] |= c < 64 ? 0ull : e;
          any |= C[i];
        }
      }
#pragma unroll
      for (int i = 0; i < K1; ++i) X[i] |= C[i];          // C != 0 here only after the last column
    }
    // ---- hits: hit_ends on the planes ----
    u64 rise0 = 0, rise1 = 0, drop0 = 0, drop1 = 0;        // v_j > v_{j-1}; v_j < v_{j+1}
    int v_first = K1, v_last = K1;                         // v of the round's first and last column (uniform)
#pragma unroll
    for (int i = 0; i < K1; ++i) {
      u64 before = __shfl_up(E1[i] >> 63, 1, 64);          // the lane before's last column
      if (lane == 0) before = pv <= i ? 1ull : 0ull;
      u64 after = __shfl_down(E0[i] & 1ull, 1, 64);        // the next lane's first column
      if (lane == 63) after = 0;
      rise0 |= ((E0[i] << 1) | before) & ~E0[i];
      rise1 |= ((E1[i] << 1) | (E0[i] >> 63)) & ~E1[i];
      drop0 |= E0[i] & ~((E0[i] >> 1) | (E1[i] << 63));
      drop1 |= E1[i] & ~((E1[i] >> 1) | (after << 63));
      v_first -= (int)(__shfl(E0[i], 0, 64) & 1ull);
      v_last -= (int)(__shfl(E1[i], 63, 64) >> 63);
    }
    const u64 ok1 = E1[K1 - 1] & ~rise1;                   // v_j <= k and v_j <= v_{j-1}
    u64 H0 = E0[K1 - 1] & ~rise0 & drop0, H1 = ok1 & drop1;
    const bool more = n > r0 + PG_ROUND;                   // uniform: column r0 + 8192 has a next column, in the next round
    int pend_next = 0;
    if (more) {
      pend_next = (int)(__shfl(ok1, 63, 64) >> 63);
      if (lane == 63) H1 &= ~(1ull << 63);
    }
    if (pend && pv < v_first) {                            // the pending column of the round before is a hit: before this round's hits
      if (lane == 0 && base < H) slot[base] = r0 | (pv << 16);
      base += 1;
    }
    pend = pend_next;
    pv = v_last;
#pragma unroll
    for (int i = K1 - 1; i >= 0; --i)                      // the least row with an end, and its least column: rows below it have none
      if (E0[i] | E1[i]) key = min(key, (i << 20) | (r0 + cs + 1 + (E0[i] ? __ffsll((long long)E0[i]) - 1 : 64 + __ffsll((long long)E1[i]) - 1)));
    const int mine_hits = __popcll(H0) + __popcll(H1);
    int total;
    int at = base + pg_scan(mine_hits, &total) - mine_hits;
    while (H0 != 0 && at < H) {
      const int b = __ffsll((long long)H0) - 1;
      int d = K1;
#pragma unroll
      for (int i = 0; i < K1; ++i) d -= (int)((E0[i] >> b) & 1ull);
      slot[at++] = (r0 + cs + b + 1) | (d << 16);
      H0 &= H0 - 1;
    }
    while (H1 != 0 && at < H) {
      const int b = __ffsll((long long)H1) - 1;
      int d = K1;
#pragma unroll
      for (int i = 0; i < K1; ++i) d -= (int)((E1[i] >> b) & 1ull);
      slot[at++] = (r0 + cs + 64 + b + 1) | (d << 16);
      H1 &= H1 - 1;
    }
    base += total;
#pragma unroll
    for (int i = 0; i < K1; ++i) carry[i] = __shfl(X[i], 63, 64);
    __syncthreads();                                       // the next round overwrites text; slot is read after the last round
  }
  *key_out = key;
  return base;
}

// the start of the hit (end, dist): the least s whose anchored distance of t[s, end) to the language equals dist.  T holds the tables of
// pred; `used` characters are consumed, and row i still injects last while used <= i.
template <int NB, int K1>
__device__ __forceinline__ int pr_start(const uint8_t* __restrict__ t, int end, int dist, u64 first, u64 last, int sigma, const u64* mask, const u64* T) {
  u64 R[K1], inj_old[K1], inj_new[K1];
  R[0] = 0;
#pragma unroll
  for (int i = 1; i < K1; ++i) R[i] = pr_move<NB>(T, R[i - 1]) | last;
  int s = end, found = -2, used = 0;                       // -2 cannot happen: (end, dist) is a hit
  for (;;) {
    u64 Rd = R[0];
#pragma unroll
    for (int i = 1; i < K1; ++i) Rd = dist >= i ? R[i] : Rd;
    if (used > 0 && (Rd & first)) found = s;
    if (s == 0 || (Rd == 0 && used > dist)) break;         // the rows 0 .. dist and their flags are empty: rows grow with i
    --s;
#pragma unroll
    for (int i = 0; i < K1; ++i) {
      inj_old[i] = used <= i ? last : 0ull;
      inj_new[i] = used + 1 <= i ? last : 0ull;
    }
    pr_step<NB, K1>(T, R, inj_old, inj_new, mask[min((int)t[s], sigma)]);
    ++used;
  }
  return found;
}

template <int NB, int K1>
__device__ __forceinline__ int pr_job(const uint8_t* __restrict__ t, int n, u64 first, u64 last, int sigma, int H, const u64* mask, u64* T, const u64* rows,
                                      uint8_t* text, int* slot, int32_t* jhits, int* key_out) {
  const int lane = threadIdx.x;
  pr_build<NB>(T, rows);                                   // follow
  __syncthreads();
  const int base = pr_ends<NB, K1>(t, n, first, last, sigma, H, mask, T, text, slot, key_out);
  __syncthreads();
  pr_build<NB>(T, rows + PG_POS_MAX);                      // pred, in the same LDS
  __syncthreads();
  if (lane < min(base, H)) {
    const int end = slot[lane] & 0xffff, dist = slot[lane] >> 16;
    jhits[3 * lane] = end;
    jhits[3 * lane + 1] = dist;
    jhits[3 * lane + 2] = pr_start<NB, K1>(t, end, dist, first, last, sigma, mask, T);
  }
  return base;
}

// K1 = k + 1 <= K1_MAX picks the body; an instance with K1_MAX = 1 holds the one-row body only
template <int NB, int K1_MAX>
__device__ __forceinline__ int pr_job_k(int K1, const uint8_t* __restrict__ t, int n, u64 first, u64 last, int sigma, int H, const u64* mask, u64* T,
                                        const u64* rows, uint8_t* text, int* slot, int32_t* jhits, int* key_out) {
  if constexpr (K1_MAX == 1) {
    return pr_job<NB, 1>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, key_out);
  } else {
    static_assert(K1_MAX == 5, "one case per K1");
    switch (K1) {                                          // uniform
      case 1: return pr_job<NB, 1>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, key_out);
      case 2: return pr_job<NB, 2>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, key_out);
      case 3: return pr_job<NB, 3>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, key_out);
      case 4: return pr_job<NB, 4>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, key_out);
      default: return pr_job<NB, 5>(t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, key_out);
    }
  }
}

// tol: one tolerance per expression; the instance with K1_MAX = 1 does not read it
template <int K1_MAX>
__global__ __launch_bounds__(64) void page_regex_kernel(const uint8_t* __restrict__ pool, int64_t pool_bytes, const int32_t* __restrict__ page_off,
                                                        const int32_t* __restrict__ page_len, int n_pages, const u64* __restrict__ masks,
                                                        const u64* __restrict__ firsts, const u64* __restrict__ lasts, const u64* __restrict__ follow,
                                                        const u64* __restrict__ pred, const int32_t* __restrict__ pat_len,
                                                        const int32_t* __restrict__ tol, int n_expr, const int32_t* __restrict__ jobs, int sigma, int H,
                                                        int32_t* __restrict__ best, int32_t* __restrict__ n_hits, int32_t* __restrict__ hits) {
  __shared__ __align__(16) u64 T[8 * 256];
  __shared__ __align__(16) u64 mask[PG_SIGMA_MAX + 2];
  __shared__ __align__(16) u64 rows[2 * PG_POS_MAX];       // follow | pred
  __shared__ __align__(16) uint8_t text[PR_TEXT_BYTES];
  __shared__ int slot[PG_HITS_MAX];
  const int job = blockIdx.x, lane = threadIdx.x;
  int32_t* jhits = hits + (int64_t)job * H * 3;
  const int p = jobs[2 * job], qi = jobs[2 * job + 1];
  // all of this is uniform over the wave
  bool ok = p >= 0 && p < n_pages && qi >= 0 && qi < n_expr;
  int n = 0, P = 0, k = 0;
  int64_t po = 0;
  u64 first = 0, last = 0;
  if (ok) {
    n = page_len[p];
    po = page_off[p];
    P = pat_len[qi];
    if constexpr (K1_MAX > 1) k = tol[qi];
    first = firsts[qi];
    last = lasts[qi];
    ok = n >= 0 && n <= PG_LEN_MAX && P >= 1 && P <= PG_POS_MAX && k >= 0 && k <= K1_MAX - 1 && po >= 0 && po + n <= pool_bytes && first != 0 &&
         last != 0 && (P == 64 || ((first | last) >> P) == 0);
    if (ok) {                                              // lane i holds row i of follow and of pred
      const u64 f = follow[(int64_t)qi * PG_POS_MAX + lane], b = pred[(int64_t)qi * PG_POS_MAX + lane];
      const bool mine = lane < P ? (P == 64 || ((f | b) >> P) == 0) : (f | b) == 0;
      ok = __ballot(!mine) == 0;
      rows[lane] = f;
      rows[PG_POS_MAX + lane] = b;
    }
  }
  if (!ok) {
    pg_refuse(job, H, best, n_hits, jhits);
    return;
  }
  pg_classes(mask, masks, qi, sigma);
  __syncthreads();
  const uint8_t* __restrict__ t = pool + po;
  int key = PR_NO_KEY, base = 0;
  switch ((P + 7) >> 3) {                                  // uniform
    case 1: base = pr_job_k<1, K1_MAX>(k + 1, t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &key); break;
    case 2: base = pr_job_k<2, K1_MAX>(k + 1, t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &key); break;
    case 3: base = pr_job_k<3, K1_MAX>(k + 1, t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &key); break;
    case 4: base = pr_job_k<4, K1_MAX>(k + 1, t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &key); break;
    case 5: base = pr_job_k<5, K1_MAX>(k + 1, t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &key); break;
    case 6: base = pr_job_k<6, K1_MAX>(k + 1, t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &key); break;
    case 7: base = pr_job_k<7, K1_MAX>(k + 1, t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &key); break;
    default: base = pr_job_k<8, K1_MAX>(k + 1, t, n, first, last, sigma, H, mask, T, rows, text, slot, jhits, &key); break;
  }
  pg_tail(jhits, base, H);
  for (int d = 32; d >= 1; d >>= 1) key = min(key, __shfl_xor(key, d, 64));
  if (lane == 0) {
    n_hits[job] = base;
    best[2 * job] = key == PR_NO_KEY ? k + 1 : key >> 20;
    best[2 * job + 1] = key == PR_NO_KEY ? 0 : key & 0xfffff;
  }
}

// the checks and the launch of both entry points; k is null for the exact search
template <int K1_MAX>
int pr_launch(const char* name, const uint8_t* pool, int64_t pool_bytes, const int32_t* page_off, const int32_t* page_len, int n_pages, const uint64_t* masks,
              const uint64_t* first, const uint64_t* last, const uint64_t* follow, const uint64_t* pred, const int32_t* pat_len, const int32_t* k,
              int n_expressions, const int32_t* jobs, int n_jobs, int sigma, int max_hits, int32_t* best, int32_t* n_hits, int32_t* hits, omp_stream_t s) {
  OMP_CHECK_ARG(pool && page_off && page_len && masks && first && last && follow && pred && pat_len && (k || K1_MAX == 1) && jobs && best && n_hits && hits,
                "%s: null pointer", name);
  if (const int rc = pg_check_args(name, "expressions", n_jobs, n_pages, n_expressions, pool_bytes, sigma, max_hits)) return rc;
  OMP_CHECK_ARG((((uintptr_t)masks | (uintptr_t)first | (uintptr_t)last | (uintptr_t)follow | (uintptr_t)pred) & 7) == 0,
                "%s: masks, first, last, follow and pred must be 8-byte aligned", name);
  hipLaunchKernelGGL(page_regex_kernel<K1_MAX>, dim3((unsigned)n_jobs), dim3(64), 0, (hipStream_t)s, pool, pool_bytes, page_off, page_len, n_pages,
                     reinterpret_cast<const u64*>(masks), reinterpret_cast<const u64*>(first), reinterpret_cast<const u64*>(last),
                     reinterpret_cast<const u64*>(follow), reinterpret_cast<const u64*>(pred), pat_len, k, n_expressions, jobs, sigma, max_hits, best,
                     n_hits, hits);
  OMP_CHECK_LAUNCH(name);
  return OMP_OK;
}

}  // namespace

extern "C" int omp_page_regex_search(const uint8_t* pool, int64_t pool_bytes, const int32_t* page_off, const int32_t* page_len, int n_pages,
                                     const uint64_t* masks, const uint64_t* first, const uint64_t* last, const uint64_t* follow, const uint64_t* pred,
                                     const int32_t* pat_len, int n_expressions, const int32_t* jobs, int n_jobs, int sigma, int max_hits, int32_t* best,
                                     int32_t* n_hits, int32_t* hits, omp_stream_t s) {
  return pr_launch<1>("omp_page_regex_search", pool, pool_bytes, page_off, page_len, n_pages, masks, first, last, follow, pred, pat_len, nullptr,
                      n_expressions, jobs, n_jobs, sigma, max_hits, best, n_hits, hits, s);
}

extern "C" int omp_page_regex_fuzzy_search(const uint8_t* pool, int64_t pool_bytes, const int32_t* page_off, const int32_t* page_len, int n_pages,
                                           const uint64_t* masks, const uint64_t* first, const uint64_t* last, const uint64_t* follow,
                                           const uint64_t* pred, const int32_t* pat_len, const int32_t* k, int n_expressions, const int32_t* jobs,
                                           int n_jobs, int sigma, int max_hits, int32_t* best, int32_t* n_hits, int32_t* hits, omp_stream_t s) {
  return pr_launch<PR_K_MAX + 1>("omp_page_regex_fuzzy_search", pool, pool_bytes, page_off, page_len, n_pages, masks, first, last, follow, pred, pat_len,
                                 k, n_expressions, jobs, n_jobs, sigma, max_hits, best, n_hits, hits, s);
}
