// The job frame of the page searches, held ONCE for the units that run it: page_search.hip (phrases, section 25),
// page_pattern.hip (shapes, section 29) and page_regex.hip (expressions, exactly and with errors, sections 30 and 31).
//
//   one wave (a 64-thread workgroup) per job (page, what is looked for); lane l owns the end columns cs + 1 .. cs + 128 of the text,
//   cs = 128 (64 r + l) in round r, so a page of up to 65535 characters takes up to 8 rounds.
//     pg_refuse    a job out of range is REFUSED on the device: n_hits = -1, best and the 3 H hit words -1, nothing outside the pool read.
//     pg_classes   LDS, [sigma + 1] 64-bit words copied from the job's row of the class table: bit i of mask[c] says that code c is in the
//                  class of position i.  Row sigma is 0 whatever the table holds there: every code at or above sigma reads it.
//     pg_scan      the inclusive scan of the lanes' hit counts: lane l's first slot is base + incl - cnt, in text order whatever the
//                  scheduling.  No atomics.
//     pg_tail      the hit slots at and above min(n_hits, H) are -1.  The best key and its reduction differ per unit and stay there.
//     pg_window    the round loop of the two searches with a bounded match (phrases and shapes): a lane starts `warm` columns before its
//                  chunk with a fresh column, because an alignment within the tolerance covers at most `warm` characters; the unit's
//                  Stepper holds the column.
//   pg_check_args  the host checks the four entry points share, with the entry's own name in the messages.
#pragma once
#include "common.h"

typedef unsigned long long u64;

constexpr int PG_LEN_MAX = 65535;      // characters a page: an end fits 16 bits
constexpr int PG_POS_MAX = 64;         // positions a pattern or an expression: one 64-bit word
constexpr int PG_CHUNK = 128;          // end columns per lane
constexpr int PG_HITS_MAX = 64;        // hits kept per job
constexpr int PG_SIGMA_MAX = 254;
constexpr int PG_JOBS_MAX = 1 << 20;
constexpr int PG_ROUND = 64 * PG_CHUNK;                    // end columns per round of the wave

static_assert(PG_HITS_MAX <= 64 && PG_POS_MAX == 64 && PG_CHUNK == 128 && PG_LEN_MAX < (1 << 16), "page_frame layout");

__device__ __forceinline__ void pg_refuse(int job, int H, int32_t* __restrict__ best, int32_t* __restrict__ n_hits, int32_t* jhits) {
  const int lane = threadIdx.x;
  if (lane == 0) {
    n_hits[job] = -1;
    best[2 * job] = -1;
    best[2 * job + 1] = -1;
  }
  for (int i = lane; i < 3 * H; i += 64) jhits[i] = -1;
}

// the caller's barrier follows
__device__ __forceinline__ void pg_classes(u64* mask, const u64* __restrict__ masks, int qi, int sigma) {
  const int lane = threadIdx.x;
  const u64* __restrict__ row = masks + (int64_t)qi * (sigma + 1);
  for (int c = lane; c < sigma; c += 64) mask[c] = row[c];
  if (lane == 0) mask[sigma] = 0;                          // whatever the table holds there: a code at or above sigma is in no class
}

// -> the sum of cnt over the lanes up to this one, itself included; *total that of all 64
__device__ __forceinline__ int pg_scan(int cnt, int* total) {
  const int lane = threadIdx.x;
  int incl = cnt;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  *total = __shfl(incl, 63, 64);
  return incl;
}

__device__ __forceinline__ void pg_tail(int32_t* jhits, int base, int H) {
  for (int g = min(base, H) + (int)threadIdx.x; g < H; g += 64) {
    jhits[3 * g] = -1;
    jhits[3 * g + 1] = -1;
    jhits[3 * g + 2] = -1;
  }
}

// The text of a round of pg_window in LDS: BEFORE characters before the round's first chunk to 1 after its last, 4 bytes of padding after
// every 128: the lanes walk their chunks in step, 33 dwords apart, on distinct banks.
template <int BEFORE>
struct PgText {
  static constexpr int STAGE = BEFORE + PG_ROUND + 1;      // characters staged per round
  static constexpr int BYTES = STAGE + 4 * (STAGE / PG_CHUNK + 1);
  static_assert(BYTES >= STAGE + 4 * ((STAGE - 1) / PG_CHUNK), "pg_window layout");
  // where staged character `rel` (0 = BEFORE characters before the round's first chunk) lives
  static __device__ __forceinline__ int at(int rel) { return rel + 4 * (rel / PG_CHUNK); }
};

// The rounds of one job with a bounded match, by the whole wave -> hits of all rounds; *key_out this lane's least (v << 32) | end.
// `word` is the job's table in LDS, [sigma + 1] words; text BYTES of PgText<BEFORE>; list this lane's H pairs of caller-owned scratch.
// A Stepper holds one lane's column and says
//   warm()               W <= BEFORE: the columns a lane runs before its chunk
//   stage_from()         the first staged character a round reads, 0 .. BEFORE - W
//   none()               the value of the fresh column, and of the empty match (none(), 0)
//   tol()                k: a column is a hit at v <= k
//   fresh()              the column before any text
//   step(B, v)           one column with table word B -> v_j from v_{j-1}
//   start(end, dist, at) the start of hit (end, dist), at(pos) the table word of text character pos, or -2
// A hit is a column with v_j <= k, v_j <= v_{j-1} and (j == n or v_j < v_{j+1}): one column past the chunk is read for the last test.
// A lane keeps the first H hits of its chunk as (end, dist) in its list; after the round the scan gives every lane its first slot, the lanes
// copy their lists to the LDS slot table, and lane g resolves the start of hit g while the text is still in LDS.
template <int BEFORE, class Stepper>
__device__ __forceinline__ int pg_window(Stepper& st, const uint8_t* __restrict__ t, int n, int sigma, int H, const u64* word, uint8_t* text, int2* slot,
                                         int2* list, int32_t* jhits, u64* key_out) {
  typedef PgText<BEFORE> Text;
  const int lane = threadIdx.x;
  const int k = st.tol(), W = st.warm();
  u64 key = ((u64)st.none() << 32);
  int base = 0;                                            // hits of the rounds before this one
  for (int r0 = 0; r0 < n; r0 += PG_ROUND) {
    // ---- stage t[r0 - BEFORE .. r0 + PG_ROUND] ----
    const int hi = min(Text::STAGE, n - r0 + BEFORE);      // staged characters that exist
    for (int rel = st.stage_from() + lane; rel < hi; rel += 64) {
      const int pos = r0 - BEFORE + rel;
      if (pos >= 0) text[Text::at(rel)] = t[pos];
    }
    __syncthreads();
    // ---- the lanes walk their chunks in step ----
    const int cs = r0 + lane * PG_CHUNK;
    st.fresh();
    int s0 = st.none(), s1 = s0, s2 = s0;                  // v_j, v_{j-1}, v_{j-2}
    int cnt = 0;
    const int imax = min(PG_CHUNK + 1, n - r0 + 1);        // lane 0 has the most columns left
    // the table word of column j, one column ahead of the recurrence: the two LDS reads do not depend on it
    auto word_of = [&](int j) -> u64 { return (j >= 1 && j <= n) ? word[min((int)text[Text::at(j - 1 - r0 + BEFORE)], sigma)] : 0ull; };
    u64 bn = word_of(cs + 1 - W);
    for (int i = 1 - W; i <= imax; ++i) {
      const int j = cs + i;
      const u64 B = bn;
      bn = i < imax ? word_of(j + 1) : 0ull;
      s2 = s1;
      s1 = s0;
      if (j >= 1 && j <= n) s0 = st.step(B, s0);           // a column below 1 is skipped: the chunk warms up from column 0, the fresh column
      const int e = j - 1;                                 // the column that can be judged now
      if (i >= 2 && e <= n) {                              // e is one of this lane's own columns
        const u64 ke = ((u64)s1 << 32) | (u64)e;
        if (ke < key) key = ke;
        if (s1 <= k && s1 <= s2 && (e == n || s1 < s0)) {
          if (cnt < H) list[cnt] = make_int2(e, s1);
          ++cnt;
        }
      }
    }
    int total;
    const int first = base + pg_scan(cnt, &total) - cnt;
    for (int i = 0; i < cnt && first + i < H; ++i) slot[first + i] = list[i];   // a lane reads back what it wrote itself
    __syncthreads();
    const int filled = min(base + total, H);
    if (lane >= base && lane < filled) {
      const int end = slot[lane].x, dist = slot[lane].y;
      const int start = st.start(end, dist, [&](int pos) -> u64 { return word[min((int)text[Text::at(pos - r0 + BEFORE)], sigma)]; });
      jhits[3 * lane] = end;
      jhits[3 * lane + 1] = dist;
      jhits[3 * lane + 2] = start;
    }
    base += total;
    __syncthreads();                                       // the next round overwrites text and slot
  }
  *key_out = key;
  return base;
}

// the checks the four entry points share, after the entry's own null-pointer check; `things` names what `count` counts
inline int pg_check_args(const char* name, const char* things, int n_jobs, int n_pages, int count, int64_t pool_bytes, int sigma, int max_hits) {
  OMP_CHECK_ARG(n_jobs > 0 && n_jobs <= PG_JOBS_MAX && n_pages > 0 && count > 0 && pool_bytes >= 0 && pool_bytes <= 0x7fffffffll,
                "%s: %d jobs (1 .. %d), %d pages, %d %s, %lld pool bytes", name, n_jobs, PG_JOBS_MAX, n_pages, count, things, (long long)pool_bytes);
  OMP_CHECK_ARG(sigma >= 0 && sigma <= PG_SIGMA_MAX, "%s: sigma %d (0 .. %d)", name, sigma, PG_SIGMA_MAX);
  OMP_CHECK_ARG(max_hits >= 1 && max_hits <= PG_HITS_MAX, "%s: max_hits %d (1 .. %d)", name, max_hits, PG_HITS_MAX);
  return OMP_OK;
}
