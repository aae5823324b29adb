// Page search: where a phrase stands in the text of a read page, and how badly it was misread.
// utils/page_search.py (row_cpu / search_cpu: the specification) and this kernel agree on every integer.  Sellers' table: insert /
// delete / substitute cost 1, row 0 all zeros; code 255 equals nothing, itself included; codes are below sigma or 255.
//
// A query has at most 64 characters, so Myers' bit-parallel column (1999) is ONE 64-bit word and one lane runs it by itself:
//
//   page_search_kernel   one wave (a 64-thread workgroup) per job (page, query).  The job frame -- the round loop, the hit lists, the slot
//                        scan, the refusal -- is page_frame.h's (pg_window), which page_pattern.hip shares; PsStep is the column.
//     chunks    lane l owns the end columns cs + 1 .. cs + 128 of the text, cs = 128 (64 r + l) in round r; a page of up to 65535
//               characters takes up to 8 rounds.  A lane starts 2m columns before cs with a fresh column (Pv all ones, score m):
//               every alignment of cost <= m covers at most 2m characters, so v_cs and every later score equal those of the whole
//               text.  A column below 1 is skipped, so a chunk less than 2m from the start of the text warms up from column 0, which IS
//               the fresh column.  One column past the chunk is read for the v_j < v_{j+1} test.
//     text      the round's characters, 128 before its first chunk to 1 after its last, are staged in LDS once, 4 bytes of padding
//               after every 128: the lanes walk their chunks in step, 33 dwords apart, on distinct banks.
//     Peq       LDS, [sigma + 1] 64-bit words: bit i of Peq[c] says q[i] == c, built with one ballot per query character.  Row sigma
//               stays 0: every code at or above sigma, 255 among them, reads it.
//     best      per lane the least key (dist << 32) | end over its own columns, then a wave min over lane shuffles; column 0 is (m, 0).
//     hits      a lane counts the hits of its chunk and keeps the first max_hits of them as (end, dist) in its own list in the job's
//               slice of caller-owned scratch.  After the round an exclusive scan of the counts over the lanes gives every lane its
//               first slot; the lanes copy their lists to an LDS slot table, and lane g takes slot g: it runs the anchored reverse
//               recurrence (Myers' column on the reversed query over t[end-1], t[end-2], ..., horizontal carry-in 1) to the first
//               l whose score equals dist, at most m + dist <= 127 characters, all of them still in LDS, and writes (end, dist, end - l).
//               Chunks are in text order, rounds are in text order: the hits come out in ascending end whatever the scheduling.
//   No atomics.  With m = 64 the score bit is bit 63 and no mask is ever formed; the bits above m - 1 never reach a lower bit, and the
//   carry out of the 64-bit add is dropped on purpose.
// A job out of range (a page or query index that is not there, a page above 65535 characters, a query outside 1 .. 64, a range outside
// the pool, k outside 0 .. m - 1) is REFUSED on the device: n_hits = -1, best and hits -1, and nothing outside the pool is read.
// Nothing is allocated and nothing synchronises: pool, tables, scratch and outputs are the caller's.
#include "myers.h"
#include "page_frame.h"

namespace {

constexpr int PS_QUERY_MAX = 64;       // characters a query
constexpr int PS_NONE = 255;           // the code that equals nothing
constexpr int PS_BEFORE = 2 * PS_QUERY_MAX;                // characters staged before the round's first chunk

static_assert(PS_QUERY_MAX == PG_POS_MAX, "page_search layout");

// pg_window's Stepper: Myers' column of one lane.  Only the 2m characters of the warm-up are staged before a round's first chunk
// (PS_BEFORE - W): nothing earlier is read.
struct PsStep {
  int m, k, top;
  u64 Pv, Mv;
  __device__ __forceinline__ int warm() const { return 2 * m; }
  __device__ __forceinline__ int stage_from() const { return PS_BEFORE - 2 * m; }
  __device__ __forceinline__ int none() const { return m; }
  __device__ __forceinline__ int tol() const { return k; }
  __device__ __forceinline__ void fresh() {
    Pv = ~0ull;
    Mv = 0;
  }
  __device__ __forceinline__ int step(u64 eq, int v) { return v + myers_step(eq, Pv, Mv, top, 0); }
  // the anchored reverse recurrence to the FIRST l whose score equals dist, at most m + dist <= 127 characters
  template <class At>
  __device__ __forceinline__ int start(int end, int dist, At at) const {
    u64 rPv = ~0ull, rMv = 0;
    int score = m, l = 0;
    const int lmax = min(end, m + dist);
    while (score != dist && l < lmax) {
      ++l;
      const u64 Eq = __brevll(at(end - l)) >> (64 - m);
      score += myers_step(Eq, rPv, rMv, top, 1);
    }
    return score == dist ? end - l : -2;                   // -2 cannot happen: the start exists within m + dist characters
  }
};

__global__ __launch_bounds__(64) void page_search_kernel(const uint8_t* __restrict__ pool, int64_t pool_bytes, const int32_t* __restrict__ page_off,
                                                         const int32_t* __restrict__ page_len, int n_pages, const int32_t* __restrict__ query_off,
                                                         const int32_t* __restrict__ query_len, const int32_t* __restrict__ tol, int n_queries,
                                                         const int32_t* __restrict__ jobs, int sigma, int H, int2* scratch,
                                                         int32_t* __restrict__ best, int32_t* __restrict__ n_hits, int32_t* __restrict__ hits) {
  __shared__ __align__(16) u64 peq[PG_SIGMA_MAX + 2];
  __shared__ __align__(16) uint8_t text[PgText<PS_BEFORE>::BYTES];
  __shared__ int2 slot[PG_HITS_MAX];
  const int job = blockIdx.x, lane = threadIdx.x;
  int32_t* jhits = hits + (int64_t)job * H * 3;
  const int p = jobs[2 * job], qi = jobs[2 * job + 1];
  // all of this is uniform over the wave
  bool ok = p >= 0 && p < n_pages && qi >= 0 && qi < n_queries;
  int n = 0, m = 0, k = 0;
  int64_t po = 0, qo = 0;
  if (ok) {
    n = page_len[p];
    po = page_off[p];
    m = query_len[qi];
    qo = query_off[qi];
    k = tol[qi];
    ok = n >= 0 && n <= PG_LEN_MAX && m >= 1 && m <= PS_QUERY_MAX && po >= 0 && qo >= 0 && po + n <= pool_bytes && qo + m <= pool_bytes && k >= 0 && k < m;
  }
  if (!ok) {
    pg_refuse(job, H, best, n_hits, jhits);
    return;
  }
  // ---- Peq: one ballot per query character ----
  for (int c = lane; c <= sigma; c += 64) peq[c] = 0;
  const int qc = lane < m ? (int)pool[qo + lane] : PS_NONE;
  __syncthreads();
  for (int i = 0; i < m; ++i) {
    const int c = __builtin_amdgcn_readlane(qc, i);
    const u64 mask = __ballot(qc == c);                 // lanes at or above m hold 255, and a 255 of the query is skipped below
    if (lane == 0 && c < sigma) peq[c] = mask;
  }
  __syncthreads();
  int2* list = scratch + ((int64_t)job * 64 + lane) * H;   // this lane's first H hits of the round: (end, dist)
  PsStep st{m, k, m - 1, 0, 0};
  u64 key;                                                 // from (m, 0): the empty match
  const int base = pg_window<PS_BEFORE>(st, pool + po, n, sigma, H, peq, text, slot, list, jhits, &key);
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

extern "C" int omp_page_search(const uint8_t* pool, int64_t pool_bytes, const int32_t* page_off, const int32_t* page_len, int n_pages,
                               const int32_t* query_off, const int32_t* query_len, const int32_t* k, int n_queries, const int32_t* jobs,
                               int n_jobs, int sigma, int max_hits, void* scratch, int64_t scratch_bytes, int32_t* best, int32_t* n_hits,
                               int32_t* hits, omp_stream_t s) {
  OMP_CHECK_ARG(pool && page_off && page_len && query_off && query_len && k && jobs && scratch && best && n_hits && hits, "omp_page_search: null pointer");
  if (const int rc = pg_check_args("omp_page_search", "queries", n_jobs, n_pages, n_queries, pool_bytes, sigma, max_hits)) return rc;
  const int64_t need = (int64_t)n_jobs * 64 * max_hits * (int64_t)sizeof(int2);
  OMP_CHECK_ARG(scratch_bytes >= need, "omp_page_search: %lld bytes of scratch, %d jobs at max_hits %d need %lld", (long long)scratch_bytes, n_jobs,
                max_hits, (long long)need);
  OMP_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "omp_page_search: scratch must be 8-byte aligned");
  hipLaunchKernelGGL(page_search_kernel, dim3((unsigned)n_jobs), dim3(64), 0, (hipStream_t)s, pool, pool_bytes, page_off, page_len, n_pages, query_off,
                     query_len, k, n_queries, jobs, sigma, max_hits, reinterpret_cast<int2*>(scratch), best, n_hits, hits);
  OMP_CHECK_LAUNCH("omp_page_search");
  return OMP_OK;
}
