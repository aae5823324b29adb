// Page text alignment: the optimal edit script of whole pages on the device.  utils/page_align.py (align_cpu /
// pairs_align_cpu: the specification) and this kernel agree on every integer.  a is the prediction (rows i), b the ground truth
// (columns j); codes, equality and lengths are page_text.hip's: 255 equals nothing, itself included; codes are below sigma or 255.
//
//   page_align_kernel   one wave (a 64-thread workgroup) per pair.
//     forward   page_edit_kernel's recurrence: page_forward of myers.h (Myers' block step, Peq in LDS, skewed lanes, stripes of 4096
//               pattern characters with lane 63's carries through scratch).  In addition every (pattern block, text column) RECORDS two
//               64-bit words, bit r standing for row i = 64 block + r + 1 of column j:
//                 G   the diagonal is on an optimal path: a_i == b_j, or D[i][j] - D[i-1][j-1] == 1.  (Equal characters always allow
//                     it: D[i][j] == D[i-1][j-1] then.)  D[i][j] - D[i-1][j-1] = dv_j(i) + dh_j(i-1), and both are in registers: the
//                     new Pv / Mv and the SHIFTED Ph / Mh, whose bit 0 is the carry-in (+1 in row 0).
//                 Pv  dv_j(i) == +1, that is D[i-1][j] + 1 == D[i][j].
//               The walk's rule 1 is a test of G, rule 2 a test of Pv, rule 3 what remains: two bit tests a step and no character.
//     record    by skew step: at step t lane l handles column t - l, so the cell of (block l of stripe s, column j) lies at
//               [s][(j + l) % lb][l]: the lanes of one step store 16 bytes each into ONE contiguous run of 16 x (blocks of the stripe)
//               bytes, and the record holds exactly ceil(la / 64) x lb cells -- no triangle of unused cells at either end of the skew.
//     walk      after a barrier (the wave's stores are its own loads, as between stripes).  The position (i, j) is uniform over the
//               wave.  The 64 lanes load the cells of the current block at columns j, j - 1, .. j - 63 in ONE round of loads (lane k:
//               column j - k); the walk then takes its words from lane j0 - j by readlane and needs a new round only when it leaves
//               the block upwards or has moved 64 columns left.  The walk moves in RUNS: lane k + d tests the cell d steps down the
//               diagonal (rule 1) or d columns to the left (rule 3), a ballot gives the length of the run, and the lanes of the run
//               write its map entries side by side; a run of INS up one column (rule 2) is a count of leading ones.  Every cell of a
//               run passes the test of its own rule and fails the rules before it, so the script is the step-by-step one.  What is
//               left when one side runs out is written by all lanes.  ins and del are counted, sub = dist - ins - del and
//               match = la - ins - sub (the identities of the definition), dist being the forward pass's.
//   No atomics; one wave walks one pair in a fixed order, so the result does not depend on scheduling.
// A descriptor out of range (a negative length, a length above 65535, a range outside the pool, a slice outside maps or scratch, a
// scratch offset that is not a multiple of 8) is REFUSED on the device: counts = -1 four times, nothing of the pool is read and nothing is
// written to maps or scratch.  Nothing is allocated and nothing synchronises: pool, tables, scratch, maps and counts are the caller's.
#include "myers.h"

namespace {

constexpr int PA_CARRY_BYTES = 32768;  // the head of a pair's scratch: page_forward's two carry buffers
constexpr int PA_CELL_BYTES = 16;      // the record of one (pattern block, text column): G and Pv

static_assert(PA_CARRY_BYTES == PT_SLICE_BYTES, "page_align layout");

struct __attribute__((aligned(8))) Cell {
  u64 g, pv;
};

// lane k's 64-bit v, k uniform over the wave
__device__ __forceinline__ u64 read_lane64(u64 v, int k) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, k), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), k);
  return ((u64)hi << 32) | lo;
}

__host__ __device__ inline int64_t pa_scratch_bytes(int la, int lb) { return PA_CARRY_BYTES + (int64_t)PA_CELL_BYTES * ((la + PT_BLOCK - 1) / PT_BLOCK) * lb; }

// what page_forward leaves behind for the walk: the cell of (block `lane` of the stripe, the column of step t) at [t % lb][lane]
struct Recorder {
  static constexpr bool kRecords = true;
  u64* rec;     // [stripe][(column + lane) % lb][blocks of the stripe] cells of 2 words
  u64* rec_s;   // the current stripe's
  __device__ __forceinline__ void stripe(int s, int lb) { rec_s = rec + 2 * ((int64_t)s * 64 * lb); }
  __device__ __forceinline__ void cell(int row, int nbs, int lane, u64 eq, u64 Pv, u64 Mv, u64 Ph, u64 Mh) const {
    // the diagonal is optimal where the characters are equal or dv_j(i) + dh_j(i - 1) == 1
    Cell cell;
    cell.g = eq | (Pv & ~(Ph | Mh)) | (~(Pv | Mv) & Ph);
    cell.pv = Pv;
    *reinterpret_cast<Cell*>(rec_s + 2 * ((int64_t)row * nbs + lane)) = cell;
  }
};

__global__ __launch_bounds__(64) void page_align_kernel(const uint8_t* __restrict__ pool, int64_t pool_bytes, const int32_t* __restrict__ a_off,
                                                        const int32_t* __restrict__ a_len, const int32_t* __restrict__ b_off,
                                                        const int32_t* __restrict__ b_len, const int64_t* __restrict__ map_off,
                                                        const int64_t* __restrict__ scratch_off, int sigma, uint8_t* scratch, int64_t scratch_bytes,
                                                        int32_t* maps, int64_t maps_len, int32_t* __restrict__ counts) {
  extern __shared__ __align__(16) u64 pa_peq[];   // [sigma + 1][64]
  const int p = blockIdx.x, lane = threadIdx.x;
  const int la = a_len[p], lb = b_len[p];
  const int64_t ao = a_off[p], bo = b_off[p], mo = map_off[p], so = scratch_off[p];
  // all of this is uniform over the wave
  bool bad = la < 0 || la > PT_LEN_MAX || lb < 0 || lb > PT_LEN_MAX || ao < 0 || bo < 0 || mo < 0 || so < 0 || (so & 7) != 0;
  if (!bad) bad = ao + la > pool_bytes || bo + lb > pool_bytes || mo + la + lb > maps_len || so + pa_scratch_bytes(la, lb) > scratch_bytes;
  if (bad) {
    if (lane < 4) counts[4 * (int64_t)p + lane] = -1;
    return;
  }
  int32_t* amap = maps + mo;
  int32_t* bmap = amap + la;
  if (la == 0 || lb == 0) {   // all INS or all DEL
    for (int t = lane; t < la + lb; t += 64) amap[t] = -1;
    if (lane < 4) counts[4 * (int64_t)p + lane] = lane == 2 ? la : lane == 3 ? lb : 0;
    return;
  }
  const int nb = (la + PT_BLOCK - 1) / PT_BLOCK;   // pattern blocks
  u64* cbuf = reinterpret_cast<u64*>(scratch + so);
  u64* rec = cbuf + 2 * PT_CARRY_WORDS;
  Recorder recorder{rec, rec};
  const int acc = page_forward(pool + ao, pool + bo, la, lb, sigma, pa_peq, cbuf, recorder);   // ends in a barrier: the record is the walk's
  const int dist = la + __builtin_amdgcn_readlane(acc, (nb - 1) & 63);
  // ---- the walk from (la, lb): everything here is uniform over the wave but the cells each lane holds ----
  int i = la, j = lb, ins = 0, del = 0;
  int wblk = -1, wj0 = 0;   // the block and the first column of the cells in registers: lane k holds column wj0 - k
  u64 G = 0, P = 0;
  while (i > 0 && j > 0) {
    const int blk = (i - 1) >> 6, r = (i - 1) & 63;
    if (blk != wblk || wj0 - j >= 64) {
      wblk = blk;
      wj0 = j;
      const int col = j - 1 - lane;
      if (col >= 0) {
        const int s = blk >> 6, l = blk & 63, nbs = min(64, nb - s * 64);
        const Cell cell = *reinterpret_cast<const Cell*>(rec + 2 * ((int64_t)s * 64 * lb + (int64_t)((col + l) % lb) * nbs + l));
        G = cell.g;
        P = cell.pv;
      }
    }
    const int k = wj0 - j;
    const int d = lane - k;                  // lane k + d holds column j - d
    const bool on = d >= 0 && d < j;
    // rule 1 in runs: the diagonal from (i, j) stays in the block for r + 1 rows; lane k + d tests cell (i - d, j - d)
    const bool dg = on && d <= r && ((G >> ((r - d) & 63)) & 1ull);
    u64 stop = ~__builtin_amdgcn_ballot_w64(dg) >> k;   // bit d: the run ends before its step d; the lanes past 63 end it too
    int n = stop ? __builtin_ctzll(stop) : 64 - k;
    if (n > 0) {                             // n times MATCH or SUB
      if (d >= 0 && d < n) {
        amap[i - 1 - d] = j - 1 - d;
        bmap[j - 1 - d] = i - 1 - d;
      }
      i -= n;
      j -= n;
      continue;
    }
    // rule 2 in runs, up column j: the rows whose diagonal is closed and whose dv is +1, from bit r downwards
    const u64 g = read_lane64(G, k), pv = read_lane64(P, k);
    const u64 up = (~g & pv) << (63 - r);
    n = up == ~0ull ? 64 : __builtin_clzll(~up);   // at most r + 1: the bits shifted in are 0
    if (n > 0) {                             // n times INS
      if (lane < n) amap[i - 1 - lane] = -1;
      ins += n;
      i -= n;
      continue;
    }
    // rule 3 in runs, along row i: the columns where neither rule applies
    const bool lf = on && !((G >> r) & 1ull) && !((P >> r) & 1ull);
    stop = ~__builtin_amdgcn_ballot_w64(lf) >> k;
    n = max(stop ? __builtin_ctzll(stop) : 64 - k, 1);   // lane k itself passed neither test, so n >= 1 anyway: the walk always moves
    if (d >= 0 && d < n) bmap[j - 1 - d] = -1;
    del += n;
    j -= n;
  }
  for (int t = lane; t < i; t += 64) amap[t] = -1;   // column 0: INS
  for (int t = lane; t < j; t += 64) bmap[t] = -1;   // row 0: DEL
  ins += i;
  del += j;
  const int sub = dist - ins - del, match = la - ins - sub;
  if (lane < 4) counts[4 * (int64_t)p + lane] = lane == 0 ? match : lane == 1 ? sub : lane == 2 ? ins : del;
}

}  // namespace

extern "C" int omp_page_align(const uint8_t* pool, int64_t pool_bytes, const int32_t* a_off, const int32_t* a_len, const int32_t* b_off,
                              const int32_t* b_len, const int64_t* map_off, const int64_t* scratch_off, int n_pairs, int sigma, void* scratch,
                              int64_t scratch_bytes, int32_t* maps, int64_t maps_len, int32_t* counts, omp_stream_t s) {
  OMP_CHECK_ARG(pool && a_off && a_len && b_off && b_len && map_off && scratch_off && scratch && maps && counts, "omp_page_align: null pointer");
  OMP_CHECK_ARG(n_pairs > 0 && n_pairs <= (1 << 24), "omp_page_align: %d pairs (1 .. %d)", n_pairs, 1 << 24);
  OMP_CHECK_ARG(sigma >= 0 && sigma <= PT_SIGMA_MAX, "omp_page_align: sigma %d (0 .. %d)", sigma, PT_SIGMA_MAX);
  OMP_CHECK_ARG(pool_bytes >= 0 && maps_len >= 0 && scratch_bytes >= 0, "omp_page_align: %lld pool bytes, %lld map entries, %lld bytes of scratch",
                (long long)pool_bytes, (long long)maps_len, (long long)scratch_bytes);
  OMP_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "omp_page_align: scratch must be 8-byte aligned");
  size_t lds;
  const int rc = page_forward_lds<page_align_kernel>(sigma, "omp_page_align", &lds);
  if (rc != OMP_OK) return rc;
  hipLaunchKernelGGL(page_align_kernel, dim3((unsigned)n_pairs), dim3(64), lds, (hipStream_t)s, pool, pool_bytes, a_off, a_len, b_off, b_len, map_off,
                     scratch_off, sigma, reinterpret_cast<uint8_t*>(scratch), scratch_bytes, maps, maps_len, counts);
  OMP_CHECK_LAUNCH("omp_page_align");
  return OMP_OK;
}
