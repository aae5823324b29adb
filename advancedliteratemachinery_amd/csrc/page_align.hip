// Page text alignment: the optimal edit script of whole pages on the device.  utils/page_align.py (align_cpu /
// pairs_align_cpu: the specification) and this kernel agree on every integer.  a is the prediction (rows i), b the ground truth
// (columns j); codes, equality and lengths are page_text.hip's: 255 equals nothing, itself included; codes are below sigma or 255.
//
//   page_align_kernel   one wave (a 64-thread workgroup) per pair.
//     forward   page_edit_kernel's recurrence (Myers' block step, Peq in LDS, skewed lanes, stripes of 4096 pattern characters with
//               lane 63's carries through scratch; see page_text.hip).  In addition every (pattern block, text column) RECORDS two
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
#include "common.h"

namespace {

constexpr int PA_LEN_MAX = 65535;      // characters a side
constexpr int PA_BLOCK = 64;           // pattern characters per lane
constexpr int PA_STRIPE = 4096;        // pattern characters per pass over the text
constexpr int PA_SIGMA_MAX = 254;
constexpr int PA_NONE = 255;           // the code that equals nothing
constexpr int PA_CARRY_WORDS = 2048;   // one carry buffer: 2 bit words per 64 text columns
constexpr int PA_CARRY_BYTES = 32768;  // the head of a pair's scratch: two carry buffers
constexpr int PA_CELL_BYTES = 16;      // the record of one (pattern block, text column): G and Pv

static_assert(PA_STRIPE == 64 * PA_BLOCK && PA_CARRY_WORDS == 2 * ((PA_LEN_MAX + 63) / 64) && PA_CARRY_BYTES == 2 * PA_CARRY_WORDS * 8, "page_align layout");

typedef unsigned long long u64;

struct __attribute__((aligned(8))) Cell {
  u64 g, pv;
};

// lane l takes lane l - 1's v, lane 0 takes `first`
__device__ __forceinline__ int lane_shift_up(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

// lane k's 64-bit v, k uniform over the wave
__device__ __forceinline__ u64 read_lane64(u64 v, int k) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, k), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), k);
  return ((u64)hi << 32) | lo;
}

__host__ __device__ inline int64_t pa_scratch_bytes(int la, int lb) { return PA_CARRY_BYTES + (int64_t)PA_CELL_BYTES * ((la + PA_BLOCK - 1) / PA_BLOCK) * lb; }

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
  bool bad = la < 0 || la > PA_LEN_MAX || lb < 0 || lb > PA_LEN_MAX || ao < 0 || bo < 0 || mo < 0 || so < 0 || (so & 7) != 0;
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
  const uint8_t* __restrict__ a = pool + ao;
  const uint8_t* __restrict__ b = pool + bo;
  const int nb = (la + PA_BLOCK - 1) / PA_BLOCK;   // pattern blocks
  const int ns = (nb + 63) / 64;                   // stripes
  u64* cbuf = reinterpret_cast<u64*>(scratch + so);
  u64* rec = cbuf + 2 * PA_CARRY_WORDS;            // [stripe][(column + lane) % lb][blocks of the stripe] cells of 2 words
  int acc = 0;
  for (int s = 0; s < ns; ++s) {
    const int blk = s * 64 + lane;
    const bool active = blk < nb;
    const int nbs = min(64, nb - s * 64);          // blocks of this stripe
    const bool last = s == ns - 1;
    const u64* cin = cbuf + ((s & 1) ^ 1) * PA_CARRY_WORDS;   // what stripe s - 1 wrote
    u64* cout = cbuf + (s & 1) * PA_CARRY_WORDS;
    u64* rec_s = rec + 2 * ((int64_t)s * 64 * lb);
    // ---- Peq of this stripe: lane l builds column l ----
    for (int c = 0; c <= sigma; ++c) pa_peq[c * 64 + lane] = 0;
    if (active) {
      const int base = blk * PA_BLOCK, n = min(PA_BLOCK, la - base);
      for (int i = 0; i < n; ++i) {
        const int c = a[base + i];
        if (c < sigma) pa_peq[c * 64 + lane] |= 1ull << i;
      }
    }
    const int top = (blk == nb - 1) ? ((la - 1) & 63) : 63;   // the bit the block's carry-out is read at
    u64 Pv = ~0ull, Mv = 0, outP = 0, outM = 0;
    int xout = 0;   // this lane's last carry-out: bit 0 = +1, bit 1 = -1
    acc = 0;
    const int nsteps = lb + nbs - 1;
    int chb = lane < lb ? (int)b[lane] : PA_NONE;
    u64 inP = ~0ull, inM = 0;   // stripe 0: +1 in every column
    if (s > 0) {
      inP = cin[0];
      inM = cin[1];
    }
    int c = __builtin_amdgcn_readlane(chb, 0);
    u64 eq = pa_peq[min(c, sigma) * 64 + lane];
    int row = 0;   // t % lb: the record row of this step, uniform
    for (int T = 0; T < nsteps; T += 64) {
      int chn = PA_NONE;
      u64 inPn = ~0ull, inMn = 0;
      if (T + 64 < nsteps) {   // uniform: the next batch is requested now and first read 63 steps from here
        const int j = T + 64 + lane;
        chn = j < lb ? (int)b[j] : PA_NONE;
        if (s > 0 && T + 64 < lb) {
          inPn = cin[2 * ((T + 64) >> 6)];
          inMn = cin[2 * ((T + 64) >> 6) + 1];
        }
      }
      const int kn = min(64, nsteps - T);
      for (int k = 0; k < kn; ++k) {
        const int nx = k < 63 ? __builtin_amdgcn_readlane(chb, k + 1) : __builtin_amdgcn_readlane(chn, 0);
        const int cn = lane_shift_up(c, nx);
        const u64 eqn = pa_peq[min(cn, sigma) * 64 + lane];
        const int in0 = (int)((inP >> k) & 1ull) | ((int)((inM >> k) & 1ull) << 1);
        const int hin = lane_shift_up(xout, in0);
        const int j = T + k - lane;   // this lane's text column
        if (active && (unsigned)j < (unsigned)lb) {
          const u64 hneg = (u64)(hin >> 1), hpos = (u64)(hin & 1);
          u64 Eq = eq;
          const u64 Xv = Eq | Mv;
          Eq |= hneg;
          const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
          u64 Ph = Mv | ~(Xh | Pv);
          u64 Mh = Pv & Xh;
          const int hp = (int)(Ph >> top) & 1, hm = (int)(Mh >> top) & 1;
          xout = hp | (hm << 1);
          acc += hp - hm;
          Ph = (Ph << 1) | hpos;   // now dh_j(i - 1) at the bit of row i
          Mh = (Mh << 1) | hneg;
          Pv = Mh | ~(Xv | Ph);
          Mv = Ph & Xv;
          // the record: the diagonal is optimal where the characters are equal or dv_j(i) + dh_j(i - 1) == 1
          Cell cell;
          cell.g = eq | (Pv & ~(Ph | Mh)) | (~(Pv | Mv) & Ph);
          cell.pv = Pv;
          *reinterpret_cast<Cell*>(rec_s + 2 * ((int64_t)row * nbs + lane)) = cell;
          if (!last) {   // uniform: lane 63's carry-outs are the next stripe's carry-ins
            const int bit = j & 63;
            outP |= (u64)hp << bit;
            outM |= (u64)hm << bit;
            if (bit == 63 || j == lb - 1) {
              if (lane == 63) {
                cout[2 * (j >> 6)] = outP;
                cout[2 * (j >> 6) + 1] = outM;
              }
              outP = 0;
              outM = 0;
            }
          }
        }
        c = cn;
        eq = eqn;
        if (++row == lb) row = 0;
      }
      chb = chn;
      inP = inPn;
      inM = inMn;
    }
    __syncthreads();   // lane 63's stores are lane 0's loads of the next stripe; after the last stripe, the record is the walk's
  }
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
  OMP_CHECK_ARG(sigma >= 0 && sigma <= PA_SIGMA_MAX, "omp_page_align: sigma %d (0 .. %d)", sigma, PA_SIGMA_MAX);
  OMP_CHECK_ARG(pool_bytes >= 0 && maps_len >= 0 && scratch_bytes >= 0, "omp_page_align: %lld pool bytes, %lld map entries, %lld bytes of scratch",
                (long long)pool_bytes, (long long)maps_len, (long long)scratch_bytes);
  OMP_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "omp_page_align: scratch must be 8-byte aligned");
  const size_t lds = (size_t)(sigma + 1) * 64 * sizeof(u64);
  if (lds > 64 * 1024) {
    const int rc = omp_raise_lds<page_align_kernel>("omp_page_align");
    if (rc != OMP_OK) return rc;
  }
  hipLaunchKernelGGL(page_align_kernel, dim3((unsigned)n_pairs), dim3(64), lds, (hipStream_t)s, pool, pool_bytes, a_off, a_len, b_off, b_len, map_off,
                     scratch_off, sigma, reinterpret_cast<uint8_t*>(scratch), scratch_bytes, maps, maps_len, counts);
  OMP_CHECK_LAUNCH("omp_page_align");
  return OMP_OK;
}
