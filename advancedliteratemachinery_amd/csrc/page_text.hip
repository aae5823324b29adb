// Page text scoring: the Levenshtein distance of whole pages, thousands to tens of thousands of characters a side, on the device
// (DESIGN.md section 23).  utils/page_text.py (distance_cpu / pairs_cpu: the specification) and this kernel agree on every integer.
// Insert / delete / substitute cost 1; code 255 equals nothing, itself included; codes are below sigma or 255.
//
// Myers' block-based bit-parallel recurrence (1999, advance_block with a horizontal carry in {-1, 0, +1} in and out): the multi-word
// form of the column update in lexicon.hip, pipelined across a wave.
//
//   page_edit_kernel   one wave (a 64-thread workgroup) per pair (a, b).  a is the pattern, b the text.
//     blocks    lane l owns pattern block l of the current stripe: 64 characters of a, Pv / Mv (the vertical +1 / -1 differences) in
//               registers.  A stripe is 64 blocks = 4096 pattern characters.
//     Peq       dynamic LDS, [sigma + 1][64 lanes] 64-bit words: bit i of Peq[c][l] says a[4096 s + 64 l + i] == c.  Lane l writes and
//               reads column l only (no barrier, no atomics; the 32 lanes of an LDS access group fall on 64 distinct banks).  Row sigma
//               stays 0: every code at or above sigma, 255 among them, reads it.
//     steps     skewed: at step t lane l advances its block by text character b[t - l] with the carry lane l - 1 put out at step t - 1.
//               The characters run down the lanes ONE STEP AHEAD of the carries (two full-wave lane shifts a step), so the LDS read of
//               the next step's Eq word is in flight while this step's dozen dependent integer operations run.  Text characters come in
//               batches of 64 (one byte per lane, the next batch requested while this one is consumed).
//     stripes   a pattern above 4096 characters takes ceil(la / 4096) passes over the text.  Lane 63's carry-out per text column goes
//               to the pair's slice of scratch as two bit words (+1 bits, -1 bits) per 64 columns, ping-ponged between two buffers, and
//               is lane 0's carry-in of the next stripe; the first stripe's carry-in is +1 throughout (row 0 of the table is 0, 1, 2, ...).
//     distance  la + the sum of the carry-outs of the last block, read at bit (la - 1) % 64; the unused high bits of a partial block
//               never reach a lower bit and need no cleaning.  la == 0 gives lb, lb == 0 gives la.
//   No atomics; one wave walks one pair in a fixed order, so the result does not depend on scheduling.
// A descriptor out of range (a negative length, a length above 65535, a range outside the pool) is REFUSED on the device: dist = -1,
// and nothing outside the pool is read.  Nothing is allocated and nothing synchronises: pool, tables, scratch and dist are the caller's.
#include "common.h"

namespace {

constexpr int PT_LEN_MAX = 65535;      // characters a side
constexpr int PT_BLOCK = 64;           // pattern characters per lane
constexpr int PT_STRIPE = 4096;        // pattern characters per pass over the text
constexpr int PT_SIGMA_MAX = 254;
constexpr int PT_NONE = 255;           // the code that equals nothing
constexpr int PT_CARRY_WORDS = 2048;   // one carry buffer: 2 bit words per 64 text columns, ceil(65535 / 64) = 1024 batches
constexpr int PT_SLICE_BYTES = 32768;  // scratch per pair: two carry buffers

static_assert(PT_STRIPE == 64 * PT_BLOCK && PT_CARRY_WORDS == 2 * ((PT_LEN_MAX + 63) / 64) && PT_SLICE_BYTES == 2 * PT_CARRY_WORDS * 8, "page_text layout");

typedef unsigned long long u64;

// lane l takes lane l - 1's v, lane 0 takes `first` (a full-wave shift by one lane: one data-parallel move, no LDS round trip)
__device__ __forceinline__ int lane_shift_up(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

__global__ __launch_bounds__(64) void page_edit_kernel(const uint8_t* __restrict__ pool, int64_t pool_bytes, const int32_t* __restrict__ a_off,
                                                       const int32_t* __restrict__ a_len, const int32_t* __restrict__ b_off,
                                                       const int32_t* __restrict__ b_len, int sigma, u64* scratch, int32_t* __restrict__ dist) {
  extern __shared__ __align__(16) u64 pt_peq[];   // [sigma + 1][64]
  const int p = blockIdx.x, lane = threadIdx.x;
  const int la = a_len[p], lb = b_len[p];
  const int64_t ao = a_off[p], bo = b_off[p];
  // all of this is uniform over the wave
  if (la < 0 || la > PT_LEN_MAX || lb < 0 || lb > PT_LEN_MAX || ao < 0 || bo < 0 || ao + la > pool_bytes || bo + lb > pool_bytes) {
    if (lane == 0) dist[p] = -1;
    return;
  }
  if (la == 0 || lb == 0) {
    if (lane == 0) dist[p] = la + lb;
    return;
  }
  const uint8_t* __restrict__ a = pool + ao;
  const uint8_t* __restrict__ b = pool + bo;
  const int nb = (la + PT_BLOCK - 1) / PT_BLOCK;   // pattern blocks
  const int ns = (nb + 63) / 64;                   // stripes
  u64* cbuf = scratch + (int64_t)p * (2 * PT_CARRY_WORDS);
  int acc = 0;
  for (int s = 0; s < ns; ++s) {
    const int blk = s * 64 + lane;
    const bool active = blk < nb;
    const int nbs = min(64, nb - s * 64);          // blocks of this stripe
    const bool last = s == ns - 1;
    const u64* cin = cbuf + ((s & 1) ^ 1) * PT_CARRY_WORDS;   // what stripe s - 1 wrote
    u64* cout = cbuf + (s & 1) * PT_CARRY_WORDS;
    // ---- Peq of this stripe: lane l builds column l ----
    for (int c = 0; c <= sigma; ++c) pt_peq[c * 64 + lane] = 0;
    if (active) {
      const int base = blk * PT_BLOCK, n = min(PT_BLOCK, la - base);
      for (int i = 0; i < n; ++i) {
        const int c = a[base + i];
        if (c < sigma) pt_peq[c * 64 + lane] |= 1ull << i;
      }
    }
    const int top = (blk == nb - 1) ? ((la - 1) & 63) : 63;   // the bit the block's carry-out is read at
    u64 Pv = ~0ull, Mv = 0, outP = 0, outM = 0;
    int xout = 0;   // this lane's last carry-out: bit 0 = +1, bit 1 = -1
    acc = 0;
    const int nsteps = lb + nbs - 1;
    // the batch of text columns T .. T + 63: one character per lane, and lane 0's carry-in bits
    int chb = lane < lb ? (int)b[lane] : PT_NONE;
    u64 inP = ~0ull, inM = 0;   // stripe 0: +1 in every column
    if (s > 0) {
      inP = cin[0];
      inM = cin[1];
    }
    int c = __builtin_amdgcn_readlane(chb, 0);   // lane l holds b[t - l]; only lane 0 matters at step 0
    u64 eq = pt_peq[min(c, sigma) * 64 + lane];
    for (int T = 0; T < nsteps; T += 64) {
      int chn = PT_NONE;
      u64 inPn = ~0ull, inMn = 0;
      if (T + 64 < nsteps) {   // uniform: the next batch is requested now and first read 63 steps from here
        const int j = T + 64 + lane;
        chn = j < lb ? (int)b[j] : PT_NONE;
        if (s > 0 && T + 64 < lb) {
          inPn = cin[2 * ((T + 64) >> 6)];
          inMn = cin[2 * ((T + 64) >> 6) + 1];
        }
      }
      const int kn = min(64, nsteps - T);
      for (int k = 0; k < kn; ++k) {
        // the characters of step t + 1 and their Eq words, ahead of the recurrence
        const int nx = k < 63 ? __builtin_amdgcn_readlane(chb, k + 1) : __builtin_amdgcn_readlane(chn, 0);
        const int cn = lane_shift_up(c, nx);
        const u64 eqn = pt_peq[min(cn, sigma) * 64 + lane];
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
          Ph = (Ph << 1) | hpos;
          Mh = (Mh << 1) | hneg;
          Pv = Mh | ~(Xv | Ph);
          Mv = Ph & Xv;
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
      }
      chb = chn;
      inP = inPn;
      inM = inMn;
    }
    if (!last) __syncthreads();   // lane 63's stores are lane 0's loads of the next stripe
  }
  if (lane == ((nb - 1) & 63)) dist[p] = la + acc;
}

}  // namespace

extern "C" int omp_page_edit_distance(const uint8_t* pool, int64_t pool_bytes, const int32_t* a_off, const int32_t* a_len, const int32_t* b_off,
                                      const int32_t* b_len, int n_pairs, int sigma, void* scratch, int64_t scratch_bytes, int32_t* dist,
                                      omp_stream_t s) {
  OMP_CHECK_ARG(pool && a_off && a_len && b_off && b_len && scratch && dist, "omp_page_edit_distance: null pointer");
  OMP_CHECK_ARG(n_pairs > 0 && n_pairs <= (1 << 24) && pool_bytes >= 0 && pool_bytes <= 0x7fffffffll, "omp_page_edit_distance: %d pairs, %lld pool bytes",
                n_pairs, (long long)pool_bytes);
  OMP_CHECK_ARG(sigma >= 0 && sigma <= PT_SIGMA_MAX, "omp_page_edit_distance: sigma %d (0 .. %d)", sigma, PT_SIGMA_MAX);
  OMP_CHECK_ARG(scratch_bytes >= (int64_t)n_pairs * PT_SLICE_BYTES, "omp_page_edit_distance: %lld bytes of scratch, %d pairs need %lld",
                (long long)scratch_bytes, n_pairs, (long long)n_pairs * PT_SLICE_BYTES);
  OMP_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "omp_page_edit_distance: scratch must be 8-byte aligned");
  const size_t lds = (size_t)(sigma + 1) * 64 * sizeof(u64);
  if (lds > 64 * 1024) {
    const int rc = omp_raise_lds<page_edit_kernel>("omp_page_edit_distance");
    if (rc != OMP_OK) return rc;
  }
  hipLaunchKernelGGL(page_edit_kernel, dim3((unsigned)n_pairs), dim3(64), lds, (hipStream_t)s, pool, pool_bytes, a_off, a_len, b_off, b_len, sigma,
                     reinterpret_cast<u64*>(scratch), dist);
  OMP_CHECK_LAUNCH("omp_page_edit_distance");
  return OMP_OK;
}
