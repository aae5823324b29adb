// Myers' bit-parallel edit-distance recurrence (1999), held ONCE for the kernels that run it:
//
//   myers_step     one text character against one 64-bit column: page_search.hip calls it from one lane each for Sellers' search and
//                  for the anchored reverse distance.  (lexicon.hip keeps the same step with carry 1 inline: DESIGN.md section 28.)
//   page_forward   the multi-word form, advance_block with a horizontal carry in {-1, 0, +1} in and out, pipelined across a wave:
//                  page_text.hip takes the distance from it, page_align.hip in addition a record of every (block, column) for its walk.
//
// page_forward: one wave (a 64-thread workgroup) per pair (a, b).  a is the pattern, b the text.  Insert / delete / substitute cost 1;
// code 255 equals nothing, itself included; codes are below sigma or 255.
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
//               to the pair's carry buffers as two bit words (+1 bits, -1 bits) per 64 columns, ping-ponged between two buffers, and
//               is lane 0's carry-in of the next stripe; the first stripe's carry-in is +1 throughout (row 0 of the table is 0, 1, 2, ...).
//     distance  la + the sum of the carry-outs of the last block (the `acc` of lane (blocks - 1) % 64, which page_forward returns), read
//               at bit (la - 1) % 64; the unused high bits of a partial block never reach a lower bit and need no cleaning.
//   No atomics; one wave walks one pair in a fixed order, so the result does not depend on scheduling.
#pragma once
#include "common.h"

constexpr int PT_LEN_MAX = 65535;      // characters a side
constexpr int PT_BLOCK = 64;           // pattern characters per lane
constexpr int PT_STRIPE = 4096;        // pattern characters per pass over the text
constexpr int PT_SIGMA_MAX = 254;
constexpr int PT_NONE = 255;           // the code that equals nothing
constexpr int PT_CARRY_WORDS = 2048;   // one carry buffer: 2 bit words per 64 text columns, ceil(65535 / 64) = 1024 batches
constexpr int PT_SLICE_BYTES = 32768;  // a pair's two carry buffers: page_text's scratch per pair, the head of page_align's

static_assert(PT_STRIPE == 64 * PT_BLOCK && PT_CARRY_WORDS == 2 * ((PT_LEN_MAX + 63) / 64) && PT_SLICE_BYTES == 2 * PT_CARRY_WORDS * 8, "page_forward layout");

typedef unsigned long long u64;

// lane l takes lane l - 1's v, lane 0 takes `first` (a full-wave shift by one lane: one data-parallel move, no LDS round trip)
__device__ __forceinline__ int lane_shift_up(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

// one column of Myers' recurrence in one 64-bit word -> the change of the score, read at bit `top`; `carry` is the horizontal difference
// of row 0: 0 for a search (row 0 all zeros), 1 for a distance (row 0 is 0, 1, 2, ...)
__device__ __forceinline__ int myers_step(u64 Eq, u64& Pv, u64& Mv, int top, u64 carry) {
  const u64 Xv = Eq | Mv;
  const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  u64 Ph = Mv | ~(Xh | Pv);
  u64 Mh = Pv & Xh;
  const int d = (int)((Ph >> top) & 1ull) - (int)((Mh >> top) & 1ull);
  Ph = (Ph << 1) | carry;
  Mh <<= 1;
  Pv = Mh | ~(Xv | Ph);
  Mv = Ph & Xv;
  return d;
}

// The forward pass of one pair, la and lb in 1 .. PT_LEN_MAX, by the whole wave -> this lane's `acc` of the last stripe.  peq: the
// [sigma + 1][64] words of LDS; cbuf: the pair's two carry buffers (2 * PT_CARRY_WORDS words).  Rec says what else a cell leaves behind:
//   Rec::kRecords                                  the cells are read after the pass, so the last stripe ends in a barrier too
//   rec.stripe(s, lb)                              stripe s begins
//   rec.cell(row, nbs, lane, eq, Pv, Mv, Ph, Mh)   a (block, column) is done: row = t % lb of its step t, nbs the blocks of the stripe,
//                                                  eq its Eq word, Pv / Mv the NEW vertical and Ph / Mh the SHIFTED horizontal differences
template <class Rec>
__device__ __forceinline__ int page_forward(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int la, int lb, int sigma, u64* peq,
                                            u64* cbuf, Rec& rec) {
  const int lane = threadIdx.x;
  const int nb = (la + PT_BLOCK - 1) / PT_BLOCK;   // pattern blocks
  const int ns = (nb + 63) / 64;                   // stripes
  int acc = 0;
  for (int s = 0; s < ns; ++s) {
    const int blk = s * 64 + lane;
    const bool active = blk < nb;
    const int nbs = min(64, nb - s * 64);          // blocks of this stripe
    const bool last = s == ns - 1;
    const u64* cin = cbuf + ((s & 1) ^ 1) * PT_CARRY_WORDS;   // what stripe s - 1 wrote
    u64* cout = cbuf + (s & 1) * PT_CARRY_WORDS;
    rec.stripe(s, lb);
    // ---- Peq of this stripe: lane l builds column l ----
    for (int c = 0; c <= sigma; ++c) peq[c * 64 + lane] = 0;
    if (active) {
      const int base = blk * PT_BLOCK, n = min(PT_BLOCK, la - base);
      for (int i = 0; i < n; ++i) {
        const int c = a[base + i];
        if (c < sigma) peq[c * 64 + lane] |= 1ull << i;
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
    u64 eq = peq[min(c, sigma) * 64 + lane];
    int row = 0;   // t % lb, uniform: dead code under a recorder that ignores it
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
        const u64 eqn = peq[min(cn, sigma) * 64 + lane];
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
          rec.cell(row, nbs, lane, eq, Pv, Mv, Ph, Mh);
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
    if (!last || Rec::kRecords) __syncthreads();   // lane 63's stores are lane 0's loads of the next stripe; a record is read after the last
  }
  return acc;
}

// The launch prologue of a kernel that runs page_forward: *lds = its dynamic LDS (Peq), and above 64 KiB the kernel's limit is raised first.
template <auto Kern>
inline int page_forward_lds(int sigma, const char* what, size_t* lds) {
  *lds = (size_t)(sigma + 1) * 64 * sizeof(u64);
  return *lds > 64 * 1024 ? omp_raise_lds<Kern>(what) : OMP_OK;
}
