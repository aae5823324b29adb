// Reading order: words -> text lines -> the order a reader takes them in.
// Integers only: utils/reading.py (features_cpu, links_cpu, lines_cpu: the specification) and these kernels agree on every output.
//
// Geometry is done on scaled bins (x ax, y ay), ax, ay <= 256, bins <= 4095: a coordinate is below 2^20, L and R (sums of two) below 2^21,
// the components of d and v below 2^21 in magnitude (int32).  A product of two such components is below 2^42, a dot or cross product below
// 2^43, H (eight cross products with T - B, whose components are below 2^20) below 2^45; 10000 H is below 2^59 and 4000 times a dot or
// cross product below 2^55: int64 throughout, no overflow.  cost = |v|^2 < 2^43.
//
//   reading_links_kernel  a thread per word a, workgroups of 256 words that never leave a group (block = group x chunk; a chunk past the
//                         group's end leaves at once).  The thread computes its own L, R, d, H once; the group's candidates b go through
//                         LDS in tiles of 256 (L, d as one int4, offset H as one int64): every lane reads the same b, a broadcast.  Five
//                         64-bit multiply-compares per pair, cheapest rejection first; candidates run in ascending b and only a strictly
//                         smaller cost replaces the best, which is the tie rule.
//   reading_lines_kernel  a workgroup of 1024 threads per group, thread t owns words t, t + 1024, ... (at most 8), dynamic LDS of 16 bytes
//                         per word of the LARGEST group of the call (two regions of 8 bytes per word, reused step by step) + 16:
//                           1 key[b] = min (cost << 13 | a) over the a that chose b (64-bit LDS atomicMin)  -> pred, succ
//                           2 pointer doubling over pred carrying the least index: a word whose pointer never reaches -1 is on a cycle,
//                             and the member that equals the least index cuts the cycle in front of itself
//                           3 pointer doubling again: head and distance from it
//                           4 one 64-bit LDS atomicAdd of (sum_k y_k ay) << 14 | 1 on the head's slot: sum (< 2^37) and count (< 2^14)
//                           5 every head counts the heads that compare less (the specification's comparator, sums and counts cross-
//                             multiplied in int64), and the words they hold: the line's number and its first rank
// Every index is clamped or tested: group bounds into [0, n], aspects into 1 .. 256, a successor read from succ0 must lie inside the group.
#include "common.h"

namespace {

constexpr int RD_MAX_GRID = 4096;
constexpr int RD_MAX_GROUP = 8192;
constexpr int RD_MAX_ASPECT = 256;
constexpr int RD_MAX_PARAM = 10000;
constexpr int RD_TILE = 256;
constexpr int RD_THREADS = 1024;                       // of reading_lines_kernel
constexpr int RD_OWN = RD_MAX_GROUP / RD_THREADS;      // words per thread there
constexpr unsigned long long RD_NONE = ~0ull;

struct Feat {
  int lx, ly, rx, ry, dx, dy;
  int64_t H;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int64_t abs64(int64_t v) { return v < 0 ? -v : v; }

// the 16 scaled points of word idx
__device__ __forceinline__ void load_points(const int32_t* __restrict__ polys, int idx, int grid, int ax, int ay, int (&x)[16], int (&y)[16]) {
  const int4* p = reinterpret_cast<const int4*>(polys + (int64_t)idx * 32);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int4 v = p[q];
    x[2 * q] = clampi(v.x, 0, grid - 1) * ax;
    y[2 * q] = clampi(v.y, 0, grid - 1) * ay;
    x[2 * q + 1] = clampi(v.z, 0, grid - 1) * ax;
    y[2 * q + 1] = clampi(v.w, 0, grid - 1) * ay;
  }
}

__device__ __forceinline__ Feat word_features(const int32_t* __restrict__ polys, int idx, int grid, int ax, int ay) {
  int x[16], y[16];
  load_points(polys, idx, grid, ax, ay, x, y);
  Feat f;
  f.lx = x[0] + x[15];
  f.ly = y[0] + y[15];
  f.rx = x[7] + x[8];
  f.ry = y[7] + y[8];
  f.dx = f.rx - f.lx;
  f.dy = f.ry - f.ly;
  if (f.dx == 0 && f.dy == 0) f.dx = 1;
  int64_t H = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) H += abs64((int64_t)(x[k] - x[15 - k]) * f.dy - (int64_t)(y[k] - y[15 - k]) * f.dx);
  f.H = H;
  return f;
}

struct Group {
  int g0, g1, ax, ay;
};

__device__ __forceinline__ Group load_group(const int32_t* __restrict__ tables, int n_groups, int g, int n) {
  Group G;
  G.g0 = clampi(tables[g], 0, n);
  G.g1 = clampi(tables[g + 1], G.g0, n);
  G.ax = clampi(tables[n_groups + 1 + 2 * g], 1, RD_MAX_ASPECT);
  G.ay = clampi(tables[n_groups + 2 + 2 * g], 1, RD_MAX_ASPECT);
  return G;
}

__global__ __launch_bounds__(RD_TILE) void reading_links_kernel(const int32_t* __restrict__ polys, int n, const int32_t* __restrict__ tables, int n_groups,
                                                               int chunks, int grid, int gap, int back, int offset, int32_t* __restrict__ succ0,
                                                               int64_t* __restrict__ cost0) {
  __shared__ int4 s_ld[RD_TILE];       // L.x, L.y, d.x, d.y of the tile's words
  __shared__ int64_t s_oh[RD_TILE];    // offset * H
  const int tid = threadIdx.x;
  const int g = blockIdx.x / chunks, chunk = blockIdx.x - g * chunks;
  if (g >= n_groups) return;
  const Group G = load_group(tables, n_groups, g, n);
  const int ng = G.g1 - G.g0;
  if (chunk * RD_TILE >= ng) return;   // block-uniform, before any barrier
  const int a = G.g0 + chunk * RD_TILE + tid;
  const bool live = a < G.g1;
  Feat A = {0, 0, 0, 0, 1, 0, 0};
  if (live) A = word_features(polys, a, grid, G.ax, G.ay);
  const int64_t gapH = (int64_t)gap * A.H, backH = -(int64_t)back * A.H, offH = (int64_t)offset * A.H;
  int best = -1;
  int64_t best_cost = INT64_MAX;
  for (int t0 = 0; t0 < ng; t0 += RD_TILE) {
    __syncthreads();   // the previous tile has been read
    const int b = G.g0 + t0 + tid;
    if (b < G.g1) {
      const Feat B = word_features(polys, b, grid, G.ax, G.ay);
      s_ld[tid] = make_int4(B.lx, B.ly, B.dx, B.dy);
      s_oh[tid] = (int64_t)offset * B.H;
    }
    __syncthreads();
    const int m = min(RD_TILE, ng - t0);
    if (live) {
      for (int j = 0; j < m; ++j) {
        const int4 q = s_ld[j];
        const int vx = q.x - A.rx, vy = q.y - A.ry;
        const int64_t along4 = 4000 * ((int64_t)vx * A.dx + (int64_t)vy * A.dy);
        if (along4 > gapH || along4 < backH) continue;
        if (4000 * abs64((int64_t)vx * A.dy - (int64_t)vy * A.dx) > offH) continue;
        if ((int64_t)A.dx * q.z + (int64_t)A.dy * q.w <= 0) continue;
        if (4000 * abs64((int64_t)vx * q.w - (int64_t)vy * q.z) > s_oh[j]) continue;
        const int bb = G.g0 + t0 + j;
        if (bb == a) continue;
        const int64_t cost = (int64_t)vx * vx + (int64_t)vy * vy;
        if (cost < best_cost) {
          best_cost = cost;
          best = bb;
        }
      }
    }
  }
  if (live) {
    succ0[a] = best;
    cost0[a] = best >= 0 ? best_cost : -1;
  }
}

// thread tid's k-th word of a group of ng (local index), or -1
#define RD_FOR_OWN(k, i)            \
  _Pragma("unroll") for (int k = 0; k < RD_OWN; ++k) \
    if (const int i = tid + k * RD_THREADS; i < ng)

__global__ __launch_bounds__(RD_THREADS) void reading_lines_kernel(const int32_t* __restrict__ polys, int n, const int32_t* __restrict__ tables, int n_groups,
                                                                  int cap, int grid, const int32_t* __restrict__ succ0, const int64_t* __restrict__ cost0,
                                                                  int32_t* __restrict__ succ, int32_t* __restrict__ pred, int32_t* __restrict__ line,
                                                                  int32_t* __restrict__ line_pos, int32_t* __restrict__ rank, int32_t* __restrict__ n_lines) {
  extern __shared__ __align__(16) unsigned char rd_lds[];   // 16 cap + 16 bytes; no static LDS beside it: omp_raise_lds asks for all 160 KB as dynamic
  const int tid = threadIdx.x, g = blockIdx.x;
  const Group G = load_group(tables, n_groups, g, n);
  const int g0 = G.g0, ng = G.g1 - G.g0;
  if (ng > RD_MAX_GROUP || ng > cap) {   // refused: nothing else is written
    if (tid == 0) n_lines[g] = -1;
    return;
  }
  if (ng == 0) {
    if (tid == 0) n_lines[g] = 0;
    return;
  }
  // region A: key (64-bit) -> jmp, val (32-bit); region B: s_pred, s_succ (32-bit) -> packed (64-bit) -> s_start (32-bit)
  unsigned long long* key = reinterpret_cast<unsigned long long*>(rd_lds);
  int* jmp = reinterpret_cast<int*>(rd_lds);
  int* val = jmp + cap;
  int* s_pred = reinterpret_cast<int*>(rd_lds + 8 * (size_t)cap);
  int* s_succ = s_pred + cap;
  unsigned long long* packed = reinterpret_cast<unsigned long long*>(rd_lds + 8 * (size_t)cap);
  int* s_start = s_pred;
  int& s_heads = *reinterpret_cast<int*>(rd_lds + 16 * (size_t)cap);
  int rounds = 1;   // ceil(log2 ng) + 1
  while ((1 << (rounds - 1)) < ng) ++rounds;

  // 1. predecessor resolution
  if (tid == 0) s_heads = 0;
  RD_FOR_OWN(k, i) key[i] = RD_NONE;
  __syncthreads();
  int sb[RD_OWN];
  RD_FOR_OWN(k, i) {
    const int b = succ0[g0 + i] - g0;
    sb[k] = (b >= 0 && b < ng && b != i) ? b : -1;
    if (sb[k] >= 0) {
      const unsigned long long c = (unsigned long long)min(max(cost0[g0 + i], (int64_t)0), (int64_t)((1ll << 46) - 1));
      atomicMin(&key[sb[k]], (c << 13) | (unsigned long long)i);
    }
  }
  __syncthreads();
  int pr[RD_OWN];
  RD_FOR_OWN(k, i) {
    const unsigned long long mine = key[i];
    pr[k] = mine == RD_NONE ? -1 : (int)(mine & 8191ull);
    if (sb[k] >= 0 && (int)(key[sb[k]] & 8191ull) != i) sb[k] = -1;   // lost: no second choice
  }
  __syncthreads();   // key has been read: region A changes its meaning
  RD_FOR_OWN(k, i) {
    s_pred[i] = pr[k];
    s_succ[i] = sb[k];
    jmp[i] = pr[k];
    val[i] = i;
  }
  __syncthreads();

  // 2. cycles: after `rounds` doublings val = the least index among the word and its 2^rounds - 1 predecessors >= a whole cycle
  for (int r = 0; r < rounds; ++r) {
    int nj[RD_OWN], nv[RD_OWN];
    RD_FOR_OWN(k, i) {
      const int j = jmp[i];
      nj[k] = j >= 0 ? jmp[j] : -1;
      nv[k] = j >= 0 ? min(val[i], val[j]) : val[i];
    }
    __syncthreads();
    RD_FOR_OWN(k, i) {
      jmp[i] = nj[k];
      val[i] = nv[k];
    }
    __syncthreads();
  }
  RD_FOR_OWN(k, i) {
    const int p = s_pred[i];
    if (jmp[i] >= 0 && val[i] == i && p >= 0) {   // on a cycle, and its lowest member: cut in front of it
      s_succ[p] = -1;
      s_pred[i] = -1;
    }
  }
  __syncthreads();

  // 3. list ranking: jmp = an ancestor (the head once reached, which points at itself), val = the distance to it
  RD_FOR_OWN(k, i) {
    const int p = s_pred[i], s = s_succ[i];
    pred[g0 + i] = p >= 0 ? g0 + p : -1;
    succ[g0 + i] = s >= 0 ? g0 + s : -1;
    jmp[i] = p >= 0 ? p : i;
    val[i] = p >= 0 ? 1 : 0;
  }
  __syncthreads();   // s_pred / s_succ have been read: region B changes its meaning below
  for (int r = 0; r < rounds; ++r) {
    int nj[RD_OWN], nv[RD_OWN];
    RD_FOR_OWN(k, i) {
      const int j = jmp[i];
      nj[k] = jmp[j];
      nv[k] = val[i] + val[j];
    }
    __syncthreads();
    RD_FOR_OWN(k, i) {
      jmp[i] = nj[k];
      val[i] = nv[k];
    }
    __syncthreads();
  }

  // 4. per-line sums and counts on the head's slot; val becomes L.x of the word (read for heads only)
  int pos[RD_OWN], head[RD_OWN], cy[RD_OWN];
  RD_FOR_OWN(k, i) {
    pos[k] = val[i];
    head[k] = jmp[i];
    line_pos[g0 + i] = pos[k];
    int x[16], y[16];
    load_points(polys, g0 + i, grid, G.ax, G.ay, x, y);
    int s = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += y[q];
    cy[k] = s;
    val[i] = x[0] + x[15];   // the thread's own slot: nobody else reads val between the barriers around this step
    packed[i] = 0ull;
  }
  __syncthreads();
  RD_FOR_OWN(k, i) atomicAdd(&packed[head[k]], ((unsigned long long)cy[k] << 14) | 1ull);
  __syncthreads();

  // 5. line ordering: a head's line number = the heads that compare less, its first rank = the words on their lines
  int less[RD_OWN], before[RD_OWN];
  RD_FOR_OWN(k, i) {
    less[k] = before[k] = 0;
    if (head[k] != i) continue;
    const unsigned long long P = packed[i];
    const int64_t cnt = (int64_t)(P & 16383ull), sum = (int64_t)(P >> 14);
    const int lx = val[i];
    int nl = 0, nb = 0;
    for (int j = 0; j < ng; ++j) {   // every lane reads the same j: a broadcast
      const unsigned long long Q = packed[j];
      if (Q == 0ull) continue;       // not a head
      const int64_t cj = (int64_t)(Q & 16383ull), lhs = (int64_t)(Q >> 14) * cnt, rhs = sum * cj;
      bool lt = lhs < rhs;
      if (lhs == rhs) {
        const int lj = val[j];
        lt = lj < lx || (lj == lx && j < i);
      }
      if (lt) {
        ++nl;
        nb += (int)cj;
      }
    }
    less[k] = nl;
    before[k] = nb;
    atomicAdd(&s_heads, 1);
  }
  __syncthreads();   // packed and L.x have been read
  RD_FOR_OWN(k, i) {
    if (head[k] == i) {
      val[i] = less[k];
      s_start[i] = before[k];
    }
  }
  __syncthreads();

  // 6. outputs
  RD_FOR_OWN(k, i) {
    line[g0 + i] = val[head[k]];
    rank[g0 + i] = s_start[head[k]] + pos[k];
  }
  if (tid == 0) n_lines[g] = s_heads;
}

// what both entry points refuse before a launch; *max_group = the largest group
int reading_check(const char* who, const int32_t* polys, int n, const int32_t* tables, const int32_t* host_tables, int n_groups, int grid, int* max_group) {
  OMP_CHECK_ARG(n >= 0 && n <= (1 << 24) && n_groups >= 0 && n_groups <= (1 << 24), "%s: %d words, %d groups", who, n, n_groups);
  OMP_CHECK_ARG(grid >= 2 && grid <= RD_MAX_GRID, "%s: grid %d (2 .. %d)", who, grid, RD_MAX_GRID);
  OMP_CHECK_ARG(host_tables, "%s: null host_tables", who);
  OMP_CHECK_ARG(host_tables[0] == 0 && host_tables[n_groups] == n, "%s: group_start must run from 0 to %d, got %d .. %d", who, n, host_tables[0],
                host_tables[n_groups]);
  int mx = 0;
  for (int g = 0; g < n_groups; ++g) {
    const int ng = host_tables[g + 1] - host_tables[g];
    OMP_CHECK_ARG(ng >= 0, "%s: group_start falls at group %d (%d -> %d)", who, g, host_tables[g], host_tables[g + 1]);
    const int ax = host_tables[n_groups + 1 + 2 * g], ay = host_tables[n_groups + 2 + 2 * g];
    OMP_CHECK_ARG(ax >= 1 && ax <= RD_MAX_ASPECT && ay >= 1 && ay <= RD_MAX_ASPECT, "%s: aspect (%d, %d) of group %d (1 .. %d)", who, ax, ay, g, RD_MAX_ASPECT);
    mx = ng > mx ? ng : mx;
  }
  OMP_CHECK_ARG(n == 0 || (polys && tables), "%s: null pointer", who);
  OMP_CHECK_ARG((reinterpret_cast<uintptr_t>(polys) & 15) == 0, "%s: polys must be 16-byte aligned", who);
  *max_group = mx;
  return OMP_OK;
}

// ---------------------------------------------------------------------------------------------
// blocks: a recursive XY-cut over the lines (utils/reading.py: blocks_cpu is the specification)
// ---------------------------------------------------------------------------------------------
//   reading_blocks_kernel  a workgroup of 1024 threads per group, dynamic LDS of 16 bytes per slot + 64, slots = the call's largest group
//                          rounded up to a power of two (the sort's size), at least 8.  Thread t owns words / atoms / sorted positions
//                          t, t + 1024, ... (at most 8) everywhere but in the scans, where it owns the 8 consecutive positions 8 t ...
//     1 per axis (y, then x): every word's inflated interval, biased by 2^38 into an unsigned below 2^39; per-line min / max by 64-bit
//       LDS atomics (region A = lo, region B = hi, 8 bytes per slot each)
//     2 region A becomes the keys lo << 13 | line and is sorted (bitonic, 64-bit) ONCE per axis: the position is the atom's rank r under
//       (lo, line number).  hr = the number of atoms whose lo is <= the atom's hi (a binary search in the sorted keys): lo_b > hi_a is
//       exactly r_b >= hr_a, and hr rises with hi, so the levels never see an interval again.  Kept in registers across the axes:
//       r of the own atoms, (hr << 13 | atom) of the own ranks.
//     3 regions for the levels, 4 bytes per slot each: keys | TY | TX | seg (T?[rank] = hr << 13 | atom).  Per level: keys =
//       seg << 13 | r (26 bits; pads 0xffffffff), bitonic sort (32-bit), then over the sorted order a max-scan of seg << 14 | hr -- segments
//       rise along the order, so the plain maximum IS the segmented one -- the flags (first of its segment, or r >= the maximum before
//       it), their sum-scan = the new segment ids, and the total, which every thread reads: the stopping rule is block-uniform.
//     4 keys = seg << 13 | old line, sorted: the position is the new line number
//     5 line lengths (LDS atomicAdd) in the new order, exclusive scan -> the first rank of every line; per-word outputs
// Every index is clamped or tested: a word's line into [0, atoms - 1], the atoms of a group into [1, words].
constexpr int RB_MIN_SLOTS = 8;
constexpr int RB_MAX_DEPTH = 16;
constexpr int RB_EXTRA = 64;                            // bytes behind the slots: 16 wave partials
constexpr long long RB_BIAS = 1ll << 38;

#define RB_FOR_OWN(k, i, count)                         \
  _Pragma("unroll") for (int k = 0; k < RD_OWN; ++k)    \
    if (const int i = tid + k * RD_THREADS; i < (count))

// a[0 .. n2 - 1] ascending, n2 a power of two; a barrier behind every step, the caller has one in front
template <typename T>
__device__ __forceinline__ void rb_sort(T* a, int n2, int tid) {
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += RD_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const T x = a[i], y = a[p];
        if ((x > y) == ((i & k) == 0)) {
          a[i] = y;
          a[p] = x;
        }
      }
      __syncthreads();
    }
  }
}

// scan of one NON-NEGATIVE value per thread over the workgroup, maximum or sum (identity 0): returns the inclusive value, *excl = over
// the threads in front, *total = over all.  Two barriers; every thread of the workgroup calls it.
template <bool MAX>
__device__ __forceinline__ int rb_scan(int v, int* part, int tid, int* excl, int* total) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v = MAX ? max(v, o) : v + o;
  }
  int ex = __shfl_up(v, 1, 64);
  if (lane == 0) ex = 0;
  if (lane == 63) part[wave] = v;
  __syncthreads();
  int base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < RD_THREADS / 64; ++w) {
    const int pw = part[w];
    if (w < wave) base = MAX ? max(base, pw) : base + pw;
    all = MAX ? max(all, pw) : all + pw;
  }
  __syncthreads();   // part may be written again
  *total = all;
  *excl = MAX ? max(base, ex) : base + ex;
  return MAX ? max(base, v) : base + v;
}

__global__ __launch_bounds__(RD_THREADS) void reading_blocks_kernel(const int32_t* __restrict__ polys, int n, const int32_t* __restrict__ tables, int n_groups,
                                                                   int slots, int grid, int gap_x, int gap_y, int depth, const int32_t* __restrict__ line_in,
                                                                   const int32_t* __restrict__ pos_in, const int32_t* __restrict__ n_lines_in,
                                                                   int32_t* __restrict__ block, int32_t* __restrict__ line, int32_t* __restrict__ rank,
                                                                   int32_t* __restrict__ n_blocks, int32_t* __restrict__ levels) {
  extern __shared__ __align__(16) unsigned char rb_lds[];   // 16 slots + RB_EXTRA bytes; no static LDS beside it (omp_raise_lds)
  const int tid = threadIdx.x, g = blockIdx.x;
  const Group G = load_group(tables, n_groups, g, n);
  const int g0 = G.g0, ng = G.g1 - G.g0;
  if (ng > RD_MAX_GROUP || ng > slots) {   // refused: nothing else is written
    if (tid == 0) n_blocks[g] = -1;
    return;
  }
  if (ng == 0) {
    if (tid == 0) n_blocks[g] = levels[g] = 0;
    return;
  }
  const int na = clampi(n_lines_in[g], 1, ng);   // atoms = lines
  int n2 = RB_MIN_SLOTS;
  while (n2 < na) n2 <<= 1;                      // <= slots: a power of two >= 8 and >= ng >= na
  unsigned long long* A = reinterpret_cast<unsigned long long*>(rb_lds);
  unsigned long long* B = reinterpret_cast<unsigned long long*>(rb_lds + 8 * (size_t)slots);
  int* Bi = reinterpret_cast<int*>(B);
  unsigned* keys = reinterpret_cast<unsigned*>(rb_lds);
  int* TY = reinterpret_cast<int*>(rb_lds + 4 * (size_t)slots);
  int* TX = reinterpret_cast<int*>(rb_lds + 8 * (size_t)slots);
  int* seg = reinterpret_cast<int*>(rb_lds + 12 * (size_t)slots);
  int* part = reinterpret_cast<int*>(rb_lds + 16 * (size_t)slots);

  // 1, 2. per axis: intervals -> per-line ends -> rank r and hr
  int r_y[RD_OWN], r_x[RD_OWN], t_y[RD_OWN], t_x[RD_OWN];   // register arrays, constant indices
#pragma unroll
  for (int ax = 0; ax < 2; ++ax) {   // 0 = y, 1 = x
    RB_FOR_OWN(k, a, n2) {
      A[a] = RD_NONE;
      B[a] = 0ull;
    }
    __syncthreads();
    RB_FOR_OWN(k, i, ng) {
      int x[16], y[16];
      load_points(polys, g0 + i, grid, G.ax, G.ay, x, y);
      int sx = 0, sy = 0, lo = ax ? x[0] : y[0], hi = lo;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        sx += x[15 - q] - x[q];
        sy += y[15 - q] - y[q];
      }
#pragma unroll
      for (int q = 1; q < 16; ++q) {
        lo = min(lo, ax ? x[q] : y[q]);
        hi = max(hi, ax ? x[q] : y[q]);
      }
      const int64_t m = (int64_t)(ax ? gap_x : gap_y) * max(abs(sx), abs(sy));   // < 10000 * 2^23 < 2^37
      const int l = clampi(line_in[g0 + i], 0, na - 1);
      atomicMin(&A[l], (unsigned long long)(16000ll * lo - m + RB_BIAS));   // in (0, 2^39)
      atomicMax(&B[l], (unsigned long long)(16000ll * hi + m + RB_BIAS));
    }
    __syncthreads();
    RB_FOR_OWN(k, a, na) A[a] = (min(A[a], (1ull << 39) - 1) << 13) | (unsigned long long)a;   // the own slot; pads stay RD_NONE
    __syncthreads();
    rb_sort(A, n2, tid);
    RB_FOR_OWN(k, p, na) {
      const int a = (int)(A[p] & 8191ull);
      const unsigned long long hi = B[a];
      int b0 = 0, b1 = na;                     // the first position whose lo exceeds hi = the number of atoms with lo <= hi
      while (b0 < b1) {
        const int mid = (b0 + b1) >> 1;
        if ((A[mid] >> 13) <= hi) b0 = mid + 1; else b1 = mid;
      }
      if (ax) t_x[k] = (b0 << 13) | a; else t_y[k] = (b0 << 13) | a;
    }
    __syncthreads();   // hi has been read: region B becomes the ranks by atom
    RB_FOR_OWN(k, p, na) Bi[(int)(A[p] & 8191ull)] = p;
    __syncthreads();
    RB_FOR_OWN(k, a, na) {
      if (ax) r_x[k] = Bi[a]; else r_y[k] = Bi[a];
    }
    __syncthreads();
  }

  // 3. the levels
  RB_FOR_OWN(k, p, na) {
    TY[p] = t_y[k];
    TX[p] = t_x[k];
    seg[p] = 0;
  }
  __syncthreads();
  const int p0 = 8 * tid;
  int n_seg = 1, lv = 0, excl, total;
  bool idle = false;
  for (int l = 0; l < depth; ++l) {
    const int* T = (l & 1) ? TX : TY;
    RB_FOR_OWN(k, a, n2) keys[a] = a < na ? ((unsigned)seg[a] << 13) | (unsigned)((l & 1) ? r_x[k] : r_y[k]) : 0xffffffffu;
    __syncthreads();
    rb_sort(keys, n2, tid);
    int s[8], r[8], at[8], v[8];
    int run = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s[e] = r[e] = at[e] = 0;
      if (p0 + e < na) {
        const unsigned key = keys[p0 + e];
        s[e] = (int)(key >> 13);
        r[e] = (int)(key & 8191u);
        const int tv = T[r[e]];
        at[e] = tv & 8191;
        run = max(run, (s[e] << 14) | (tv >> 13));   // hr <= 8192: 14 bits under the segment's 13
      }
      v[e] = run;                                    // inclusive inside the thread
    }
    rb_scan<true>(run, part, tid, &excl, &total);
    int flags = 0, f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int prev = e ? max(excl, v[e - 1]) : excl;   // the maximum over everything in front of position p0 + e
      f[e] = (p0 + e < na) && (p0 + e == 0 || (prev >> 14) != s[e] || r[e] >= (prev & 16383));
      flags += f[e];
    }
    rb_scan<false>(flags, part, tid, &excl, &total);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      excl += f[e];
      if (p0 + e < na) seg[at[e]] = excl - 1;
    }
    lv = l + 1;
    const bool created = total > n_seg;   // block-uniform: every thread holds the same total
    n_seg = total;
    __syncthreads();                      // seg is complete
    if (!created && idle) break;
    idle = !created;
  }

  // 4. the new line numbers: the position of (segment, old line)
  RB_FOR_OWN(k, a, n2) {
    keys[a] = a < na ? ((unsigned)seg[a] << 13) | (unsigned)a : 0xffffffffu;
    TY[a] = 0;   // the line's length, then its first rank
  }
  __syncthreads();
  RB_FOR_OWN(k, i, ng) atomicAdd(&TY[clampi(line_in[g0 + i], 0, na - 1)], 1);
  rb_sort(keys, n2, tid);   // its barriers also end the counting
  // 5. the first rank of every line in the new order
  int at[8], len[8], sum = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    at[e] = len[e] = 0;
    if (p0 + e < na) {
      at[e] = (int)(keys[p0 + e] & 8191u);
      len[e] = TY[at[e]];
      TX[at[e]] = p0 + e;
    }
    sum += len[e];
  }
  rb_scan<false>(sum, part, tid, &excl, &total);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (p0 + e < na) TY[at[e]] = excl;   // the slot this thread alone has read
    excl += len[e];
  }
  __syncthreads();
  RB_FOR_OWN(k, i, ng) {
    const int l = clampi(line_in[g0 + i], 0, na - 1);
    block[g0 + i] = seg[l];
    line[g0 + i] = TX[l];
    rank[g0 + i] = TY[l] + pos_in[g0 + i];
  }
  if (tid == 0) {
    n_blocks[g] = n_seg;
    levels[g] = lv;
  }
}

}  // namespace

extern "C" int omp_reading_links(const int32_t* polys, int n, const int32_t* tables, const int32_t* host_tables, int n_groups, int grid, int gap, int back,
                                 int offset, int32_t* succ0, int64_t* cost0, omp_stream_t s) {
  int max_group = 0;
  if (const int rc = reading_check("omp_reading_links", polys, n, tables, host_tables, n_groups, grid, &max_group)) return rc;
  OMP_CHECK_ARG(gap >= 0 && gap <= RD_MAX_PARAM && back >= 0 && back <= RD_MAX_PARAM && offset >= 0 && offset <= RD_MAX_PARAM,
                "omp_reading_links: gap %d, back %d, offset %d permille (0 .. %d)", gap, back, offset, RD_MAX_PARAM);
  if (n == 0) return OMP_OK;
  OMP_CHECK_ARG(succ0 && cost0, "omp_reading_links: null output");
  const int chunks = (max_group + RD_TILE - 1) / RD_TILE;   // >= 1: n > 0
  OMP_CHECK_ARG((int64_t)chunks * n_groups <= (1ll << 30), "omp_reading_links: %d groups of up to %d words", n_groups, max_group);
  hipLaunchKernelGGL(reading_links_kernel, dim3((unsigned)(chunks * n_groups)), dim3(RD_TILE), 0, (hipStream_t)s, polys, n, tables, n_groups, chunks, grid, gap,
                     back, offset, succ0, cost0);
  OMP_CHECK_LAUNCH("omp_reading_links");
  return OMP_OK;
}

extern "C" int omp_reading_lines(const int32_t* polys, int n, const int32_t* tables, const int32_t* host_tables, int n_groups, int grid,
                                 const int32_t* succ0, const int64_t* cost0, int32_t* succ, int32_t* pred, int32_t* line, int32_t* line_pos,
                                 int32_t* rank, int32_t* n_lines, omp_stream_t s) {
  int max_group = 0;
  if (const int rc = reading_check("omp_reading_lines", polys, n, tables, host_tables, n_groups, grid, &max_group)) return rc;
  if (n == 0) return OMP_OK;
  OMP_CHECK_ARG(succ0 && cost0 && succ && pred && line && line_pos && rank && n_lines, "omp_reading_lines: null pointer");
  const int cap = max_group < RD_MAX_GROUP ? max_group : RD_MAX_GROUP;
  constexpr auto kern = reading_lines_kernel;
  if (const int rc = omp_raise_lds<kern>("omp_reading_lines")) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)n_groups), dim3(RD_THREADS), 16 * (size_t)cap + 16, (hipStream_t)s, polys, n, tables, n_groups, cap, grid, succ0, cost0,
                     succ, pred, line, line_pos, rank, n_lines);
  OMP_CHECK_LAUNCH("omp_reading_lines");
  return OMP_OK;
}

extern "C" int omp_reading_blocks(const int32_t* polys, int n, const int32_t* tables, const int32_t* host_tables, int n_groups, int grid, int gap_x,
                                  int gap_y, int depth, const int32_t* line_in, const int32_t* line_pos_in, const int32_t* n_lines_in, int32_t* block,
                                  int32_t* line, int32_t* rank, int32_t* n_blocks, int32_t* levels, omp_stream_t s) {
  int max_group = 0;
  if (const int rc = reading_check("omp_reading_blocks", polys, n, tables, host_tables, n_groups, grid, &max_group)) return rc;
  OMP_CHECK_ARG(gap_x >= 0 && gap_x <= RD_MAX_PARAM && gap_y >= 0 && gap_y <= RD_MAX_PARAM, "omp_reading_blocks: gap_x %d, gap_y %d permille (0 .. %d)", gap_x,
                gap_y, RD_MAX_PARAM);
  OMP_CHECK_ARG(depth >= 1 && depth <= RB_MAX_DEPTH, "omp_reading_blocks: depth %d (1 .. %d)", depth, RB_MAX_DEPTH);
  if (n == 0) return OMP_OK;
  OMP_CHECK_ARG(line_in && line_pos_in && n_lines_in && block && line && rank && n_blocks && levels, "omp_reading_blocks: null pointer");
  int slots = RB_MIN_SLOTS;
  while (slots < max_group && slots < RD_MAX_GROUP) slots <<= 1;   // a larger group is refused on the device
  constexpr auto kern = reading_blocks_kernel;
  if (const int rc = omp_raise_lds<kern>("omp_reading_blocks")) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)n_groups), dim3(RD_THREADS), 16 * (size_t)slots + RB_EXTRA, (hipStream_t)s, polys, n, tables, n_groups, slots, grid,
                     gap_x, gap_y, depth, line_in, line_pos_in, n_lines_in, block, line, rank, n_blocks, levels);
  OMP_CHECK_LAUNCH("omp_reading_blocks");
  return OMP_OK;
}
