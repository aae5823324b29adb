// Overlap suppression: which decoded 16-point polygons are the same word.
// Polygons live on the coordinate-bin grid; a polygon covers the bin centres (i + 0.5, j + 0.5), 0 <= i, j < grid - 1, that lie inside it
// under the even-odd rule, stated in doubled integer coordinates (vertices even, samples odd: no tie can occur).  Integers only:
// utils/overlap.py (coverage_cpu, pair_overlap_cpu, suppress_cpu: the specification) and these kernels agree on every output.
//
// The row routine.  For the sample row ys = 2 j + 1 an edge (x1, y1) -> (x2, y2), oriented so that q = y2 - y1 > 0, counts for the sample
// xs = 2 i + 1 when (y1 < ys) != (y2 < ys) and xs q < R, R = x1 q + (ys - y1) (x2 - x1).  The samples it counts for are i < c with
//     c = ceil((R - q) / (2 q)) = (R + q - 1) / (2 q)          (R >= 0: R / q is the crossing, which lies between x1 and x2)
// so a row of a polygon is at most 16 such thresholds (an edge that does not cross the row gets c = BIG), sample i is inside when an odd
// number of them exceeds i, and with the thresholds sorted the inside samples are the spans [c0, c1), [c2, c3), ... -- the number of
// crossings of a closed polygon is even, and so is the number of BIGs, which pair off into empty spans.  A lane holds the 16 thresholds in
// registers and sorts them with an unrolled bitonic network (80 compare-exchanges, constant indices: no scratch); the row's area is the sum
// of the span lengths, the row's intersection with another polygon the 8 x 8 span-against-span sum (spans of one list are disjoint).
//
//   overlap_prep_kernel   a wave per polygon: bounding box of the clamped points, area = the wave's sum over the rows of the box
//   overlap_pair_kernel   a wave per mask word (group g, priority position p, word w): for the up to 64 positions q = 64 w + b, q > p, the
//                         prefilters (boxes share no sample; an area is 0; min / max of the areas cannot reach t), then lanes over the
//                         sample rows the two boxes share, a wave sum, the pair test in 64 bits -> bit b.  ONE plain store of the word; with
//                         `inter` also inter[a][b] and inter[b][a].  Work per pair: rows x (32 divisions + 2 sorts + 64 span pairs).
//   overlap_keep_kernel   a workgroup per group, thread t owns word t of the running "removed" set in a register: per 64 positions the
//                         diagonal word is resolved by wave 0 (serial over the 64 bits, the rows passed by lane broadcast), the kept bits
//                         go through LDS, then every thread ORs the kept rows' words in priority order.  owner comes from the bits a kept
//                         row removes first.
// Every index is clamped or tested: polygon indices into [0, n), group bounds into [0, n], the mask word a wave writes is its own task
// index (below mask_words), inter indices are tested against inter_total.
#include "common.h"

namespace {

constexpr int OV_MAX_GRID = 4096;
constexpr int OV_MAX_GROUP = 8192;
constexpr int OV_KEEP_THREADS = OV_MAX_GROUP / 64;   // one thread per word of the removed set
constexpr int OV_BIG = 0x7fff;                       // the threshold of an edge that does not cross the row (> any c <= grid - 1)

struct Poly16 {
  int x[16], y[16];   // doubled, clamped
};

__device__ __forceinline__ Poly16 load_poly(const int32_t* __restrict__ polys, int idx, int grid) {
  Poly16 P;
  const int32_t* p = polys + (int64_t)idx * 32;   // idx is wave-uniform: scalar loads
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    P.x[k] = 2 * min(max(p[2 * k], 0), grid - 1);
    P.y[k] = 2 * min(max(p[2 * k + 1], 0), grid - 1);
  }
  return P;
}

__device__ __forceinline__ void cmpx(int& a, int& b) {
  const int lo = min(a, b), hi = max(a, b);
  a = lo;
  b = hi;
}

// ascending bitonic network on 16 registers
__device__ __forceinline__ void sort16(int (&c)[16]) {
#pragma unroll
  for (int k = 2; k <= 16; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int l = i ^ j;
        if (l > i) {
          if ((i & k) == 0) cmpx(c[i], c[l]);
          else cmpx(c[l], c[i]);
        }
      }
    }
  }
}

// the sorted thresholds of sample row j
__device__ __forceinline__ void row_thresholds(const Poly16& P, int j, int (&c)[16]) {
  const int ys = 2 * j + 1;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    int x1 = P.x[e], y1 = P.y[e], x2 = P.x[(e + 1) & 15], y2 = P.y[(e + 1) & 15];
    const bool cross = (y1 < ys) != (y2 < ys);
    if (y1 > y2) {
      int t = x1; x1 = x2; x2 = t;
      t = y1; y1 = y2; y2 = t;
    }
    const int q = cross ? y2 - y1 : 1;
    const int R = cross ? x1 * q + (ys - y1) * (x2 - x1) : 0;
    c[e] = cross ? (int)((uint32_t)(R + q - 1) / (uint32_t)(2 * q)) : OV_BIG;
  }
  sort16(c);
}

__device__ __forceinline__ int row_area(const int (&c)[16]) {
  int s = 0;
#pragma unroll
  for (int k = 0; k < 16; k += 2) s += c[k + 1] - c[k];
  return s;
}

__device__ __forceinline__ int row_inter(const int (&a)[16], const int (&b)[16]) {
  int s = 0;
#pragma unroll
  for (int k = 0; k < 16; k += 2) {
#pragma unroll
    for (int m = 0; m < 16; m += 2) s += max(min(a[k + 1], b[m + 1]) - max(a[k], b[m]), 0);
  }
  return s;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void overlap_prep_kernel(const int32_t* __restrict__ polys, int n, int grid, int32_t* __restrict__ area,
                                                           int32_t* __restrict__ bbox) {
  const int lane = threadIdx.x & 63;
  const int idx = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (idx >= n) return;   // wave-uniform
  const Poly16 P = load_poly(polys, idx, grid);
  int x0 = P.x[0], x1 = P.x[0], y0 = P.y[0], y1 = P.y[0];
#pragma unroll
  for (int k = 1; k < 16; ++k) {
    x0 = min(x0, P.x[k]); x1 = max(x1, P.x[k]);
    y0 = min(y0, P.y[k]); y1 = max(y1, P.y[k]);
  }
  x0 >>= 1; x1 >>= 1; y0 >>= 1; y1 >>= 1;
  int s = 0;
  for (int j = y0 + lane; j < y1; j += 64) {   // the sample rows y0 .. y1 - 1 (<= grid - 2)
    int c[16];
    row_thresholds(P, j, c);
    s += row_area(c);
  }
  s = wave_sum_i(s);
  if (lane == 0) {
    area[idx] = s;
    *reinterpret_cast<u32x4*>(bbox + 4 * (int64_t)idx) = u32x4{(uint32_t)x0, (uint32_t)y0, (uint32_t)x1, (uint32_t)y1};
  }
}

// g with start[g] <= task < start[g + 1] (groups without words have equal starts and are never found)
__device__ __forceinline__ int find_group(const int64_t* __restrict__ start, int n_groups, int64_t task) {
  int lo = 0, hi = n_groups;   // the answer is in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= task) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void overlap_pair_kernel(const int32_t* __restrict__ polys, int n, const int32_t* __restrict__ group_start,
                                                           int n_groups, const int32_t* __restrict__ order, const int64_t* __restrict__ mask_start,
                                                           int64_t mask_words, int grid, int t, int measure, const int32_t* __restrict__ area,
                                                           const int32_t* __restrict__ bbox, unsigned long long* __restrict__ mask,
                                                           int32_t* __restrict__ inter, const int64_t* __restrict__ inter_start, int64_t inter_total) {
  const int lane = threadIdx.x & 63;
  const int64_t task = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (task >= mask_words) return;   // wave-uniform
  const int g = find_group(mask_start, n_groups, task);
  const int g0 = min(max(group_start[g], 0), n), g1 = min(max(group_start[g + 1], g0), n);
  const int ng = g1 - g0, W = (ng + 63) >> 6;
  const int64_t local = task - mask_start[g];
  unsigned long long word = 0ull;
  const int p = W > 0 ? (int)(local / W) : ng;
  const int w = W > 0 ? (int)(local - (int64_t)p * W) : 0;
  if (local >= 0 && p < ng && w >= (p >> 6)) {   // else: a word of the lower triangle, or tables that do not fit each other -> 0
    const int a = __builtin_amdgcn_readfirstlane(min(max(order[g0 + p], g0), g1 - 1));
    const Poly16 A = load_poly(polys, a, grid);
    const int area_a = area[a];
    const int ax0 = bbox[4 * (int64_t)a], ay0 = bbox[4 * (int64_t)a + 1], ax1 = bbox[4 * (int64_t)a + 2], ay1 = bbox[4 * (int64_t)a + 3];
    const int64_t ibase = inter ? inter_start[g] : 0;
    for (int bit = 0; bit < 64; ++bit) {
      const int qpos = 64 * w + bit;
      if (qpos <= p || qpos >= ng) continue;   // wave-uniform
      const int b = __builtin_amdgcn_readfirstlane(min(max(order[g0 + qpos], g0), g1 - 1));
      const int area_b = area[b];
      const int x0 = max(ax0, bbox[4 * (int64_t)b]), y0 = max(ay0, bbox[4 * (int64_t)b + 1]);
      const int x1 = min(ax1, bbox[4 * (int64_t)b + 2]), y1 = min(ay1, bbox[4 * (int64_t)b + 3]);
      const int lo_area = min(area_a, area_b), hi_area = max(area_a, area_b);
      bool live = x0 < x1 && y0 < y1 && lo_area > 0 && a != b;   // a == b: an order that names a polygon twice; nothing overlaps itself
      // inter <= min(area), so IoU <= min / max: below t the pair cannot pass; with `inter` wanted only the exact zero is skipped
      if (!inter && measure == 0 && 1000ll * lo_area < (int64_t)t * hi_area) live = false;
      int s = 0;
      if (live) {
        const Poly16 B = load_poly(polys, b, grid);
        for (int j = y0 + lane; j < y1; j += 64) {
          int ca[16], cb[16];
          row_thresholds(A, j, ca);
          row_thresholds(B, j, cb);
          s += row_inter(ca, cb);
        }
        s = wave_sum_i(s);
      }
      if (inter && a != b) {
        const int64_t ab = ibase + (int64_t)(a - g0) * ng + (b - g0), ba = ibase + (int64_t)(b - g0) * ng + (a - g0);
        if (lane == 0 && ab >= 0 && ab < inter_total && ba >= 0 && ba < inter_total) {
          inter[ab] = s;
          inter[ba] = s;
        }
      }
      const int64_t denom = measure == 0 ? (int64_t)area_a + area_b - s : (int64_t)lo_area;
      if (s > 0 && 1000ll * s >= (int64_t)t * denom) word |= 1ull << bit;
    }
    if (inter) {   // the diagonal: a polygon's intersection with itself is its area (written by the wave of the row's first word)
      const int64_t aa = ibase + (int64_t)(a - g0) * ng + (a - g0);
      if (lane == 0 && w == (p >> 6) && aa >= 0 && aa < inter_total) inter[aa] = area_a;
    }
  }
  if (lane == 0) mask[task] = word;
}

__global__ __launch_bounds__(OV_KEEP_THREADS) void overlap_keep_kernel(const unsigned long long* __restrict__ mask, const int64_t* __restrict__ mask_start,
                                                                       int64_t mask_words, const int32_t* __restrict__ group_start, int n,
                                                                       const int32_t* __restrict__ order, int32_t* __restrict__ owner,
                                                                       int32_t* __restrict__ kept) {
  __shared__ unsigned long long cur_s, keep_s;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int g0 = min(max(group_start[g], 0), n), g1 = min(max(group_start[g + 1], g0), n);
  const int ng = g1 - g0, W = (ng + 63) >> 6;
  const int64_t base = mask_start[g];
  if (ng > OV_MAX_GROUP || base < 0 || base + (int64_t)ng * W > mask_words) {   // refused: nothing is suppressed, kept = -1
    for (int i = g0 + tid; i < g1; i += OV_KEEP_THREADS) owner[i] = i;
    if (tid == 0) kept[g] = -1;
    return;
  }
  // a position's polygon, clamped into the group: owner is indexed by it
  auto poly_at = [&](int pos) { return min(max(order[g0 + pos], g0), g1 - 1); };
  unsigned long long rem = 0ull;   // word tid of the removed set (positions 64 tid .. 64 tid + 63)
  int n_kept = 0;
  for (int c = 0; c < W; ++c) {
    const int p0 = 64 * c;
    if (tid == c) cur_s = rem;
    __syncthreads();
    if (tid < 64) {   // wave 0 resolves the 64 positions of the diagonal word
      const unsigned long long d = p0 + lane < ng ? mask[base + (int64_t)(p0 + lane) * W + c] : 0ull;
      unsigned long long cur = cur_s, keep = 0ull;
      for (int k = 0; k < 64 && p0 + k < ng; ++k) {
        const unsigned long long dk = __shfl(d, k, 64);
        if ((cur >> k) & 1ull) continue;   // wave-uniform
        keep |= 1ull << k;
        const int me = poly_at(p0 + k);
        if (lane == k) owner[me] = me;
        if ((((dk & ~cur) >> lane) & 1ull) && p0 + lane < ng) owner[poly_at(p0 + lane)] = me;   // the pair kernel sets bits above k only
        cur |= dk;
      }
      if (lane == 0) {
        cur_s = cur;
        keep_s = keep;
      }
    }
    __syncthreads();
    const unsigned long long keep = keep_s;
    n_kept += __popcll(keep);
    if (tid == c) rem = cur_s;
    if (tid > c && tid < W) {
      for (unsigned long long left = keep; left; left &= left - 1ull) {   // the kept rows in priority order
        const int k = __ffsll((long long)left) - 1;
        const unsigned long long m = mask[base + (int64_t)(p0 + k) * W + tid];
        unsigned long long fresh = m & ~rem;
        rem |= m;
        if (fresh) {
          const int me = poly_at(p0 + k);
          for (; fresh; fresh &= fresh - 1ull) {
            const int pos = 64 * tid + __ffsll((long long)fresh) - 1;
            if (pos < ng) owner[poly_at(pos)] = me;
          }
        }
      }
    }
    // the next iteration's thread c + 1 rewrites cur_s: not before every thread has read cur_s / keep_s above
    __syncthreads();
  }
  if (tid == 0) kept[g] = n_kept;
}

}  // namespace

extern "C" int omp_polygon_overlap(const int32_t* polys, int n, const int32_t* group_start, int n_groups, const int32_t* order,
                                   const int64_t* mask_start, int64_t mask_words, int grid, int t, int measure, int32_t* area, int32_t* bbox,
                                   uint64_t* mask, int32_t* inter, const int64_t* inter_start, int64_t inter_total, omp_stream_t s) {
  OMP_CHECK_ARG(polys && group_start && order && mask_start && area && bbox && mask, "omp_polygon_overlap: null pointer");
  OMP_CHECK_ARG(n > 0 && n <= (1 << 24) && n_groups > 0 && n_groups <= (1 << 24), "omp_polygon_overlap: %d polygons, %d groups", n, n_groups);
  OMP_CHECK_ARG(grid >= 2 && grid <= OV_MAX_GRID, "omp_polygon_overlap: grid %d (2 .. %d)", grid, OV_MAX_GRID);
  OMP_CHECK_ARG(t >= 1 && t <= 1000 && (measure == 0 || measure == 1), "omp_polygon_overlap: t %d permille (1 .. 1000), measure %d (0 iou, 1 iomin)", t,
                measure);
  OMP_CHECK_ARG(mask_words > 0 && mask_words <= (1ll << 32), "omp_polygon_overlap: %lld mask words (1 .. 2^32)", (long long)mask_words);
  OMP_CHECK_ARG(!inter || (inter_start && inter_total > 0), "omp_polygon_overlap: inter without inter_start / inter_total");
  const hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(overlap_prep_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, polys, n, grid, area, bbox);
  OMP_CHECK_LAUNCH("omp_polygon_overlap (prep)");
  hipLaunchKernelGGL(overlap_pair_kernel, dim3((unsigned)((mask_words + 3) / 4)), dim3(256), 0, st, polys, n, group_start, n_groups, order, mask_start,
                     mask_words, grid, t, measure, area, bbox, reinterpret_cast<unsigned long long*>(mask), inter, inter_start, inter ? inter_total : 0);
  OMP_CHECK_LAUNCH("omp_polygon_overlap (pairs)");
  return OMP_OK;
}

extern "C" int omp_polygon_keep(const uint64_t* mask, const int64_t* mask_start, int64_t mask_words, const int32_t* group_start, int n_groups, int n,
                                const int32_t* order, int32_t* owner, int32_t* kept, omp_stream_t s) {
  OMP_CHECK_ARG(mask && mask_start && group_start && order && owner && kept, "omp_polygon_keep: null pointer");
  OMP_CHECK_ARG(n > 0 && n <= (1 << 24) && n_groups > 0 && n_groups <= (1 << 24) && mask_words > 0, "omp_polygon_keep: %d polygons, %d groups, %lld mask words",
                n, n_groups, (long long)mask_words);
  hipLaunchKernelGGL(overlap_keep_kernel, dim3((unsigned)n_groups), dim3(OV_KEEP_THREADS), 0, (hipStream_t)s, reinterpret_cast<const unsigned long long*>(mask),
                     mask_start, mask_words, group_start, n, order, owner, kept);
  OMP_CHECK_LAUNCH("omp_polygon_keep");
  return OMP_OK;
}
