// Tiled pages: the device stage between the tiles' words and the pages' words.
// A tiled call reads every tile of every page in one engine flow; the decoders leave the words' ids in TILE bins.  omp_tile_remap carries
// them into PAGE bins, flags the words that reach an inner side of their tile (fragments of words the neighbouring tile sees whole) and
// compacts the others into one list in tile order -- the input of overlap suppression, reading order and the crops.  Integers only:
// utils/tiles.py: remap_cpu (the specification) and these kernels agree on every output.
//
//   tile_flag_kernel   a workgroup of 4 waves per tile, a wave per word: the lanes hold the word's 34 ids (32 polygon coordinates and the
//                      point), clamp them, reduce min / max per axis with shuffles that keep a lane's parity, set the cut bits and remap
//                      their id with one 64-bit division each -> cut, the remapped row at scratch[word], the tile's keep count
//   tile_scan_kernel   ONE workgroup: exclusive prefix sum of the tiles' counts (1024 tiles per pass, as window_scan_kernel) -> out_start
//                      [T + 1]; and the per-page sums through tile_page (integer atomics on counters this workgroup zeroed itself)
//   tile_copy_kernel   a wave per tile: 64 words per pass, ballot of the kept ones, then row by row in bit order (a STABLE compaction):
//                      lanes 0..33 move the row, lane 34 writes src_row, while the position is below cap and inside the tile's range
// Three launches on the caller's stream; nothing is allocated and nothing synchronises.  A tile is accepted only when its row range lies in
// [0, n], its page is in the table and 1 .. 65535 pixels a side, and its rectangle lies inside the page (tile_desc): every polys / points /
// scratch / cut index is a word of an accepted range, every output index is below cap.  A refused tile writes its two counts and nothing else.
#include "common.h"

namespace {

constexpr int TL_SCAN_THREADS = 1024;
constexpr int TL_ROW = 34;          // ids per word
constexpr int TL_MAX_BINS = 4096;   // utils/tiles.py: BINS_MAX
constexpr int TL_MAX_SIDE = 65535;  // utils/tiles.py: SIDE_MAX

struct TileDesc {
  int ok;
  int lo, hi;            // the tile's words
  int x0, y0, x1, y1;    // its rectangle in page pixels
  int W, H;              // its page
};

// tables = row_start [T + 1] | tile_rect [T][4] | tile_page [T] | page_size [pages][2]
__device__ __forceinline__ TileDesc tile_desc(const int32_t* __restrict__ tables, int k, int n_tiles, int n_pages, int n) {
  TileDesc t;
  const int32_t* rect = tables + (n_tiles + 1) + 4 * k;
  t.lo = tables[k];
  t.hi = tables[k + 1];
  t.x0 = rect[0]; t.y0 = rect[1]; t.x1 = rect[2]; t.y1 = rect[3];
  const int page = tables[(n_tiles + 1) + 4 * n_tiles + k];
  t.W = t.H = 0;
  t.ok = t.lo >= 0 && t.lo <= t.hi && t.hi <= n && page >= 0 && page < n_pages;
  if (t.ok) {
    const int32_t* size = tables + (n_tiles + 1) + 5 * n_tiles + 2 * page;
    t.W = size[0];
    t.H = size[1];
    t.ok = t.W >= 1 && t.W <= TL_MAX_SIDE && t.H >= 1 && t.H <= TL_MAX_SIDE && t.x0 >= 0 && t.x0 < t.x1 && t.x1 <= t.W && t.y0 >= 0 &&
           t.y0 < t.y1 && t.y1 <= t.H;
  }
  return t;
}

__global__ __launch_bounds__(256) void tile_flag_kernel(const int32_t* __restrict__ polys, const int32_t* __restrict__ points, int n,
                                                        const int32_t* __restrict__ tables, int n_tiles, int n_pages, int nb, int page_bins,
                                                        int edge, int drop_cut, int32_t* __restrict__ scratch, int32_t* __restrict__ cut,
                                                        int32_t* __restrict__ tile_count, int32_t* __restrict__ tile_dropped) {
  __shared__ int wave_kept[4];
  const int k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const TileDesc t = tile_desc(tables, k, n_tiles, n_pages, n);   // workgroup-uniform
  if (!t.ok) {
    if (threadIdx.x == 0) {
      tile_count[k] = -1;
      tile_dropped[k] = 0;
    }
    return;
  }
  const bool live = lane < TL_ROW, is_x = (lane & 1) == 0;   // lanes 32 / 33 hold the point's x / y: the parity is the axis
  const int64_t org = is_x ? t.x0 : t.y0, ext = is_x ? t.x1 - t.x0 : t.y1 - t.y0, side = is_x ? t.W : t.H;
  const int64_t den = 2 * (int64_t)nb * side;
  int kept = 0;
  for (int w = t.lo + wave; w < t.hi; w += 4) {   // wave-uniform
    int c = 0;
    if (lane < 32) c = polys[(int64_t)w * 32 + lane];
    else if (live) c = points[(int64_t)w * 2 + (lane - 32)];
    c = min(max(c, 0), nb - 1);
    int lo = live ? c : 0x7fffffff, hi = live ? c : -1;
#pragma unroll
    for (int o = 32; o > 1; o >>= 1) {   // offsets 32 .. 2 keep the parity: lane 0 ends with x, lane 1 with y
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    const int min_x = __shfl(lo, 0, 64), min_y = __shfl(lo, 1, 64), max_x = __shfl(hi, 0, 64), max_y = __shfl(hi, 1, 64);
    const int bits = ((t.x0 > 0 && min_x <= edge) ? 1 : 0) | ((t.y0 > 0 && min_y <= edge) ? 2 : 0) |
                     ((t.x1 < t.W && max_x >= nb - 1 - edge) ? 4 : 0) | ((t.y1 < t.H && max_y >= nb - 1 - edge) ? 8 : 0);
    if (live) {
      const uint64_t num = (uint64_t)(2 * (org * nb + (int64_t)c * ext) * page_bins + (int64_t)nb * side);   // below 2^43
      const int64_t q = (int64_t)(num / (uint64_t)den);
      scratch[(int64_t)w * TL_ROW + lane] = (int32_t)(q < page_bins - 1 ? q : page_bins - 1);
    }
    if (lane == 0) cut[w] = bits;
    kept += (!drop_cut || bits == 0) ? 1 : 0;
  }
  if (lane == 0) wave_kept[wave] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = wave_kept[0] + wave_kept[1] + wave_kept[2] + wave_kept[3];
    tile_count[k] = total;
    tile_dropped[k] = (t.hi - t.lo) - total;
  }
}

__global__ __launch_bounds__(TL_SCAN_THREADS) void tile_scan_kernel(const int32_t* __restrict__ tile_count, const int32_t* __restrict__ tile_page,
                                                                    int n_tiles, int n_pages, int32_t* __restrict__ out_start,
                                                                    int32_t* __restrict__ page_count) {
  __shared__ int wave_tot[TL_SCAN_THREADS / OMP_WAVE];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < n_pages; i += TL_SCAN_THREADS) page_count[i] = 0;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n_tiles; base += TL_SCAN_THREADS) {
    const int k = base + tid;
    const int v = k < n_tiles ? max(tile_count[k], 0) : 0;   // a refused tile (-1) holds no rows
    int inc = v;   // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) wave_tot[wave] = inc;
    const int carry = carry_s;
    __syncthreads();
    int before = 0;
    for (int i = 0; i < wave; ++i) before += wave_tot[i];
    if (k < n_tiles) {
      out_start[k] = carry + before + inc - v;
      const int page = tile_page[k];
      if (v != 0 && page >= 0 && page < n_pages) atomicAdd(page_count + page, v);
    }
    if (tid == TL_SCAN_THREADS - 1) carry_s = carry + before + inc;   // every thread read the old carry ahead of the barrier above
    __syncthreads();   // ... and has read wave_tot before the next pass rewrites it
  }
  if (tid == 0) out_start[n_tiles] = carry_s;
}

__global__ __launch_bounds__(256) void tile_copy_kernel(const int32_t* __restrict__ tables, int n_tiles, int n_pages, int n, int drop_cut,
                                                        const int32_t* __restrict__ scratch, const int32_t* __restrict__ cut,
                                                        const int32_t* __restrict__ tile_count, const int32_t* __restrict__ out_start,
                                                        int32_t* __restrict__ page_polys, int32_t* __restrict__ page_points,
                                                        int32_t* __restrict__ src_row, int cap) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n_tiles) return;   // wave-uniform
  if (tile_count[k] <= 0) return;   // refused or empty
  const TileDesc t = tile_desc(tables, k, n_tiles, n_pages, n);
  if (!t.ok) return;
  int64_t at = out_start[k];
  const int64_t lim = min((int64_t)cap, (int64_t)out_start[k + 1]);
  for (int w0 = t.lo; w0 < t.hi && at < lim; w0 += 64) {   // wave-uniform
    const int w = w0 + lane;
    const bool keep = w < t.hi && (!drop_cut || cut[w] == 0);
    unsigned long long m = __ballot(keep);
    while (m != 0ull && at < lim) {
      const int src = w0 + (__ffsll((long long)m) - 1);
      m &= m - 1ull;
      if (lane < 32) page_polys[at * 32 + lane] = scratch[(int64_t)src * TL_ROW + lane];
      else if (lane < TL_ROW) page_points[at * 2 + (lane - 32)] = scratch[(int64_t)src * TL_ROW + lane];
      else if (lane == TL_ROW) src_row[at] = src;
      ++at;
    }
  }
}

}  // namespace

extern "C" int omp_tile_remap(const int32_t* polys, const int32_t* points, int n, const int32_t* tables, int n_tiles, int n_pages, int nb,
                              int page_bins, int edge, int drop_cut, int32_t* scratch, int32_t* cut, int32_t* page_polys, int32_t* page_points,
                              int32_t* src_row, int cap, int32_t* tile_count, int32_t* tile_dropped, int32_t* out_start, int32_t* page_count,
                              omp_stream_t s) {
  OMP_CHECK_ARG(polys && points && tables && scratch && cut && page_polys && page_points && src_row && tile_count && tile_dropped && out_start &&
                    page_count,
                "omp_tile_remap: null pointer");
  OMP_CHECK_ARG(n > 0 && n <= (1 << 24) && n_tiles > 0 && n_tiles <= (1 << 20) && n_pages > 0 && n_pages <= (1 << 20) && cap >= 0,
                "omp_tile_remap: %d words, %d tiles, %d pages, cap %d", n, n_tiles, n_pages, cap);
  OMP_CHECK_ARG(nb >= 2 && nb <= TL_MAX_BINS && page_bins >= 2 && page_bins <= TL_MAX_BINS && edge >= 0 && edge <= TL_MAX_BINS,
                "omp_tile_remap: %d tile bins, %d page bins (2 .. %d), edge %d (0 .. %d)", nb, page_bins, TL_MAX_BINS, edge, TL_MAX_BINS);
  const hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(tile_flag_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, polys, points, n, tables, n_tiles, n_pages, nb, page_bins, edge,
                     drop_cut ? 1 : 0, scratch, cut, tile_count, tile_dropped);
  OMP_CHECK_LAUNCH("omp_tile_remap (flag)");
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(TL_SCAN_THREADS), 0, st, tile_count, tables + (n_tiles + 1) + 4 * n_tiles, n_tiles, n_pages,
                     out_start, page_count);
  OMP_CHECK_LAUNCH("omp_tile_remap (scan)");
  hipLaunchKernelGGL(tile_copy_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, st, tables, n_tiles, n_pages, n, drop_cut ? 1 : 0, scratch,
                     cut, tile_count, out_start, page_polys, page_points, src_row, cap);
  OMP_CHECK_LAUNCH("omp_tile_remap (copy)");
  return OMP_OK;
}
