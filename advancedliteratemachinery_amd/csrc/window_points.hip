// Window prompts: the device step between the point phase and the polygon / recognition phases.
// A point phase of `rows` rows (W windows per image, rows sorted by image) leaves its tokens in seq [rows][seq_ld] with the sampling
// kernels' finished / lengths flags beside them.  omp_window_points turns these buffers, as they lie, into ONE compacted list of
// (x, y) points in row order -- the input of the polygon and recognition phases -- and the counts that size those phases.  Integers
// only: utils/windows.py: gather_points_cpu (the specification) and these kernels agree on every output.
//
//   window_count_kernel   a wave per row: the row's token range (reference transformer.py:126-139: tokens before the EOS, odd tail
//                         dropped), its pairs tested against the row's own window when clip is set -> row_count, dropped
//   window_scan_kernel    ONE workgroup: exclusive prefix sum of row_count over all rows (1024 rows per pass: shuffle scan inside a wave,
//                         the 16 wave totals through LDS, a running carry) -> row_start [rows + 1]; and the per-image sums through the
//                         row -> image table (integer atomics on counters this workgroup zeroed itself: order does not matter)
//   window_copy_kernel    a wave per row again: 64 pairs per pass, ballot + popcount ranks the kept pairs in the decoder's order
//                         (a STABLE compaction), points and inst_row written at row_start[r] + rank while that is below cap
// Three launches on the caller's stream; nothing is allocated and nothing synchronises.  Every seq index is below seq_ld (the token
// range is clamped), every output index below cap / rows / n_images.
#include "common.h"

namespace {

constexpr int WP_SCAN_THREADS = 1024;

struct WinRow {
  int n_pairs;            // pairs in the row's token range
  int x0, y0, x1, y1;     // the row's window (only read when clip)
};

__device__ __forceinline__ WinRow win_row(const int32_t* __restrict__ seq_row, int seq_ld, int fin, int len, int n_prompt, int sampled, int clip) {
  WinRow w;
  int end = fin ? len : n_prompt + sampled;
  end = min(max(end, n_prompt), seq_ld);
  w.n_pairs = (end - n_prompt) >> 1;
  w.x0 = w.y0 = w.x1 = w.y1 = 0;
  if (clip) { w.x0 = seq_row[0]; w.y0 = seq_row[1]; w.x1 = seq_row[2]; w.y1 = seq_row[3]; }
  return w;
}

// the reference's membership rule (dataset/collate_fn.py:80-81): strict lower bounds, inclusive upper bounds
__device__ __forceinline__ bool win_keep(const WinRow& w, int x, int y, int clip) {
  return !clip || (x > w.x0 && x <= w.x1 && y > w.y0 && y <= w.y1);
}

__global__ __launch_bounds__(256) void window_count_kernel(const int32_t* __restrict__ seq, int seq_ld, const int32_t* __restrict__ finished,
                                                           const int32_t* __restrict__ lengths, int rows, int n_prompt, int sampled, int clip,
                                                           int32_t* __restrict__ row_count, int32_t* __restrict__ dropped) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;   // wave-uniform
  const int32_t* sr = seq + (int64_t)r * seq_ld;
  const WinRow w = win_row(sr, seq_ld, finished[r], lengths[r], n_prompt, sampled, clip);
  int kept = 0;
  for (int j = lane; j < w.n_pairs; j += 64) {
    kept += win_keep(w, sr[n_prompt + 2 * j], sr[n_prompt + 2 * j + 1], clip) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
  if (lane == 0) {
    row_count[r] = kept;
    dropped[r] = w.n_pairs - kept;
  }
}

__global__ __launch_bounds__(WP_SCAN_THREADS) void window_scan_kernel(const int32_t* __restrict__ row_count, const int32_t* __restrict__ row_image,
                                                                      int rows, int n_images, int32_t* __restrict__ row_start,
                                                                      int32_t* __restrict__ image_count) {
  __shared__ int wave_tot[WP_SCAN_THREADS / OMP_WAVE];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < n_images; i += WP_SCAN_THREADS) image_count[i] = 0;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < rows; base += WP_SCAN_THREADS) {
    const int r = base + tid;
    const int v = r < rows ? row_count[r] : 0;
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
    if (r < rows) {
      row_start[r] = carry + before + inc - v;
      const int img = row_image[r];
      if (v != 0 && img >= 0 && img < n_images) atomicAdd(image_count + img, v);
    }
    if (tid == WP_SCAN_THREADS - 1) carry_s = carry + before + inc;   // every thread read the old carry ahead of the barrier above
    __syncthreads();   // ... and has read wave_tot before the next pass rewrites it
  }
  if (tid == 0) row_start[rows] = carry_s;
}

__global__ __launch_bounds__(256) void window_copy_kernel(const int32_t* __restrict__ seq, int seq_ld, const int32_t* __restrict__ finished,
                                                          const int32_t* __restrict__ lengths, int rows, int n_prompt, int sampled, int clip,
                                                          const int32_t* __restrict__ row_start, int32_t* __restrict__ points,
                                                          int32_t* __restrict__ inst_row, int cap) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;   // wave-uniform
  const int32_t* sr = seq + (int64_t)r * seq_ld;
  const WinRow w = win_row(sr, seq_ld, finished[r], lengths[r], n_prompt, sampled, clip);
  int64_t at = row_start[r];
  for (int j0 = 0; j0 < w.n_pairs; j0 += 64) {   // wave-uniform trip count
    const int j = j0 + lane;
    int x = 0, y = 0;
    bool keep = false;
    if (j < w.n_pairs) {
      x = sr[n_prompt + 2 * j];
      y = sr[n_prompt + 2 * j + 1];
      keep = win_keep(w, x, y, clip);
    }
    const unsigned long long m = __ballot(keep);
    const int64_t dst = at + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && dst < cap) {
      *reinterpret_cast<u32x2*>(points + 2 * dst) = u32x2{(uint32_t)x, (uint32_t)y};
      inst_row[dst] = r;
    }
    at += __popcll(m);
  }
}

}  // namespace

extern "C" int omp_window_points(const int32_t* seq, int seq_ld, const int32_t* finished, const int32_t* lengths, const int32_t* row_image,
                                 int rows, int n_images, int n_prompt, int sampled, int clip, int32_t* points, int32_t* inst_row, int cap,
                                 int32_t* row_count, int32_t* dropped, int32_t* row_start, int32_t* image_count, omp_stream_t s) {
  OMP_CHECK_ARG(seq && finished && lengths && row_image && points && inst_row && row_count && dropped && row_start && image_count,
                "omp_window_points: null pointer");
  OMP_CHECK_ARG(rows > 0 && rows <= (1 << 24) && n_images > 0 && cap >= 0, "omp_window_points: %d rows, %d images, cap %d", rows, n_images, cap);
  OMP_CHECK_ARG(n_prompt >= (clip ? 4 : 0) && n_prompt <= seq_ld && sampled >= 0 && sampled <= (1 << 30) && (int64_t)rows * (seq_ld / 2) <= 0x7fffffff,
                "omp_window_points: n_prompt %d (clip reads seq[r, 0:4]), sampled %d, seq_ld %d (rows x seq_ld / 2 must fit int32)", n_prompt, sampled,
                seq_ld);
  const hipStream_t st = (hipStream_t)s;
  const dim3 per_row((unsigned)((rows + 3) / 4));
  hipLaunchKernelGGL(window_count_kernel, per_row, dim3(256), 0, st, seq, seq_ld, finished, lengths, rows, n_prompt, sampled, clip ? 1 : 0, row_count,
                     dropped);
  OMP_CHECK_LAUNCH("omp_window_points (count)");
  hipLaunchKernelGGL(window_scan_kernel, dim3(1), dim3(WP_SCAN_THREADS), 0, st, row_count, row_image, rows, n_images, row_start, image_count);
  OMP_CHECK_LAUNCH("omp_window_points (scan)");
  hipLaunchKernelGGL(window_copy_kernel, per_row, dim3(256), 0, st, seq, seq_ld, finished, lengths, rows, n_prompt, sampled, clip ? 1 : 0, row_start,
                     points, inst_row, cap);
  OMP_CHECK_LAUNCH("omp_window_points (copy)");
  return OMP_OK;
}
