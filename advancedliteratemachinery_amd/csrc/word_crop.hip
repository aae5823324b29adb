// Word crops for the recogniser, a whole chunk per launch.
//
// Two kernels, run back to back on the caller's stream:
//   omp_polygon_rectify  every crop's 16-point polygon (OmniParser's records: 8 points along the top edge, 8 back along the
//                        bottom, utils/misc.py: bezier2polygon) -> a uint8 strip of the word's own resolution, sampled
//                        bilinearly along the polygon.  What BezierAlign does for a curved-text spotter, in integer
//                        arithmetic (16 fractional bits) so that utils/word_crops.py: rectify_polygon_cpu and this kernel
//                        agree on every byte.
//   omp_resize_crops     every strip (or any uint8 crop) -> fp32 [N, 3, out_h, out_w]: the per-pixel arithmetic of
//                        resize_norm_pad_kernel (csrc/preprocess.hip: Pillow's 8-bit resampler, horizontal pass rounded to
//                        uint8, then vertical, then the ToTensor table) with the crop's tables found through a descriptor.
// Neither allocates: descriptors, tables, the strip scratch and the output are the caller's.
#include "common.h"

namespace {

constexpr int WC_Q = 16;
constexpr int64_t WC_ONE = (int64_t)1 << WC_Q;
constexpr int WC_SMAX = 4096;

// floor(n / d), d > 0 (C++ division truncates towards zero)
__device__ __forceinline__ int64_t floordiv(int64_t n, int64_t d) {
  int64_t q = n / d;
  if (n - q * d < 0) --q;
  return q;
}

// the crop whose tile range holds `tile`: the last descriptor with tile0 <= tile (tile0 is ascending, desc[0].tile0 = 0)
__device__ __forceinline__ int find_crop(const omp_rectify_desc* d, int n, int64_t tile) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void polygon_rectify_kernel(const omp_rectify_desc* __restrict__ desc, int n, uint8_t* __restrict__ scratch,
                                                              int64_t scratch_bytes) {
  __shared__ int64_t edge[2][64][2];   // [top | bottom][column of the tile][x | y], Q16
  const omp_rectify_desc& d = desc[find_crop(desc, n, blockIdx.x)];
  const int sh = d.sh, sw = d.sw, W = d.w, H = d.h;
  // a descriptor this kernel cannot honour writes nothing (the host wrapper checks what it can see; the table is on the device)
  if (sh < 1 || sw < 1 || sh > WC_SMAX || sw > WC_SMAX || W < 1 || H < 1 || d.strip_off < 0 ||
      d.strip_off + (int64_t)sh * sw * 3 > scratch_bytes)
    return;
  const int tiles_x = (sw + 63) >> 6;
  const int64_t t = (int64_t)blockIdx.x - d.tile0;
  if (t >= (int64_t)tiles_x * ((sh + 3) >> 2)) return;
  const int c0 = (int)(t % tiles_x) * 64, j0 = (int)(t / tiles_x) * 4;
  // top(c) / bot(c) once per column of the tile: threads 0..63 the top edge, 64..127 the bottom edge
  if (threadIdx.x < 128) {
    const int e = threadIdx.x >> 6, lc = threadIdx.x & 63;
    const int c = min(c0 + lc, sw - 1);
    const int64_t nn = 7 * (2 * (int64_t)c + 1), den = 2 * (int64_t)sw;
    const int k = (int)min(nn / den, (int64_t)6);
    const int64_t r = nn - k * den;
    // T[k] = P[k], B[k] = P[15 - k]
    const int64_t* p0 = d.pq + 2 * (e ? 15 - k : k);
    const int64_t* p1 = d.pq + 2 * (e ? 14 - k : k + 1);
    edge[e][lc][0] = p0[0] + floordiv(2 * (p1[0] - p0[0]) * r + den, 2 * den);
    edge[e][lc][1] = p0[1] + floordiv(2 * (p1[1] - p0[1]) * r + den, 2 * den);
  }
  __syncthreads();
  const int lc = threadIdx.x & 63;
  const int c = c0 + lc, j = j0 + (threadIdx.x >> 6);
  if (c >= sw || j >= sh) return;
  const int64_t m = 2 * (int64_t)j + 1, dv = 2 * (int64_t)sh;
  const int64_t tx = edge[0][lc][0], ty = edge[0][lc][1];
  const int64_t px = tx + floordiv(2 * (edge[1][lc][0] - tx) * m + dv, 2 * dv);
  const int64_t py = ty + floordiv(2 * (edge[1][lc][1] - ty) * m + dv, 2 * dv);
  const int64_t sx = min(max(px - WC_ONE / 2, (int64_t)0), (int64_t)(W - 1) << WC_Q);
  const int64_t sy = min(max(py - WC_ONE / 2, (int64_t)0), (int64_t)(H - 1) << WC_Q);
  const int ix = (int)(sx >> WC_Q), iy = (int)(sy >> WC_Q);
  const uint32_t fx = (uint32_t)(sx & (WC_ONE - 1)), fy = (uint32_t)(sy & (WC_ONE - 1));
  const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
  const uint8_t* r0 = d.src + (int64_t)iy * d.pitch;
  const uint8_t* r1 = d.src + (int64_t)iy1 * d.pitch;
  uint8_t* o = scratch + d.strip_off + ((int64_t)j * sw + c) * 3;
  const uint32_t gx = (uint32_t)WC_ONE - fx;
  const uint64_t gy = (uint64_t)WC_ONE - fy;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const uint32_t a = (uint32_t)r0[3 * ix + ch] * gx + (uint32_t)r0[3 * ix1 + ch] * fx;
    const uint32_t b = (uint32_t)r1[3 * ix + ch] * gx + (uint32_t)r1[3 * ix1 + ch] * fx;
    o[ch] = (uint8_t)(((uint64_t)a * gy + (uint64_t)b * fy + ((uint64_t)1 << 31)) >> 32);
  }
}

constexpr int WC_BITS = 32 - 8 - 2;   // Pillow Resample.c PRECISION_BITS

__device__ __forceinline__ int wc_clip8(int acc) {
  const int v = acc >> WC_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void resize_crops_kernel(const omp_resize_desc* __restrict__ desc, const int32_t* __restrict__ table,
                                                           int64_t table_len, const float* __restrict__ lut, float* __restrict__ dst, int out_h,
                                                           int out_w, int tiles_x, int tiles) {
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int x = (t % tiles_x) * 64 + (threadIdx.x & 63);
  const int y = (t / tiles_x) * 4 + (threadIdx.x >> 6);
  if (x >= out_w || y >= out_h) return;
  const omp_resize_desc& d = desc[n];
  const int need_h = d.ksx > 0, need_v = d.ksy > 0;
  int x0 = x, nx = 1, y0 = y, ny = 1;
  const int32_t* kx = nullptr;
  const int32_t* ky = nullptr;
  // table offsets are checked against the table, source indices against the crop: a bad descriptor writes nothing
  if (need_h) {
    if (d.xb < 0 || d.kx < 0 || d.xb + 2 * (int64_t)out_w > table_len || d.kx + (int64_t)out_w * d.ksx > table_len) return;
    x0 = table[d.xb + 2 * x]; nx = table[d.xb + 2 * x + 1];
    kx = table + d.kx + (int64_t)x * d.ksx;
    if (nx > d.ksx) return;
  }
  if (need_v) {
    if (d.yb < 0 || d.ky < 0 || d.yb + 2 * (int64_t)out_h > table_len || d.ky + (int64_t)out_h * d.ksy > table_len) return;
    y0 = table[d.yb + 2 * y]; ny = table[d.yb + 2 * y + 1];
    ky = table + d.ky + (int64_t)y * d.ksy;
    if (ny > d.ksy) return;
  }
  if (x0 < 0 || nx < 0 || x0 + nx > d.in_w || y0 < 0 || ny < 0 || y0 + ny > d.in_h) return;
  const int half = 1 << (WC_BITS - 1);
  int v0 = half, v1 = half, v2 = half;
  int h0 = 0, h1 = 0, h2 = 0;
  const int64_t plane = (int64_t)out_h * out_w;
  float* o = dst + (int64_t)n * 3 * plane + (int64_t)y * out_w + x;
  // Image.resize runs the vertical pass first on a crop more than 100 times as high as wide that gets lower (csrc/preprocess.hip)
  if (need_h && need_v && (int64_t)d.in_h > (int64_t)d.in_w * 100 && out_h < d.in_h) {
    int a0 = half, a1 = half, a2 = half;
    for (int i = 0; i < nx; ++i) {
      const uint8_t* col = d.src + (int64_t)y0 * d.pitch + (int64_t)(x0 + i) * 3;
      int c0 = half, c1 = half, c2 = half;
      for (int r = 0; r < ny; ++r) {
        const int k = ky[r];
        c0 += (int)col[0] * k; c1 += (int)col[1] * k; c2 += (int)col[2] * k;
        col += d.pitch;
      }
      const int k = kx[i];
      a0 += wc_clip8(c0) * k; a1 += wc_clip8(c1) * k; a2 += wc_clip8(c2) * k;
    }
    o[0] = lut[wc_clip8(a0)];
    o[plane] = lut[256 + wc_clip8(a1)];
    o[2 * plane] = lut[512 + wc_clip8(a2)];
    return;
  }
  for (int r = 0; r < ny; ++r) {
    const uint8_t* row = d.src + (int64_t)(y0 + r) * d.pitch + (int64_t)x0 * 3;
    if (need_h) {
      int a0 = half, a1 = half, a2 = half;
      for (int i = 0; i < nx; ++i) {
        const int k = kx[i];
        a0 += (int)row[3 * i] * k; a1 += (int)row[3 * i + 1] * k; a2 += (int)row[3 * i + 2] * k;
      }
      h0 = wc_clip8(a0); h1 = wc_clip8(a1); h2 = wc_clip8(a2);
    } else {
      h0 = row[0]; h1 = row[1]; h2 = row[2];
    }
    if (need_v) {
      const int k = ky[r];
      v0 += h0 * k; v1 += h1 * k; v2 += h2 * k;
    }
  }
  if (need_v) { h0 = wc_clip8(v0); h1 = wc_clip8(v1); h2 = wc_clip8(v2); }
  o[0] = lut[h0];
  o[plane] = lut[256 + h1];
  o[2 * plane] = lut[512 + h2];
}

}  // namespace

extern "C" int omp_polygon_rectify(const omp_rectify_desc* desc, int n, int64_t total_tiles, uint8_t* scratch, int64_t scratch_bytes,
                                   omp_stream_t s) {
  OMP_CHECK_ARG(desc && scratch, "omp_polygon_rectify: null pointer");
  OMP_CHECK_ARG(n > 0 && scratch_bytes > 0, "omp_polygon_rectify: %d crops, %lld scratch bytes", n, (long long)scratch_bytes);
  // every crop has at least one tile and at most (SMAX / 64) * (SMAX / 4)
  OMP_CHECK_ARG(total_tiles >= n && total_tiles <= (int64_t)n * (WC_SMAX / 64) * (WC_SMAX / 4) && total_tiles <= 0x7fffffffLL,
                "omp_polygon_rectify: %lld tiles for %d crops", (long long)total_tiles, n);
  hipLaunchKernelGGL(polygon_rectify_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)s, desc, n, scratch, scratch_bytes);
  OMP_CHECK_LAUNCH("omp_polygon_rectify");
  return OMP_OK;
}

extern "C" int omp_resize_crops(const omp_resize_desc* desc, int n, const int32_t* table, int64_t table_len, const float* lut, float* dst,
                                int out_h, int out_w, omp_stream_t s) {
  OMP_CHECK_ARG(desc && lut && dst, "omp_resize_crops: null pointer");
  OMP_CHECK_ARG(table_len >= 0 && (table || table_len == 0), "omp_resize_crops: %lld table entries but no table", (long long)table_len);
  OMP_CHECK_ARG(n > 0 && out_h > 0 && out_w > 0, "omp_resize_crops: %d crops, out %dx%d", n, out_h, out_w);
  const int tiles_x = (out_w + 63) / 64;
  const int64_t tiles = (int64_t)tiles_x * ((out_h + 3) / 4);
  OMP_CHECK_ARG(tiles * n <= 0x7fffffffLL, "omp_resize_crops: %d crops of %dx%d exceed one grid", n, out_h, out_w);
  hipLaunchKernelGGL(resize_crops_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, (hipStream_t)s, desc, table, table_len, lut, dst, out_h,
                     out_w, tiles_x, (int)tiles);
  OMP_CHECK_LAUNCH("omp_resize_crops");
  return OMP_OK;
}
