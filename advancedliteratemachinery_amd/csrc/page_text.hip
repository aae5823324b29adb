// Page text scoring: the Levenshtein distance of whole pages, thousands to tens of thousands of characters a side, on the device
// (DESIGN.md section 23).  utils/page_text.py (distance_cpu / pairs_cpu: the specification) and this kernel agree on every integer.
// Insert / delete / substitute cost 1; code 255 equals nothing, itself included; codes are below sigma or 255.
//
// Myers' block-based bit-parallel recurrence, pipelined across a wave: the forward pass is page_forward of myers.h, which explains blocks,
// Peq, steps, stripes and the distance; page_align.hip runs the same pass with a record.
//
//   page_edit_kernel   one wave (a 64-thread workgroup) per pair (a, b).  a is the pattern, b the text.  The distance is la + the sum of
//                      the carry-outs of the last block; la == 0 gives lb, lb == 0 gives la.  The pair's slice of scratch holds
//                      page_forward's two carry buffers (PT_SLICE_BYTES).
//   No atomics; one wave walks one pair in a fixed order, so the result does not depend on scheduling.
// A descriptor out of range (a negative length, a length above 65535, a range outside the pool) is REFUSED on the device: dist = -1,
// and nothing outside the pool is read.  Nothing is allocated and nothing synchronises: pool, tables, scratch and dist are the caller's.
#include "myers.h"

namespace {

// the distance needs no record of the table
struct NoRecord {
  static constexpr bool kRecords = false;
  __device__ __forceinline__ void stripe(int, int) {}
  __device__ __forceinline__ void cell(int, int, int, u64, u64, u64, u64, u64) {}
};

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
  NoRecord rec;
  const int acc = page_forward(pool + ao, pool + bo, la, lb, sigma, pt_peq, scratch + (int64_t)p * (2 * PT_CARRY_WORDS), rec);
  const int nb = (la + PT_BLOCK - 1) / PT_BLOCK;   // pattern blocks: the last one's lane holds the sum
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
  size_t lds;
  const int rc = page_forward_lds<page_edit_kernel>(sigma, "omp_page_edit_distance", &lds);
  if (rc != OMP_OK) return rc;
  hipLaunchKernelGGL(page_edit_kernel, dim3((unsigned)n_pairs), dim3(64), lds, (hipStream_t)s, pool, pool_bytes, a_off, a_len, b_off, b_len, sigma,
                     reinterpret_cast<u64*>(scratch), dist);
  OMP_CHECK_LAUNCH("omp_page_edit_distance");
  return OMP_OK;
}
