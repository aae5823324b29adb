// Scoring: one-to-one matching of detections to ground-truth words under the IoU protocol, for a sweep of score thresholds
// (DESIGN.md section 21).  utils/scoring.py (match_cpu / match_pages_cpu: the specification) and this kernel agree on every output.
// The intersections are omp_polygon_overlap's dense matrices (csrc/overlap.hip), one per image, polygons ordered ground truth first;
// nothing here looks at a polygon.
//
//   score_match_kernel   a workgroup per (image g, threshold index k), 256 threads.
//     setup     the threads stride over the image's detections: area (the diagonal) into LDS, ACTIVE = level > k, DON'T-CARE = active
//               and covered to t_dc by a don't-care ground-truth word (the rows of those words only, each contiguous).  A wave ballot
//               is the 64-detection word of the FREE set (active, not don't-care, not taken), which lives in LDS; the ballots'
//               popcounts add up to the care detections.
//     matching  per care ground-truth row, in order: the waves stride over the row of inter in words of 64 detections, a ballot of
//               "free and passes t_iou" gives a wave its lowest qualifying detection (its first non-zero ballot: the words ascend),
//               one LDS min joins the waves, and between a pair of barriers thread 0 takes the detection out of the free set.
//               Rows of don't-care words are skipped by all threads alike (gt_dc is read uniformly).
//   Work per (image, threshold): (don't-care rows + care rows) x detections reads of inter; the sweep re-reads the rows per threshold
//   from L2.  An image without ground truth or without detections reads nothing of inter.
// Every index is clamped or tested: group bounds into [0, n], n_gt into the group, the matrix of a group against the end of the inter
// table (inter_start[n_groups]); a group that does not fit is REFUSED on the device: its counts are -1 and its assignment rows -4.
#include "common.h"

namespace {

constexpr int SC_MAX_GROUP = 8192;
constexpr int SC_MAX_THR = 64;
constexpr int SC_THREADS = 256;
constexpr int SC_WORDS = SC_MAX_GROUP / 64;
constexpr int SC_NONE = 0x7fffffff;
constexpr int SC_DET_UNMATCHED = -1, SC_DET_DONT_CARE = -2, SC_DET_INACTIVE = -3, SC_GT_UNMATCHED = -1, SC_GT_DONT_CARE = -2, SC_NA = -4;

__global__ __launch_bounds__(SC_THREADS) void score_match_kernel(const int32_t* __restrict__ inter, const int64_t* __restrict__ inter_start,
                                                                 const int32_t* __restrict__ group_start, const int32_t* __restrict__ n_gt,
                                                                 const int32_t* __restrict__ gt_dc, const int32_t* __restrict__ text,
                                                                 const int32_t* __restrict__ level, int n, int n_groups, int n_thr, int t_iou, int t_dc,
                                                                 int report, int32_t* __restrict__ counts, int32_t* __restrict__ det_gt,
                                                                 int32_t* __restrict__ gt_det) {
  __shared__ int area_s[SC_MAX_GROUP];                  // the detections' areas
  __shared__ unsigned long long free_s[SC_WORDS];       // bit d: detection d is active, not don't-care and not taken
  __shared__ int best_s, care_s;
  const int g = blockIdx.x / n_thr, k = blockIdx.x - g * n_thr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g0 = min(max(group_start[g], 0), n), g1 = min(max(group_start[g + 1], g0), n);
  const int ng = g1 - g0, m = n_gt[g];
  const int64_t base = inter_start[g], total = inter_start[n_groups];
  const bool rep = k == report && det_gt && gt_det;
  const bool clear = report < 0 && k == 0 && det_gt && gt_det;   // no report: the image's first workgroup marks its rows "not applicable"
  int32_t* cnt = counts + ((int64_t)g * n_thr + k) * 4;
  if (ng > SC_MAX_GROUP || m < 0 || m > ng || base < 0 || base + (int64_t)ng * ng > total) {   // refused (block-uniform)
    if (tid < 4) cnt[tid] = -1;
    if (rep || clear) {
      for (int i = g0 + tid; i < g1; i += SC_THREADS) {
        det_gt[i] = SC_NA;
        gt_det[i] = SC_NA;
      }
    }
    return;
  }
  if (clear) {
    for (int i = g0 + tid; i < g1; i += SC_THREADS) {
      det_gt[i] = SC_NA;
      gt_det[i] = SC_NA;
    }
  }
  const int nd = ng - m;
  const int32_t* __restrict__ mat = inter + base;   // [ng][ng]; only read when m > 0 and nd > 0
  if (tid == 0) {
    best_s = SC_NONE;
    care_s = 0;
  }
  __syncthreads();
  // ---- setup: areas, the free set, care detections ----
  int care_det = 0;
  for (int c = wave * 64; c < nd; c += SC_THREADS) {   // wave-uniform trip count: word c / 64 belongs to this wave
    const int d = c + lane;
    const bool valid = d < nd;
    const bool active = valid && level[g0 + m + d] > k;
    int area_d = 0;
    bool dc = false;
    if (valid && m > 0) {
      area_d = mat[(int64_t)(m + d) * ng + (m + d)];
      area_s[d] = area_d;
    }
    if (m > 0) {
      for (int i = 0; i < m; ++i) {
        if (gt_dc[g0 + i] == 0) continue;   // uniform
        if (active && area_d > 0) {
          const int v = mat[(int64_t)i * ng + m + d];
          if (v > 0 && 1000ll * v >= (int64_t)t_dc * area_d) dc = true;
        }
      }
    }
    const unsigned long long word = __ballot(active && !dc);
    if (lane == 0) free_s[c >> 6] = word;
    care_det += __popcll(word);
    if (rep && valid) det_gt[g0 + m + d] = dc ? SC_DET_DONT_CARE : (active ? SC_DET_UNMATCHED : SC_DET_INACTIVE);
  }
  if (lane == 0 && care_det) atomicAdd(&care_s, care_det);
  if (rep) {   // the rows the two arrays do not apply to
    for (int i = tid; i < m; i += SC_THREADS) det_gt[g0 + i] = SC_NA;
    for (int d = tid; d < nd; d += SC_THREADS) gt_det[g0 + m + d] = SC_NA;
  }
  __syncthreads();
  // ---- matching: the care ground-truth rows in order ----
  int care_gt = 0, matched = 0, matched_text = 0;   // thread 0's are the image's
  for (int i = 0; i < m; ++i) {
    if (gt_dc[g0 + i] != 0) {   // uniform
      if (rep && tid == 0) gt_det[g0 + i] = SC_GT_DONT_CARE;
      continue;
    }
    ++care_gt;
    if (nd > 0) {
      const int area_i = mat[(int64_t)i * ng + i];
      const int32_t* __restrict__ row = mat + (int64_t)i * ng + m;
      if (area_i > 0) {
        for (int c = wave * 64; c < nd; c += SC_THREADS) {
          const int d = c + lane;
          bool ok = false;
          if (d < nd && ((free_s[c >> 6] >> lane) & 1ull)) {
            const int v = row[d];
            ok = v > 0 && 1000ll * v >= (int64_t)t_iou * ((int64_t)area_i + area_s[d] - v);
          }
          const unsigned long long hit = __ballot(ok);
          if (hit) {   // wave-uniform: this wave's lowest qualifying detection
            if (lane == 0) atomicMin(&best_s, c + __ffsll((long long)hit) - 1);
            break;
          }
        }
      }
      __syncthreads();
      if (tid == 0) {
        const int d = best_s;
        if (d != SC_NONE) {
          free_s[d >> 6] &= ~(1ull << (d & 63));
          ++matched;
          matched_text += text[g0 + i] == text[g0 + m + d] ? 1 : 0;
          best_s = SC_NONE;
        }
        if (rep) {
          gt_det[g0 + i] = d != SC_NONE ? d : SC_GT_UNMATCHED;
          if (d != SC_NONE) det_gt[g0 + m + d] = i;
        }
      }
      __syncthreads();   // the next row reads the free set and best_s as thread 0 left them
    } else if (rep && tid == 0) {
      gt_det[g0 + i] = SC_GT_UNMATCHED;
    }
  }
  if (tid == 0) {
    cnt[0] = care_gt;
    cnt[1] = care_s;
    cnt[2] = matched;
    cnt[3] = matched_text;
  }
}

}  // namespace

extern "C" int omp_spotting_match(const int32_t* inter, const int64_t* inter_start, const int32_t* group_start, const int32_t* n_gt,
                                  const int32_t* gt_dc, const int32_t* text, const int32_t* level, int n, int n_groups, int n_thr, int t_iou,
                                  int t_dc, int report, int32_t* counts, int32_t* det_gt, int32_t* gt_det, omp_stream_t s) {
  OMP_CHECK_ARG(inter_start && group_start && n_gt && counts, "omp_spotting_match: null pointer");
  OMP_CHECK_ARG(n >= 0 && n <= (1 << 24) && n_groups > 0 && n_groups <= (1 << 24), "omp_spotting_match: %d polygons, %d groups", n, n_groups);
  OMP_CHECK_ARG(n == 0 || (inter && gt_dc && text && level), "omp_spotting_match: null pointer (inter, gt_dc, text, level with %d polygons)", n);
  OMP_CHECK_ARG(n_thr >= 1 && n_thr <= SC_MAX_THR, "omp_spotting_match: %d thresholds (1 .. %d)", n_thr, SC_MAX_THR);
  OMP_CHECK_ARG(t_iou >= 1 && t_iou <= 1000 && t_dc >= 1 && t_dc <= 1000, "omp_spotting_match: t_iou %d, t_dc %d permille (1 .. 1000)", t_iou, t_dc);
  OMP_CHECK_ARG(report >= -1 && report < n_thr, "omp_spotting_match: report %d (-1 .. %d)", report, n_thr - 1);
  OMP_CHECK_ARG((!det_gt == !gt_det) && (report < 0 || n == 0 || det_gt), "omp_spotting_match: det_gt and gt_det come together, and report %d needs them", report);
  OMP_CHECK_ARG((int64_t)n_groups * n_thr <= 0x7fffffffll, "omp_spotting_match: %d groups x %d thresholds exceed a launch", n_groups, n_thr);
  const hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(score_match_kernel, dim3((unsigned)(n_groups * n_thr)), dim3(SC_THREADS), 0, st, inter, inter_start, group_start, n_gt, gt_dc, text,
                     level, n, n_groups, n_thr, t_iou, t_dc, report, counts, det_gt, gt_det);
  OMP_CHECK_LAUNCH("omp_spotting_match");
  return OMP_OK;
}
