"""Scoring: spotting results against ground truth under the IoU protocol.

Detections and ground-truth words are 16-point polygons on one grid of `bins` bins a side; their areas and intersections are the
exact integers of utils/overlap.py (pair_overlap_cpu / omp_polygon_overlap).  On top of those this module matches every
ground-truth word to at most one detection, applies the don't-care rules and counts, for a whole sweep of score thresholds at once.
The numpy functions here are the DEFINITION; csrc/score.hip (omp_spotting_match) equals match_pages_cpu on every integer.

Quantising  quantise(): a coordinate x in pixels of an image w wide becomes clip(floor(x * bins / w), 0, bins - 1), in float64 on the
            host; predictions (their `polys`, original pixels) and ground truth go through the same function.
Groups      one group per image, ordered ground truth first: polygons group_start[g] .. group_start[g] + n_gt[g] - 1 are image g's
            ground-truth words, the rest of the group its detections.  gt_dc, text and level are indexed like the polygons; gt_dc
            matters for ground truth only, level for detections only.
Thresholds  levels(): level[d] = the number of thresholds <= score[d]; detection d is ACTIVE at threshold index k iff level[d] > k.
Texts       text_ids(): equal normalised strings get equal ids; the matcher compares one integer per pair.
Matching    with m = n_gt, area[p] = inter[p, p], t_iou and t_dc in permille (1 .. 1000), 64-bit products, per threshold index k:
            a detection d is DON'T-CARE when it is active and some ground-truth word i has gt_dc[i], inter[i, d] > 0 and
            1000 inter[i, d] >= t_dc area[d];
            the ground-truth words i = 0 .. m - 1 that are not don't-care are visited in order, and each takes the lowest-index
            detection d that is active, not don't-care, not yet taken, and has inter[i, d] > 0 and
            1000 inter[i, d] >= t_iou (area[i] + area[d] - inter[i, d])   (the >= of overlap_matrix);
            counts[k] = (care ground truth, care detections, matched, matched with text[i] == text[d]); a care detection is
            active and not don't-care.  A detection of area 0 never matches and is never don't-care: it counts as a care detection.
Report      for ONE threshold index (`report`; -1 = none) the assignment itself: det_gt[d] = the matched i, DET_UNMATCHED (-1),
            DET_DONT_CARE (-2) or DET_INACTIVE (-3); gt_det[i] = the matched detection's index among the image's detections,
            GT_UNMATCHED (-1) or GT_DONT_CARE (-2).  In the flat [n] arrays of match_pages_cpu / omp_spotting_match det_gt sits
            at the detections' rows and gt_det at the ground truth's; the rows an array does not apply to hold NOT_APPLICABLE (-4),
            and both arrays are all NOT_APPLICABLE without a report.

This is the ICDAR 2015 / Total-Text IoU protocol as far as it is public knowledge: ground truth outer, detections inner, don't-care
detections by their precision against don't-care ground truth, the text checked after the geometric match.  The official script
tests IoU > 0.5 strictly; this definition tests >= at permille resolution.  Agreement with the official script has NOT been checked.
"""
import numpy as np

from . import overlap as OV

T_MAX = 64                      # thresholds per call
GROUP_MAX = OV.GROUP_MAX        # ground truth + detections of one image
ENTRY_CAP = 1 << 26             # dense inter entries per device chunk (256 MiB of int32)
DET_UNMATCHED, DET_DONT_CARE, DET_INACTIVE = -1, -2, -3
GT_UNMATCHED, GT_DONT_CARE = -1, -2
NOT_APPLICABLE = -4


# ---------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------
def quantise(polys_px, size_hw, bins):
    """polygons of 3 .. 16 (x, y) vertices in the pixels of an image of size (h, w) -> int32 [n, 32] on a grid of `bins` bins;
    fewer than 16 vertices are padded by repeating the last one"""
    bins = int(bins)
    if bins < 2 or bins > OV.GRID_MAX:
        raise ValueError('bins must be 2 .. %d, got %d' % (OV.GRID_MAX, bins))
    h, w = float(size_hw[0]), float(size_hw[1])
    if not (h > 0 and w > 0):
        raise ValueError('size_hw must be a positive (h, w), got %r' % (size_hw,))
    out = np.zeros((len(polys_px), 32), dtype=np.int32)
    for n, poly in enumerate(polys_px):
        p = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
        if p.shape[0] < 3 or p.shape[0] > 16:
            raise ValueError('a polygon has 3 .. 16 vertices, polygon %d has %d' % (n, p.shape[0]))
        if not np.isfinite(p).all():
            raise ValueError('polygon %d holds a coordinate that is not finite' % n)
        p = np.concatenate([p, np.repeat(p[-1:], 16 - p.shape[0], 0)], 0)
        out[n, 0::2] = np.clip(np.floor(p[:, 0] * bins / w), 0, bins - 1)
        out[n, 1::2] = np.clip(np.floor(p[:, 1] * bins / h), 0, bins - 1)
    return out


def bezier_polygon(bezier16):
    """the reference's annotation geometry (dataset/text_spotting.py:55-72, utils/misc.py:74-79): 16 floats = the control points of two
    cubic Beziers, upper curve then lower, each sampled at 8 equally spaced parameters -> float64 [16, 2]"""
    c = np.asarray(bezier16, dtype=np.float64).reshape(-1)
    if c.size != 16:
        raise ValueError('bezier_pts holds 16 floats (2 curves x 4 control points), got %d' % c.size)
    c = c.reshape(2, 4, 2)
    t = np.linspace(0.0, 1.0, 8)[:, None]
    basis = np.concatenate([(1 - t) ** 3, 3 * t * (1 - t) ** 2, 3 * t ** 2 * (1 - t), t ** 3], 1)       # Bernstein, [8, 4]
    return np.concatenate([basis @ c[0], basis @ c[1]], 0)


def check_thresholds(thresholds):
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if th.size < 1 or th.size > T_MAX or not np.isfinite(th).all() or (np.diff(th) <= 0).any():
        raise ValueError('thresholds must be 1 .. %d finite floats in strictly ascending order, got %s' % (T_MAX, th.tolist()[:8]))
    return th


def levels(scores, thresholds):
    """-> int32 [n]: the number of thresholds at or below each score"""
    th = check_thresholds(thresholds)
    return np.searchsorted(th, np.asarray(scores, dtype=np.float64).reshape(-1), side='right').astype(np.int32)


def text_ids(gt_texts, det_texts, normalise=str.casefold):
    """-> (int32 [len(gt_texts)], int32 [len(det_texts)]): equal normalised strings get equal ids"""
    table = {}

    def ids(texts):
        return np.asarray([table.setdefault(normalise(str(t)) if normalise is not None else str(t), len(table)) for t in texts], dtype=np.int32)
    return ids(gt_texts), ids(det_texts)


def permille(x, what):
    """the float overlap bound of the public interface -> permille"""
    x = float(x)
    if not (0.0 < x <= 1.0):
        raise ValueError('%s must be a float in (0, 1], got %r' % (what, x))
    return min(1000, max(1, int(round(1000 * x))))


def _check_match_args(n_thr, t_iou, t_dc, report):
    n_thr, t_iou, t_dc, report = int(n_thr), int(t_iou), int(t_dc), int(report)
    if n_thr < 1 or n_thr > T_MAX:
        raise ValueError('n_thr must be 1 .. %d, got %d' % (T_MAX, n_thr))
    if not (1 <= t_iou <= 1000 and 1 <= t_dc <= 1000):
        raise ValueError('t_iou and t_dc are permille thresholds 1 .. 1000, got %d and %d' % (t_iou, t_dc))
    if report < -1 or report >= n_thr:
        raise ValueError('report must be -1 or a threshold index below %d, got %d' % (n_thr, report))
    return n_thr, t_iou, t_dc, report


def match_cpu(inter, n_gt, gt_dc, text, level, n_thr, t_iou=500, t_dc=500, report=-1):
    """one image.  inter: int32 [n, n] as pair_overlap_cpu gives it, ground truth first; gt_dc, text, level: [n].
    -> (counts int32 [n_thr, 4], det_gt int32 [n - n_gt], gt_det int32 [n_gt]); the two assignments are those of threshold `report`
    and hold NOT_APPLICABLE everywhere when report is -1"""
    n_thr, t_iou, t_dc, report = _check_match_args(n_thr, t_iou, t_dc, report)
    inter = np.asarray(inter).astype(np.int64)
    n, m = inter.shape[0], int(n_gt)
    if inter.shape != (n, n) or m < 0 or m > n:
        raise ValueError('inter must be [n, n] with 0 <= n_gt <= n, got %s and n_gt %d' % (inter.shape, m))
    nd = n - m
    dc_gt = np.asarray(gt_dc).reshape(-1)[:m].astype(bool)
    text = np.asarray(text).reshape(-1)
    level = np.asarray(level).reshape(-1)[m:]
    area = np.diag(inter)
    cross = inter[:m, m:]                                                        # [m, nd]
    # neither test depends on the threshold index
    passes = (cross > 0) & (1000 * cross >= t_iou * (area[:m, None] + area[None, m:] - cross))
    covered = ((cross > 0) & (1000 * cross >= t_dc * area[None, m:]) & dc_gt[:, None]).any(0) if m else np.zeros(nd, bool)
    same = text[:m, None] == text[None, m:]
    counts = np.zeros((n_thr, 4), dtype=np.int32)
    det_gt = np.full(nd, NOT_APPLICABLE, dtype=np.int32)
    gt_det = np.full(m, NOT_APPLICABLE, dtype=np.int32)
    care_gt = np.flatnonzero(~dc_gt)
    for k in range(n_thr):
        active = level > k
        dont_care = active & covered
        free = active & ~dont_care
        counts[k, 0], counts[k, 1] = care_gt.size, int(free.sum())
        if k == report:
            det_gt[:] = np.where(dont_care, DET_DONT_CARE, np.where(active, DET_UNMATCHED, DET_INACTIVE))
            gt_det[:] = np.where(dc_gt, GT_DONT_CARE, GT_UNMATCHED)
        for i in care_gt.tolist():
            cand = passes[i] & free
            if not cand.any():
                continue
            d = int(np.argmax(cand))
            free[d] = False
            counts[k, 2] += 1
            counts[k, 3] += int(same[i, d])
            if k == report:
                det_gt[d], gt_det[i] = i, d
    return counts, det_gt, gt_det


def inter_layout(group_start):
    """-> inter_start int64 [G + 1]: group g's dense matrix is n_g^2 int32 from inter_start[g] (utils.overlap.mask_layout's)"""
    return OV.mask_layout(group_start)[1]


def _check_tables(group_start, n_gt, gt_dc, text, level):
    level = np.asarray(level, dtype=np.int32).reshape(-1)
    n = level.size
    gs = OV._check_groups(group_start, n)
    G = gs.size - 1
    n_gt = np.asarray(n_gt, dtype=np.int64).reshape(-1)
    if n_gt.size != G or (n_gt < 0).any() or (n_gt > np.diff(gs.astype(np.int64))).any():
        raise ValueError('n_gt holds one count per group, each between 0 and the size of its group')
    gt_dc = np.asarray(gt_dc).reshape(-1).astype(np.int32)
    text = np.asarray(text, dtype=np.int32).reshape(-1)
    if gt_dc.size != n or text.size != n:
        raise ValueError('gt_dc, text and level are indexed like the polygons (%d), got %d, %d' % (n, gt_dc.size, text.size))
    return gs, n_gt.astype(np.int32), gt_dc, text, level


def match_pages_cpu(inter, inter_start, group_start, n_gt, gt_dc, text, level, n_thr, t_iou=500, t_dc=500, report=-1):
    """match_cpu over all images of a call, for the flat inputs omp_spotting_match takes: inter int32 [inter_start[G]] (group g's
    matrix from inter_start[g]), group_start int32 [G + 1], n_gt int32 [G], gt_dc / text / level int32 [n].
    -> (counts int32 [G, n_thr, 4], det_gt int32 [n], gt_det int32 [n])"""
    gs, n_gt, gt_dc, text, level = _check_tables(group_start, n_gt, gt_dc, text, level)
    n_thr, t_iou, t_dc, report = _check_match_args(n_thr, t_iou, t_dc, report)
    G, n = gs.size - 1, int(gs[-1])
    ist = np.asarray(inter_start, dtype=np.int64).reshape(-1)
    inter = np.asarray(inter).reshape(-1)
    counts = np.zeros((G, n_thr, 4), dtype=np.int32)
    det_gt = np.full(n, NOT_APPLICABLE, dtype=np.int32)
    gt_det = np.full(n, NOT_APPLICABLE, dtype=np.int32)
    for g in range(G):
        lo, hi, m = int(gs[g]), int(gs[g + 1]), int(n_gt[g])
        mat = inter[int(ist[g]):int(ist[g]) + (hi - lo) ** 2].reshape(hi - lo, hi - lo)
        counts[g], det_gt[lo + m:hi], gt_det[lo:lo + m] = match_cpu(mat, m, gt_dc[lo:hi], text[lo:hi], level[lo:hi], n_thr, t_iou, t_dc, report)
    return counts, det_gt, gt_det


def _prf(tp, n_det, n_gt):
    p = tp / n_det if n_det else 0.0
    r = tp / n_gt if n_gt else 0.0
    return p, r, (2 * p * r / (p + r) if p + r else 0.0)


def metrics(counts):
    """counts [T, 4] summed over the images -> dict(det, e2e: dict(precision, recall, hmean: lists of T Python floats, best: the index of
    the highest hmean, ties to the lowest index)); 0 / 0 is 0.0"""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    out = {}
    for name, col in (('det', 2), ('e2e', 3)):
        rows = [_prf(int(r[col]), int(r[1]), int(r[0])) for r in c]
        h = [r[2] for r in rows]
        out[name] = dict(precision=[r[0] for r in rows], recall=[r[1] for r in rows], hmean=h, best=h.index(max(h)) if h else 0)
    return out


def chunk_groups(group_start, cap=ENTRY_CAP):
    """-> [(g_lo, g_hi)]: consecutive images whose dense inter matrices hold at most `cap` entries together"""
    sizes = np.diff(np.asarray(group_start, dtype=np.int64))
    out, lo, acc = [], 0, 0
    for g, s in enumerate(sizes.tolist()):
        if s * s > cap:
            raise ValueError('image %d holds %d words: its %d x %d intersection matrix exceeds the %d entries of a device chunk' % (g, s, s, s, cap))
        if acc + s * s > cap:
            out.append((lo, g))
            lo, acc = g, 0
        acc += s * s
    if lo < sizes.size:
        out.append((lo, sizes.size))
    return out


class HostScorer(object):
    """SpottingScorer's `run` from the specification (pair_overlap_cpu + match_pages_cpu): what the device stage must equal"""

    def __init__(self, bins):
        self.bins = OV._check_grid(bins)

    def run(self, polys, group_start, n_gt, gt_dc, text, level, n_thr, t_iou=500, t_dc=500, report=-1):
        polys = np.asarray(polys).reshape(-1, 32)
        gs = OV._check_groups(group_start, len(polys))
        mats = OV.pair_overlap_cpu(polys, gs, self.bins)
        flat = np.concatenate([m.reshape(-1) for m in mats] + [np.zeros(0, np.int32)])
        counts, det_gt, gt_det = match_pages_cpu(flat, inter_layout(gs), gs, n_gt, gt_dc, text, level, n_thr, t_iou, t_dc, report)
        return dict(counts=counts, det_gt=det_gt, gt_det=gt_det)


# ---------------------------------------------------------------------------------------------
# the device stage
# ---------------------------------------------------------------------------------------------
class SpottingScorer(object):
    """match_pages_cpu on the device, intersections included.  The images of a call are cut into chunks whose dense intersection
    matrices hold at most `entry_cap` int32 together; a chunk is ONE packed upload of the tables, omp_polygon_overlap with `inter`,
    omp_spotting_match, and ONE download of counts and assignments.  There is no CPU fallback: HostScorer is the specification."""

    def __init__(self, device, bins, entry_cap=ENTRY_CAP):
        import torch
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('SpottingScorer runs on MI355X only (got device %s); there is no CPU fallback -- '
                               'HostScorer is the host specification' % (self.device,))
        self.bins = OV._check_grid(bins)
        self.entry_cap = int(entry_cap)
        if self.entry_cap < 1 or self.entry_cap > ENTRY_CAP:
            raise ValueError('entry_cap must be 1 .. %d, got %d' % (ENTRY_CAP, self.entry_cap))
        self.chunks = 0             # chunks of the last run

    def run(self, polys, group_start, n_gt, gt_dc, text, level, n_thr, t_iou=500, t_dc=500, report=-1):
        """polys: int32 [n, 32] (host or device), ground truth first inside every group; the tables as match_pages_cpu takes them.
        -> dict(counts int32 [G, n_thr, 4], det_gt int32 [n], gt_det int32 [n]) as numpy"""
        import torch

        from .. import ops
        polys = torch.as_tensor(polys)
        if polys.dim() != 2 or polys.shape[1] != 32:
            raise ValueError('polys must be [n, 32], got %s' % (tuple(polys.shape),))
        n = int(polys.shape[0])
        if np.asarray(level).size != n:
            raise ValueError('level holds %d entries for %d polygons' % (np.asarray(level).size, n))
        gs, n_gt, gt_dc, text, level = _check_tables(group_start, n_gt, gt_dc, text, level)
        n_thr, t_iou, t_dc, report = _check_match_args(n_thr, t_iou, t_dc, report)
        G = gs.size - 1
        counts = np.zeros((G, n_thr, 4), dtype=np.int32)
        det_gt = np.full(n, NOT_APPLICABLE, dtype=np.int32)
        gt_det = np.full(n, NOT_APPLICABLE, dtype=np.int32)
        chunks = chunk_groups(gs, self.entry_cap)
        self.chunks = len(chunks)
        with torch.cuda.device(self.device):
            d_polys = polys.to(self.device).clamp(-1, OV.GRID_MAX).to(torch.int32).contiguous() if n else None
            for g_lo, g_hi in chunks:
                lo, hi = int(gs[g_lo]), int(gs[g_hi])
                g, c = g_hi - g_lo, hi - lo
                cgs = (gs[g_lo:g_hi + 1] - lo).astype(np.int32)
                ms, ist = OV.mask_layout(cgs)
                # the tables' one upload: int64 starts first (8-byte aligned), then the int32 tables
                parts = [ms, ist, cgs, n_gt[g_lo:g_hi], np.arange(c, dtype=np.int32), gt_dc[lo:hi], text[lo:hi], level[lo:hi]]
                blob = torch.from_numpy(np.concatenate([np.ascontiguousarray(p).view(np.uint8) for p in parts])).to(self.device)
                starts = blob[:16 * (g + 1)].view(torch.int64)
                ints = blob[16 * (g + 1):].view(torch.int32)
                d_gs, d_ngt, ints = ints[:g + 1], ints[g + 1:2 * g + 1], ints[2 * g + 1:]
                d_order, d_dc, d_text, d_level = ints[:c], ints[c:2 * c], ints[2 * c:3 * c], ints[3 * c:]
                inter = None
                if c:
                    inter = ops.polygon_overlap(d_polys[lo:hi], d_gs, d_order, starts[:g + 1], max(int(ms[-1]), 1), self.bins, t_iou, 0,
                                                inter_start=starts[g + 1:], inter_total=int(ist[-1]))['inter']
                out = ops.spotting_match(inter, starts[g + 1:], d_gs, d_ngt, d_dc, d_text, d_level, n_thr, t_iou, t_dc, report)
                host = out.cpu().numpy()                                                     # the one download
                cc, dg, gd = ops.split_match_ints(host, c, g, n_thr)
                if (cc < 0).any():
                    raise RuntimeError('omp_spotting_match refused an image (more than %d words, or tables that do not fit each other)' % GROUP_MAX)
                counts[g_lo:g_hi], det_gt[lo:hi], gt_det[lo:hi] = cc, dg, gd
        return dict(counts=counts, det_gt=det_gt, gt_det=gt_det)
