"""Overlap suppression: drop the records of a call that read the same word.

Windows that overlap, the whole-page window next to a grid, or the autoregressive point decoder itself return a word more than
once.  Two records are the same word when their decoded polygons overlap on the coordinate-bin grid; a greedy pass in priority
order keeps the first of them.  The numpy functions here are the DEFINITION; csrc/overlap.hip equals them on every integer.

Polygons   int32 [N, 32]: 16 points (x0, y0, ..., x15, y15) in coordinate bins -- the polygon decoder's tokens as
           decode_seq(..., 'poly') reads them -- every coordinate clamped to [0, grid - 1], grid = args.num_bins (at most 4096).
Groups     group_start int32 [G + 1]: polygons group_start[g] .. group_start[g + 1] - 1 are image g's; only polygons of one group
           interact; at most GROUP_MAX = 8192 per group.
Coverage   the samples are the bin centres (i + 0.5, j + 0.5), 0 <= i, j < grid - 1.  In doubled integer coordinates vertices are
           even and samples odd, so no sample lies on a vertex's row: edge (x1, y1) -> (x2, y2) counts for sample (xs, ys) when
           (y1 < ys) != (y2 < ys) and, with the edge oriented so that q = y2 - y1 > 0, xs q < x1 q + (ys - y1) (x2 - x1) -- the
           crossing lies strictly to the right.  A sample is inside when an odd number of the 16 edges count (even-odd rule);
           self-intersecting and collinear polygons and repeated points need no special case.  All of it fits int32.
Quantities area[n] = samples inside polygon n; inter[a, b] = samples inside both.
Pair test  threshold t in permille (1 .. 1000; permille(suppress) from the float) and a measure:
           'iou'    b overlaps a when inter > 0 and 1000 inter >= t (area[a] + area[b] - inter)
           'iomin'  b overlaps a when inter > 0 and 1000 inter >= t min(area[a], area[b])
           with 64-bit products.  A polygon of area 0 overlaps nothing.
Suppression greedy inside each group along `order` int32 [N] (a permutation grouped like the polygons: order[group_start[g] + p] is
           the polygon at priority position p): a polygon is kept unless an earlier kept polygon overlaps it.  owner[n] = n when kept,
           else the first kept polygon, in priority order, that overlaps n.
"""
import numpy as np

GRID_MAX = 4096
GROUP_MAX = 8192
MEASURES = ('iou', 'iomin')


# ---------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------
def _check_grid(grid):
    grid = int(grid)
    if grid < 2 or grid > GRID_MAX:
        raise ValueError('grid must be 2 .. %d, got %d' % (GRID_MAX, grid))
    return grid


def _check_polys(polys, grid):
    p = np.asarray(polys)
    if p.ndim != 2 or p.shape[1] != 32:
        raise ValueError('polys must be [N, 32] (16 points x0, y0, ..., x15, y15), got shape %s' % (tuple(p.shape),))
    return np.clip(p.astype(np.int64), 0, grid - 1).astype(np.int32)


def _check_groups(group_start, n):
    gs = np.asarray(group_start, dtype=np.int64).reshape(-1)
    if gs.size < 1 or gs[0] != 0 or gs[-1] != n or (np.diff(gs) < 0).any():
        raise ValueError('group_start must rise from 0 to the number of polygons (%d), got %s' % (n, gs.tolist()[:8]))
    if gs.size > 1 and int(np.diff(gs).max()) > GROUP_MAX:
        raise ValueError('a group holds at most %d polygons, got %d' % (GROUP_MAX, int(np.diff(gs).max())))
    return gs.astype(np.int32)


def _check_order(order, gs):
    o = np.asarray(order, dtype=np.int64).reshape(-1)
    if o.size != int(gs[-1]):
        raise ValueError('order holds %d entries for %d polygons' % (o.size, int(gs[-1])))
    for g in range(gs.size - 1):
        if sorted(o[gs[g]:gs[g + 1]].tolist()) != list(range(int(gs[g]), int(gs[g + 1]))):
            raise ValueError('order must permute every group inside itself (group %d)' % g)
    return o.astype(np.int32)


def permille(suppress):
    """the float threshold of the public interface -> t"""
    s = float(suppress)
    if not (0.0 < s <= 1.0):
        raise ValueError('suppress must be a float in (0, 1], got %r' % (suppress,))
    return min(1000, max(1, int(round(1000 * s))))


def _check_t(t, measure):
    if measure not in MEASURES:
        raise ValueError("measure must be 'iou' or 'iomin', got %r" % (measure,))
    t = int(t)
    if t < 1 or t > 1000:
        raise ValueError('t is a permille threshold 1 .. 1000, got %d' % t)
    return t


def bbox_cpu(polys, grid):
    """-> int32 [N, 4]: x0, y0, x1, y1 of the clamped points"""
    p = _check_polys(polys, _check_grid(grid))
    x, y = p[:, 0::2], p[:, 1::2]
    return np.stack([x.min(1), y.min(1), x.max(1), y.max(1)], 1).astype(np.int32) if len(p) else np.zeros((0, 4), np.int32)


def _raster(poly, box):
    """the samples of one (clamped) polygon inside its box -> bool [y1 - y0, x1 - x0]; sample (i, j) sits at [j - y0, i - x0]"""
    x0, y0, x1, y1 = (int(v) for v in box)
    xs = (2 * np.arange(x0, x1, dtype=np.int32) + 1)[None, :]
    ys = (2 * np.arange(y0, y1, dtype=np.int32) + 1)[:, None]
    X, Y = 2 * poly[0::2].astype(np.int32), 2 * poly[1::2].astype(np.int32)
    inside = np.zeros((y1 - y0, x1 - x0), dtype=bool)
    for e in range(16):
        xa, ya, xb, yb = X[e], Y[e], X[(e + 1) % 16], Y[(e + 1) % 16]
        if ya > yb:
            xa, ya, xb, yb = xb, yb, xa, ya
        q = yb - ya
        if q == 0:
            continue
        cross = (ya < ys) != (yb < ys)
        inside ^= cross & (xs * q < xa * q + (ys - ya) * (xb - xa))
    return inside


def coverage_cpu(polys, grid):
    """-> area int32 [N]: the samples inside each polygon"""
    grid = _check_grid(grid)
    p = _check_polys(polys, grid)
    box = bbox_cpu(p, grid)
    return np.asarray([int(_raster(p[i], box[i]).sum()) for i in range(len(p))], dtype=np.int32)


def _group_inter(p, box, lo, hi):
    """dense inter matrix of polygons lo .. hi - 1 (int32 [n, n]); pairs whose boxes share no sample are 0 by definition"""
    n = hi - lo
    rast = [_raster(p[i], box[i]) for i in range(lo, hi)]
    inter = np.zeros((n, n), dtype=np.int32)
    b = box[lo:hi].astype(np.int64)
    x0 = np.maximum(b[:, None, 0], b[None, :, 0])
    y0 = np.maximum(b[:, None, 1], b[None, :, 1])
    x1 = np.minimum(b[:, None, 2], b[None, :, 2])
    y1 = np.minimum(b[:, None, 3], b[None, :, 3])
    cand = np.argwhere((x0 < x1) & (y0 < y1))
    for i, j in cand.tolist():
        if j < i:
            continue
        if i == j:
            inter[i, i] = int(rast[i].sum())
            continue
        u0, v0, u1, v1 = int(x0[i, j]), int(y0[i, j]), int(x1[i, j]), int(y1[i, j])
        ra = rast[i][v0 - b[i, 1]:v1 - b[i, 1], u0 - b[i, 0]:u1 - b[i, 0]]
        rb = rast[j][v0 - b[j, 1]:v1 - b[j, 1], u0 - b[j, 0]:u1 - b[j, 0]]
        inter[i, j] = inter[j, i] = int((ra & rb).sum())
    return inter


def pair_overlap_cpu(polys, group_start, grid):
    """-> list of G dense matrices int32 [n_g, n_g] in polygon order: inter[a, b] = samples inside both; the diagonal is the area"""
    grid = _check_grid(grid)
    p = _check_polys(polys, grid)
    gs = _check_groups(group_start, len(p))
    box = bbox_cpu(p, grid)
    return [_group_inter(p, box, int(gs[g]), int(gs[g + 1])) for g in range(gs.size - 1)]


def overlap_matrix(inter, t, measure):
    """the pair test on one group's inter matrix -> bool [n, n] (the diagonal False)"""
    t = _check_t(t, measure)
    inter = inter.astype(np.int64)
    area = np.diag(inter)
    if measure == 'iou':
        denom = area[:, None] + area[None, :] - inter
    else:
        denom = np.minimum(area[:, None], area[None, :])
    ov = (inter > 0) & (1000 * inter >= t * denom)
    np.fill_diagonal(ov, False)
    return ov


def suppress_from_inter(inter, group_start, order, t, measure):
    """the greedy pass on the groups' dense inter matrices (pair_overlap_cpu) -> (owner int32 [N], area int32 [N])"""
    gs = np.asarray(group_start, dtype=np.int64)
    N = int(gs[-1])
    order = _check_order(order, gs)
    _check_t(t, measure)
    owner = np.arange(N, dtype=np.int32)
    area = np.zeros(N, dtype=np.int32)
    for g in range(gs.size - 1):
        lo, hi = int(gs[g]), int(gs[g + 1])
        area[lo:hi] = np.diag(inter[g])
        ov = overlap_matrix(inter[g], t, measure)
        decided = np.zeros(hi - lo, dtype=bool)
        for a in (order[lo:hi] - lo).tolist():
            if decided[a]:
                continue                        # suppressed by an earlier kept polygon
            decided[a] = True                   # kept
            hit = ov[a] & ~decided
            owner[lo:hi][hit] = lo + a
            decided |= hit
    return owner, area


def suppress_cpu(polys, group_start, order, t, measure, grid):
    """-> (owner int32 [N], area int32 [N])"""
    grid = _check_grid(grid)
    p = _check_polys(polys, grid)
    gs = _check_groups(group_start, len(p))
    _check_order(order, gs)
    _check_t(t, measure)
    return suppress_from_inter(pair_overlap_cpu(p, gs, grid), gs, order, t, measure)


def score_order(scores, group_start):
    """suppress_order='score': inside every group by descending score, ties to the lower index -> order int32 [N]"""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    gs = _check_groups(group_start, s.size)
    out = np.arange(s.size, dtype=np.int32)
    for g in range(gs.size - 1):
        lo, hi = int(gs[g]), int(gs[g + 1])
        out[lo:hi] = lo + np.argsort(-s[lo:hi], kind='stable')
    return out


def mask_layout(group_start):
    """-> (mask_start int64 [G + 1], inter_start int64 [G + 1]): group g's bitmask is n_g rows of ceil(n_g / 64) uint64 words from
    word mask_start[g]; its dense inter matrix is n_g^2 int32 from inter_start[g]"""
    n = np.diff(np.asarray(group_start, dtype=np.int64))
    ms = np.zeros(n.size + 1, dtype=np.int64)
    ist = np.zeros(n.size + 1, dtype=np.int64)
    ms[1:] = np.cumsum(n * ((n + 63) // 64))
    ist[1:] = np.cumsum(n * n)
    return ms, ist


def split_inter(flat, group_start):
    """the flat dense inter buffer of omp_polygon_overlap -> list of G matrices [n_g, n_g] (an empty group gives [0, 0])"""
    gs = np.asarray(group_start, dtype=np.int64)
    _, ist = mask_layout(gs)
    return [flat[int(ist[g]):int(ist[g + 1])].reshape(int(gs[g + 1] - gs[g]), int(gs[g + 1] - gs[g])) for g in range(gs.size - 1)]


def mask_cpu(polys, group_start, order, t, measure, grid, inter=None):
    """the bitmask omp_polygon_overlap writes, from the specification -> uint64 [mask words]: row p, bit q set when q > p and the
    polygons at priority positions p and q overlap.  inter: pair_overlap_cpu's matrices if the caller has them."""
    grid = _check_grid(grid)
    p = _check_polys(polys, grid)
    gs = _check_groups(group_start, len(p))
    order = _check_order(order, gs)
    ms, _ = mask_layout(gs)
    out = np.zeros(int(ms[-1]), dtype=np.uint64)
    for g, inter_g in enumerate(pair_overlap_cpu(p, gs, grid) if inter is None else inter):
        lo, hi = int(gs[g]), int(gs[g + 1])
        n, W = hi - lo, (hi - lo + 63) // 64
        if n == 0:
            continue
        o = order[lo:hi] - lo
        ov = np.triu(overlap_matrix(inter_g, t, measure)[np.ix_(o, o)], 1)
        bits = np.zeros((n, W * 64), dtype=np.uint64)
        bits[:, :n] = ov
        words = (bits.reshape(n, W, 64) << np.arange(64, dtype=np.uint64)[None, None, :]).sum(2, dtype=np.uint64)
        out[int(ms[g]):int(ms[g + 1])] = words.reshape(-1)
    return out


# ---------------------------------------------------------------------------------------------
# the device stage
# ---------------------------------------------------------------------------------------------
class OverlapSuppressor(object):
    """suppress_cpu on the device.  A call packs group_start, order and the mask layout into ONE upload, sizes the caller-owned
    bitmask, runs omp_polygon_overlap and omp_polygon_keep on the current stream and downloads owner, area and kept in ONE copy.
    There is no CPU fallback: suppress_cpu is the host specification."""

    def __init__(self, device, grid):
        import torch
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('OverlapSuppressor runs on MI355X only (got device %s); there is no CPU fallback -- '
                               'suppress_cpu is the host specification' % (self.device,))
        self.grid = _check_grid(grid)

    def run(self, polys, group_start, order=None, t=500, measure='iou', want_inter=False):
        """polys: int32 / int64 [N, 32] on the device or the host.  -> dict(owner, area, kept, bbox as numpy; mask (device uint64 words as
        int64), inter (list of numpy [n_g, n_g]) when want_inter)"""
        import torch

        from .. import ops
        t = _check_t(t, measure)
        polys = torch.as_tensor(polys)
        if polys.dim() != 2 or polys.shape[1] != 32:
            raise ValueError('polys must be [N, 32], got %s' % (tuple(polys.shape),))
        N = int(polys.shape[0])
        gs = _check_groups(group_start, N)
        G = gs.size - 1
        order = np.arange(N, dtype=np.int32) if order is None else _check_order(order, gs)
        if N == 0 or G == 0:
            return dict(owner=np.zeros(0, np.int32), area=np.zeros(0, np.int32), kept=np.zeros(G, np.int32), bbox=np.zeros((0, 4), np.int32),
                        mask=None, inter=[np.zeros((0, 0), np.int32)] * G if want_inter else None)
        ms, ist = mask_layout(gs)
        with torch.cuda.device(self.device):
            # the tables' one upload: int64 starts first (8-byte aligned), then the int32 tables
            blob = torch.from_numpy(np.concatenate([ms.view(np.uint8), ist.view(np.uint8), gs.view(np.uint8), order.view(np.uint8)])).to(self.device)
            starts = blob[:16 * (G + 1)].view(torch.int64)
            ints = blob[16 * (G + 1):].view(torch.int32)
            d_polys = polys.to(self.device).clamp(-1, GRID_MAX).to(torch.int32).contiguous()   # int64 tokens fit int32 once out-of-range ones are cut
            res = ops.polygon_overlap(d_polys, ints[:G + 1], ints[G + 1:], starts[:G + 1], int(ms[-1]), self.grid, t, MEASURES.index(measure),
                                      inter_start=starts[G + 1:] if want_inter else None, inter_total=int(ist[-1]))
            out_i = ops.polygon_keep(res['mask'], starts[:G + 1], ints[:G + 1], ints[G + 1:], N, out=res['ints'])
            host = out_i.cpu().numpy()                                                      # the one download
        out = dict(bbox=host[:4 * N].reshape(N, 4).copy(), area=host[4 * N:5 * N].copy(), owner=host[5 * N:6 * N].copy(), kept=host[6 * N:6 * N + G].copy(),
                   mask=res['mask'], inter=None)
        if want_inter:
            flat = res['inter'].cpu().numpy()
            out['inter'] = split_inter(flat, gs)
        if (out['kept'] < 0).any():
            raise RuntimeError('omp_polygon_keep refused a group (more than %d polygons, or tables that do not fit the mask)' % GROUP_MAX)
        return out

    def __call__(self, polys, group_start, order=None, t=500, measure='iou'):
        """-> (owner int32 [N], area int32 [N]) as suppress_cpu"""
        r = self.run(polys, group_start, order, t, measure)
        return r['owner'], r['area']


# ---------------------------------------------------------------------------------------------
# the engine's side: `suppress=` of predict / predict_images / spot_and_recognize
# ---------------------------------------------------------------------------------------------
def check_suppress_args(suppress, measure, order, infer_vie=False):
    """the refusals of the public interface -> t"""
    if infer_vie:
        raise ValueError('suppress= needs text-spotting records; with args.infer_vie the engine returns entity tuples')
    if measure not in MEASURES:
        raise ValueError("suppress_measure must be 'iou' or 'iomin', got %r" % (measure,))
    if order not in ('first', 'score'):
        raise ValueError("suppress_order must be 'first' or 'score', got %r" % (order,))
    return permille(suppress)


def suppress_records(records, raw_polys, grid, suppress, measure='iou', order='first', suppressor=None, device=None, kept_rows=None):
    """records: per image the list of record dicts, in the engine's order.  raw_polys: per image the polygon decoder's ids for those
    records ([n_b, 32] tensors, None or empty for an image without records), on the device.  One device call for all images
    (`suppressor`: an OverlapSuppressor, or anything with its __call__; default: one on `device`).  -> the filtered lists: suppressed
    records are removed, every survivor gains `merged`, the (window, index) of the records it absorbed -- plain indices without
    windows; index counts the image's records before suppression.  kept_rows: a list that receives, per image, the rows of raw_polys
    (indices before suppression) of the survivors, in the order of the returned records."""
    import torch
    t = check_suppress_args(suppress, measure, order)
    counts = [len(r) for r in records]
    gs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    N = int(gs[-1])
    if N == 0:
        if kept_rows is not None:
            kept_rows.extend([] for _ in records)
        return [list(r) for r in records]
    parts = []
    for b, (n, rp) in enumerate(zip(counts, raw_polys)):
        if n == 0:
            continue
        rp = torch.as_tensor(rp).reshape(-1, 32)
        if rp.shape[0] != n:
            raise ValueError('image %d: %d polygons for %d records' % (b, rp.shape[0], n))
        parts.append(rp)
    polys = torch.cat(parts, 0)
    prio = None
    if order == 'score':
        prio = score_order([r['score'] for recs in records for r in recs], gs)
    if suppressor is None:
        suppressor = OverlapSuppressor(polys.device if device is None else device, grid)
    owner, _ = suppressor(polys, gs, prio, t, measure)
    out = []
    for b, recs in enumerate(records):
        lo = int(gs[b])
        kept, rows = [], []
        for i, r in enumerate(recs):
            if int(owner[lo + i]) == lo + i:
                r['merged'] = []
                kept.append(r)
                rows.append(i)
        if kept_rows is not None:
            kept_rows.append(rows)
        for i, r in enumerate(recs):
            o = int(owner[lo + i]) - lo
            if o != i:
                recs[o]['merged'].append((r['window'], i) if 'window' in r else i)
        out.append(kept)
    return out
