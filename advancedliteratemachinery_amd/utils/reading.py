"""Reading order: group a call's words into text lines and order them as a reader would.

The engine returns an image's words in decoder order (window order first with windows= / grid=).  This stage links every word to the
word that follows it on its line, resolves the links into lines and orders the lines top to bottom.  The numpy functions here are the
DEFINITION; csrc/reading.hip equals them on every integer.  Integers only, no square root, no division.

Polygons   int32 [N, 32]: 16 points (x0, y0, ..., x15, y15) in coordinate bins, clamped to [0, grid - 1], grid at most GRID_MAX = 4096.
Groups     group_start int32 [G + 1]; only words of one group (image) interact; at most GROUP_MAX = 8192 per group.
Aspect     int32 [G, 2] = (ax, ay), each 1 .. ASPECT_MAX = 256.  Bins are anisotropic (x is a fraction of the width, y of the height), so
           all geometry is done on the scaled points (x ax, y ay); aspect_of(h, w) = (max(1, rint(256 w / m)), max(1, rint(256 h / m))),
           m = max(w, h), from the image's orig_size.
Parameters gap, back, offset in permille, each 0 .. PARAM_MAX = 10000 (permille(2.0) = 2000 from the public floats).
Features   per word, int64, on the scaled points P[0..15]; T[k] = P[k], B[k] = P[15 - k], k = 0 .. 7 (top left to right, bottom under it):
             L = T[0] + B[0], R = T[7] + B[7]   the doubled midpoints of the word's two ends
             d = R - L, and (1, 0) when that is (0, 0)
             H = sum_k |(T[k] - B[k]) x d|      8 * mean perpendicular height * |d|   (u x w = u.x w.y - u.y w.x)
             C = sum of the 16 points
Link a -> b ("b follows a on a's line"), a != b in one group, with v = L_b - R_a, along = v . d_a, pa = v x d_a, pb = v x d_b:
             d_a . d_b > 0,  4000 along <= gap H_a,  4000 along >= -back H_a,  4000 |pa| <= offset H_a,  4000 |pb| <= offset H_b
           (along = 2 * gap length * |d| and H = 8 * height * |d|, hence 4000 for permille of the height; the perpendicular test runs in
           both words' frames so that a footnote-sized word does not join a headline).  cost(a, b) = |v|^2.
Bounds     a scaled coordinate is at most 4095 * 256 < 2^20; L, R < 2^21; the components of d and v are below 2^21 in magnitude, those
           of T - B below 2^20.  A dot or cross product of d / v vectors is below 2 * 2^42 = 2^43; H < 8 * 2 * 2^41 = 2^45;
           10000 H < 2^59 and 4000 * 2^43 < 2^55: every product stays below 2^63.  cost < 2^43 (the kernels pack it into 46 bits).
           C_y < 2^24; a line's sum of C_y < 2^37, times a count (at most 2^13) < 2^50.  features_cpu asserts these on its inputs.
Successor  succ0[a] = the passing b of least cost, ties to the lower b; -1 if none (links_cpu, before resolution).
Resolution a word claimed by several a keeps the one of least (cost, a) as pred; the losers get succ = -1 -- no second choice.  Every
           word now has at most one successor and one predecessor: components are paths or simple cycles (text around a circle).
Cycles     a cycle is cut in front of its lowest-index member: that member's pred and its former predecessor's succ become -1.
Lines      a line is a path; line_pos = distance from the head.  Lines of a group are ordered by the mean of C_y over their members
           (compared exactly: sum_1 count_2 against sum_2 count_1), then L_x of the head, then the head's index; numbered from 0.
           rank = the word's position in its group with the lines concatenated in that order.
Blocks     blocks_cpu, behind `blocks=True`: a recursive XY-cut over the LINES, level-synchronous.  Per word, on the
           scaled points: the bounding box x0, x1, y0, y1 (min / max over the 16 points), s = sum_k (B[k] - T[k]) (8 * the mean height
           vector), t = max(|s_x|, |s_y|); the inflated intervals, in 1 / 16000 of a scaled bin (8 of s, 1000 of permille, 2 for half a
           gap on each side): X = [16000 x0 - gap_x t, 16000 x1 + gap_x t], Y the same with gap_y.  Two words are apart on an axis
           exactly when their raw gap exceeds gap / 1000 times the mean of their two heights.  |16000 x| < 2^34, t < 2^23,
           gap t < 2^37: every end stays below 2^38 in magnitude (asserted).  The atoms are the lines: an atom's interval is the min of
           the lower and the max of the upper ends of its words; a line is never cut.  All atoms of a group start in segment 0.  Level
           l = 0, 1, ... works on y when l is even (bands first) and on x when l is odd: inside every segment the atoms are walked in
           (lo, line number) order and an atom starts a new component when its lo is STRICTLY greater than the running maximum of hi
           over the atoms before it in its segment; components numbered in (old segment, position) order are the new segments, so
           segment numbers are always in reading order.  Stop after `depth` levels, or as soon as two consecutive levels created no
           new segment (neither axis cuts anything any more).  block = the final segment of the word's line; line = the position of
           (block, old line) in sorted order; rank = the position with the lines concatenated in the new order; n_blocks per group;
           levels = the levels actually run (0 for a group without words).
Not done   L-shaped regions are not cut (XY-cut only finds gaps that cross a whole segment).  A line that the linker joined across a
           gutter holds its two columns in one block: the remedy is a smaller line_gap.  Without blocks, lines are ordered by y only:
           two columns at the same height interleave line by line; a page of vertical lines is grouped correctly and ordered by the
           lines' mean y, then by the heads' x.  The defaults block_gap_x = 1.0 and block_gap_y = 1.5 are choices that no data set
           has tested; no accuracy is claimed.
"""
import functools

import numpy as np

from .overlap import GRID_MAX, GROUP_MAX, _check_grid, _check_groups, _check_polys

ASPECT_MAX = 256
PARAM_MAX = 10000
DEFAULTS = dict(gap=2000, back=500, offset=500)
DEPTH_MAX = 16
BLOCK_DEFAULTS = dict(gap_x=1000, gap_y=1500, depth=8)


# ---------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------
def aspect_of(h, w):
    """an image's (h, w) -> (ax, ay): 256 for the longer side, the shorter in proportion"""
    h, w = float(h), float(w)
    m = max(h, w)
    if not (h > 0 and w > 0):
        raise ValueError('an image size must be positive, got (%r, %r)' % (h, w))
    return max(1, int(np.rint(256.0 * w / m))), max(1, int(np.rint(256.0 * h / m)))


def permille(value, name='line_gap'):
    """a float of the public interface (in units of the word height) -> permille"""
    v = float(value)
    if not (0.0 <= v <= 10.0):
        raise ValueError('%s must be a float in [0, 10], got %r' % (name, value))
    return int(round(1000 * v))


def _check_aspect(aspect, n_groups):
    a = np.asarray(aspect, dtype=np.int64).reshape(-1, 2) if np.size(aspect) else np.zeros((0, 2), np.int64)
    if a.shape[0] != n_groups:
        raise ValueError('aspect must be [G, 2] for %d groups, got %s' % (n_groups, tuple(np.shape(aspect))))
    if a.size and (a.min() < 1 or a.max() > ASPECT_MAX):
        raise ValueError('aspect entries are 1 .. %d, got %d .. %d' % (ASPECT_MAX, int(a.min()), int(a.max())))
    return a.astype(np.int32)


def _check_params(gap, back, offset):
    out = []
    for name, v in (('gap', gap), ('back', back), ('offset', offset)):
        if int(v) != v or int(v) < 0 or int(v) > PARAM_MAX:
            raise ValueError('%s is a permille parameter 0 .. %d, got %r' % (name, PARAM_MAX, v))
        out.append(int(v))
    return tuple(out)


def features_cpu(polys, aspect_per_word):
    """polys int [N, 32] (clamped bins), aspect_per_word int [N, 2] -> dict(L, R, d, C: int64 [N, 2]; H: int64 [N])"""
    p = np.asarray(polys, dtype=np.int64).reshape(-1, 32)
    a = np.asarray(aspect_per_word, dtype=np.int64).reshape(-1, 2)
    assert p.shape[0] == a.shape[0], 'one aspect per word'
    assert p.size == 0 or (p.min() >= 0 and p.max() <= GRID_MAX - 1 and a.min() >= 1 and a.max() <= ASPECT_MAX), 'bins 0 .. 4095, aspects 1 .. 256'
    P = p.reshape(-1, 16, 2) * a[:, None, :]
    T, B = P[:, :8], P[:, :7:-1]                             # B[k] = P[15 - k]
    L, R = T[:, 0] + B[:, 0], T[:, 7] + B[:, 7]
    d = R - L
    d[(d == 0).all(1)] = (1, 0)
    u = T - B
    H = np.abs(u[:, :, 0] * d[:, None, 1] - u[:, :, 1] * d[:, None, 0]).sum(1)
    C = P.sum(1)
    assert p.size == 0 or (max(L.max(), R.max()) < 2 ** 21 and np.abs(d).max() < 2 ** 21 and np.abs(u).max() < 2 ** 20 and H.max() < 2 ** 45
                           and PARAM_MAX * int(H.max()) < 2 ** 59 and C.max() < 2 ** 24), 'the bounds of the docstring'
    return dict(L=L, R=R, d=d, H=H, C=C)


def _aspect_per_word(gs, aspect):
    return np.repeat(aspect.astype(np.int64), np.diff(gs.astype(np.int64)), axis=0).reshape(-1, 2)


def _link_block(f, lo, hi, r0, r1, gap, back, offset):
    """rows r0 .. r1 - 1 against the whole group lo .. hi - 1 -> (pass bool [r1 - r0, hi - lo], cost int64 of the same shape)"""
    Ra, da, Ha = f['R'][r0:r1], f['d'][r0:r1], f['H'][r0:r1]
    Lb, db, Hb = f['L'][lo:hi], f['d'][lo:hi], f['H'][lo:hi]
    vx = Lb[None, :, 0] - Ra[:, None, 0]
    vy = Lb[None, :, 1] - Ra[:, None, 1]
    along = vx * da[:, None, 0] + vy * da[:, None, 1]
    pa = vx * da[:, None, 1] - vy * da[:, None, 0]
    pb = vx * db[None, :, 1] - vy * db[None, :, 0]
    dot = da[:, None, 0] * db[None, :, 0] + da[:, None, 1] * db[None, :, 1]
    assert max(np.abs(along).max(), np.abs(pa).max(), np.abs(pb).max(), np.abs(dot).max()) < 2 ** 43, 'the bounds of the docstring'
    ok = ((dot > 0) & (4000 * along <= gap * Ha[:, None]) & (4000 * along >= -back * Ha[:, None])
          & (4000 * np.abs(pa) <= offset * Ha[:, None]) & (4000 * np.abs(pb) <= offset * Hb[None, :]))
    ok[np.arange(r1 - r0), np.arange(r0 - lo, r1 - lo)] = False             # a != b
    cost = vx * vx + vy * vy
    assert cost.max() < 2 ** 43
    return ok, cost


def links_cpu(polys, group_start, aspect, gap=2000, back=500, offset=500, grid=GRID_MAX, block=256):
    """-> (succ0 int32 [N], cost0 int64 [N]) before resolution: the passing b of least cost (ties to the lower b) and its cost; -1, -1
    if none.  Evaluated in blocks of `block` rows against a group: no [N, N] temporaries beyond [block, n_g]."""
    grid = _check_grid(grid)
    p = _check_polys(polys, grid)
    gs = _check_groups(group_start, len(p))
    asp = _check_aspect(aspect, gs.size - 1)
    gap, back, offset = _check_params(gap, back, offset)
    f = features_cpu(p, _aspect_per_word(gs, asp))
    succ = np.full(len(p), -1, dtype=np.int32)
    cost = np.full(len(p), -1, dtype=np.int64)
    big = np.int64(2 ** 62)
    for g in range(gs.size - 1):
        lo, hi = int(gs[g]), int(gs[g + 1])
        for r0 in range(lo, hi, int(block)):
            r1 = min(hi, r0 + int(block))
            ok, c = _link_block(f, lo, hi, r0, r1, gap, back, offset)
            c = np.where(ok, c, big)
            b = c.argmin(1)                                                   # the first minimum: ties to the lower b
            cb = c[np.arange(r1 - r0), b]
            hit = cb < big
            succ[r0:r1] = np.where(hit, lo + b, -1)
            cost[r0:r1] = np.where(hit, cb, -1)
    return succ, cost


def resolve_cpu(succ0, cost0, group_start, f):
    """links -> lines, on the features f of features_cpu -> dict(succ, pred, line, line_pos, rank: int32 [N]; n_lines: int32 [G])"""
    gs = np.asarray(group_start, dtype=np.int64)
    N, G = int(gs[-1]), gs.size - 1
    succ = np.asarray(succ0, dtype=np.int64).copy()
    cost0 = np.asarray(cost0, dtype=np.int64)
    pred = np.full(N, -1, dtype=np.int64)
    line = np.zeros(N, dtype=np.int32)
    line_pos = np.zeros(N, dtype=np.int32)
    rank = np.zeros(N, dtype=np.int32)
    n_lines = np.zeros(G, dtype=np.int32)
    claim = {}
    for a in range(N):
        b = int(succ[a])
        if b >= 0:
            k = (int(cost0[a]), a)
            if b not in claim or k < claim[b]:
                claim[b] = k
    for a in range(N):
        b = int(succ[a])
        if b >= 0 and claim[b][1] != a:
            succ[a] = -1                                                      # lost: no second choice
    for b, (_, a) in claim.items():
        pred[b] = a
    seen = np.zeros(N, dtype=bool)
    for i in range(N):                                                        # ascending: the first member met of a cycle is its lowest
        if seen[i]:
            continue
        j = i
        while j >= 0 and not seen[j]:
            seen[j] = True
            j = int(succ[j])
        if j == i and pred[i] >= 0:
            succ[pred[i]] = -1
            pred[i] = -1
    Cy, Lx = f['C'][:, 1], f['L'][:, 0]
    for g in range(G):
        lo, hi = int(gs[g]), int(gs[g + 1])
        lines = []
        for h in range(lo, hi):
            if pred[h] >= 0:
                continue
            members, j = [], h
            while j >= 0:
                members.append(j)
                j = int(succ[j])
            lines.append((sum(int(Cy[m]) for m in members), len(members), int(Lx[h]), h, members))
        assert sum(l[1] for l in lines) == hi - lo

        def less(p, q):
            if p[0] * q[1] != q[0] * p[1]:
                return -1 if p[0] * q[1] < q[0] * p[1] else 1
            return -1 if p[2:4] < q[2:4] else 1

        lines.sort(key=functools.cmp_to_key(less))
        n_lines[g] = len(lines)
        r = 0
        for ln, (_, _, _, _, members) in enumerate(lines):
            for k, m in enumerate(members):
                line[m], line_pos[m], rank[m] = ln, k, r
                r += 1
    return dict(succ=succ.astype(np.int32), pred=pred.astype(np.int32), line=line, line_pos=line_pos, rank=rank, n_lines=n_lines)


def lines_cpu(polys, group_start, aspect, gap=2000, back=500, offset=500, grid=GRID_MAX):
    """-> dict(succ, pred: global indices or -1; line, line_pos, rank: inside the group; all int32 [N]; n_lines int32 [G])"""
    grid = _check_grid(grid)
    p = _check_polys(polys, grid)
    gs = _check_groups(group_start, len(p))
    asp = _check_aspect(aspect, gs.size - 1)
    succ0, cost0 = links_cpu(p, gs, asp, gap, back, offset, grid)
    return resolve_cpu(succ0, cost0, gs, features_cpu(p, _aspect_per_word(gs, asp)))

def _check_block_params(gap_x, gap_y, depth):
    out = []
    for name, v in (('gap_x', gap_x), ('gap_y', gap_y)):
        if int(v) != v or int(v) < 0 or int(v) > PARAM_MAX:
            raise ValueError('%s is a permille parameter 0 .. %d, got %r' % (name, PARAM_MAX, v))
        out.append(int(v))
    if isinstance(depth, bool) or int(depth) != depth or int(depth) < 1 or int(depth) > DEPTH_MAX:
        raise ValueError('depth is an integer 1 .. %d, got %r' % (DEPTH_MAX, depth))
    return out[0], out[1], int(depth)


def intervals_cpu(polys, aspect_per_word, gap_x, gap_y):
    """-> the inflated intervals of every word, int64 [N] each: (x_lo, x_hi, y_lo, y_hi), in 1 / 16000 of a scaled bin"""
    p = np.asarray(polys, dtype=np.int64).reshape(-1, 32)
    a = np.asarray(aspect_per_word, dtype=np.int64).reshape(-1, 2)
    assert p.shape[0] == a.shape[0], 'one aspect per word'
    assert p.size == 0 or (p.min() >= 0 and p.max() <= GRID_MAX - 1 and a.min() >= 1 and a.max() <= ASPECT_MAX), 'bins 0 .. 4095, aspects 1 .. 256'
    assert 0 <= gap_x <= PARAM_MAX and 0 <= gap_y <= PARAM_MAX
    P = p.reshape(-1, 16, 2) * a[:, None, :]
    s = (P[:, :7:-1] - P[:, :8]).sum(1)                      # sum_k (B[k] - T[k]), B[k] = P[15 - k]
    t = np.abs(s).max(1) if len(P) else np.zeros(0, np.int64)
    lo, hi = P.min(1), P.max(1)
    out = (16000 * lo[:, 0] - gap_x * t, 16000 * hi[:, 0] + gap_x * t, 16000 * lo[:, 1] - gap_y * t, 16000 * hi[:, 1] + gap_y * t)
    assert p.size == 0 or (t.max() < 2 ** 23 and max(int(np.abs(v).max()) for v in out) < 2 ** 38), 'the bounds of the docstring'
    return out


def blocks_cpu(polys, group_start, aspect, line, line_pos, n_lines, gap_x=1000, gap_y=1500, depth=8, grid=GRID_MAX):
    """The XY-cut of the docstring over the lines of lines_cpu (its `line`, `line_pos`, `n_lines`; line_pos places a word inside its
    line, which no cut changes).  -> dict(block, line, rank: int32 [N]; n_blocks, levels: int32 [G])"""
    grid = _check_grid(grid)
    p = _check_polys(polys, grid)
    gs = _check_groups(group_start, len(p))
    asp = _check_aspect(aspect, gs.size - 1)
    gap_x, gap_y, depth = _check_block_params(gap_x, gap_y, depth)
    N, G = len(p), gs.size - 1
    line = np.asarray(line, dtype=np.int64).reshape(-1)
    line_pos = np.asarray(line_pos, dtype=np.int64).reshape(-1)
    n_lines = np.asarray(n_lines, dtype=np.int64).reshape(-1)
    if line.size != N or line_pos.size != N or n_lines.size != G:
        raise ValueError('line, line_pos are per word (%d) and n_lines per group (%d)' % (N, G))
    xl, xh, yl, yh = intervals_cpu(p, _aspect_per_word(gs, asp), gap_x, gap_y)
    block = np.zeros(N, dtype=np.int32)
    new_line = np.zeros(N, dtype=np.int32)
    rank = np.zeros(N, dtype=np.int32)
    n_blocks = np.zeros(G, dtype=np.int32)
    levels = np.zeros(G, dtype=np.int32)
    big = np.int64(2 ** 62)
    for g in range(G):
        w0, w1 = int(gs[g]), int(gs[g + 1])
        n = int(n_lines[g])
        if w1 == w0:
            if n != 0:
                raise ValueError('group %d has no words and %d lines' % (g, n))
            continue
        ln = line[w0:w1]
        count = np.bincount(ln[(ln >= 0) & (ln < n)], minlength=max(n, 1))[:max(n, 1)]
        if n < 1 or ln.min() < 0 or ln.max() >= n or (count == 0).any():
            raise ValueError('group %d: its words must fill the lines 0 .. n_lines - 1' % g)
        ends = {}
        for name, v, red, init in (('xl', xl, np.minimum, big), ('xh', xh, np.maximum, -big), ('yl', yl, np.minimum, big), ('yh', yh, np.maximum, -big)):
            ends[name] = np.full(n, init, dtype=np.int64)
            red.at(ends[name], ln, v[w0:w1])
        seg = np.zeros(n, dtype=np.int64)
        n_seg, idle, lv = 1, False, 0
        for lv in range(1, depth + 1):
            lo, hi = (ends['yl'], ends['yh']) if lv % 2 else (ends['xl'], ends['xh'])    # level lv - 1: even levels cut y
            order = np.lexsort((np.arange(n), lo, seg))                                    # (segment, lo, line number)
            new = np.zeros(n, dtype=np.int64)
            comp, top, last = -1, 0, -1
            for a in order.tolist():
                if seg[a] != last or lo[a] > top:
                    comp += 1
                    top = hi[a]
                    last = seg[a]
                else:
                    top = max(top, hi[a])
                new[a] = comp
            created = comp + 1 > n_seg
            seg, n_seg = new, comp + 1
            if not created and idle:
                break
            idle = not created
        order = np.lexsort((np.arange(n), seg))                                            # (block, old line)
        pos = np.empty(n, dtype=np.int64)
        pos[order] = np.arange(n)
        start = np.zeros(n, dtype=np.int64)
        start[order] = np.concatenate([[0], np.cumsum(count[order])[:-1]])
        block[w0:w1] = seg[ln]
        new_line[w0:w1] = pos[ln]
        rank[w0:w1] = start[ln] + line_pos[w0:w1]
        n_blocks[g], levels[g] = n_seg, lv
    return dict(block=block, line=new_line, rank=rank, n_blocks=n_blocks, levels=levels)


# ---------------------------------------------------------------------------------------------
# the device stage
# ---------------------------------------------------------------------------------------------
class ReadingOrder(object):
    """lines_cpu on the device.  A call packs group_start and aspect into ONE upload, runs omp_reading_links and omp_reading_lines on
    the current stream and downloads the int32 outputs in ONE copy.  There is no CPU fallback: lines_cpu is the host specification.
    With blocks=(gap_x, gap_y, depth) a third launch, omp_reading_blocks, follows on the same stream and tables, and the same ONE
    download also carries blocks_cpu's outputs."""

    def __init__(self, device, grid):
        import torch
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('ReadingOrder runs on MI355X only (got device %s); there is no CPU fallback -- '
                               'lines_cpu is the host specification' % (self.device,))
        self.grid = _check_grid(grid)

    def run(self, polys, group_start, aspect, gap=2000, back=500, offset=500, want_links=False, blocks=None):
        """polys: int32 / int64 [N, 32] on the device or the host -> lines_cpu's dict as numpy (plus succ0, cost0 when want_links).
        blocks: None, or (gap_x, gap_y, depth) of blocks_cpu: the dict gains `blocks`, blocks_cpu's dict on this call's lines."""
        import torch

        from .. import ops
        gap, back, offset = _check_params(gap, back, offset)
        if blocks is not None:
            blocks = _check_block_params(*blocks)
        polys = torch.as_tensor(polys)
        if polys.dim() != 2 or polys.shape[1] != 32:
            raise ValueError('polys must be [N, 32], got %s' % (tuple(polys.shape),))
        N = int(polys.shape[0])
        gs = np.asarray(group_start, dtype=np.int64).reshape(-1)
        if gs.size < 1 or gs[0] != 0 or gs[-1] != N or (np.diff(gs) < 0).any():
            raise ValueError('group_start must rise from 0 to the number of words (%d), got %s' % (N, gs.tolist()[:8]))
        G = gs.size - 1
        asp = _check_aspect(aspect, G)
        if N == 0 or G == 0:
            z = np.zeros(0, np.int32)
            out = dict(succ=z, pred=z.copy(), line=z.copy(), line_pos=z.copy(), rank=z.copy(), n_lines=np.zeros(G, np.int32))
            if want_links:
                out.update(succ0=z.copy(), cost0=np.zeros(0, np.int64))
            if blocks is not None:
                out['blocks'] = dict(block=z.copy(), line=z.copy(), rank=z.copy(), n_blocks=np.zeros(G, np.int32), levels=np.zeros(G, np.int32))
            return out
        host = np.concatenate([gs.astype(np.int32), asp.reshape(-1)]).astype(np.int32)
        with torch.cuda.device(self.device):
            tables = torch.from_numpy(host).to(self.device)                   # the one upload
            d_polys = polys.to(self.device).clamp(-1, GRID_MAX).to(torch.int32).contiguous()
            succ0, cost0 = ops.reading_links(d_polys, tables, host, G, self.grid, gap, back, offset)
            if blocks is None:
                ints = ops.reading_lines(d_polys, tables, host, G, self.grid, succ0, cost0)
            else:                                                             # one tensor behind both launches: still one download
                ints = torch.empty(8 * N + 3 * G, dtype=torch.int32, device=self.device)
                ops.reading_lines(d_polys, tables, host, G, self.grid, succ0, cost0, out=ints[:5 * N + G])
                ops.reading_blocks(d_polys, tables, host, G, self.grid, ints[:5 * N + G], *blocks, out=ints[5 * N + G:])
            h = ints.cpu().numpy()                                            # the one download
            out = dict(zip(('succ', 'pred', 'line', 'line_pos', 'rank'), (h[k * N:(k + 1) * N].copy() for k in range(5))), n_lines=h[5 * N:5 * N + G].copy())
            if blocks is not None:
                b = h[5 * N + G:]
                out['blocks'] = dict(zip(('block', 'line', 'rank'), (b[k * N:(k + 1) * N].copy() for k in range(3))), n_blocks=b[3 * N:3 * N + G].copy(),
                                     levels=b[3 * N + G:].copy())
            if want_links:
                out.update(succ0=succ0.cpu().numpy(), cost0=cost0.cpu().numpy())
        if (out['n_lines'] < 0).any():
            raise RuntimeError('omp_reading_lines refused a group (more than %d words)' % GROUP_MAX)
        if blocks is not None and (out['blocks']['n_blocks'] < 0).any():
            raise RuntimeError('omp_reading_blocks refused a group (more than %d words)' % GROUP_MAX)
        return out

    def __call__(self, polys, group_start, aspect, gap=2000, back=500, offset=500, blocks=None):
        return self.run(polys, group_start, aspect, gap, back, offset, blocks=blocks)


# ---------------------------------------------------------------------------------------------
# the engine's side: `reading_order=` of predict / predict_images / spot_and_recognize
# ---------------------------------------------------------------------------------------------
def check_block_args(blocks=False, block_gap_x=1.0, block_gap_y=1.5, block_depth=8, reading_order=True, infer_vie=False):
    """the refusals of `blocks=` -> None without it, else (gap_x, gap_y) in permille and the depth"""
    if not blocks:
        return None
    if infer_vie:
        raise ValueError('blocks= needs text-spotting records; with args.infer_vie the engine returns entity tuples')
    if not reading_order:
        raise ValueError('blocks=True orders the lines of reading_order=True: pass both')
    return _check_block_params(permille(block_gap_x, 'block_gap_x'), permille(block_gap_y, 'block_gap_y'), block_depth)


def check_reading_args(line_gap=2.0, line_back=0.5, line_offset=0.5, infer_vie=False, blocks=False, block_gap_x=1.0, block_gap_y=1.5, block_depth=8):
    """the refusals of the public interface -> (gap, back, offset) in permille; the block arguments are checked when blocks is set
    (check_block_args converts them)"""
    if infer_vie:
        raise ValueError('reading_order= needs text-spotting records; with args.infer_vie the engine returns entity tuples')
    check_block_args(blocks, block_gap_x, block_gap_y, block_depth)
    return permille(line_gap, 'line_gap'), permille(line_back, 'line_back'), permille(line_offset, 'line_offset')


def order_records(records, raw_polys, sizes, grid, line_gap=2.0, line_back=0.5, line_offset=0.5, rows=None, reader=None, device=None, blocks=False,
                  block_gap_x=1.0, block_gap_y=1.5, block_depth=8):
    """records: per image the list of record dicts.  raw_polys: per image the polygon decoder's ids ([n_b, 32] tensors, None or empty
    for an image without records), on the device; rows: per image the rows of raw_polys its records stand for (None: all of them, in
    order -- after suppress= the survivors').  sizes: per image (h, w), the orig_size the polygons were scaled by.  One device call for
    all images (`reader`: a ReadingOrder, or anything with its __call__; default: one on `device`).
    -> the lists reordered by rank; every record gains `line` and `line_pos`.  blocks=True (block_gap_x, block_gap_y, block_depth): the
    same call also cuts the lines into blocks (blocks_cpu); every record gains `block`, `line` counts through the blocks and the lists
    come in the blocks' order."""
    import torch
    gap, back, offset = check_reading_args(line_gap, line_back, line_offset)
    cut = check_block_args(blocks, block_gap_x, block_gap_y, block_depth)
    counts = [len(r) for r in records]
    gs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    if int(gs[-1]) == 0:
        return [list(r) for r in records]
    parts = []
    for b, (n, rp) in enumerate(zip(counts, raw_polys)):
        if n == 0:
            continue
        rp = torch.as_tensor(rp).reshape(-1, 32)
        if rows is not None and rows[b] is not None:
            rp = rp[torch.as_tensor(list(rows[b]), dtype=torch.long, device=rp.device)]
        if rp.shape[0] != n:
            raise ValueError('image %d: %d polygons for %d records' % (b, rp.shape[0], n))
        parts.append(rp)
    polys = torch.cat(parts, 0)
    aspect = np.asarray([aspect_of(*sizes[b]) for b in range(len(records))], dtype=np.int32).reshape(-1, 2)
    if reader is None:
        reader = ReadingOrder(polys.device if device is None else device, grid)
    if cut is None:
        res = reader(polys, gs, aspect, gap, back, offset)
        line, rank = res['line'], res['rank']
    else:
        res = reader(polys, gs, aspect, gap, back, offset, blocks=cut)
        line, rank = res['blocks']['line'], res['blocks']['rank']
    out = []
    for b, recs in enumerate(records):
        lo = int(gs[b])
        ordered = [None] * len(recs)
        for i, r in enumerate(recs):
            r['line'], r['line_pos'] = int(line[lo + i]), int(res['line_pos'][lo + i])
            if cut is not None:
                r['block'] = int(res['blocks']['block'][lo + i])
            ordered[int(rank[lo + i])] = r
        out.append(ordered)
    return out


def page_lines(records, field='rec', sep=' '):
    """one image's ordered records -> its lines as strings: `field` of the records of one `line`, joined by sep"""
    lines = []
    last = None
    for r in records:
        if r['line'] != last:
            lines.append([])
            last = r['line']
        lines[-1].append(str(r[field]))
    return [sep.join(l) for l in lines]


def page_blocks(records, field='rec', sep=' ', line_sep='\n'):
    """one image's records of a blocks=True call -> one string per block: the block's lines (page_lines) joined by line_sep"""
    blocks = []
    last = None
    for r in records:
        if r['block'] != last:
            blocks.append([])
            last = r['block']
        blocks[-1].append(r)
    return [line_sep.join(page_lines(b, field, sep)) for b in blocks]
