"""GPU checks of overlap suppression: omp_polygon_overlap / omp_polygon_keep against their numpy specification
(utils/overlap.py) on every output integer -- area, bounding boxes, every word of the bitmask, the dense intersection matrices, owner,
kept -- and `suppress=` of predict / spot_and_recognize against suppress_cpu applied on the host to the same call's records.  Every
check returns records {name, err, tol, ok, note} like tests/gpu_checks.py."""
import numpy as np
import torch

from advancedliteratemachinery_amd.utils import overlap as OV
from advancedliteratemachinery_amd.utils import synthetic as weights
from advancedliteratemachinery_amd.utils import windows as WN
from advancedliteratemachinery_amd.utils.parser import make_args

GROUP_SIZES = (1, 2, 0, 63, 64, 65, 129)    # the bitmask word and the wave boundary from both sides, an empty group in between
THRESHOLDS = (1, 500, 1000)


# ---------------------------------------------------------------------------------------------------------------------------------
# polygons
# ---------------------------------------------------------------------------------------------------------------------------------
def word_polys(rng, n, grid, centres=6):
    """word-like rotated rectangles resampled to 16 points (8 along the top, 8 back along the bottom, as the polygon decoder draws
    them), clustered around a few centres so that many of them overlap"""
    cx = rng.randint(grid // 8, grid - grid // 8, centres)
    cy = rng.randint(grid // 8, grid - grid // 8, centres)
    out = np.zeros((n, 32), dtype=np.int32)
    for i in range(n):
        k = rng.randint(centres)
        w, h = rng.randint(grid // 25 + 2, grid // 6 + 3), rng.randint(grid // 60 + 2, grid // 20 + 3)
        th = rng.uniform(-np.pi, np.pi) if rng.rand() < 0.3 else rng.uniform(-0.3, 0.3)
        x = cx[k] + rng.randint(-grid // 30 - 1, grid // 30 + 2)
        y = cy[k] + rng.randint(-grid // 60 - 1, grid // 60 + 2)
        u = np.linspace(-w / 2.0, w / 2.0, 8)
        px = np.concatenate([u, u[::-1]])
        py = np.concatenate([np.full(8, -h / 2.0), np.full(8, h / 2.0)])
        out[i, 0::2] = np.round(x + px * np.cos(th) - py * np.sin(th))
        out[i, 1::2] = np.round(y + px * np.sin(th) + py * np.cos(th))
    return out                                  # tokens may leave [0, grid - 1]: both sides clamp


def _orders(rng, gs):
    N = int(gs[-1])
    ident = np.arange(N, dtype=np.int32)
    rev, rand = ident.copy(), ident.copy()
    for g in range(len(gs) - 1):
        lo, hi = int(gs[g]), int(gs[g + 1])
        rev[lo:hi] = ident[lo:hi][::-1]
        rand[lo:hi] = lo + rng.permutation(hi - lo)
    return (('identity', ident), ('reversed', rev), ('random', rand))


def _cases():
    """(name, polys, group_start, grid): the smallest shapes that can break the kernels"""
    rng = np.random.RandomState(17)
    gs = np.concatenate([[0], np.cumsum(GROUP_SIZES)])
    p = word_polys(rng, int(gs[-1]), 1000)
    p[5::9] = p[4::9][:len(p[5::9])]             # exact duplicates, next to their originals ...
    p[gs[-1] - 1] = p[gs[-2]]                    # ... and at the two ends of the 129-polygon group
    p[gs[4] + 7] = np.tile(p[gs[4] + 7, :2], 16)   # all points equal: area 0
    yield 'words grid=1000 groups=%s' % (list(GROUP_SIZES),), p, gs, 1000
    yield 'words grid=1000 G=1 n=129', word_polys(rng, 129, 1000, centres=3), np.array([0, 129]), 1000
    sizes = rng.randint(0, 13, 40)
    gs40 = np.concatenate([[0], np.cumsum(sizes)])
    yield 'words grid=64 G=40', word_polys(rng, int(gs40[-1]), 64, centres=2), gs40, 64
    yield 'random 16-gons grid=64 groups=[65, 20]', rng.randint(0, 64, size=(85, 32)).astype(np.int32), np.array([0, 65, 85]), 64
    yield 'random 16-gons grid=1000 n=12', rng.randint(-20, 1020, size=(12, 32)).astype(np.int32), np.array([0, 12]), 1000
    # one pair spanning the whole grid: every sample row, the largest sums
    full = np.array([0, 0, 999, 0, 999, 999, 0, 999] + [0, 999] * 12, dtype=np.int32)
    star = rng.randint(0, 1000, size=32).astype(np.int32)
    star[:8] = [0, 0, 999, 999, 999, 0, 0, 999]
    yield 'whole grid pair grid=1000', np.stack([full, star, full]), np.array([0, 3]), 1000
    g = OV.GRID_MAX
    full = np.array([0, 0, g - 1, 0, g - 1, g - 1, 0, g - 1] + [0, g - 1] * 12, dtype=np.int32)
    diamond = np.array([g // 2, 0, g - 1, g // 2, g // 2, g - 1, 0, g // 2] + [0, g // 2] * 12, dtype=np.int32)
    yield 'whole grid pair grid=%d' % g, np.stack([full, diamond]), np.array([0, 2]), g


def check_overlap_op():
    from tests.gpu_checks import DEV, rec
    out = []
    for name, polys, gs, grid in _cases():
        gs = np.asarray(gs, dtype=np.int32)
        N, G = len(polys), len(gs) - 1
        inter = OV.pair_overlap_cpu(polys, gs, grid)          # the reference, once per case
        area = np.concatenate([np.diag(m) for m in inter]).astype(np.int32)
        bbox = OV.bbox_cpu(polys, grid)
        sup = OV.OverlapSuppressor(DEV, grid)
        d_polys = torch.from_numpy(polys).to(DEV)
        rng = np.random.RandomState(3)
        combo = 0
        n_removed = 0
        for measure in OV.MEASURES:
            for t in THRESHOLDS:
                for oname, order in _orders(rng, gs):
                    want_inter = combo % 2 == 0
                    combo += 1
                    tag = 'overlap[%s] %s t=%d order=%s inter=%d' % (name, measure, t, oname, want_inter)
                    owner, _ = OV.suppress_from_inter(inter, gs, order, t, measure)
                    mask = OV.mask_cpu(polys, gs, order, t, measure, grid, inter=inter)
                    kept = np.array([int((owner[gs[g]:gs[g + 1]] == np.arange(gs[g], gs[g + 1])).sum()) for g in range(G)], dtype=np.int32)
                    n_removed += N - int(kept.sum())
                    got = sup.run(d_polys, gs, order, t, measure, want_inter=want_inter)
                    out.append(rec(tag + ' area, bbox', int((got['area'] != area).sum()) + int((got['bbox'] != bbox).sum()), 0, '%d polygons' % N))
                    g_mask = got['mask'].cpu().numpy().view(np.uint64)
                    bad = int((g_mask != mask).sum()) if g_mask.shape == mask.shape else -1
                    out.append(rec(tag + ' every mask word', bad if bad >= 0 else float('inf'), 0, '%d words, %d bits set' % (
                        mask.size, int(np.unpackbits(mask.view(np.uint8)).sum()))))
                    out.append(rec(tag + ' owner, kept', int((got['owner'] != owner).sum()) + int((got['kept'] != kept).sum()), 0,
                                   '%d kept of %d' % (int(kept.sum()), N)))
                    if want_inter:
                        bad = sum(int((a != b).sum()) if a.shape == b.shape else 1 for a, b in zip(got['inter'], inter))
                        out.append(rec(tag + ' dense inter', bad, 0))
        out.append(rec('overlap[%s] something is suppressed somewhere' % name, 0 if n_removed > 0 else 1, 0, '%d removals over all combinations' % n_removed))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# groups above 4096 polygons: overlap_keep_kernel's second wave (threads 64 .. 127 own the positions >= 4096)
# ---------------------------------------------------------------------------------------------------------------------------------
LARGE_CALLS = ((4097,), (4032, 4096, 4161), (8192,))    # W = 65 | 63, 64, 66 | 128 words
LARGE_COMBOS = (('iou', 500, 'identity'), ('iou', 500, 'reversed'), ('iou', 500, 'random'), ('iomin', 1000, 'random'), ('iou', 1, 'identity'))
LARGE_INTER = ('iou', 500, 'reversed')                  # the combination that also asks for the dense matrices (calls up to 4161 only)
HALF = 4096                                             # the first position of wave 1
FIXED_ROWS = (0, 63, 64, 4095, 4096, 8190, 8191)
EVENTS = ('owner below 4096 removes a position >= 4096', 'owner and victim >= 4096 in one word', 'owner and victim >= 4096 in different words',
          'kept at >= 4096 although it overlaps a removed polygon')


def _plant_large(p):
    """p: one group's distinct, non-overlapping words [n, 32], changed in place BY POLYGON INDEX.  Every plant is made twice, at index i
    and at its mirror n - 1 - i, so that the identity and the reversed order both meet it with the roles of the two ends exchanged:
      (a) exact duplicates at 4096 + k of the polygons k < 8
      (b) duplicates with original and copy at >= 4096, inside one 64-position word and (n = 8192) in different words
      (c) chains A, B, C, each 4 bins below the one before (words are 16 bins high: neighbours have IoU 12 / 20, the ends 8 / 24), A below
          4096, B and C above: B is removed by A, so C is kept although it overlaps B
    The low ends use the indices 0 .. 11, the high ends the offsets 0 .. 40 behind 4096 (and 70 .. 4083 at 8192); at n = 4161 the mirrors of
    the one fall on the offsets 53 .. 64 of the other end, and no index is used twice."""
    n = len(p)
    hi = n - HALF

    def shifted(src, dy):
        q = p[src].copy()
        q[1::2] += dy
        return q

    if hi < 1:                                           # every position is wave 0's: duplicates at the two ends and one chain across them
        for k in range(8):
            p[n - 1 - k] = p[k]
        p[n - 30], p[n - 29] = shifted(20, 4), shifted(20, 8)
        return
    for at in ((lambda i: i), (lambda i: n - 1 - i)):
        if hi == 1:
            p[at(HALF)] = p[at(0)]                       # the one position of wave 1
            continue
        assert hi >= 65
        for k in range(8):
            p[at(HALF + k)] = p[at(k)]
        for a, b in ((8, 9), (10, 11), (12, 19), (13, 20), (14, 33), (15, 34), (16, 40)):
            p[at(HALF + b)] = p[at(HALF + a)]
        for j in range(4):
            p[at(HALF + 21 + 2 * j)], p[at(HALF + 22 + 2 * j)] = shifted(at(8 + j), 4), shifted(at(8 + j), 8)
        if hi == HALF:
            for a, b in ((70, 200), (71, 1000), (72, 2000), (73, 3000), (74, 4000), (75, 4083), (130, 195), (131, 3900)):
                p[at(HALF + b)] = p[at(HALF + a)]


def _page_words(rng, n):
    """n of the 128 x 64 distinct, non-overlapping words (40 x 16 bins) of a page on grid 4096, shuffled"""
    from tests import reading_cases as RC
    page = RC.to_bins(RC.page_points(128, 64, w=40, h=16, gap=12, pitch=30, centre=(2048.0, 2048.0)))
    return page[rng.permutation(len(page))[:n]].copy()


def _large_case(sizes, seed):
    """-> (polys, group_start): per group its own shuffle of the page, planted"""
    rng = np.random.RandomState(seed)
    parts = []
    for n in sizes:
        p = _page_words(rng, n)
        _plant_large(p)
        parts.append(p)
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _large_events(inter_g, owner_g, order_g):
    """one group, local indices, read from the REFERENCE's inter and owner at (iou, 500) -> the counts of EVENTS"""
    n = len(owner_g)
    pos = np.empty(n, dtype=np.int64)
    pos[order_g] = np.arange(n)
    victims = np.nonzero(owner_g != np.arange(n))[0]
    po, pv = pos[owner_g[victims]], pos[victims]
    both = (po >= HALF) & (pv >= HALF)
    ov = OV.overlap_matrix(inter_g, 500, 'iou')
    removed = owner_g != np.arange(n)
    touched = ov[:, removed].any(1) & ~removed & (pos >= HALF)
    return np.array([int(((po < HALF) & (pv >= HALF)).sum()), int((both & (po >> 6 == pv >> 6)).sum()), int((both & (po >> 6 != pv >> 6)).sum()),
                     int(touched.sum())])


def _mask_rows(ov, o, rows):
    """rows (priority positions) of the bitmask of one group from its overlap matrix -> uint64 [len(rows), W]"""
    n = len(o)
    W = (n + 63) // 64
    bits = np.zeros((len(rows), W * 64), dtype=np.uint8)
    bits[:, :n] = ov[o[rows]][:, o] & (np.arange(n)[None, :] > np.asarray(rows)[:, None])
    return np.packbits(bits, axis=1, bitorder='little').view(np.uint64).reshape(len(rows), W)


def _needed(n):
    """how many of each of EVENTS a group of n polygons must hold (0: the group has no room for it): one position behind 4096 can only
    be a victim of wave 0; one word and a bit hold everything but a pair in different words; 8192 holds a handful of each"""
    if n <= HALF:
        return (0, 0, 0, 0)
    if n == HALF + 1:
        return (1, 0, 0, 0)
    return (5, 5, 5 if n - HALF >= 128 else 0, 5)


def check_overlap_large_groups(call):
    """LARGE_CALLS[call]: groups of 4097 | 4032, 4096, 4161 | 8192 polygons (65 | 63, 64, 66 | 128 mask words): area, bbox, owner and kept
    everywhere; every mask word against mask_cpu up to 4161 (and the dense matrices once per call); at 8192 the mask rows of a fixed
    sample of priority positions, built from overlap_matrix.  The preconditions are read from the REFERENCE's inter and owner at
    (iou, 500) under the identity and the reversed order; without them the check fails."""
    from tests.gpu_checks import DEV, rec
    out = []
    grid = 4096
    sup = OV.OverlapSuppressor(DEV, grid)
    sizes = LARGE_CALLS[call]
    polys, gs = _large_case(sizes, 40 + call)
    N, G = len(polys), len(sizes)
    name = 'groups=%s' % (list(sizes),)
    inter = OV.pair_overlap_cpu(polys, gs, grid)          # the reference, once per call
    area = np.concatenate([np.diag(m) for m in inter]).astype(np.int32)
    bbox = OV.bbox_cpu(polys, grid)
    d_polys = torch.from_numpy(polys).to(DEV)
    orders = dict(_orders(np.random.RandomState(3), gs))
    full_mask = max(sizes) <= 4161
    for measure, t, oname in LARGE_COMBOS:
        order = orders[oname]
        want_inter = full_mask and (measure, t, oname) == LARGE_INTER
        tag = 'overlap large[%s] %s t=%d order=%s inter=%d' % (name, measure, t, oname, want_inter)
        owner, _ = OV.suppress_from_inter(inter, gs, order, t, measure)
        kept = np.array([int((owner[gs[g]:gs[g + 1]] == np.arange(gs[g], gs[g + 1])).sum()) for g in range(G)], dtype=np.int32)
        if t == 500 and oname in ('identity', 'reversed'):
            for g, n in enumerate(sizes):
                if n <= HALF:
                    continue
                lo, hi = int(gs[g]), int(gs[g + 1])
                ev = _large_events(inter[g], owner[lo:hi] - lo, order[lo:hi] - lo)
                out.append(rec('precondition: overlap large[n=%d] order=%s holds its wave-1 events' % (n, oname), int((ev < np.array(_needed(n))).sum()), 0,
                               ', '.join('%d (of %d) x %s' % (ev[k], _needed(n)[k], EVENTS[k]) for k in range(4))))
        got = sup.run(d_polys, gs, order, t, measure, want_inter=want_inter)
        out.append(rec(tag + ' area, bbox', int((got['area'] != area).sum()) + int((got['bbox'] != bbox).sum()), 0, '%d polygons' % N))
        out.append(rec(tag + ' owner, kept', int((got['owner'] != owner).sum()) + int((got['kept'] != kept).sum()), 0,
                       '%d kept of %d' % (int(kept.sum()), N)))
        g_mask = got['mask'].cpu().numpy().view(np.uint64)
        if full_mask:
            mask = OV.mask_cpu(polys, gs, order, t, measure, grid, inter=inter)
            bad = int((g_mask != mask).sum()) if g_mask.shape == mask.shape else -1
            out.append(rec(tag + ' every mask word', bad if bad >= 0 else float('inf'), 0, '%d words, %d bits set' % (
                mask.size, int(np.unpackbits(mask.view(np.uint8)).sum()))))
        else:                                                           # mask_cpu at 8192 builds a 512 MB bit table: sampled rows instead
            n = sizes[0]
            rows = np.unique(np.concatenate([FIXED_ROWS, np.random.RandomState(9).randint(0, n, 300)])).astype(np.int64)
            want = _mask_rows(OV.overlap_matrix(inter[0], t, measure), order.astype(np.int64), rows)
            ok = g_mask.size == n * ((n + 63) // 64)
            bad = int((g_mask.reshape(n, -1)[rows] != want).sum()) if ok else float('inf')
            out.append(rec(tag + ' the mask rows of %d sampled positions' % len(rows), bad, 0, '%d bits set' % int(np.unpackbits(want.view(np.uint8)).sum())))
        if want_inter:
            bad = sum(int((a != b).sum()) if a.shape == b.shape else 1 for a, b in zip(got['inter'], inter))
            out.append(rec(tag + ' dense inter', bad, 0))
        del got, g_mask
    return out


def check_overlap_device_refusals():
    """what only the device tables show: omp_polygon_keep answers kept = -1 and owner = identity for the group, processes the other
    groups, and writes nothing else; omp_polygon_overlap writes zeros for the mask words that belong to no row and nothing behind the
    mask.  Straight through ops / the C entry with prefilled sentinels (OverlapSuppressor.run raises on the host first)."""
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    out = []
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)      # noqa: E731
    big = OV.GROUP_MAX + 1
    words = _page_words(np.random.RandomState(7), 5)
    words[3] = words[1]                                                          # one duplicate: 3 is removed by 1
    for what, tail in (('all-zero polygons', np.zeros((5, 32), np.int32)), ('a duplicate in the small group', words)):
        polys = np.concatenate([np.zeros((big, 32), np.int32), tail])
        n = len(polys)
        gs = np.array([0, big, n], np.int32)
        ms, _ = OV.mask_layout(gs)
        d_gs, d_ms, d_order = t(gs, torch.int32), t(ms, torch.int64), t(np.arange(n), torch.int32)
        res = ops.polygon_overlap(t(polys, torch.int32), d_gs, d_order, d_ms, int(ms[-1]), 4096, 500, 0)
        ints = ops.polygon_keep(res['mask'], d_ms, d_gs, d_order, n, out=torch.full((6 * n + 2,), -7, dtype=torch.int32, device=DEV)).cpu().numpy()
        owner, _ = OV.suppress_cpu(tail, [0, 5], np.arange(5), 500, 'iou', 4096)
        want_owner = np.concatenate([np.arange(big), big + owner])
        want_kept = [-1, int((owner == np.arange(5)).sum())]
        out.append(rec('keep refuses the group of %d on the device (%s): kept = -1, owner = identity' % (big, what),
                       int((ints[5 * n:5 * n + big] != np.arange(big)).sum()) + int(ints[6 * n] != -1), 0))
        out.append(rec('keep beside the refused group (%s): the group of 5 is processed' % what,
                       int((ints[5 * n + big:6 * n] != want_owner[big:]).sum()) + int(ints[6 * n + 1] != want_kept[1]), 0, 'kept %d of 5' % want_kept[1]))
        out.append(rec('keep beside the refused group (%s): nothing is written outside owner and kept' % what, int((ints[:5 * n] != -7).sum()), 0))
    # a mask layout that the mask does not hold: groups of 5 and 3 with 10 words reserved for the first and 12 words in all
    polys = np.concatenate([words, words[:3]])
    polys[6] = polys[5]                                                           # a duplicate in the second group too
    gs, ms, mask_words, pad = np.array([0, 5, 8], np.int32), np.array([0, 10, 13], np.int64), 12, 64
    d_gs, d_ms, d_order, d_polys = t(gs, torch.int32), t(ms, torch.int64), t(np.arange(8), torch.int32), t(polys, torch.int32)
    mask = torch.full((mask_words + pad,), -7, dtype=torch.int64, device=DEV)
    ints = torch.full((6 * 8 + 2,), -7, dtype=torch.int32, device=DEV)
    rc = _lib.lib().omp_polygon_overlap(ops.ptr(d_polys), 8, ops.ptr(d_gs), 2, ops.ptr(d_order), ops.ptr(d_ms), mask_words, 4096, 500, 0, ops.ptr(ints[32:40]),
                                        ops.ptr(ints[:32]), ops.ptr(mask), None, None, 0, ops.stream())
    out.append(rec('overlap accepts a mask layout with a gap (the device tables are not read on the host)', abs(int(rc)), 0))
    ops.polygon_keep(mask[:mask_words], d_ms, d_gs, d_order, 8, out=ints)
    h_mask, h = mask.cpu().numpy(), ints.cpu().numpy()
    rows0 = OV.mask_cpu(polys[:5], [0, 5], np.arange(5), 500, 'iou', 4096).view(np.int64)
    rows1 = OV.mask_cpu(polys[5:], [0, 3], np.arange(3), 500, 'iou', 4096).view(np.int64)
    bad = int((h_mask[:5] != rows0).sum()) + int((h_mask[5:10] != 0).sum()) + int((h_mask[10:12] != rows1[:2]).sum())
    out.append(rec('overlap with a gap in the layout: the rows that fit are written, the words of no row are 0', bad, 0,
                   '%d bits set' % int(np.unpackbits(np.concatenate([rows0, rows1[:2]]).view(np.uint8)).sum())))
    out.append(rec('overlap with a gap in the layout: nothing is written behind the mask', int((h_mask[mask_words:] != -7).sum()), 0))
    owner, _ = OV.suppress_cpu(polys[:5], [0, 5], np.arange(5), 500, 'iou', 4096)
    bad = int((h[40:45] != owner).sum()) + int((h[45:48] != np.arange(5, 8)).sum()) + int(h[48:].tolist() != [int((owner == np.arange(5)).sum()), -1])
    out.append(rec('keep refuses the group whose rows do not fit the mask: kept = -1, owner = identity, the other group processed', bad, 0))
    return out


def check_overlap_refusals():
    """what the entry points refuse comes back as an error code and a message; nothing aborts"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV, rec
    polys = torch.zeros(2, 32, dtype=torch.int32, device=DEV)
    gs = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    order = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    ms = torch.tensor([0, 2], dtype=torch.int64, device=DEV)
    out = []
    for what, kw in (('grid 4097', dict(grid=4097)), ('grid 1', dict(grid=1)), ('t 0', dict(t=0)), ('t 1001', dict(t=1001)), ('measure 2', dict(measure=2))):
        a = dict(grid=1000, t=500, measure=0)
        a.update(kw)
        try:
            ops.polygon_overlap(polys, gs, order, ms, 2, a['grid'], a['t'], a['measure'])
            bad = 1
        except RuntimeError as e:
            bad = 0 if 'omp_polygon_overlap' in str(e) else 1
        out.append(rec('overlap refuses %s with an error code' % what, bad, 0))
    try:
        OV.OverlapSuppressor(DEV, 1000).run(torch.zeros(8193, 32, dtype=torch.int32), [0, 8193])
        bad = 1
    except ValueError:
        bad = 0
    out.append(rec('overlap refuses a group of 8193 polygons', bad, 0))
    r = OV.OverlapSuppressor(DEV, 1000).run(torch.zeros(0, 32, dtype=torch.int32), [0, 0, 0])
    out.append(rec('overlap: no polygons, no launch', int(r['owner'].size) + int(r['kept'].tolist() != [0, 0]), 0))
    return out + check_overlap_device_refusals()


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
def _windows(args):
    return [WN.default_window(args), WN.default_window(args)] + WN.grid_windows(2, 2, args.num_bins)


def _expected(records, raw, args, t, measure='iou', order='first'):
    """suppress_cpu on the host, on the raw polygon ids of the call that made `records` -> (kept indices, merged lists) per image"""
    counts = [len(r) for r in records]
    gs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    polys = np.concatenate([r[0][1].reshape(-1, 32).cpu().numpy() for r in raw if r is not None] or [np.zeros((0, 32), np.int64)])
    prio = np.arange(int(gs[-1])) if order == 'first' else OV.score_order([r['score'] for recs in records for r in recs], gs)
    owner, _ = OV.suppress_cpu(polys, gs, prio, t, measure, args.num_bins)
    out = []
    for b, recs in enumerate(records):
        lo = int(gs[b])
        kept = [i for i in range(len(recs)) if owner[lo + i] == lo + i]
        merged = {i: [(recs[j]['window'], j) for j in range(len(recs)) if owner[lo + j] == lo + i and j != i] for i in kept}
        out.append((kept, merged))
    return out


def _minus(r, keys=('merged',)):
    return {k: v for k, v in r.items() if k not in keys}


def check_engine_suppress(dtype_name):
    """spot_windows' image and weights, windows = [default, default, 2 x 2 grid]: predict(suppress=0.5) == suppress_cpu on the host"""
    from advancedliteratemachinery_amd.engine import inference as inf
    from advancedliteratemachinery_amd.utils.nested_tensor import NestedTensor
    from tests.gpu_checks import DEV, ENGINES, build_model, golden, rec
    from tests.gpu_checks_windows import fixture_case
    gold = golden('spot_windows')
    args, sd, img, mask, _ = fixture_case(gold, 'eos')
    model = build_model(args, sd, gold['case']['depths'], ENGINES[dtype_name])
    nt = NestedTensor(img.to(DEV), mask.to(DEV))
    wins = _windows(args)
    tag = 'suppress engine[%s]' % dtype_name
    out = []
    plain = inf.predict(model, nt, args, windows=wins)
    again = inf.predict(model, nt, args, windows=wins, suppress=None)
    out.append(rec(tag + ' suppress=None is today\'s predict', 0 if again == plain and all('merged' not in r for r in plain[0]) else 1, 0,
                   '%d records' % len(plain[0])))
    raw, _ = inf.predict_raw(model, nt, args, windows=WN.resolve_windows(wins, 1))
    for kw in (dict(), dict(suppress_measure='iomin'), dict(suppress_order='score')):
        got = inf.predict(model, nt, args, windows=wins, suppress=0.5, **kw)
        want = _expected(plain, raw, args, 500, kw.get('suppress_measure', 'iou'), kw.get('suppress_order', 'first'))
        name = '%s %s' % (tag, kw or 'iou, first')
        for b, (kept, merged) in enumerate(want):
            same = [_minus(r) for r in got[b]] == [plain[b][i] for i in kept]
            out.append(rec(name + ' survivors == suppress_cpu on the host', 0 if same else 1, 0, '%d of %d' % (len(kept), len(plain[b]))))
            same = len(got[b]) == len(kept) and all(r['merged'] == merged[i] for r, i in zip(got[b], kept))
            out.append(rec(name + ' merged lists', 0 if same else 1, 0))
            out.append(rec(name + ' at least one record is removed', 0 if len(got[b]) < len(plain[b]) else 1, 0))
    # plain call (no windows): merged holds plain indices, and lexicon= annotates the survivors only
    plain = inf.predict(model, nt, args)
    raw, _ = inf.predict_raw(model, nt, args)
    got = inf.predict(model, nt, args, suppress=0.3, lexicon=['word', 'text'])
    gs = [0, len(plain[0])]
    owner, _ = OV.suppress_cpu(raw[0][0][1].reshape(-1, 32).cpu().numpy(), gs, np.arange(gs[1]), 300, 'iou', args.num_bins)
    kept = [i for i in range(gs[1]) if owner[i] == i]
    same = [_minus(r, ('merged', 'lex', 'lex_index', 'lex_dist')) for r in got[0]] == [plain[0][i] for i in kept]
    same = same and all(r['merged'] == [j for j in range(gs[1]) if owner[j] == i and j != i] and 'lex_dist' in r for r, i in zip(got[0], kept))
    out.append(rec(tag + ' no windows: survivors, plain merged indices, lexicon on the survivors', 0 if same else 1, 0, '%d of %d' % (len(kept), gs[1])))
    return out


def check_two_stage_suppress():
    """spot_and_recognize(crop='polygon', suppress=...): duplicates are removed before the crops; the crops recognised are exactly the
    survivors' crops"""
    from advancedliteratemachinery_amd.engine import inference as inf
    from advancedliteratemachinery_amd.engine.two_stage import recognize_crops, spot_and_recognize
    from oracle import mgp_str_ref as R
    from tests.gpu_checks import DEV, build_model, rec
    from tests.gpu_checks_mgp import build
    depths = (2, 2, 2, 2)
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, pt_seq_length=6, test_min_size=64, test_max_size=112)
    sd = weights.make_state_dict(args, seed=5, depths=depths)
    omni = build_model(args, sd, depths, torch.float32)
    c = R.cfg(depth=2)
    mgp = build(c, R.make_state_dict(c, seed=17), torch.float32)
    rng = np.random.RandomState(3)
    images = [torch.from_numpy(rng.randint(0, 256, (90, 140, 3), dtype=np.uint8)), torch.from_numpy(rng.randint(0, 256, (70, 100, 3), dtype=np.uint8))]
    wins = _windows(args)
    out = []
    plain, pre = inf.predict_images(omni, images, args, windows=wins, ragged=True)
    dev_imgs = [i.to(DEV).contiguous() for i in images]
    nt, _ = pre(dev_imgs)
    raw, _ = inf.predict_raw(omni, nt, args, ragged=True, windows=WN.resolve_windows(wins, 2))
    want = _expected(plain, raw, args, 500)
    seen = []
    recognize = mgp.recognize
    mgp.recognize = lambda batch: seen.append(int(batch.shape[0])) or recognize(batch)
    try:
        got, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon', windows=wins, ragged=True, suppress=0.5)
    finally:
        del mgp.recognize
    n_kept = sum(len(k) for k, _ in want)
    out.append(rec('two-stage suppress: crops recognised == survivors', abs(sum(seen) - n_kept), 0, '%d crops for %d records' % (sum(seen), sum(len(p) for p in plain))))
    out.append(rec('two-stage suppress: at least one record is removed', 0 if n_kept < sum(len(p) for p in plain) else 1, 0))
    keys = ('merged', 'box', 'crop', 'strip', 'mgp_text', 'mgp_conf', 'mgp_choice', 'mgp_ids')
    bad = 0
    for b, (kept, merged) in enumerate(want):
        bad += int([_minus(r, keys) for r in got[b]] != [plain[b][i] for i in kept])
        bad += int(len(got[b]) != len(kept) or any(r['merged'] != merged[i] for r, i in zip(got[b], kept)))
    out.append(rec('two-stage suppress: survivors and merged lists == suppress_cpu on the host', bad, 0))
    flat = [(b, r) for b, recs in enumerate(got) for r in recs]
    reads, _ = recognize_crops(mgp, dev_imgs, None, polys=[(b, r['polys']) for b, r in flat])
    bad = int(len(reads) != len(flat))
    for (_, r), m in zip(flat, reads):
        bad += int(r['mgp_text'] != m['char_text']) + int(r['mgp_choice'] != m['choice']) + int(tuple(r['mgp_conf']) != tuple(m['conf']))
    out.append(rec('two-stage suppress: mgp_* == recognize_crops on the survivors\' polygons', bad, 0))
    return out
