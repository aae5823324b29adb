"""Shared by tests/test_scoring_host.py and tests/gpu_checks_scoring.py: the hand-worked cases of DESIGN.md section 21, seeded pages of
word-like rectangles (ground truth first, then detections), and a deliberately naive matcher in plain Python integers."""
import numpy as np

# (ground truth, detections) per image: nothing at all, one side empty, a pair, the 64-detection word and the 256-thread stride from
# both sides
SIZES = ((0, 0), (0, 3), (3, 0), (1, 1), (63, 65), (64, 64), (130, 257))


def rect(x0, x1, y0, y1):
    """[x0, x1] x [y0, y1] as its 4 corners"""
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


# name -> (ground truth [(rect, text, dc)], detections [(rect, text)]) on grid 64, every score 1.0
HAND = {
    'A': ([(rect(0, 10, 0, 10), 'AB', False)], [(rect(0, 10, 0, 5), 'ab'), (rect(0, 10, 0, 10), 'AB')]),
    'B': ([(rect(20, 30, 20, 30), 'x', True)], [(rect(20, 30, 20, 26), 'x'), (rect(18, 30, 18, 30), 'x'), (rect(10, 30, 10, 30), 'x')]),
    'C': ([(rect(0, 10, 0, 10), 'a', False), (rect(0, 10, 0, 4), 'b', False)], [(rect(0, 10, 0, 7), 'a'), (rect(0, 10, 0, 10), 'b')]),
}


def word(rng, grid):
    """an axis-near word rectangle resampled to 16 points, as the polygon decoder draws it"""
    w, h = rng.randint(grid // 25 + 2, grid // 6 + 3), rng.randint(grid // 60 + 2, grid // 20 + 3)
    x, y = rng.randint(0, grid), rng.randint(0, grid)
    th = rng.uniform(-0.3, 0.3)
    u = np.linspace(-w / 2.0, w / 2.0, 8)
    px, py = np.concatenate([u, u[::-1]]), np.concatenate([np.full(8, -h / 2.0), np.full(8, h / 2.0)])
    out = np.zeros(32, dtype=np.int32)
    out[0::2] = np.round(x + px * np.cos(th) - py * np.sin(th))
    out[1::2] = np.round(y + px * np.sin(th) + py * np.cos(th))
    return np.clip(out, 0, grid - 1)


def page(rng, m, nd, grid):
    """one image: m ground-truth words, then nd detections -- jittered copies of ground-truth words (several per word, so that the
    greedy order matters), exact duplicates, words of their own, and detections of area 0"""
    gt = np.stack([word(rng, grid) for _ in range(m)]) if m else np.zeros((0, 32), np.int32)
    det = np.zeros((nd, 32), dtype=np.int32)
    for d in range(nd):
        u = rng.rand()
        if m and u < 0.55:
            det[d] = gt[rng.randint(m)] + rng.randint(-max(1, grid // 200), max(1, grid // 200) + 1, 32)
        elif m and u < 0.7:
            det[d] = gt[rng.randint(m)]
        elif d and u < 0.8:
            det[d] = det[rng.randint(d)]
        elif u < 0.88:
            det[d] = np.tile(rng.randint(0, grid, 2), 16)          # all points equal: area 0
        else:
            det[d] = word(rng, grid)
    if m and nd:
        det[0] = gt[0] + rng.randint(-1, 2, 32)                    # the smallest images match something too
    return np.clip(np.concatenate([gt, det]), 0, grid - 1).astype(np.int32)


def pages(seed, sizes, grid, n_thr, all_dc=False):
    """-> dict(polys [n, 32], group_start, n_gt, gt_dc, text, level): the flat inputs of match_pages_cpu / SpottingScorer.run"""
    rng = np.random.RandomState(seed)
    polys = [page(rng, m, nd, grid) for m, nd in sizes]
    gs = np.concatenate([[0], np.cumsum([m + nd for m, nd in sizes])]).astype(np.int32)
    n = int(gs[-1])
    gt_dc = np.ones(n, np.int32) if all_dc else (rng.rand(n) < 0.25).astype(np.int32)
    text = rng.randint(0, 3, n).astype(np.int32)
    level = rng.randint(0, n_thr + 1, n).astype(np.int32)
    level[rng.rand(n) < 0.3] = n_thr                              # many detections live through the whole sweep
    return dict(polys=np.concatenate(polys + [np.zeros((0, 32), np.int32)]), group_start=gs, n_gt=np.asarray([m for m, _ in sizes], np.int32),
                gt_dc=gt_dc, text=text, level=level)


def naive_match(inter, m, gt_dc, text, level, n_thr, t_iou, t_dc, report):
    """the protocol of utils/scoring.py read off its docstring, one Python integer at a time"""
    inter = [[int(v) for v in row] for row in np.asarray(inter).tolist()]
    n = len(inter)
    counts = [[0, 0, 0, 0] for _ in range(n_thr)]
    det_gt, gt_det = [-4] * (n - m), [-4] * m
    for k in range(n_thr):
        state = {}
        for d in range(m, n):
            if not level[d] > k:
                state[d] = 'inactive'
                continue
            state[d] = 'care'
            for i in range(m):
                if gt_dc[i] and inter[i][d] > 0 and 1000 * inter[i][d] >= t_dc * inter[d][d]:
                    state[d] = 'dc'
        counts[k][0] = sum(1 for i in range(m) if not gt_dc[i])
        counts[k][1] = sum(1 for d in range(m, n) if state[d] == 'care')
        taken, pair = set(), {}
        for i in range(m):
            if gt_dc[i]:
                continue
            for d in range(m, n):
                if state[d] != 'care' or d in taken or not inter[i][d] > 0:
                    continue
                if 1000 * inter[i][d] >= t_iou * (inter[i][i] + inter[d][d] - inter[i][d]):
                    taken.add(d)
                    pair[i] = d
                    counts[k][2] += 1
                    counts[k][3] += int(text[i] == text[d])
                    break
        if k == report:
            back = {d: i for i, d in pair.items()}
            det_gt = [back.get(d, {'inactive': -3, 'dc': -2, 'care': -1}[state[d]]) for d in range(m, n)]
            gt_det = [-2 if gt_dc[i] else (pair[i] - m if i in pair else -1) for i in range(m)]
    return np.asarray(counts, np.int32).reshape(n_thr, 4), np.asarray(det_gt, np.int32), np.asarray(gt_det, np.int32)
