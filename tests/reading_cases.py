"""Synthetic words for the reading-order tests (host and GPU): word polygons as the polygon decoder draws them (8 points along the
top, left to right in the word's own frame, 8 back along the bottom), pages of rows, a ring, and how to read lines out of a result."""
import numpy as np


def word(x, y, w, h):
    """an upright word with its top-left corner at (x, y) -> float [16, 2]"""
    u = x + np.linspace(0.0, w, 8)
    return np.concatenate([np.stack([u, np.full(8, float(y))], 1), np.stack([u[::-1], np.full(8, float(y + h))], 1)])


def rotate(pts, degrees, centre):
    t = np.deg2rad(degrees)
    c, s = np.cos(t), np.sin(t)
    q = np.asarray(pts, dtype=np.float64) - centre
    return np.stack([q[..., 0] * c - q[..., 1] * s, q[..., 0] * s + q[..., 1] * c], -1) + centre


def to_bins(pts, sx=1.0):
    """float [N, 16, 2] -> int32 [N, 32], x scaled by sx before rounding"""
    p = np.asarray(pts, dtype=np.float64).copy()
    p[..., 0] *= sx
    return np.rint(p).astype(np.int32).reshape(len(p), 32)


def page_points(rows=5, cols=6, w=60, h=20, gap=12, pitch=34, centre=(500.0, 500.0), jitter=0.0):
    """rows x cols words, row-major -> float [rows * cols, 16, 2]; jitter: alternate words of a row sit that far above / below it"""
    x0 = centre[0] - (cols * w + (cols - 1) * gap) / 2.0
    y0 = centre[1] - ((rows - 1) * pitch + h) / 2.0
    return np.stack([word(x0 + c * (w + gap), y0 + r * pitch + (jitter if c % 2 else -jitter), w, h) for r in range(rows) for c in range(cols)])


def page(rows=5, cols=6, degrees=0.0, seed=None, sx=1.0, **kw):
    """-> (polys int32 [rows * cols, 32], ids): ids[i] = the row-major word that sits at index i (shuffled with a seed)"""
    centre = np.asarray(kw.get('centre', (500.0, 500.0)))
    kw['centre'] = tuple(centre)
    pts = rotate(page_points(rows, cols, **kw), degrees, centre)
    ids = np.arange(rows * cols) if seed is None else np.random.RandomState(seed).permutation(rows * cols)
    return to_bins(pts[ids], sx), ids


def ring(n=10, r=150.0, w=80, h=20, centre=(500.0, 500.0)):
    """n words set clockwise around a circle, word k at index k -> int32 [n, 32]"""
    c = np.asarray(centre)
    top = word(c[0] - w / 2.0, c[1] - r - h / 2.0, w, h)
    return to_bins(np.stack([rotate(top, 360.0 * k / n, c) for k in range(n)]))


def lines_of(res, lo=0, hi=None, ids=None):
    """a result of lines_cpu / ReadingOrder -> the group's lines, each the list of its members (ids[member] when given) in line_pos
    order, in line order; checks that rank is the concatenation"""
    hi = len(res['line']) if hi is None else hi
    n = int(res['line'][lo:hi].max()) + 1 if hi > lo else 0
    out = [[] for _ in range(n)]
    for i in sorted(range(lo, hi), key=lambda i: int(res['rank'][i])):
        assert int(res['line_pos'][i]) == len(out[int(res['line'][i])])
        out[int(res['line'][i])].append(int(i - lo if ids is None else ids[i - lo]))
    flat = [m for l in out for m in l]
    assert len(flat) == hi - lo and sorted(int(r) for r in res['rank'][lo:hi]) == list(range(hi - lo))
    assert [int(res['line'][i]) for i in sorted(range(lo, hi), key=lambda i: int(res['rank'][i]))] == sorted(int(v) for v in res['line'][lo:hi])
    return out
