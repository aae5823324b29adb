"""Shared inputs of the tile-stage tests (tests/test_tiles_host.py, tests/gpu_checks_tiles.py): seeded random words, tiles and pages for
utils/tiles.py::remap_cpu / ops.tile_remap, and an independent per-coordinate reference written with fractions.Fraction."""
from fractions import Fraction

import numpy as np

from advancedliteratemachinery_amd.utils import tiles as TL


def random_case(seed, n, n_pages, nb=1000, max_side=3000, max_tiles=8, empty=0.2, corner=False):
    """-> dict(polys [n, 32], points [n, 2], row_start, tile_rect, tile_page, page_size): n words spread over the tiles of n_pages pages
    (1 .. max_tiles x-by-y tiles each, from plan_tiles); some tiles and some pages hold no words; ids at 0, nb - 1, -5 and nb + 7 occur;
    words hug the tile sides often enough that every cut bit shows.  corner: pages of 65535 pixels a side."""
    rng = np.random.RandomState(seed)
    rects, owner, sizes = [], [], []
    for p in range(n_pages):
        if corner:
            h, w = 65535, 65535 - int(rng.randint(0, 3))
        else:
            h, w = int(rng.randint(64, max_side + 1)), int(rng.randint(64, max_side + 1))
        nx = int(rng.randint(1, max_tiles + 1))
        ny = int(rng.randint(1, max(1, min(max_tiles, 64 // nx)) + 1))
        nx, ny = min(nx, w // 8), min(ny, h // 8)
        r = TL.plan_tiles(h, w, nx, ny, int(rng.randint(0, 501)))
        rects.append(r)
        owner.append(np.full(len(r), p, np.int32))
        sizes.append([w, h])
    rect, page = np.concatenate(rects, 0), np.concatenate(owner, 0)
    T = len(rect)
    # words per tile: some tiles empty, some pages empty (the first page with more than one page always gets words)
    weight = rng.rand(T) * (rng.rand(T) >= empty)
    if n_pages > 2:
        weight[page == n_pages - 1] = 0.0            # an empty page
    if weight.sum() == 0:
        weight[0] = 1.0
    counts = rng.multinomial(n, weight / weight.sum())
    row_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    polys = rng.randint(0, nb, size=(n, 32)).astype(np.int32)
    points = rng.randint(0, nb, size=(n, 2)).astype(np.int32)
    # compact words well inside the tile (no cut bit) for about half of them, so that every tile keeps some and drops some
    inner = rng.rand(n) < 0.5
    lo = rng.randint(nb // 10, nb // 2, size=(n, 1))
    polys[inner] = (lo + rng.randint(0, nb // 4, size=(n, 32)))[inner]
    points[inner] = (lo + rng.randint(0, nb // 4, size=(n, 2)))[inner]
    for value in (0, nb - 1, -5, nb + 7):           # the clamp's corners, also among the inner words
        polys[rng.rand(n, 32) < 0.01] = value
        points[rng.rand(n, 2) < 0.01] = value
    return dict(polys=polys, points=points, row_start=row_start, tile_rect=rect.astype(np.int32), tile_page=page.astype(np.int32),
                page_size=np.asarray(sizes, np.int32))


def remap_reference(case, nb, P, edge, drop_cut):
    """remap_cpu by its definition, one coordinate at a time in exact rational arithmetic: c / nb of the tile -> page pixels -> P bins,
    rounded half up.  Accepted tiles only (the cases of random_case).  -> (cut, page_polys, page_points, src_row, tile_count)"""
    polys, points = case['polys'], case['points']
    cut = np.full(len(polys), -1, np.int32)
    rows, src, tile_count = [], [], []
    for k, (x0, y0, x1, y1) in enumerate(case['tile_rect'].tolist()):
        W, H = (int(v) for v in case['page_size'][case['tile_page'][k]])
        kept = 0
        for n in range(int(case['row_start'][k]), int(case['row_start'][k + 1])):
            ids = [min(max(int(c), 0), nb - 1) for c in polys[n].tolist() + points[n].tolist()]
            xs, ys = ids[0::2], ids[1::2]
            bits = (1 if x0 > 0 and min(xs) <= edge else 0) | (2 if y0 > 0 and min(ys) <= edge else 0) \
                | (4 if x1 < W and max(xs) >= nb - 1 - edge else 0) | (8 if y1 < H and max(ys) >= nb - 1 - edge else 0)
            cut[n] = bits
            if drop_cut and bits:
                continue
            row = []
            for j, c in enumerate(ids):
                o, e, S = (x0, x1 - x0, W) if j % 2 == 0 else (y0, y1 - y0, H)
                pixel = o + Fraction(c, nb) * e                       # decode_seq's c / nb in page pixels
                b = pixel / S * P + Fraction(1, 2)                    # ... in P bins, half up
                row.append(min(P - 1, b.numerator // b.denominator))
            rows.append(row)
            src.append(n)
            kept += 1
        tile_count.append(kept)
    rows = np.asarray(rows, np.int32).reshape(-1, 34)
    return cut, rows[:, :32], rows[:, 32:], np.asarray(src, np.int32), np.asarray(tile_count, np.int32)
