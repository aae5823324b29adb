"""Tiled pages: read a large page as overlapping full-resolution tiles.

Every entry point scales a page to test_min_size / test_max_size before the model sees it; small print on an A4 scan or a poster does
not survive that.  A tiled call cuts the page into overlapping tiles, reads every tile at the model's full input size, carries the words
back into page coordinates and drops the fragments at the seams.  This module holds the stage between a tile's records and a page's:

  plan_tiles     the nx * ny overlapping pixel rectangles of a page
  remap_cpu      the numpy SPECIFICATION of omp_tile_remap (csrc/tiles.hip): tile ids -> page bins, the cut bits, the stable compaction
  TileStage      remap_cpu on the device: one upload, ops.tile_remap, one download; page_polys stays on the device
  check_tile_args, tile_records   the engine's side: `tiles=` / `tile_size=` of predict_images / spot_and_recognize

The numpy functions here are the DEFINITION; csrc/tiles.hip equals them on every integer.  Integers only.

Tiles      tile_rect int32 [T, 4]: [x0, y0, x1, y1] in page pixels, x1 / y1 exclusive; tile_page int32 [T]: the page of every tile;
           page_size int32 [pages, 2]: (W, H), 1 .. 65535 each.  The tiles of a call are sorted by page.
Words      polys int32 [N, 32] and points int32 [N, 2]: the decoders' raw ids in TILE bins; words row_start[k] .. row_start[k + 1] - 1
           are tile k's.  Every id is first clamped to [0, nb - 1] (as overlap._check_polys does).
Remapping  an x id c of a tile [x0, x1) on a page of width W becomes the page bin
               min(P - 1, (2 (x0 nb + c (x1 - x0)) P + nb W) // (2 nb W)),   P = page_bins
           which is decode_seq's c / nb carried into page pixels and back into P bins, rounded half up (64-bit: the numerator reaches
           4.4e12 at 65535 pixels and 4096 bins on both sides).  y uses y0, y1 and H.  One tile over the whole page with P == nb is
           the identity.
Cut bits   per word, from the clamped tile ids of its 17 points (16 polygon points and the centre point):
               1  x0 > 0 and min x <= edge              2  y0 > 0 and min y <= edge
               4  x1 < W and max x >= nb - 1 - edge     8  y1 < H and max y >= nb - 1 - edge
           A word that reaches an INNER side of its tile is a fragment of a word the neighbouring tile sees whole; a side on the page
           border never cuts.
Refusals   a tile whose rectangle leaves its page (or is empty), whose page index is outside the table (or whose page is not 1 ..
           65535 pixels a side), or whose row range is not 0 <= row_start[k] <= row_start[k + 1] <= N is REFUSED: tile_count -1,
           tile_dropped 0, no rows, and the cut entries of its words stay -1.
"""
import numpy as np

TILE_MAX = 256         # tiles per page
SIDE_MAX = 65535       # pixels per page side
CORE_MIN = 8           # pixels: the narrowest core a tile may have
OVERLAP_MAX = 500      # permille of a core: neighbouring tiles then share one whole core
BINS_MAX = 4096        # utils/overlap.py: GRID_MAX
ROW = 34               # ids per word: 32 polygon coordinates and the point


# ---------------------------------------------------------------------------------------------
# the tiles of a page
# ---------------------------------------------------------------------------------------------
def overlap_permille(tile_overlap):
    """the float of the public interface -> o in permille, 0 .. 500 (as overlap.permille converts `suppress`)"""
    s = float(tile_overlap)
    if not (0.0 <= s <= 0.5):
        raise ValueError('tile_overlap must be a float in [0, 0.5], got %r' % (tile_overlap,))
    return min(OVERLAP_MAX, max(0, int(round(1000 * s))))


def tile_grid(height, width, tiles=None, tile_size=None):
    """`tiles=(nx, ny)` or `tile_size=s` (shorthand for nx = ceil(width / s), ny = ceil(height / s)) -> (nx, ny)"""
    if tiles is not None and tile_size is not None:
        raise ValueError('give tiles= or tile_size=, not both')
    if tiles is None and tile_size is None:
        raise ValueError('tile_grid: tiles= or tile_size=')
    if tile_size is not None:
        if isinstance(tile_size, bool) or int(tile_size) != tile_size or int(tile_size) < 1:
            raise ValueError('tile_size must be a positive integer, got %r' % (tile_size,))
        s = int(tile_size)
        return (int(width) + s - 1) // s, (int(height) + s - 1) // s
    if len(tiles) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 for v in tiles):
        raise ValueError('tiles must be two positive integers (nx, ny), got %r' % (tiles,))
    return int(tiles[0]), int(tiles[1])


def plan_tiles(height, width, nx, ny, overlap):
    """The nx * ny tiles [x0, y0, x1, y1] (pixels, x1 / y1 exclusive) of a height x width page, x the outer loop as in grid_windows;
    overlap: o in permille of a core, 0 .. 500 (overlap_permille).  Core edges cx[i] = (i width) // nx; tile (i, j) is its core grown by
    ox = (ceil(width / nx) o) // 1000 and oy likewise on every side, clipped to the page: neighbours share 2 ox pixels.
    -> int32 [nx * ny, 4]"""
    height, width, nx, ny, o = int(height), int(width), int(nx), int(ny), int(overlap)
    if min(height, width) < 1 or max(height, width) > SIDE_MAX:
        raise ValueError('plan_tiles: a page side is 1 .. %d pixels (got %d x %d)' % (SIDE_MAX, width, height))
    if nx < 1 or ny < 1 or nx * ny > TILE_MAX:
        raise ValueError('plan_tiles: 1 .. %d tiles per page (got %d x %d)' % (TILE_MAX, nx, ny))
    if o < 0 or o > OVERLAP_MAX:
        raise ValueError('plan_tiles: overlap is 0 .. %d permille, got %d' % (OVERLAP_MAX, o))
    if width // nx < CORE_MIN or height // ny < CORE_MIN:
        raise ValueError('plan_tiles: a core of %d x %d tiles on a %d x %d page is narrower than %d pixels' % (nx, ny, width, height, CORE_MIN))
    ox, oy = ((width + nx - 1) // nx * o) // 1000, ((height + ny - 1) // ny * o) // 1000
    cx, cy = [(i * width) // nx for i in range(nx + 1)], [(j * height) // ny for j in range(ny + 1)]
    out = [[max(0, cx[i] - ox), max(0, cy[j] - oy), min(width, cx[i + 1] + ox), min(height, cy[j + 1] + oy)] for i in range(nx) for j in range(ny)]
    return np.asarray(out, dtype=np.int32).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------
def _check_bins(nb, page_bins, edge):
    nb, P, edge = int(nb), int(page_bins), int(edge)
    if nb < 2 or nb > BINS_MAX or P < 2 or P > BINS_MAX:
        raise ValueError('nb and page_bins must be 2 .. %d, got %d and %d' % (BINS_MAX, nb, P))
    if edge < 0 or edge > BINS_MAX:
        raise ValueError('edge must be 0 .. %d tile bins, got %d' % (BINS_MAX, edge))
    return nb, P, edge


def _check_words(polys, points):
    p, q = np.asarray(polys), np.asarray(points)
    if p.ndim != 2 or p.shape[1] != 32 or q.ndim != 2 or q.shape[1] != 2 or q.shape[0] != p.shape[0]:
        raise ValueError('polys must be [N, 32] and points [N, 2], got %s and %s' % (tuple(p.shape), tuple(q.shape)))
    return np.concatenate([p.astype(np.int64), q.astype(np.int64)], 1)


def _check_tables(row_start, tile_rect, tile_page, page_size):
    rs = np.asarray(row_start, dtype=np.int64).reshape(-1)
    rect = np.asarray(tile_rect, dtype=np.int64).reshape(-1, 4)
    page = np.asarray(tile_page, dtype=np.int64).reshape(-1)
    size = np.asarray(page_size, dtype=np.int64).reshape(-1, 2)
    T = rect.shape[0]
    if T < 1 or rs.size != T + 1 or page.size != T or size.shape[0] < 1:
        raise ValueError('tables: %d tiles need row_start [%d], tile_page [%d] and at least one page (got %d, %d, %d)'
                         % (T, T + 1, T, rs.size, page.size, size.shape[0]))
    return rs, rect, page, size


def tile_ok(rs, rect, page, size, k, n):
    """the device's test of tile k (see Refusals above)"""
    x0, y0, x1, y1 = (int(v) for v in rect[k])
    if not (0 <= int(rs[k]) <= int(rs[k + 1]) <= n) or not (0 <= int(page[k]) < size.shape[0]):
        return False
    W, H = int(size[page[k], 0]), int(size[page[k], 1])
    return 1 <= W <= SIDE_MAX and 1 <= H <= SIDE_MAX and 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H


def remap_cpu(polys, points, row_start, tile_rect, tile_page, page_size, nb, page_bins, edge=2, drop_cut=True):
    """-> dict(cut int32 [N] (-1 for the words of a refused tile or of none), page_polys int32 [R, 32], page_points int32 [R, 2], src_row
    int32 [R] (the stable compaction of the words with cut == 0 -- of all words of accepted tiles when drop_cut is false -- in tile
    order and, inside a tile, in the decoder's order), tile_count, tile_dropped int32 [T], out_start int32 [T + 1], page_count int32
    [pages])"""
    nb, P, edge = _check_bins(nb, page_bins, edge)
    ids = np.clip(_check_words(polys, points), 0, nb - 1)
    rs, rect, page, size = _check_tables(row_start, tile_rect, tile_page, page_size)
    N, T = ids.shape[0], rect.shape[0]
    cut = np.full(N, -1, np.int32)
    rows = np.zeros((N, ROW), np.int32)
    tile_count, tile_dropped = np.zeros(T, np.int32), np.zeros(T, np.int32)
    page_count = np.zeros(size.shape[0], np.int32)
    keep = []
    for k in range(T):
        if not tile_ok(rs, rect, page, size, k, N):
            tile_count[k] = -1
            continue
        lo, hi = int(rs[k]), int(rs[k + 1])
        x0, y0, x1, y1 = (int(v) for v in rect[k])
        W, H = int(size[page[k], 0]), int(size[page[k], 1])
        c = ids[lo:hi]
        x, y = c[:, 0::2], c[:, 1::2]
        bits = np.zeros(hi - lo, np.int32)
        if hi > lo:
            bits |= 1 * ((x0 > 0) & (x.min(1) <= edge))
            bits |= 2 * ((y0 > 0) & (y.min(1) <= edge))
            bits |= 4 * ((x1 < W) & (x.max(1) >= nb - 1 - edge))
            bits |= 8 * ((y1 < H) & (y.max(1) >= nb - 1 - edge))
        cut[lo:hi] = bits
        rows[lo:hi, 0::2] = np.minimum(P - 1, (2 * (x0 * nb + x * (x1 - x0)) * P + nb * W) // (2 * nb * W))
        rows[lo:hi, 1::2] = np.minimum(P - 1, (2 * (y0 * nb + y * (y1 - y0)) * P + nb * H) // (2 * nb * H))
        kept = lo + (np.nonzero(bits == 0)[0] if drop_cut else np.arange(hi - lo))
        tile_count[k], tile_dropped[k] = kept.size, (hi - lo) - kept.size
        page_count[page[k]] += kept.size
        keep.append(kept)
    src = np.concatenate(keep).astype(np.int32) if keep else np.zeros(0, np.int32)
    out_start = np.concatenate([[0], np.cumsum(np.maximum(tile_count, 0))]).astype(np.int32)
    return dict(cut=cut, page_polys=rows[src, :32].reshape(-1, 32), page_points=rows[src, 32:].reshape(-1, 2), src_row=src, tile_count=tile_count,
                tile_dropped=tile_dropped, out_start=out_start, page_count=page_count)


def pack_tables(row_start, tile_rect, tile_page, page_size):
    """-> the int32 table omp_tile_remap reads: row_start [T + 1] | tile_rect [T, 4] | tile_page [T] | page_size [pages, 2]"""
    rs, rect, page, size = _check_tables(row_start, tile_rect, tile_page, page_size)
    big = max(int(np.abs(a).max()) for a in (rs, rect, page, size))
    if big > 0x7fffffff:
        raise ValueError('tables: an entry does not fit int32')
    return np.concatenate([rs, rect.reshape(-1), page, size.reshape(-1)]).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# the device stage
# ---------------------------------------------------------------------------------------------
class TileStage(object):
    """remap_cpu on the device.  A call packs the four tables into ONE upload, runs omp_tile_remap on the current stream and downloads the
    integer outputs in ONE copy; page_polys (and page_points) stay on the device for the stages that follow.  There is no CPU fallback:
    remap_cpu is the host specification."""

    def __init__(self, device, nb):
        import torch
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('TileStage runs on MI355X only (got device %s); there is no CPU fallback -- '
                               'remap_cpu is the host specification' % (self.device,))
        self.nb = _check_bins(nb, 2, 0)[0]

    def run(self, polys, points, row_start, tile_rect, tile_page, page_size, page_bins, edge=2, drop_cut=True):
        """polys int32 / int64 [N, 32], points [N, 2], on the device or the host; the tables as remap_cpu takes them, and a row_start
        that rises from 0 to N.  -> remap_cpu's dict: cut, src_row and the counts as numpy, page_polys and page_points as DEVICE int32
        tensors [R, 32] / [R, 2]."""
        import torch

        from .. import ops
        nb, P, edge = _check_bins(self.nb, page_bins, edge)
        polys, points = torch.as_tensor(polys), torch.as_tensor(points)
        if polys.dim() != 2 or polys.shape[1] != 32 or points.dim() != 2 or points.shape[1] != 2 or points.shape[0] != polys.shape[0]:
            raise ValueError('polys must be [N, 32] and points [N, 2], got %s and %s' % (tuple(polys.shape), tuple(points.shape)))
        N = int(polys.shape[0])
        host = pack_tables(row_start, tile_rect, tile_page, page_size)
        T, pages = np.asarray(tile_page).size, np.asarray(page_size).size // 2
        rs = host[:T + 1]
        if rs[0] != 0 or rs[-1] != N or (np.diff(rs) < 0).any():
            raise ValueError('row_start must rise from 0 to the number of words (%d), got %s' % (N, rs.tolist()[:8]))
        if N == 0:                                                                                   # nothing to launch: the specification's answer
            res = remap_cpu(np.zeros((0, 32), np.int32), np.zeros((0, 2), np.int32), row_start, tile_rect, tile_page, page_size, nb, P, edge, drop_cut)
            res['page_polys'] = torch.zeros(0, 32, dtype=torch.int32, device=self.device)
            res['page_points'] = torch.zeros(0, 2, dtype=torch.int32, device=self.device)
            return res
        with torch.cuda.device(self.device):
            tables = torch.from_numpy(host).to(self.device)                                          # the one upload
            d_polys = polys.to(self.device).clamp(-1, BINS_MAX).to(torch.int32).contiguous()       # int64 tokens fit int32 once out-of-range ones are cut
            d_points = points.to(self.device).clamp(-1, BINS_MAX).to(torch.int32).contiguous()
            res = ops.tile_remap(d_polys, d_points, tables, T, pages, nb, P, edge, drop_cut)
            h = res['ints'].cpu().numpy()                                                            # the one download
        cut, src_row, tile_count, tile_dropped, out_start, page_count = (a.copy() for a in ops.split_tile_ints(h, N, T, pages))
        R = int(out_start[-1])
        if (tile_count < 0).any():
            raise RuntimeError('omp_tile_remap refused %d tiles (a rectangle that leaves its page, or a page outside the table)' % int((tile_count < 0).sum()))
        return dict(cut=cut, src_row=src_row[:R], tile_count=tile_count, tile_dropped=tile_dropped, out_start=out_start, page_count=page_count,
                    page_polys=res['page_polys'][:R], page_points=res['page_points'][:R])

    __call__ = run


# ---------------------------------------------------------------------------------------------
# the engine's side: `tiles=` / `tile_size=` of predict_images / spot_and_recognize
# ---------------------------------------------------------------------------------------------
def check_tile_args(tiles=None, tile_size=None, tile_overlap=0.125, tile_edge=2, tile_cut='drop', page_bins=None, num_bins=1000, infer_vie=False,
                    windows=None):
    """the refusals of the public interface -> None without tiles= / tile_size=, else dict(o (permille), edge, drop_cut, page_bins)"""
    if tiles is None and tile_size is None:
        return None
    if infer_vie:
        raise ValueError('tiles= / tile_size= need text-spotting records; with args.infer_vie the engine returns entity tuples')
    tile_grid(64, 64, tiles, tile_size)     # both given, or values that are no positive integers
    if windows is not None and len(windows) and len(windows[0]) and isinstance(windows[0][0], (list, tuple)):
        raise ValueError('tiles= reads every tile under the same windows: pass windows= in its shared form, not one list per image')
    if tile_cut not in ('drop', 'keep'):
        raise ValueError("tile_cut must be 'drop' or 'keep', got %r" % (tile_cut,))
    if isinstance(tile_edge, bool) or int(tile_edge) != tile_edge:
        raise ValueError('tile_edge is a whole number of tile bins, got %r' % (tile_edge,))
    nb, _, edge = _check_bins(num_bins, 2 if page_bins is None else page_bins, tile_edge)
    return dict(o=overlap_permille(tile_overlap), edge=edge, drop_cut=tile_cut == 'drop', page_bins=None if page_bins is None else int(page_bins))


def default_page_bins(num_bins, grids):
    """page_bins=None: min(4096, num_bins max(nx, ny)) over the call's pages -- a page bin about as fine as a tile bin"""
    return min(BINS_MAX, int(num_bins) * max([1] + [max(nx, ny) for nx, ny in grids]))


def plan_pages(page_hw, tiles=None, tile_size=None, o=125):
    """the tiles of a call: page_hw [(h, w)] per page -> (tile_rect int32 [T, 4], tile_page int32 [T], page_size int32 [pages, 2] as
    (W, H), grids [(nx, ny)] per page); tiles sorted by page, inside a page x-outer"""
    rects, owner, grids = [], [], []
    for p, (h, w) in enumerate(page_hw):
        nx, ny = tile_grid(h, w, tiles, tile_size)
        r = plan_tiles(h, w, nx, ny, o)
        rects.append(r)
        owner.append(np.full(len(r), p, np.int32))
        grids.append((nx, ny))
    if not rects:
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32), grids
    return (np.concatenate(rects, 0), np.concatenate(owner, 0),
            np.asarray([[w, h] for h, w in page_hw], dtype=np.int32).reshape(-1, 2), grids)


def tile_records(records, res, tile_rect, tile_page, n_pages, image_ids=None):
    """records: per TILE the record dicts decode_pred_seq gave with orig_size = the tile's (h, w); res: the stage's dict for those
    words (cut, src_row, tile_count, out_start).  -> per PAGE the records of its tiles that the stage kept, in the stage's order:
    `pts` and `polys` moved by the tile's (x0, y0) into page pixels, `image_id` the page's (image_ids[p]; default: as it is), and
    `tile` (the tile's index within its page), `tile_rect` ([x0, y0, x1, y1] in page pixels) and `tile_cut` (the cut bits)."""
    rs = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.int64)
    tile_page = np.asarray(tile_page).reshape(-1)
    first = {}
    for k, p in enumerate(tile_page.tolist()):
        first.setdefault(p, k)
    out = [[] for _ in range(int(n_pages))]
    src, start = np.asarray(res['src_row']), np.asarray(res['out_start'])
    for k, recs in enumerate(records):
        p = int(tile_page[k])
        x0, y0, x1, y1 = (int(v) for v in tile_rect[k])
        for n in src[int(start[k]):int(start[k + 1])].tolist():
            r = recs[n - int(rs[k])]
            r['pts'] = [[q[0] + x0, q[1] + y0] for q in r['pts']]
            r['polys'] = [[q[0] + x0, q[1] + y0] for q in r['polys']]
            if image_ids is not None:
                r['image_id'] = image_ids[p]
            r['tile'], r['tile_rect'], r['tile_cut'] = k - first[p], [x0, y0, x1, y1], int(res['cut'][n])
            out[p].append(r)
    return out
