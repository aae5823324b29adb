"""Tiled pages on the host (no GPU): plan_tiles on random pages, the numpy specification remap_cpu (utils/tiles.py) against an
independent per-coordinate loop in exact rational arithmetic, the identity, the cut bits on planted rectangles, the compaction with
empty and refused tiles, how predict_images / spot_and_recognize route `tiles=` (the engine and the device stages replaced by stubs and
their specifications), what they refuse, and that nothing changes without the arguments.  The kernels and the end-to-end answers are
tests/test_gpu_tiles.py."""
import copy
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from advancedliteratemachinery_amd.engine import inference as inf
from advancedliteratemachinery_amd.engine import two_stage
from advancedliteratemachinery_amd.utils import overlap as OV
from advancedliteratemachinery_amd.utils import reading as RD
from advancedliteratemachinery_amd.utils import tiles as TL
from advancedliteratemachinery_amd.utils.nested_tensor import NestedTensor
from advancedliteratemachinery_amd.utils.parser import make_args
from tests.tiles_cases import random_case, remap_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def square(x, y, w, h):
    pts = [(x, y), (x + w, y), (x + w, y + h), (x, y + h)] + [(x, y + h)] * 12
    return [c for p in pts for c in p]


# -- plan_tiles -------------------------------------------------------------------------------------------------------------------
def test_plan_tiles_on_random_pages():
    rng = np.random.RandomState(0)
    seen = 0
    for _ in range(400):
        h, w = (int(v) for v in rng.choice([rng.randint(8, 300), rng.randint(8, 65536), 65535], 2))
        nx, ny, o = int(rng.randint(1, 17)), int(rng.randint(1, 17)), int(rng.choice([0, 1, 125, 499, 500, rng.randint(0, 501)]))
        if w // nx < TL.CORE_MIN or h // ny < TL.CORE_MIN:
            with pytest.raises(ValueError):
                TL.plan_tiles(h, w, nx, ny, o)
            continue
        seen += 1
        r = TL.plan_tiles(h, w, nx, ny, o)
        assert r.dtype == np.int32 and r.shape == (nx * ny, 4)
        ox, oy = (-(-w // nx) * o) // 1000, (-(-h // ny) * o) // 1000
        g = r.reshape(nx, ny, 4).astype(np.int64)                            # x is the outer loop
        cx, cy = [(i * w) // nx for i in range(nx + 1)], [(j * h) // ny for j in range(ny + 1)]
        for i in range(nx):
            for j in range(ny):
                x0, y0, x1, y1 = g[i, j]
                assert (x0, y0, x1, y1) == (max(0, cx[i] - ox), max(0, cy[j] - oy), min(w, cx[i + 1] + ox), min(h, cy[j + 1] + oy))
                assert 0 <= x0 <= cx[i] < cx[i + 1] <= x1 <= w and 0 <= y0 <= cy[j] < cy[j + 1] <= y1 <= h   # every tile holds its core
        assert cx[0] == 0 and cx[-1] == w and cy[0] == 0 and cy[-1] == h     # the cores partition the page, so the tiles cover it
        assert (g[0, :, 0] == 0).all() and (g[-1, :, 2] == w).all() and (g[:, 0, 1] == 0).all() and (g[:, -1, 3] == h).all()
        for i in range(nx - 1):                                              # neighbours share exactly 2 ox pixels away from the borders
            if g[i, 0, 2] < w and g[i + 1, 0, 0] > 0:
                assert g[i, 0, 2] - g[i + 1, 0, 0] == 2 * ox
            assert g[i, 0, 2] >= g[i + 1, 0, 0]                              # no gap either way
        for j in range(ny - 1):
            if g[0, j, 3] < h and g[0, j + 1, 1] > 0:
                assert g[0, j, 3] - g[0, j + 1, 1] == 2 * oy
            assert g[0, j, 3] >= g[0, j + 1, 1]
    assert seen > 100


def test_plan_tiles_refuses():
    for h, w, nx, ny in ((65536, 100, 1, 1), (100, 65536, 1, 1), (0, 100, 1, 1),      # a page side above 65535 (or none)
                         (4000, 4000, 17, 16), (4000, 4000, 257, 1),                  # more than TILE_MAX tiles
                         (100, 63, 8, 1), (15, 100, 1, 2), (100, 100, 0, 1)):         # a core narrower than 8 pixels; no tile
        with pytest.raises(ValueError):
            TL.plan_tiles(h, w, nx, ny, 125)
    assert TL.TILE_MAX == 256 and TL.plan_tiles(4000, 4000, 16, 16, 125).shape == (256, 4)
    assert TL.plan_tiles(100, 64, 1, 8, 0).shape == (8, 4)
    for o in (-1, 501):
        with pytest.raises(ValueError):
            TL.plan_tiles(100, 100, 2, 2, o)
    with pytest.raises(ValueError):
        TL.tile_grid(100, 100, tiles=(2, 2), tile_size=50)                            # both
    with pytest.raises(ValueError):
        TL.tile_grid(100, 100)
    for bad in (dict(tiles=(2,)), dict(tiles=(0, 1)), dict(tiles=(1.5, 1)), dict(tile_size=0), dict(tile_size=2.5)):
        with pytest.raises(ValueError):
            TL.tile_grid(100, 100, **bad)
    assert TL.tile_grid(3508, 2480, tile_size=1024) == (3, 4) and TL.tile_grid(100, 100, tiles=(3, 2)) == (3, 2)
    assert [TL.overlap_permille(v) for v in (0, 0.125, 0.5, 0.0004)] == [0, 125, 500, 0]
    for v in (-0.1, 0.51, 2):
        with pytest.raises(ValueError):
            TL.overlap_permille(v)


# -- remap_cpu --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb', [1000, 4096])
@pytest.mark.parametrize('P', [2, 1000, 4096])
def test_remap_equals_the_rational_loop(nb, P):
    for seed, (n, pages, corner) in enumerate(((40, 1, False), (120, 3, False), (60, 2, True))):
        case = random_case(100 * seed + nb + P, n, pages, nb=nb, corner=corner)
        for edge, drop in ((0, True), (2, True), (2, False), (nb, True)):
            got = TL.remap_cpu(case['polys'], case['points'], case['row_start'], case['tile_rect'], case['tile_page'], case['page_size'], nb, P, edge, drop)
            cut, polys, points, src, count = remap_reference(case, nb, P, edge, drop)
            assert (got['cut'] == cut).all() and (got['src_row'] == src).all() and (got['tile_count'] == count).all()
            assert (got['page_polys'] == polys).all() and (got['page_points'] == points).all()
            assert got['page_polys'].dtype == np.int32 and got['page_polys'].min(initial=0) >= 0 and got['page_polys'].max(initial=0) <= P - 1
            assert (got['tile_count'] + got['tile_dropped'] == np.diff(case['row_start'])).all()
            assert (got['out_start'] == np.concatenate([[0], np.cumsum(count)])).all()
            assert (got['page_count'] == np.bincount(case['tile_page'], weights=count, minlength=len(case['page_size']))).all()
            if edge == nb:                                                   # everything with an inner side is cut
                for k, (x0, y0, x1, y1) in enumerate(case['tile_rect'].tolist()):
                    W, H = case['page_size'][case['tile_page'][k]]
                    want = (1 if x0 > 0 else 0) | (2 if y0 > 0 else 0) | (4 if x1 < W else 0) | (8 if y1 < H else 0)
                    assert (got['cut'][case['row_start'][k]:case['row_start'][k + 1]] == want).all()


def test_the_corner_needs_64_bits():
    """the largest numerator, at 65535 pixels and 4096 bins on both sides, is far above 2^32 and the answer is still exact"""
    rect = np.asarray([[61439, 0, 65535, 4096]], np.int32)
    polys = np.full((1, 32), 4095, np.int32)
    got = TL.remap_cpu(polys, polys[:, :2], [0, 1], rect, [0], [[65535, 65535]], 4096, 4096, 0, False)
    assert 2 * (61439 * 4096 + 4095 * 4096) * 4096 + 4096 * 65535 > 2 ** 41
    assert got['page_polys'][0, 0] == 4095 and got['page_polys'][0, 1] == (2 * 4095 * 4096 * 4096 + 4096 * 65535) // (2 * 4096 * 65535)


@pytest.mark.parametrize('nb', [2, 1000, 4096])
def test_one_tile_with_page_bins_equal_to_nb_is_the_identity(nb):
    rng = np.random.RandomState(nb)
    for h, w in ((1, 1), (75, 110), (65535, 65535), (3508, 2480)):
        polys, points = rng.randint(0, nb, (50, 32)), rng.randint(0, nb, (50, 2))
        polys[0], polys[1] = 0, nb - 1
        for edge in (0, 2, nb):
            got = TL.remap_cpu(polys, points, [0, 50], [[0, 0, w, h]], [0], [[w, h]], nb, nb, edge, True)
            assert (got['cut'] == 0).all() and (got['page_polys'] == polys).all() and (got['page_points'] == points).all()
            assert (got['src_row'] == np.arange(50)).all() and got['tile_count'].tolist() == [50] and got['tile_dropped'].tolist() == [0]


def test_cut_bits_on_planted_rectangles():
    nb = 1000
    words = {'inside': square(400, 400, 100, 50), 'left': square(0, 400, 100, 50), 'top': square(400, 1, 100, 50),
             'right': square(899, 400, 100, 50), 'bottom': square(400, 948, 100, 50), 'near left': square(3, 400, 100, 50),
             'corner': square(0, 0, 999, 999)}
    polys = np.asarray(list(words.values()), np.int32)
    points = np.full((len(words), 2), 450, np.int32)
    names = list(words)
    page = [[300, 300]]
    tiles = {'middle': [100, 100, 200, 200], 'whole page': [0, 0, 300, 300], 'top left': [0, 0, 150, 150], 'bottom right': [150, 150, 300, 300]}

    def bits(tile, edge):
        got = TL.remap_cpu(polys, points, [0, len(words)], [tiles[tile]], [0], page, nb, 1000, edge, True)
        return dict(zip(names, got['cut'].tolist()))
    assert bits('middle', 2) == {'inside': 0, 'left': 1, 'top': 2, 'right': 4, 'bottom': 8, 'near left': 0, 'corner': 15}
    assert bits('middle', 0) == {'inside': 0, 'left': 1, 'top': 0, 'right': 4, 'bottom': 0, 'near left': 0, 'corner': 15}
    assert bits('middle', 3)['near left'] == 1
    assert set(bits('whole page', 2).values()) == {0} and set(bits('whole page', nb).values()) == {0}   # a page-border side never cuts
    assert bits('top left', 2) == {'inside': 0, 'left': 0, 'top': 0, 'right': 4, 'bottom': 8, 'near left': 0, 'corner': 12}
    assert bits('bottom right', 2) == {'inside': 0, 'left': 1, 'top': 2, 'right': 0, 'bottom': 0, 'near left': 0, 'corner': 3}
    assert set(bits('middle', nb).values()) == {15} and set(bits('top left', nb).values()) == {12}    # edge = nb: every inner side cuts
    # the point counts as the word's 17th point
    far = points.copy()
    far[0] = [999, 450]
    assert TL.remap_cpu(polys, far, [0, len(words)], [tiles['middle']], [0], page, nb, 1000, 2, True)['cut'][0] == 4


def test_compaction_is_stable_and_skips_empty_and_refused_tiles():
    nb = 1000
    cutw, keepw = square(0, 400, 100, 50), square(400, 400, 100, 50)
    polys = np.asarray([keepw, cutw, keepw, cutw, cutw, keepw, keepw, keepw], np.int32)
    polys[:, 1] += np.arange(8)                                             # tell the words apart
    points = np.full((8, 2), 450, np.int32)
    rect = [[100, 0, 200, 100], [100, 0, 200, 100], [0, 0, 100, 100], [100, 0, 250, 100], [100, 0, 200, 100], [100, 0, 200, 100]]
    page, size = [0, 0, 1, 1, 5, 2], [[200, 100], [200, 100], [200, 100]]
    rs = [0, 3, 3, 5, 6, 7, 8]                                             # tile 1 is empty; tile 3 leaves its page; tile 4 names no page
    got = TL.remap_cpu(polys, points, rs, rect, page, size, nb, 2000, 2, True)
    assert got['cut'].tolist() == [0, 1, 0, 0, 0, -1, -1, 0]
    assert got['src_row'].tolist() == [0, 2, 3, 4, 7] and got['tile_count'].tolist() == [2, 0, 2, -1, -1, 1]
    assert got['tile_dropped'].tolist() == [1, 0, 0, 0, 0, 0] and got['out_start'].tolist() == [0, 2, 2, 4, 4, 4, 5]
    assert got['page_count'].tolist() == [2, 2, 1]                          # page 2 keeps one word; an empty page would give 0
    assert got['page_polys'].shape == (5, 32) and got['page_points'].shape == (5, 2)
    keep = TL.remap_cpu(polys, points, rs, rect, page, size, nb, 2000, 2, False)
    assert keep['src_row'].tolist() == [0, 1, 2, 3, 4, 7] and keep['tile_count'].tolist() == [3, 0, 2, -1, -1, 1] and (keep['cut'] == got['cut']).all()
    # a row_start that falls refuses the tile it falls in; one that leaves [0, N] too
    fall = TL.remap_cpu(polys, points, [0, 3, 2, 5, 6, 7, 9], rect, [0] * 6, size, nb, 2000, 2, True)
    assert fall['tile_count'].tolist() == [2, -1, 3, -1, 1, -1]                  # tile 2 starts at the page's left border: nothing of it is cut
    empty_page = TL.remap_cpu(polys[:2], points[:2], [0, 2], rect[:1], [1], size, nb, 2000, 2, True)
    assert empty_page['page_count'].tolist() == [0, 1, 0]
    none = TL.remap_cpu(np.zeros((0, 32)), np.zeros((0, 2)), [0, 0], rect[:1], [0], size, nb, 2000, 2, True)
    assert none['page_polys'].shape == (0, 32) and none['tile_count'].tolist() == [0] and none['out_start'].tolist() == [0, 0]
    for bad in (dict(nb=1), dict(nb=4097), dict(page_bins=1), dict(page_bins=4097), dict(edge=-1)):
        kw = dict(nb=1000, page_bins=1000, edge=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            TL.remap_cpu(polys, points, rs, rect, page, size, kw['nb'], kw['page_bins'], kw['edge'], True)
    with pytest.raises(ValueError):
        TL.remap_cpu(polys[:, :30], points, rs, rect, page, size, nb, 1000, 2, True)
    with pytest.raises(RuntimeError):
        TL.TileStage('cpu', 1000)                                           # there is no CPU stage


# -- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_entry_point_matches_the_header():
    from advancedliteratemachinery_amd import _lib, build, ops
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24   # the library only gains an entry point
    m = re.search(r'int omp_tile_remap\((.*?)\);', text, re.S)
    want = []
    for p in (' '.join(p.split()) for p in m.group(1).split(',')):
        if '*' in p or p.startswith('omp_stream_t'):
            want.append(ctypes.c_void_p)
        else:
            assert p.startswith('int '), p
            want.append(ctypes.c_int)
    res, args = _lib._SIGS['omp_tile_remap']
    assert res is ctypes.c_int and args == want and 'omp_tile_remap' in _lib.EXPORTS
    assert 'tiles.hip' in build.SOURCES and callable(ops.tile_remap)
    src = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'tiles.hip')).read()
    assert 'extern "C" int omp_tile_remap(' in src
    assert 'TL_MAX_BINS = %d' % TL.BINS_MAX in src and 'TL_MAX_SIDE = %d' % TL.SIDE_MAX in src and 'TL_ROW = %d' % TL.ROW in src
    assert TL.BINS_MAX == OV.GRID_MAX == RD.GRID_MAX


# -- routing: predict_images / spot_and_recognize with the engine, the preprocessor and the device stages stubbed out -------------------
class _Stub(torch.nn.Module):
    """infer() answering the same three words for every tile: one in the middle, one on the left side, one on the right side"""
    WORDS = (square(400, 400, 100, 50), square(0, 300, 100, 50), square(899, 600, 100, 50))
    POINTS = ((450, 425), (50, 325), (949, 625))
    PROBS = (0.5, 0.9, 0.7)
    calls = []

    def __init__(self, rec_length):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.rec_length = rec_length

    def infer(self, img, mask, seqs, has_padding=None, ragged=False, windows=None, char_windows=None, clip_windows=False):
        type(self).calls.append(dict(n=len(img), ragged=ragged, windows=windows))
        out = []
        for b in range(len(img)):
            W = 1 if windows is None else len(windows[b])
            n = 3 * W
            pt = torch.tensor([self.POINTS[k % 3] for k in range(n)], dtype=torch.long).reshape(1, -1)
            poly = torch.tensor([self.WORDS[k % 3] for k in range(n)], dtype=torch.long).reshape(1, -1)
            probs = torch.tensor([self.PROBS[k % 3] for k in range(n)])[:, None].repeat(1, self.rec_length)
            res = ([pt, poly, torch.full((1, n, self.rec_length), 1000)], [probs])
            out.append(res if windows is None else res + (torch.arange(W).repeat_interleave(3),))
        return out


class _Pre(object):
    """DevicePreprocessor without a device: remembers what it was given"""

    def __init__(self):
        self.seen = []

    def __call__(self, images):
        self.seen.append(list(images))
        return NestedTensor(torch.zeros(len(images), 3, 32, 32), torch.zeros(len(images), 32, 32, dtype=torch.bool)), None


class _HostStage(object):
    """TileStage without a device: the specification behind the same interface, and a log of its calls"""
    calls = []

    def __init__(self, device, nb):
        self.nb = nb

    def run(self, polys, points, row_start, tile_rect, tile_page, page_size, page_bins, edge=2, drop_cut=True):
        res = TL.remap_cpu(torch.as_tensor(polys).numpy(), torch.as_tensor(points).numpy(), row_start, tile_rect, tile_page, page_size, self.nb,
                           page_bins, edge, drop_cut)
        type(self).calls.append(dict(n=len(polys), row_start=np.asarray(row_start).tolist(), rect=np.asarray(tile_rect).tolist(),
                                     page=np.asarray(tile_page).tolist(), size=np.asarray(page_size).tolist(), page_bins=page_bins, edge=edge,
                                     drop_cut=drop_cut, res=res))
        return dict(res, page_polys=torch.from_numpy(res['page_polys']), page_points=torch.from_numpy(res['page_points']))


class _HostSuppressor(object):
    calls = []

    def __init__(self, device, grid):
        self.grid = grid

    def __call__(self, polys, group_start, order=None, t=500, measure='iou'):
        polys = torch.as_tensor(polys).numpy()
        type(self).calls.append(dict(polys=polys.copy(), groups=np.asarray(group_start).tolist(), grid=self.grid))
        return OV.suppress_cpu(polys, group_start, np.arange(len(polys)) if order is None else order, t, measure, self.grid)


class _HostReader(object):
    calls = []

    def __init__(self, device, grid):
        self.grid = grid

    def __call__(self, polys, group_start, aspect, gap=2000, back=500, offset=500):
        polys = torch.as_tensor(polys).numpy()
        type(self).calls.append(dict(polys=polys.copy(), groups=np.asarray(group_start).tolist(), aspect=np.asarray(aspect).tolist(), grid=self.grid))
        return RD.lines_cpu(polys, group_start, aspect, gap, back, offset, self.grid)


PAGES = ((100, 200), (90, 64))      # (h, w)


@pytest.fixture
def stubbed(monkeypatch):
    _Stub.calls, _HostStage.calls, _HostSuppressor.calls, _HostReader.calls = [], [], [], []
    monkeypatch.setattr(TL, 'TileStage', _HostStage)
    monkeypatch.setattr(OV, 'OverlapSuppressor', _HostSuppressor)
    monkeypatch.setattr(RD, 'ReadingOrder', _HostReader)
    a = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    rng = np.random.RandomState(1)
    pages = [torch.from_numpy(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in PAGES]
    return a, _Stub(a.rec_length), pages


def test_without_tile_arguments_nothing_changes(stubbed):
    a, stub, pages = stubbed
    plain, _ = inf.predict_images(stub, pages, a, preprocessor=_Pre())
    assert [len(r) for r in plain] == [3, 3] and all(not {'tile', 'tile_rect', 'tile_cut'} & set(r) for recs in plain for r in recs)
    again, _ = inf.predict_images(stub, pages, a, preprocessor=_Pre(), tiles=None, tile_size=None, tile_overlap=0.3, tile_edge=7, tile_cut='keep',
                                  page_bins=77)
    assert again == plain and _HostStage.calls == []
    assert inf.predict(stub, torch.zeros(2, 3, 32, 32), a) == inf.predict(stub, torch.zeros(2, 3, 32, 32), a, suppress=None)
    for fn in (inf.predict_images, two_stage.spot_and_recognize):
        p = inspect.signature(fn).parameters
        assert p['tiles'].default is None and p['tile_size'].default is None and p['tile_overlap'].default == 0.125
        assert p['tile_edge'].default == 2 and p['tile_cut'].default == 'drop' and p['page_bins'].default is None
    from advancedliteratemachinery_amd.model import omniparser as omp
    for fn in (inf.predict, omp.OmniParser.infer, omp.OmniParser.forward):
        assert not [k for k in inspect.signature(fn).parameters if k.startswith('tile') or k == 'page_bins']


def test_tiled_call_is_one_flow_and_one_stage_call(stubbed):
    a, stub, pages = stubbed
    pre = _Pre()
    got, _ = inf.predict_images(stub, pages, a, preprocessor=pre, ragged=True, tiles=(2, 1), file_names=['a.png', 'b.png'])
    assert len(_Stub.calls) == 1 and _Stub.calls[0]['n'] == 4 and _Stub.calls[0]['ragged'] is True     # ONE flow for all tiles of all pages
    assert len(pre.seen) == 1 and len(_HostStage.calls) == 1                                             # ONE stage call
    call = _HostStage.calls[0]
    rect = np.concatenate([TL.plan_tiles(h, w, 2, 1, 125) for h, w in PAGES]).tolist()
    assert call['rect'] == rect and call['page'] == [0, 0, 1, 1] and call['size'] == [[200, 100], [64, 90]]
    assert call['row_start'] == [0, 3, 6, 9, 12] and call['n'] == 12 and call['edge'] == 2 and call['drop_cut'] is True
    assert call['page_bins'] == 2000                                                                     # min(4096, num_bins max(nx, ny))
    # the tiles are VIEWS of the page images
    for view, (x0, y0, x1, y1), p in zip(pre.seen[0], rect, call['page']):
        assert tuple(view.shape) == (y1 - y0, x1 - x0, 3) and view.data_ptr() == pages[p][y0:y1, x0:x1].data_ptr()
        assert view.stride(0) == pages[p].stride(0) and torch.equal(view, pages[p][y0:y1, x0:x1])
    # left tiles lose the word on their right (inner) side, right tiles the one on their left side; the page borders cut nothing
    assert call['res']['cut'].tolist() == [0, 0, 4, 0, 1, 0] * 2
    for p, recs in enumerate(got):
        assert [(r['tile'], r['tile_cut']) for r in recs] == [(0, 0), (0, 0), (1, 0), (1, 0)]
        assert [r['tile_rect'] for r in recs] == [rect[2 * p]] * 2 + [rect[2 * p + 1]] * 2
        assert all(r['image_id'] == ('a.png', 'b.png')[p] for r in recs)
        # pts / polys: decode_pred_seq's values for the tile's own size, plus the tile's origin
        for r, word in zip(recs, (0, 1, 0, 2)):
            x0, y0, x1, y1 = r['tile_rect']
            seqs = [torch.tensor(_Stub.POINTS[word]), torch.tensor(_Stub.WORDS[word]), torch.full((a.rec_length,), 1000)]
            one = inf.decode_pred_seq(seqs, torch.full((1, a.rec_length), _Stub.PROBS[word]), {'file_name': 'x', 'orig_size': (y1 - y0, x1 - x0)}, a)[0]
            assert r['pts'] == [[one['pts'][0][0] + x0, one['pts'][0][1] + y0]]
            assert r['polys'] == [[q[0] + x0, q[1] + y0] for q in one['polys']]
            assert r['pts'][0][0] == pytest.approx(x0 + _Stub.POINTS[word][0] / 1000 * (x1 - x0), rel=1e-6)
            assert r['score'] == one['score'] and r['rec'] == one['rec']
    keep, _ = inf.predict_images(stub, pages, a, preprocessor=_Pre(), tiles=(2, 1), tile_cut='keep', tile_edge=0, page_bins=512, tile_overlap=0)
    assert _HostStage.calls[-1]['drop_cut'] is False and _HostStage.calls[-1]['edge'] == 0 and _HostStage.calls[-1]['page_bins'] == 512
    assert _HostStage.calls[-1]['rect'][:2] == [[0, 0, 100, 100], [100, 0, 200, 100]] and _Stub.calls[-1]['ragged'] is False
    assert [[r['tile_cut'] for r in recs] for recs in keep] == [[0, 0, 4, 0, 1, 0]] * 2
    size, _ = inf.predict_images(stub, pages, a, preprocessor=_Pre(), tile_size=64)
    assert _HostStage.calls[-1]['page'] == [0] * 8 + [1] * 2 and _HostStage.calls[-1]['page_bins'] == 4000   # 4 x 2 and 1 x 2 tiles
    assert [len(r) for r in size] == [sum(c for c in _HostStage.calls[-1]['res']['tile_count'][:8]), sum(_HostStage.calls[-1]['res']['tile_count'][8:])]


def test_identity_tiling_returns_the_plain_records(stubbed):
    a, stub, pages = stubbed
    plain, _ = inf.predict_images(stub, pages, a, preprocessor=_Pre())
    got, _ = inf.predict_images(stub, pages, a, preprocessor=_Pre(), tiles=(1, 1), tile_overlap=0, page_bins=a.num_bins)
    strip = [[{k: v for k, v in r.items() if k not in ('tile', 'tile_rect', 'tile_cut')} for r in recs] for recs in got]
    assert strip == plain
    assert [[(r['tile'], r['tile_rect'], r['tile_cut']) for r in recs] for recs in got] == [[(0, [0, 0, w, h], 0)] * 3 for h, w in PAGES]
    res = _HostStage.calls[-1]['res']
    assert (res['page_polys'] == np.asarray(_Stub.WORDS * 2)).all()


def test_the_page_stages_receive_page_polygons_page_bins_and_page_sizes(stubbed):
    a, stub, pages = stubbed
    got, _ = inf.predict_images(stub, pages, a, preprocessor=_Pre(), tiles=(2, 1), suppress=0.5, reading_order=True)
    res = _HostStage.calls[-1]['res']
    for calls in (_HostSuppressor.calls, _HostReader.calls):
        assert len(calls) == 1 and calls[0]['grid'] == 2000 and calls[0]['groups'] == [0, 4, 8]          # one group per PAGE, at page_bins
        assert (calls[0]['polys'] == res['page_polys']).all()
    assert _HostReader.calls[0]['aspect'] == [list(RD.aspect_of(h, w)) for h, w in PAGES]
    line, = [RD.lines_cpu(res['page_polys'], [0, 4, 8], _HostReader.calls[0]['aspect'], 2000, 500, 500, 2000)]
    flat = [r for recs in got for r in recs]
    assert sorted((r['line'], r['line_pos']) for r in flat[:4]) == sorted(zip(line['line'][:4].tolist(), line['line_pos'][:4].tolist()))
    assert all(r['merged'] == [] for r in flat) and len(flat) == 8
    # `merged` counts the PAGE's records after the tile stage (here: two windows answering the same three words)
    wide, _ = inf.predict_images(stub, pages[:1], a, preprocessor=_Pre(), tiles=(1, 1), suppress=0.5, windows=[[0, 0, 999, 999], [0, 0, 999, 999]])
    assert [r['merged'] for r in wide[0]] == [[(1, 3)], [(1, 4)], [(1, 5)]]                             # indices count the page's records


def test_entry_points_refuse(stubbed):
    a, stub, pages = stubbed
    bad = (dict(tiles=(2, 2), tile_size=64), dict(tiles=(0, 1)), dict(tiles=(2,)), dict(tile_size=0), dict(tiles=(2, 1), tile_overlap=0.6),
           dict(tiles=(2, 1), tile_overlap=-0.1), dict(tiles=(2, 1), tile_cut='merge'), dict(tiles=(2, 1), tile_edge=-1),
           dict(tiles=(2, 1), tile_edge=1.5), dict(tiles=(2, 1), page_bins=1), dict(tiles=(2, 1), page_bins=5000),
           dict(tiles=(2, 1), windows=[[[0, 0, 999, 999]], [[0, 0, 999, 999]]]),                          # per-image windows
           dict(tiles=(40, 1)), dict(tiles=(20, 20)))                                                     # cores below 8 pixels; too many tiles
    for kw in bad:
        with pytest.raises(ValueError):
            inf.predict_images(stub, pages, a, preprocessor=_Pre(), **kw)
        with pytest.raises(ValueError):
            two_stage.spot_and_recognize(stub, None, pages, a, preprocessor=_Pre(), **kw)
    assert _Stub.calls == [] and _HostStage.calls == []                                                   # refused ahead of any work
    kie = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, infer_vie=True, vie_categories=4, val_dataset=['sroie_val'])
    for call in (lambda: inf.predict_images(stub, pages, kie, preprocessor=_Pre(), tiles=(2, 1)),
                 lambda: inf.predict_images(stub, [], kie, tile_size=64),
                 lambda: two_stage.spot_and_recognize(stub, None, pages, kie, tiles=(2, 1))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        inf.predict(stub, torch.zeros(1, 3, 32, 32), a, tiles=(2, 1))                                     # predict is unchanged
    # the shared form of windows= composes
    got, _ = inf.predict_images(stub, pages, a, preprocessor=_Pre(), tiles=(2, 1), grid=(2, 1))
    assert _Stub.calls[-1]['n'] == 4 and len(_Stub.calls[-1]['windows']) == 4 and all(len(w) == 2 for w in _Stub.calls[-1]['windows'])
    assert all({'window', 'window_bins', 'tile'} <= set(r) for recs in got for r in recs)


def test_tile_records_on_empty_tiles():
    recs = [[], [dict(pts=[[1.0, 2.0]], polys=[[1.0, 2.0]] * 16, image_id='0', score=1.0, rec='a')], []]
    res = dict(cut=np.asarray([0]), src_row=np.asarray([0]), out_start=np.asarray([0, 0, 1, 1]))
    out = TL.tile_records(copy.deepcopy(recs), res, [[0, 0, 10, 10], [10, 0, 20, 10], [0, 0, 20, 10]], [0, 0, 1], 3, ['p', 'q', 'r'])
    assert out[1] == [] and out[2] == [] and len(out[0]) == 1
    assert out[0][0] == dict(pts=[[11.0, 2.0]], polys=[[11.0, 2.0]] * 16, image_id='p', score=1.0, rec='a', tile=1, tile_rect=[10, 0, 20, 10], tile_cut=0)
