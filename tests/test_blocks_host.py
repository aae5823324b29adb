"""Blocks on the host (no GPU): the numpy specification blocks_cpu (utils/reading.py) on column pages, a nested
page, the strictness of the gap rule, a spanning line, degenerate inputs and the integer extremes; against an independent recursive
XY-cut (tests/blocks_cases.py) on seeded random pages; every refusal; the header; how predict routes `blocks=` (the device stage
replaced by its specification); page_blocks.  The kernel and the end-to-end answers are tests/test_gpu_blocks.py."""
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
from advancedliteratemachinery_amd.utils.parser import make_args
from tests import blocks_cases as BC
from tests import reading_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 1000
OUTS = ('block', 'line', 'rank', 'n_blocks', 'levels')


def alone(polys, aspect=((1, 1),), grid=GRID, **kw):
    """every word its own line, numbered as given: blocks_cpu without the linker"""
    n = len(polys)
    return RD.blocks_cpu(polys, [0, n], aspect, np.arange(n), np.zeros(n, np.int32), [n], grid=grid, **kw)


def reading(names, res, key='rank'):
    """the names of the words in the order `res` reads them"""
    return [names[i] for i in np.argsort(res[key])]


# -- pages -------------------------------------------------------------------------------------------------------------------------
def test_two_columns_under_a_headline_read_column_by_column():
    pts, names = BC.column_page(cols=2, rows=5, words=2)
    order = np.random.RandomState(3).permutation(len(pts))
    polys, names = RC.to_bins(pts[order]), [names[i] for i in order]
    lines, res = BC.blocks_of(polys)
    want = [('head',)] + [('col', c, r, k) for c in range(2) for r in range(5) for k in range(2)] + [('foot',)]
    assert reading(names, res) == want                                       # headline, all left lines, all right lines, footer
    assert res['n_blocks'].tolist() == [4] and res['levels'].tolist() == [4]  # y, x, then two levels that cut nothing
    by_name = dict(zip(names, range(len(names))))
    assert [int(res['block'][by_name[n]]) for n in want] == [0] + [1] * 10 + [2] * 10 + [3]
    assert [int(res['line'][by_name[n]]) for n in want] == [0] + [1 + l for l in range(10) for _ in range(2)] + [11]
    assert all(v.dtype == np.int32 for v in res.values())
    # the page is a real case: the lines alone interleave the columns
    assert lines['n_lines'].tolist() == [12]
    assert reading(names, lines) == [('head',)] + [('col', c, r, k) for r in range(5) for c in range(2) for k in range(2)] + [('foot',)]


def test_three_columns():
    pts, names = BC.column_page(cols=3, rows=4, words=2, headline=False, footer=False)
    order = np.random.RandomState(8).permutation(len(pts))
    polys, names = RC.to_bins(pts[order]), [names[i] for i in order]
    lines, res = BC.blocks_of(polys)
    assert reading(names, res) == [('col', c, r, k) for c in range(3) for r in range(4) for k in range(2)]
    assert res['n_blocks'].tolist() == [3] and res['levels'].tolist() == [4]  # y cuts nothing, x cuts, y and x cut nothing
    assert reading(names, lines) == [('col', c, r, k) for r in range(4) for c in range(3) for k in range(2)]


def test_nesting_needs_four_levels_and_block_depth_truncates():
    pts, labels = BC.nested_page()
    order = np.random.RandomState(2).permutation(len(pts))
    polys, labels = RC.to_bins(pts[order]), [labels[i] for i in order]
    full = ['head'] + ['left'] * 8 + ['upper'] * 3 + ['sub0'] * 3 + ['sub1'] * 3
    cut2 = ['head'] + ['left'] * 8 + ['upper'] * 3 + ['sub0', 'sub1'] * 3     # depth 2: band, columns -- the right column stays whole
    cut3 = ['head'] + ['left'] * 8 + ['upper'] * 3 + ['sub0', 'sub1'] * 3     # depth 3: upper | lower are blocks, the sub-columns are not
    for depth, want, n_blocks, levels in ((8, full, 5, 6), (4, full, 5, 4), (16, full, 5, 6), (2, cut2, 3, 2), (3, cut3, 4, 3), (1, None, 2, 1)):
        _, res = BC.blocks_of(polys, depth=depth)
        assert (res['n_blocks'].tolist(), res['levels'].tolist()) == ([n_blocks], [levels]), depth
        if want is not None:
            assert reading(labels, res) == want, depth
        y = polys[np.argsort(res['rank'])][:, 1]
        for name in set(labels):                                              # inside a region the lines still run top to bottom
            assert (np.diff([v for v, l in zip(y, reading(labels, res)) if l == name]) > 0).all()
    _, res = BC.blocks_of(polys, depth=2)
    assert [int(b) for b in res['block'][np.argsort(res['rank'])]] == [0] + [1] * 8 + [2] * 9


def test_the_gap_rule_is_strict():
    w = lambda x, y, ww=60, h=20: RC.word(x, y, ww, h)                        # noqa: E731
    # x: heights 20 and 20, block_gap_x = 1.0: the threshold is 20 bins (aspect 1: a bin is a unit)
    for gap, n in ((20, 1), (21, 2), (0, 1), (19, 1)):
        assert alone(RC.to_bins(np.stack([w(100, 100), w(160 + gap, 100)])))['n_blocks'].tolist() == [n], gap
    # heights 20 and 10: the mean is 15
    for gap, n in ((15, 1), (16, 2)):
        assert alone(RC.to_bins(np.stack([w(100, 100), w(160 + gap, 100, h=10)])))['n_blocks'].tolist() == [n], gap
    # y: block_gap_y = 1.5: 30 bins
    for gap, n in ((30, 1), (31, 2)):
        assert alone(RC.to_bins(np.stack([w(100, 100), w(100, 120 + gap)])))['n_blocks'].tolist() == [n], gap
    # gap = 0: any positive raw gap cuts, touching boxes do not
    for gap, n in ((0, 1), (1, 2)):
        assert alone(RC.to_bins(np.stack([w(100, 100), w(160 + gap, 100)])), gap_x=0, gap_y=0)['n_blocks'].tolist() == [n]
        assert alone(RC.to_bins(np.stack([w(100, 100), w(100, 120 + gap)])), gap_x=0, gap_y=0)['n_blocks'].tolist() == [n]
    # anisotropic bins: x bins half as wide halve the raw gap, the heights (along y) stay
    p = RC.to_bins(np.stack([w(100, 100), w(200, 100)]))                      # 40 bins apart: 2 heights under (256, 256), 1 under (128, 256)
    assert alone(p, aspect=[[256, 256]])['n_blocks'].tolist() == [2] and alone(p, aspect=[[128, 256]])['n_blocks'].tolist() == [1]
    assert alone(p, aspect=[[128, 256]], gap_x=999)['n_blocks'].tolist() == [2]


def test_a_line_that_spans_the_gutter_holds_the_columns_together():
    pts, names = BC.column_page(cols=2, rows=5, words=2, headline=False, footer=False)
    _, res = BC.blocks_of(RC.to_bins(pts))
    assert res['n_blocks'].tolist() == [2]
    keep = [i for i, n in enumerate(names) if n[2] != 2]                      # row 2 of both columns becomes one wide line
    span = np.concatenate([pts[keep], RC.word(100, 120 + 2 * 34, 2 * 132 + 80, 20)[None]])
    lines, res = BC.blocks_of(RC.to_bins(span))
    assert res['n_blocks'].tolist() == [1] and res['levels'].tolist() == [2]
    assert (res['rank'] == lines['rank']).all() and (res['line'] == lines['line']).all() and (res['block'] == 0).all()
    # a line is never cut: words far apart that are GIVEN as one line stay in one block
    far = RC.to_bins(np.stack([RC.word(100, 100, 60, 20), RC.word(700, 100, 60, 20), RC.word(100, 134, 60, 20), RC.word(700, 134, 60, 20)]))
    res = RD.blocks_cpu(far, [0, 4], [[1, 1]], [0, 0, 1, 2], [0, 1, 0, 0], [3], grid=GRID)
    assert res['n_blocks'].tolist() == [1]
    assert RD.blocks_cpu(far, [0, 4], [[1, 1]], [0, 1, 2, 3], [0, 0, 0, 0], [4], grid=GRID)['n_blocks'].tolist() == [2]


def test_degenerate_inputs():
    one = RC.to_bins(RC.word(100, 100, 60, 20)[None])
    for depth, levels in ((8, 2), (2, 2), (1, 1)):
        res = alone(one, depth=depth)
        assert [res[k].tolist() for k in OUTS] == [[0], [0], [0], [1], [levels]]
    _, res = BC.blocks_of(RC.to_bins(np.stack(BC.line_words(100, 100, 5))))  # one line of five words
    assert res['n_blocks'].tolist() == [1] and res['line'].tolist() == [0] * 5 and res['rank'].tolist() == list(range(5))
    # 40 groups, some empty, one page each
    rng = np.random.RandomState(7)
    sizes = [0 if g in (0, 3, 4, 17, 39) else int(rng.randint(1, 12)) for g in range(40)]
    parts = [BC.random_lines_page(rng, n, GRID) for n in sizes if n]
    polys = np.concatenate([p[0] for p in parts])
    line, pos = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    gs = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])])
    gs = np.asarray([0] + [int(gs[sum(1 for m in sizes[:g + 1] if m)]) for g in range(40)])
    asp = [[256, 200]] * 40
    res = RD.blocks_cpu(polys, gs, asp, line, pos, sizes, grid=GRID)
    ref = BC.xy_cut_reference(polys, gs, asp, line, pos, sizes, grid=GRID)
    assert all((res[k] == ref[k]).all() for k in OUTS)
    for g, n in enumerate(sizes):
        if n == 0:
            assert res['n_blocks'][g] == 0 and res['levels'][g] == 0
        else:
            assert sorted(res['rank'][gs[g]:gs[g + 1]].tolist()) == list(range(gs[g + 1] - gs[g])) and 1 <= res['n_blocks'][g] <= n
    # all-degenerate polygons: points have no height, so any distance is a gap; equal points never part
    dots = np.asarray([[x, y] * 16 for x, y in ((5, 5), (5, 5), (6, 5), (5, 6), (900, 5))], dtype=np.int32)
    res = alone(dots)
    assert res['n_blocks'].tolist() == [4] and res['block'].tolist() == [0, 0, 1, 3, 2]    # band y = 5: x = 5, 5 | 6 | 900; band y = 6
    assert all((res[k] == BC.xy_cut_reference(dots, [0, 5], [[1, 1]], np.arange(5), np.zeros(5), [5], grid=GRID)[k]).all() for k in OUTS)
    res = RD.blocks_cpu(np.zeros((0, 32), np.int32), [0, 0, 0], [[1, 1], [2, 2]], [], [], [0, 0], grid=GRID)
    assert res['n_blocks'].tolist() == [0, 0] and res['levels'].tolist() == [0, 0] and res['rank'].size == 0


def test_extremes_keep_the_bounds():
    g = OV.GRID_MAX
    far = [0, 0] * 8 + [g - 1, g - 1] * 8                                    # the largest thickness vector there is
    p = np.asarray([far, far[::-1], [g - 1, 0] * 16, [0, g - 1] * 16, RC.to_bins(RC.word(0, 0, g - 1, g - 1)[None])[0]], dtype=np.int32)
    for asp in ([[256, 256]], [[256, 1]], [[1, 256]]):
        for v in (0, 10000):
            for depth in (1, 16):
                res = alone(p, aspect=asp, grid=g, gap_x=v, gap_y=v, depth=depth)      # the assertions inside hold
                assert sorted(res['rank'].tolist()) == list(range(len(p)))
    ends = RD.intervals_cpu(p, np.repeat([[256, 256]], len(p), 0), 10000, 10000)
    big = max(int(np.abs(e).max()) for e in ends)
    assert big == 16000 * 4095 * 256 + 10000 * 8 * 4095 * 256 < 2 ** 37       # the largest end there is; the specification asserts 2^38
    with pytest.raises(AssertionError):
        RD.intervals_cpu(np.full((1, 32), g), [[256, 256]], 1000, 1000)
    with pytest.raises(AssertionError):
        RD.intervals_cpu(np.zeros((1, 32)), [[257, 1]], 1000, 1000)


# -- against the independent recursion -------------------------------------------------------------------------------------------------
def test_blocks_cpu_equals_the_recursive_xy_cut_on_random_pages():
    rng = np.random.RandomState(19)
    sizes = [1, 2, 3, 299, 300] + [int(np.exp(rng.uniform(0, np.log(300)))) for _ in range(195)]
    aspects = ([256, 256], [256, 128], [37, 256], [1, 1])
    gaps = ((1000, 1500), (0, 0), (10000, 10000), (300, 200), (2500, 700))
    seen_blocks, seen_levels = set(), set()
    for t, n in enumerate(sizes):
        grid = (1000, 4096, 64)[t % 3]
        polys, line, pos = BC.random_lines_page(rng, n, grid)
        gs, asp = [0, len(polys)], [aspects[t % 4]]
        gx, gy = gaps[t % 5]
        for depth in (1, 2, 3, 8, 16):
            got = RD.blocks_cpu(polys, gs, asp, line, pos, [n], gx, gy, depth, grid)
            ref = BC.xy_cut_reference(polys, gs, asp, line, pos, [n], gx, gy, depth, grid)
            for k in OUTS:
                assert (got[k] == ref[k]).all(), (t, n, depth, k)
            assert sorted(got['rank'].tolist()) == list(range(len(polys))) and got['levels'][0] <= depth
            seen_blocks.add(int(got['n_blocks'][0]))
            seen_levels.add(int(got['levels'][0]))
    assert len(seen_blocks) > 20 and seen_levels >= {1, 2, 3, 4, 5, 6}        # the pages do nest


# -- refusals -----------------------------------------------------------------------------------------------------------------------
def test_specification_refusals():
    p = RC.to_bins(np.stack(BC.line_words(100, 100, 2)))
    for bad in (dict(gap_x=-1), dict(gap_x=10001), dict(gap_y=10001), dict(gap_y=0.5), dict(depth=0), dict(depth=17), dict(depth=2.5),
                dict(depth=True), dict(grid=4097)):
        with pytest.raises(ValueError):
            alone(p, **bad)
    for line, pos, n in (([0, 2], [0, 0], [2]), ([0, 0], [0, 1], [2]), ([0, -1], [0, 0], [2]), ([0], [0], [1]), ([0, 1], [0, 0], [2, 0])):
        with pytest.raises(ValueError):
            RD.blocks_cpu(p, [0, 2], [[1, 1]], line, pos, n, grid=GRID)
    assert RD.check_block_args(False, -5, 'x', 99) is None                     # without blocks nothing is looked at
    assert RD.check_block_args(True) == (1000, 1500, 8) == tuple(RD.BLOCK_DEFAULTS[k] for k in ('gap_x', 'gap_y', 'depth'))
    assert RD.check_block_args(True, 0, 10, 16) == (0, 10000, 16)
    for kw in (dict(block_gap_x=-0.1), dict(block_gap_x=10.5), dict(block_gap_y=11), dict(block_gap_y=float('nan')), dict(block_depth=0),
               dict(block_depth=17), dict(block_depth=1.5), dict(reading_order=False), dict(infer_vie=True)):
        with pytest.raises(ValueError):
            RD.check_block_args(True, **kw)
        if 'reading_order' not in kw and 'infer_vie' not in kw:
            with pytest.raises(ValueError):
                RD.check_reading_args(blocks=True, **kw)
    assert RD.check_reading_args(blocks=True) == (2000, 500, 500) == RD.check_reading_args()


def test_entry_point_matches_the_header():
    from advancedliteratemachinery_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24   # the library only gains an entry point
    m = re.search(r'int omp_reading_blocks\((.*?)\);', text, re.S)
    want = []
    for p in (' '.join(p.split()) for p in m.group(1).split(',')):
        if '*' in p or p.startswith('omp_stream_t'):
            want.append(ctypes.c_void_p)
        else:
            assert p.startswith('int '), p
            want.append(ctypes.c_int)
    res, args = _lib._SIGS['omp_reading_blocks']
    assert res is ctypes.c_int and args == want and 'omp_reading_blocks' in _lib.EXPORTS
    assert 'blocks_cpu' in text[text.index('Blocks: a recursive XY-cut'):m.start()]           # the declaration names what it stands for
    src = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'reading.hip')).read()
    assert 'RB_MAX_DEPTH = %d' % RD.DEPTH_MAX in src and 'extern "C" int omp_reading_blocks(' in src
    kernel = src[src.index('constexpr int RB_MIN_SLOTS'):src.index('extern "C" int omp_reading_links')]
    assert kernel.count('__shared__') == kernel.count('extern __shared__') == 1                # dynamic LDS only: omp_raise_lds needs that
    assert 'asm' not in kernel


# -- routing: predict / predict_images / spot_and_recognize with the engine and the device stages stubbed out ------------------------
def _w(x, y):
    return RC.to_bins(RC.word(x, y, 60, 20)[None])[0].tolist()


class _Stub(torch.nn.Module):
    """infer() answering the same five words under every window: two columns of two single-word lines, out of order, and a
    near-duplicate of word 1.  R1, L0, L0', R0, L1"""
    WORDS = (_w(300, 134), _w(100, 100), _w(100, 102), _w(300, 100), _w(100, 134))
    PROBS = (0.5, 0.9, 0.7, 0.6, 0.8)

    def __init__(self, rec_length):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.rec_length = rec_length

    def infer(self, img, mask, seqs, has_padding=None, ragged=False, windows=None, char_windows=None, clip_windows=False):
        out = []
        for b in range(len(img)):
            pt = torch.arange(10).reshape(1, -1)
            poly = torch.tensor(self.WORDS, dtype=torch.long).reshape(1, -1)
            probs = torch.tensor(self.PROBS)[:, None].repeat(1, self.rec_length)
            out.append(([pt, poly, torch.full((1, 5, self.rec_length), 1000)], [probs]))
        return out


class _HostSuppressor(object):
    def __init__(self, device, grid):
        self.grid = grid

    def __call__(self, polys, group_start, order=None, t=500, measure='iou'):
        polys = torch.as_tensor(polys).numpy()
        return OV.suppress_cpu(polys, group_start, np.arange(len(polys)) if order is None else order, t, measure, self.grid)


class _HostReader(object):
    """ReadingOrder without a device: the two specifications behind the same interface, and a log of its calls"""
    calls = []

    def __init__(self, device, grid):
        self.grid = grid

    def __call__(self, polys, group_start, aspect, gap=2000, back=500, offset=500, blocks=None):
        polys = torch.as_tensor(polys).numpy()
        type(self).calls.append(dict(polys=polys.tolist(), groups=np.asarray(group_start).tolist(), aspect=np.asarray(aspect).tolist(),
                                     params=(gap, back, offset), blocks=blocks))
        res = RD.lines_cpu(polys, group_start, aspect, gap, back, offset, self.grid)
        if blocks is not None:
            res['blocks'] = RD.blocks_cpu(polys, group_start, aspect, res['line'], res['line_pos'], res['n_lines'], *blocks, grid=self.grid)
        return res


@pytest.fixture
def stubbed(monkeypatch):
    _HostReader.calls = []
    monkeypatch.setattr(OV, 'OverlapSuppressor', _HostSuppressor)
    monkeypatch.setattr(RD, 'ReadingOrder', _HostReader)
    a = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    return a, _Stub(a.rec_length), torch.zeros(2, 3, 32, 64)


def _minus(r, keys=('line', 'line_pos', 'block')):
    return {k: v for k, v in r.items() if k not in keys}


def test_predict_without_blocks_is_unchanged(stubbed):
    a, stub, imgs = stubbed
    plain = inf.predict(stub, imgs, a, reading_order=True)
    assert all('block' not in r for recs in plain for r in recs)
    assert inf.predict(stub, imgs, a, reading_order=True, blocks=False, block_gap_x=9.0, block_gap_y=-3, block_depth=99) == plain
    assert [c['blocks'] for c in _HostReader.calls] == [None, None]           # the reader is called as before: no new code runs
    for recs in plain:                                                        # the lines alone interleave the stub's columns
        assert [r['polys'] for r in recs] == [inf.predict(stub, imgs, a)[0][i]['polys'] for i in (1, 3, 2, 4, 0)]
    for fn in (inf.predict, inf.predict_images, two_stage.spot_and_recognize):
        p = inspect.signature(fn).parameters
        assert p['blocks'].default is False
        assert (p['block_gap_x'].default, p['block_gap_y'].default, p['block_depth'].default) == (1.0, 1.5, 8)


def test_predict_blocks_reorders_in_one_call(stubbed):
    a, stub, imgs = stubbed
    plain = inf.predict(stub, imgs, a)
    got = inf.predict(stub, imgs, a, reading_order=True, blocks=True)
    assert len(_HostReader.calls) == 1                                        # both images, lines and blocks, in ONE call
    c = _HostReader.calls[0]
    assert c['groups'] == [0, 5, 10] and c['blocks'] == (1000, 1500, 8) and c['polys'] == [list(w) for w in _Stub.WORDS] * 2
    assert c['aspect'] == [[256, 128]] * 2
    for recs, before in zip(got, plain):
        assert [_minus(r) for r in recs] == [before[i] for i in (1, 2, 4, 3, 0)]          # the left column with the duplicate, then the right
        assert [(r['block'], r['line'], r['line_pos']) for r in recs] == [(0, 0, 0), (0, 1, 0), (0, 2, 0), (1, 3, 0), (1, 4, 0)]
    assert RD.page_lines(got[0], field='block') == ['0', '0', '0', '1', '1']  # page_lines works on the result as it is
    assert RD.page_blocks(got[0], field='line') == ['0\n1\n2', '3\n4']
    got = inf.predict(stub, imgs, a, reading_order=True, blocks=True, block_gap_x=4.0, block_gap_y=0.5, block_depth=3)
    assert _HostReader.calls[-1]['blocks'] == (4000, 500, 3)
    # rows 12 bins apart against half a height of 20: bands first now, the columns inside each band; the duplicate 2 bins under word 1
    # stays with it
    assert [[(r['block'], r['line']) for r in recs] for recs in got] == [[(0, 0), (0, 1), (1, 2), (2, 3), (3, 4)]] * 2
    assert [_minus(r) for r in got[0]] == [plain[0][i] for i in (1, 2, 3, 4, 0)]
    assert inf.predict(stub, [imgs[0], imgs[1]], a, ragged=True, reading_order=True, blocks=True, block_gap_x=4.0, block_gap_y=0.5, block_depth=3) == got


def test_predict_blocks_run_on_the_survivors_rows(stubbed):
    a, stub, imgs = stubbed
    plain = inf.predict(stub, imgs, a, suppress=0.5)
    assert [[r['merged'] for r in recs] for recs in plain] == [[[], [2], [], []]] * 2
    got = inf.predict(stub, imgs, a, suppress=0.5, reading_order=True, blocks=True)
    c = _HostReader.calls[-1]
    assert c['groups'] == [0, 4, 8] and c['polys'] == [list(_Stub.WORDS[i]) for i in (0, 1, 3, 4)] * 2   # rows of the survivors only
    for recs, before in zip(got, plain):
        assert [_minus(r) for r in recs] == [before[i] for i in (1, 3, 2, 0)]
        assert [(r['block'], r['line'], r['line_pos']) for r in recs] == [(0, 0, 0), (0, 1, 0), (1, 2, 0), (1, 3, 0)]
        assert recs[0]['merged'] == [2]


def test_entry_points_refuse(stubbed):
    a, stub, imgs = stubbed
    bad = (dict(block_gap_x=-0.1), dict(block_gap_x=10.5), dict(block_gap_y=-1), dict(block_gap_y=11), dict(block_depth=0), dict(block_depth=17),
           dict(block_depth=2.5))
    for kw in bad:
        with pytest.raises(ValueError):
            inf.predict(stub, imgs, a, reading_order=True, blocks=True, **kw)
        with pytest.raises(ValueError):
            inf.predict_images(stub, [], a, reading_order=True, blocks=True, **kw)
        with pytest.raises(ValueError):
            two_stage.spot_and_recognize(stub, None, [], a, reading_order=True, blocks=True, **kw)
    for call in (lambda: inf.predict(stub, imgs, a, blocks=True), lambda: inf.predict_images(stub, [], a, blocks=True),
                 lambda: two_stage.spot_and_recognize(stub, None, [], a, blocks=True)):
        with pytest.raises(ValueError, match='reading_order'):                 # blocks=True needs reading_order=True
            call()
    kie = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, infer_vie=True, vie_categories=4, val_dataset=['sroie_val'])
    for call in (lambda: inf.predict(stub, imgs, kie, reading_order=True, blocks=True), lambda: inf.predict_images(stub, [], kie, reading_order=True, blocks=True),
                 lambda: two_stage.spot_and_recognize(stub, None, [], kie, reading_order=True, blocks=True)):
        with pytest.raises(ValueError):
            call()
    assert _HostReader.calls == []


def test_page_blocks():
    recs = [dict(rec='Head', line=0, block=0), dict(rec='left', line=1, block=1), dict(rec='one', line=1, block=1), dict(rec='two', line=2, block=1),
            dict(rec='right', line=3, block=2, mgp_text='RIGHT')]
    assert RD.page_blocks(recs) == ['Head', 'left one\ntwo', 'right']
    assert RD.page_blocks(recs, sep='_', line_sep=' / ') == ['Head', 'left_one / two', 'right']
    assert RD.page_blocks(recs[4:], field='mgp_text') == ['RIGHT'] and RD.page_blocks([]) == []
    assert RD.page_lines(recs) == ['Head', 'left one', 'two', 'right']
