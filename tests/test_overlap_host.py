"""Overlap suppression on the host (no GPU): the numpy specification (utils/overlap.py) on hand-built polygons, against an independent
per-sample loop on seeded random polygons, the greedy pass and its orders, the bitmask layout, how predict / predict_images /
spot_and_recognize route `suppress=` (the device stage replaced by its specification), what they refuse, and that nothing changes
without the argument.  The kernels and the end-to-end answers are tests/test_gpu_overlap.py."""
import copy
import ctypes
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from advancedliteratemachinery_amd.engine import inference as inf
from advancedliteratemachinery_amd.engine import two_stage
from advancedliteratemachinery_amd.utils import overlap as OV
from advancedliteratemachinery_amd.utils import windows as WN
from advancedliteratemachinery_amd.utils.parser import make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 1000


def poly16(points):
    """up to 16 (x, y) points -> one [32] row, the last point repeated (repeated points add edges of length 0)"""
    pts = list(points) + [points[-1]] * (16 - len(points))
    return [c for p in pts for c in p]


def square(x, y, w, h=None):
    h = w if h is None else h
    return poly16([(x, y), (x + w, y), (x + w, y + h), (x, y + h)])


def P(*rows):
    return np.asarray(rows, dtype=np.int32)


def inter_of(a, b, grid=GRID):
    return OV.pair_overlap_cpu(P(a, b), [0, 2], grid)[0]


# -- coverage and intersections on hand-built polygons ----------------------------------------------------------------------------------
def test_identical_shifted_disjoint_and_touching_squares():
    assert OV.coverage_cpu(P(square(20, 30, 10)), GRID).tolist() == [100]
    assert inter_of(square(20, 30, 10), square(20, 30, 10)).tolist() == [[100, 100], [100, 100]]
    assert inter_of(square(20, 30, 10), square(25, 30, 10)).tolist() == [[100, 50], [50, 100]]
    assert inter_of(square(20, 30, 10), square(23, 34, 10))[0, 1] == 7 * 6
    assert inter_of(square(20, 30, 10), square(50, 30, 10))[0, 1] == 0
    assert inter_of(square(20, 30, 10), square(30, 30, 10))[0, 1] == 0      # they share the edge x = 30
    assert inter_of(square(20, 30, 10), square(30, 40, 10))[0, 1] == 0      # they share one corner
    # the winding direction and the starting point do not matter
    sq = [(20, 30), (30, 30), (30, 40), (20, 40)]
    for pts in (sq[::-1], sq[2:] + sq[:2]):
        assert OV.coverage_cpu(P(poly16(pts)), GRID).tolist() == [100]


def test_u_shape_and_a_bar_through_its_gap():
    u = poly16([(0, 0), (30, 0), (30, 30), (20, 30), (20, 10), (10, 10), (10, 30), (0, 30)])
    bar = square(12, 15, 6, 13)
    m = inter_of(u, bar)
    assert m.tolist() == [[700, 0], [0, 78]]                                # the boxes overlap, the shapes do not
    assert inter_of(u, square(5, 5, 20, 20))[0, 1] == 400 - 10 * 15         # the part of the square inside the gap is not the U's
    owner, area = OV.suppress_cpu(P(u, bar), [0, 2], [0, 1], 1, 'iomin', GRID)
    assert owner.tolist() == [0, 1] and area.tolist() == [700, 78]


def test_bow_tie_is_defined_by_the_even_odd_rule():
    tie = poly16([(0, 0), (10, 10), (10, 0), (0, 10)])
    # the left triangle holds min(j, 9 - j) samples in row j (20); the right one also the samples ON its slanted edges, whose crossing is
    # not strictly to their right (30): spans are closed on the left, open on the right
    assert OV.coverage_cpu(P(tie), GRID).tolist() == [50] == [len(_loop_inside(tie, 16))]
    assert inter_of(tie, square(5, 0, 5, 10))[0, 1] == 30
    assert inter_of(tie, square(0, 0, 5, 10))[0, 1] == 20                   # the left triangle
    assert inter_of(tie, square(3, 0, 4, 10))[0, 1] == _loop_inter(tie, square(3, 0, 4, 10), 16)
    # a polygon that walks its outline twice covers nothing: every sample is crossed an even number of times
    twice = poly16([(0, 0), (10, 0), (10, 10), (0, 10)] * 2)
    assert OV.coverage_cpu(P(twice), GRID).tolist() == [0]


def test_degenerate_polygons_cover_nothing_and_never_interact():
    dot = poly16([(7, 7)])
    line = poly16([(0, 0), (20, 20)])
    flat = poly16([(0, 5), (30, 5), (10, 5)])
    big = square(0, 0, 40)
    polys = P(dot, big, line, flat, dot)
    assert OV.coverage_cpu(polys, GRID).tolist() == [0, 1600, 0, 0, 0]
    for measure in OV.MEASURES:
        for order in ([0, 1, 2, 3, 4], [1, 0, 2, 3, 4], [4, 3, 2, 1, 0]):
            owner, _ = OV.suppress_cpu(polys, [0, 5], order, 1, measure, GRID)
            assert owner.tolist() == [0, 1, 2, 3, 4]                        # area 0: suppresses nothing, is never suppressed


def test_grid_border_and_clamping():
    for grid in (64, 1000, 4096):
        full = square(0, 0, grid - 1)
        assert OV.coverage_cpu(P(full), grid).tolist() == [(grid - 1) ** 2]
        assert OV.coverage_cpu(P(square(grid - 3, grid - 3, 2)), grid).tolist() == [4]
    wild = poly16([(-5, -7), (2000, -1), (5000, 70), (-1, 70)])
    assert OV.coverage_cpu(P(wild), GRID).tolist() == OV.coverage_cpu(P(square(0, 0, 999, 70)), GRID).tolist() == [999 * 70]
    assert OV.bbox_cpu(P(wild), GRID).tolist() == [[0, 0, 999, 70]]
    assert inter_of(wild, square(990, 60, 50))[0, 1] == 9 * 10


# -- the specification against an independent loop ------------------------------------------------------------------------------------
def _loop_inside(row, grid):
    """the set of samples (i, j) inside one polygon: crossing number with exact rationals, sample by sample"""
    pts = [(min(max(int(row[2 * k]), 0), grid - 1), min(max(int(row[2 * k + 1]), 0), grid - 1)) for k in range(16)]
    inside = set()
    for j in range(grid - 1):
        for i in range(grid - 1):
            sx, sy = Fraction(2 * i + 1, 2), Fraction(2 * j + 1, 2)
            odd = False
            for k in range(16):
                (xa, ya), (xb, yb) = pts[k], pts[(k + 1) % 16]
                if (ya > sy) != (yb > sy):
                    if sx < xa + (sy - ya) * Fraction(xb - xa, yb - ya):
                        odd = not odd
            if odd:
                inside.add((i, j))
    return inside


def _loop_inter(a, b, grid):
    return len(_loop_inside(a, grid) & _loop_inside(b, grid))


def test_specification_equals_a_per_sample_loop_on_random_polygons():
    rng = np.random.RandomState(11)
    grid = 14
    polys = rng.randint(0, grid, size=(200, 32)).astype(np.int32)
    polys[::7, 8:] = np.tile(polys[::7, 6:8], (1, 12))                      # some with repeated points
    polys[5::11] = rng.randint(-3, grid + 4, size=polys[5::11].shape)       # some with tokens outside the grid
    polys[50] = np.tile(polys[50, :2], 16)                                   # one with all points equal
    gs = [0, 1, 3, 3, 40, 105, 200]
    sets = [_loop_inside(r, grid) for r in polys]
    assert OV.coverage_cpu(polys, grid).tolist() == [len(s) for s in sets]
    assert max(len(s) for s in sets) > 20 and min(len(s) for s in sets) == 0
    inter = OV.pair_overlap_cpu(polys, gs, grid)
    assert [m.shape[0] for m in inter] == [1, 2, 0, 37, 65, 95]
    for g, m in enumerate(inter):
        lo = gs[g]
        want = [[len(sets[lo + a] & sets[lo + b]) for b in range(m.shape[0])] for a in range(m.shape[0])]
        assert m.tolist() == want


# -- the pair test and the greedy pass ----------------------------------------------------------------------------------------------
def test_pair_test_boundary_is_inclusive_for_both_measures():
    # IoU exactly 1/2: a 10 x 10 square inside a 10 x 20 one -> inter 100, union 200
    polys = P(square(0, 0, 10, 20), square(0, 0, 10))
    for t, want in ((499, [0, 0]), (500, [0, 0]), (501, [0, 1])):
        assert OV.suppress_cpu(polys, [0, 2], [0, 1], t, 'iou', GRID)[0].tolist() == want
    assert OV.suppress_cpu(polys, [0, 2], [0, 1], 1000, 'iomin', GRID)[0].tolist() == [0, 0]   # inter == the smaller area
    # intersection over the smaller area exactly 1/2: equal squares shifted by half a side -> inter 50, min 100 (IoU 1/3)
    polys = P(square(0, 0, 10), square(5, 0, 10))
    for t, want in ((500, [0, 0]), (501, [0, 1])):
        assert OV.suppress_cpu(polys, [0, 2], [0, 1], t, 'iomin', GRID)[0].tolist() == want
    assert OV.suppress_cpu(polys, [0, 2], [0, 1], 333, 'iou', GRID)[0].tolist() == [0, 0]      # 50000 >= 333 * 150
    assert OV.suppress_cpu(polys, [0, 2], [0, 1], 334, 'iou', GRID)[0].tolist() == [0, 1]
    # inter == 0 never overlaps, whatever t
    assert OV.suppress_cpu(P(square(0, 0, 10), square(10, 0, 10)), [0, 2], [0, 1], 1, 'iou', GRID)[0].tolist() == [0, 1]
    assert OV.permille(0.5) == 500 and OV.permille(1.0) == 1000 and OV.permille(0.0004) == 1 and OV.permille(0.3335) == 334


def test_greedy_chain_orders_and_groups():
    a, b, c = square(0, 0, 10), square(4, 0, 10), square(8, 0, 10)          # a ~ b, b ~ c (IoU 60 / 140), a !~ c (20 / 180)
    polys = P(a, b, c)
    owner, area = OV.suppress_cpu(polys, [0, 3], [0, 1, 2], 300, 'iou', GRID)
    assert owner.tolist() == [0, 0, 2] and area.tolist() == [100] * 3      # b goes to a; c stays: its only overlap was removed
    assert OV.suppress_cpu(polys, [0, 3], [1, 0, 2], 300, 'iou', GRID)[0].tolist() == [1, 1, 1]
    assert OV.suppress_cpu(polys, [0, 3], [2, 1, 0], 300, 'iou', GRID)[0].tolist() == [0, 2, 2]
    # owner is the FIRST kept polygon in priority order that overlaps: b overlaps both a and c
    assert OV.suppress_cpu(polys, [0, 3], [2, 0, 1], 300, 'iou', GRID)[0].tolist() == [0, 2, 2]
    assert OV.suppress_cpu(polys, [0, 3], [0, 2, 1], 300, 'iou', GRID)[0].tolist() == [0, 0, 2]
    # polygons of different groups never interact; an empty group in between
    assert OV.suppress_cpu(P(a, a, a), [0, 1, 1, 3], [0, 1, 2], 500, 'iou', GRID)[0].tolist() == [0, 1, 1]
    # 'score' order: descending, ties to the lower index
    assert OV.score_order([0.5, 0.9, 0.9, 0.1, 0.7, 0.7], [0, 4, 6]).tolist() == [1, 2, 0, 3, 4, 5]
    order = OV.score_order([0.5, 0.9, 0.9], [0, 3])
    assert OV.suppress_cpu(polys, [0, 3], order, 300, 'iou', GRID)[0].tolist() == [1, 1, 1]


def test_mask_layout_and_the_specification_of_the_bitmask():
    ms, ist = OV.mask_layout([0, 1, 1, 65, 194])
    assert ms.tolist() == [0, 1, 1, 1 + 64, 1 + 64 + 129 * 3] and ist.tolist() == [0, 1, 1, 1 + 64 * 64, 1 + 64 * 64 + 129 * 129]
    parts = OV.split_inter(np.arange(int(ist[-1]), dtype=np.int32), [0, 1, 1, 65, 194])   # the empty group splits to [0, 0]
    assert [m.shape for m in parts] == [(1, 1), (0, 0), (64, 64), (129, 129)] and parts[2][1, 0] == 1 + 64
    a, b, c = square(0, 0, 10), square(4, 0, 10), square(8, 0, 10)
    m = OV.mask_cpu(P(a, b, c), [0, 3], [0, 1, 2], 300, 'iou', GRID)
    assert m.dtype == np.uint64 and m.tolist() == [0b010, 0b100, 0]         # row p, bits q > p only
    assert OV.mask_cpu(P(a, b, c), [0, 3], [1, 0, 2], 300, 'iou', GRID).tolist() == [0b110, 0, 0]
    rows = [square(3 * k, 0, 10) for k in range(70)]                        # a group that crosses the word boundary
    m = OV.mask_cpu(P(*rows), [0, 70], list(range(70)), 500, 'iou', GRID).reshape(70, 2)
    assert m[62].tolist() == [1 << 63, 0] and m[63].tolist() == [0, 1] and m[69].tolist() == [0, 0]


def test_specification_refusals():
    sq = P(square(0, 0, 10))
    with pytest.raises(ValueError):
        OV.coverage_cpu(sq, 4097)
    with pytest.raises(ValueError):
        OV.coverage_cpu(np.zeros((1, 30), np.int32), GRID)
    with pytest.raises(ValueError):
        OV.suppress_cpu(np.zeros((8193, 32), np.int32), [0, 8193], np.arange(8193), 500, 'iou', GRID)
    for t in (0, 1001):
        with pytest.raises(ValueError):
            OV.suppress_cpu(sq, [0, 1], [0], t, 'iou', GRID)
    with pytest.raises(ValueError):
        OV.suppress_cpu(sq, [0, 1], [0], 500, 'giou', GRID)
    with pytest.raises(ValueError):
        OV.suppress_cpu(P(square(0, 0, 1), square(0, 0, 1)), [0, 1, 2], [1, 0], 500, 'iou', GRID)   # order leaves its groups
    with pytest.raises(ValueError):
        OV.pair_overlap_cpu(sq, [0, 2], GRID)
    for s in (0, 0.0, -0.1, 1.01, 2):
        with pytest.raises(ValueError):
            OV.permille(s)
    with pytest.raises(RuntimeError):
        OV.OverlapSuppressor('cpu', GRID)                                    # there is no CPU stage


# -- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_entry_points_match_the_header():
    from advancedliteratemachinery_amd import _lib, build
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24
    for name in ('omp_polygon_overlap', 'omp_polygon_keep'):
        m = re.search(r'int %s\((.*?)\);' % name, text, re.S)
        want = []
        for p in (' '.join(p.split()) for p in m.group(1).split(',')):
            if '*' in p or p.startswith('omp_stream_t'):
                want.append(ctypes.c_void_p)
            elif p.startswith('int64_t'):
                want.append(ctypes.c_int64)
            else:
                assert p.startswith('int '), p
                want.append(ctypes.c_int)
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and args == want, name
        assert name in _lib.EXPORTS
    assert 'overlap.hip' in build.SOURCES
    src = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'overlap.hip')).read()
    assert 'OV_MAX_GRID = %d' % OV.GRID_MAX in src and 'OV_MAX_GROUP = %d' % OV.GROUP_MAX in src


# -- routing: predict / predict_images / spot_and_recognize with the engine and the device stage stubbed out -----------------------------
class _Stub(torch.nn.Module):
    """infer() answering the same three words under every window: squares at x = 100, 104 (overlapping the first) and 300"""
    WORDS = (square(100, 100, 40, 20), square(104, 100, 40, 20), square(300, 100, 40, 20))
    PROBS = (0.5, 0.9, 0.7)

    def __init__(self, rec_length):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.rec_length = rec_length

    def infer(self, img, mask, seqs, has_padding=None, ragged=False, windows=None, char_windows=None, clip_windows=False):
        out = []
        for b in range(len(img)):
            W = 1 if windows is None else len(windows[b])
            n = 3 * W
            pt = torch.arange(2 * n).reshape(1, -1)
            poly = torch.tensor([self.WORDS[k % 3] for k in range(n)], dtype=torch.long).reshape(1, -1)
            probs = torch.tensor([self.PROBS[k % 3] for k in range(n)])[:, None].repeat(1, self.rec_length)
            res = ([pt, poly, torch.full((1, n, self.rec_length), 1000)], [probs])
            out.append(res if windows is None else res + (torch.arange(W).repeat_interleave(3),))
        return out


class _HostSuppressor(object):
    """OverlapSuppressor without a device: the specification behind the same interface, and a log of its calls"""
    calls = []

    def __init__(self, device, grid):
        self.grid = grid

    def __call__(self, polys, group_start, order=None, t=500, measure='iou'):
        polys = torch.as_tensor(polys).numpy()
        order = np.arange(len(polys)) if order is None else order
        type(self).calls.append(dict(n=len(polys), groups=np.asarray(group_start).tolist(), order=np.asarray(order).tolist(), t=t, measure=measure))
        return OV.suppress_cpu(polys, group_start, order, t, measure, self.grid)


@pytest.fixture
def stubbed(monkeypatch):
    _HostSuppressor.calls = []
    monkeypatch.setattr(OV, 'OverlapSuppressor', _HostSuppressor)
    a = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    return a, _Stub(a.rec_length), torch.zeros(2, 3, 32, 32)


def test_predict_without_suppress_is_unchanged(stubbed):
    a, stub, imgs = stubbed
    plain = inf.predict(stub, imgs, a)
    assert [len(r) for r in plain] == [3, 3] and all('merged' not in r for recs in plain for r in recs)
    assert inf.predict(stub, imgs, a, suppress=None, suppress_measure='iomin', suppress_order='score') == plain
    assert _HostSuppressor.calls == []
    for fn in (inf.predict, inf.predict_images, two_stage.spot_and_recognize):
        p = inspect.signature(fn).parameters
        assert p['suppress'].default is None and p['suppress_measure'].default == 'iou' and p['suppress_order'].default == 'first'
    from advancedliteratemachinery_amd.model import omniparser as omp
    assert 'suppress' not in inspect.signature(omp.OmniParser.infer).parameters
    assert 'suppress' not in inspect.signature(omp.OmniParser.forward).parameters


def test_predict_routes_suppress_in_one_call(stubbed):
    a, stub, imgs = stubbed
    plain = inf.predict(stub, imgs, a)
    got = inf.predict(stub, imgs, a, suppress=0.5)
    assert len(_HostSuppressor.calls) == 1                                   # both images in ONE call
    assert _HostSuppressor.calls[0] == dict(n=6, groups=[0, 3, 6], order=list(range(6)), t=500, measure='iou')
    for recs, before in zip(got, plain):
        assert [r['merged'] for r in recs] == [[1], []]                      # the second word (IoU 36 / 44) went to the first
        assert [{k: v for k, v in r.items() if k != 'merged'} for r in recs] == [before[0], before[2]]
    # 'score': the second word has the best score and absorbs the first
    got = inf.predict(stub, imgs, a, suppress=0.5, suppress_order='score')
    assert _HostSuppressor.calls[-1]['order'] == [1, 2, 0, 4, 5, 3]
    assert [[r['merged'] for r in recs] for recs in got] == [[[0], []]] * 2 and got[0][0]['polys'] == plain[0][1]['polys']
    # a threshold above the overlap keeps everything; every record still gains `merged`
    got = inf.predict(stub, imgs, a, suppress=0.9, suppress_measure='iomin')
    assert _HostSuppressor.calls[-1]['t'] == 900 and _HostSuppressor.calls[-1]['measure'] == 'iomin'
    assert [[r['merged'] for r in recs] for recs in got] == [[[1], []]] * 2  # 36 / 40 of the smaller area
    got = inf.predict(stub, imgs, a, suppress=0.95, suppress_measure='iomin')
    assert [[r['merged'] for r in recs] for recs in got] == [[[], [], []]] * 2


def test_predict_suppress_with_windows_reports_window_and_index(stubbed):
    a, stub, imgs = stubbed
    wins = [WN.default_window(a), WN.default_window(a)]
    plain = inf.predict(stub, imgs, a, windows=wins)
    got = inf.predict(stub, imgs, a, windows=wins, suppress=0.5)
    assert [len(r) for r in plain] == [6, 6] and [len(r) for r in got] == [2, 2]
    for recs in got:
        assert [(r['window'], r['merged']) for r in recs] == [(0, [(0, 1), (1, 3), (1, 4)]), (0, [(1, 5)])]
    # ragged= reaches the engine as before
    assert inf.predict(stub, [imgs[0], imgs[1]], a, ragged=True, windows=wins, suppress=0.5) == got


def test_suppress_records_on_empty_images():
    recs = [[], [dict(score=1.0)], []]
    polys = [None, torch.tensor([square(0, 0, 10)]), None]
    out = OV.suppress_records(copy.deepcopy(recs), polys, GRID, 0.5, suppressor=_HostSuppressor(None, GRID))
    assert out == [[], [dict(score=1.0, merged=[])], []]
    assert OV.suppress_records([[], []], [None, None], GRID, 0.5, suppressor=None) == [[], []]   # nothing to do: no device is touched
    with pytest.raises(ValueError):
        OV.suppress_records([[dict(score=1.0)]], [torch.zeros(2, 32)], GRID, 0.5, suppressor=_HostSuppressor(None, GRID))


def test_entry_points_refuse(stubbed):
    a, stub, imgs = stubbed
    for kw in (dict(suppress=0), dict(suppress=1.5), dict(suppress=-1), dict(suppress=0.5, suppress_measure='giou'),
               dict(suppress=0.5, suppress_order='last')):
        with pytest.raises(ValueError):
            inf.predict(stub, imgs, a, **kw)
        with pytest.raises(ValueError):
            inf.predict_images(stub, [], a, **kw)
        with pytest.raises(ValueError):
            two_stage.spot_and_recognize(stub, None, [], a, **kw)
    kie = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, infer_vie=True, vie_categories=4, val_dataset=['sroie_val'])
    for call in (lambda: inf.predict(stub, imgs, kie, suppress=0.5), lambda: inf.predict_images(stub, [], kie, suppress=0.5),
                 lambda: two_stage.spot_and_recognize(stub, None, [], kie, suppress=0.5)):
        with pytest.raises(ValueError):
            call()
    big = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    big.num_bins = 5000
    with pytest.raises(ValueError):
        OV.suppress_records([[dict(score=1.0)]], [torch.zeros(1, 32)], big.num_bins, 0.5, suppressor=_RefusingGrid(big.num_bins))


class _RefusingGrid(object):
    """the grid check of the device stage, without a device"""

    def __init__(self, grid):
        self.grid = grid

    def __call__(self, polys, group_start, order=None, t=500, measure='iou'):
        return OV.suppress_cpu(torch.as_tensor(polys).numpy(), group_start, np.arange(len(polys)), t, measure, self.grid)
