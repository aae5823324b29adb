"""Reading order on the host (no GPU): the numpy specification (utils/reading.py) on synthetic pages, rotations, a ring, contested
successors, ties, anisotropic bins, degenerate polygons and the integer extremes; the blocked links against an unblocked evaluation;
every refusal; how predict / predict_images / spot_and_recognize route `reading_order=` (the device stage replaced by its
specification); page_lines.  The kernels and the end-to-end answers are tests/test_gpu_reading.py."""
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
from advancedliteratemachinery_amd.utils import windows as WN
from advancedliteratemachinery_amd.utils.parser import make_args
from tests import reading_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 1000
SQ = [[256, 256]]
ROWS = [list(range(6 * r, 6 * r + 6)) for r in range(5)]


def run(polys, aspect=SQ, gs=None, grid=GRID, **kw):
    return RD.lines_cpu(polys, [0, len(polys)] if gs is None else gs, aspect, grid=grid, **kw)


def words(*xywh):
    return RC.to_bins(np.stack([RC.word(*a) for a in xywh]))


# -- pages -------------------------------------------------------------------------------------------------------------------------
def test_page_of_five_rows_of_six_shuffled():
    polys, ids = RC.page(seed=4)
    res = run(polys)
    assert res['n_lines'].tolist() == [5]
    assert RC.lines_of(res, ids=ids) == ROWS                               # top to bottom, left to right
    assert sorted(res['rank'].tolist()) == list(range(30))
    assert [int(res['line_pos'][i]) for i in np.argsort(ids)] == [c for _ in range(5) for c in range(6)]
    inv = np.argsort(ids)
    for r in ROWS:                                                          # succ / pred are global indices along the row
        for k, m in enumerate(r):
            assert res['succ'][inv[m]] == (inv[r[k + 1]] if k < 5 else -1) and res['pred'][inv[m]] == (inv[r[k - 1]] if k else -1)
    assert all(v.dtype == np.int32 for v in res.values())


@pytest.mark.parametrize('degrees', [30, 90, 180])
def test_rotated_page_gives_the_same_lines(degrees):
    polys, ids = RC.page(seed=5, degrees=degrees)
    got = RC.lines_of(run(polys), ids=ids)
    assert sorted(got) == ROWS                                              # the same lines, each in its words' own direction
    if degrees == 180:
        assert got == ROWS[::-1]                                            # the page is upside down: its last row is on top ...
        x = polys[np.argsort(ids)][:6, 0]
        assert (np.diff(x) < 0).all()                                       # ... and a line runs right to left in the image
    if degrees == 30:
        assert got == ROWS


def test_ring_is_one_line_cut_in_front_of_word_0():
    polys = RC.ring()
    succ0, _ = RD.links_cpu(polys, [0, 10], SQ, grid=GRID)
    assert succ0.tolist() == [(k + 1) % 10 for k in range(10)]              # a 10-cycle before the cut
    res = run(polys)
    assert res['n_lines'].tolist() == [1] and res['line'].tolist() == [0] * 10
    assert res['line_pos'].tolist() == list(range(10)) == res['rank'].tolist()
    assert res['pred'][0] == -1 and res['succ'][9] == -1 and res['succ'][:9].tolist() == list(range(1, 10))
    # shifted by three: the cut is in front of the lowest index wherever it sits on the ring
    res = run(np.roll(polys, 3, axis=0))
    assert res['line_pos'].tolist() == list(range(10)) and res['pred'][0] == -1 and res['succ'][9] == -1


# -- successor and predecessor rules -------------------------------------------------------------------------------------------------
def test_contested_successor_goes_to_the_lower_cost_then_the_lower_index():
    f = (200, 100, 60, 20)
    # equal cost: both end 12 bins before the follower, 4 bins above / below its line
    res = run(words((128, 96, 60, 20), (128, 104, 60, 20), f))
    succ0, cost0 = RD.links_cpu(words((128, 96, 60, 20), (128, 104, 60, 20), f), [0, 3], SQ, grid=GRID)
    assert succ0.tolist() == [2, 2, -1] and cost0[0] == cost0[1] > 0
    assert res['succ'].tolist() == [2, -1, -1] and res['pred'].tolist() == [-1, -1, 0]
    assert res['n_lines'].tolist() == [2] and sorted(RC.lines_of(res)) == [[0, 2], [1]]   # the loser ends its own line
    # the nearer one wins although its index is higher
    res = run(words((120, 100, 60, 20), (128, 100, 60, 20), f))
    assert res['succ'].tolist() == [-1, 2, -1] and res['pred'].tolist() == [-1, -1, 1]


def test_two_followers_at_equal_cost_the_lower_index_wins():
    a = (100, 100, 60, 20)
    for first, second in (((172, 96, 60, 20), (172, 104, 60, 20)), ((172, 104, 60, 20), (172, 96, 60, 20))):
        p = words(a, first, second)
        succ0, cost0 = RD.links_cpu(p, [0, 3], SQ, grid=GRID)
        assert succ0[0] == 1 and cost0[0] == (2 * 12 * 256) ** 2 + (2 * 4 * 256) ** 2
        assert run(p)['succ'][0] == 1
    # exact duplicates tie everywhere
    p = words(a, (172, 100, 60, 20), (172, 100, 60, 20), a)
    res = run(p)
    assert res['succ'].tolist() == [1, -1, -1, -1] and res['n_lines'].tolist() == [3]


def test_anisotropic_bins_need_the_aspect():
    """Every offset test is a ratio of cross products with one d, which a linear map of the plane leaves alone: squeezed bins change
    the answer through `along`, d_a . d_b and the cost only.  So the genuine effect is shown on the gap (vertical text, whose
    heights lie along the squeezed axis); the page with words alternately 1.5 bins off their line covers the offset."""
    orig, _ = RC.page(degrees=30, jitter=1.5)
    half, _ = RC.page(degrees=30, jitter=1.5, sx=0.5)
    want = RD.links_cpu(orig, [0, 30], SQ, grid=GRID)[0]
    assert RC.lines_of(run(orig)) == ROWS
    assert (RD.links_cpu(half, [0, 30], [[256, 128]], grid=GRID)[0] == want).all()
    assert not (RD.links_cpu(half, [0, 30], SQ, offset=100, grid=GRID)[0] == want).all()
    # vertical text, gap = one height: 12 bins of gap against 20 bins of height -- 10 once x is halved and nobody says so
    orig, _ = RC.page(degrees=90)
    half, _ = RC.page(degrees=90, sx=0.5)
    want = RD.links_cpu(orig, [0, 30], SQ, gap=1000, grid=GRID)[0]
    assert (want >= 0).sum() == 25
    assert (RD.links_cpu(half, [0, 30], [[256, 128]], gap=1000, grid=GRID)[0] == want).all()
    assert (RD.links_cpu(half, [0, 30], SQ, gap=1000, grid=GRID)[0] == -1).all()
    assert RD.aspect_of(100, 200) == (256, 128) and RD.aspect_of(200, 100) == (128, 256) and RD.aspect_of(7, 7) == (256, 256)
    assert RD.aspect_of(1, 100000) == (256, 1)


def test_degenerate_polygons_follow_the_rules_without_a_special_case():
    dot = lambda x, y: [x, y] * 16                                           # noqa: E731  all 16 points equal: d = (1, 0), H = 0
    w = words((100, 100, 60, 20))[0].tolist()                                # L = (200, 220), R = (320, 220) in doubled bins
    f = RD.features_cpu(np.asarray([dot(5, 5)]), SQ)
    assert f['d'].tolist() == [[1, 0]] and f['H'].tolist() == [0] and f['L'].tolist() == [[2560, 2560]]
    # H = 0 leaves only v = 0: a point precedes what starts exactly on it (and runs rightwards, d_a . d_b > 0), follows what ends
    # exactly on it (pb = 0 <= offset * 0), and links to nothing else -- one bin off is off
    p = np.asarray([dot(300, 300), dot(400, 300), w, dot(100, 110), dot(160, 110), dot(161, 110), dot(99, 110)], dtype=np.int32)
    succ0, cost0 = RD.links_cpu(p, [0, 7], SQ, grid=GRID)
    assert succ0.tolist() == [-1, -1, 4, 2, -1, -1, -1] and cost0.tolist() == [-1, -1, 0, 0, -1, -1, -1]
    res = run(p)
    assert res['succ'].tolist() == succ0.tolist() and res['pred'].tolist() == [-1, -1, 3, -1, 2, -1, -1]
    assert RC.lines_of(res) == [[6], [3, 2, 4], [5], [0], [1]]                # by mean y, then L_x of the head, then its index
    # identical points: v = 0 for every pair, each links to the lowest other; resolution and the cycle rule make {0, 1} a line
    res = run(np.asarray([dot(7, 7)] * 3, dtype=np.int32))
    assert RD.links_cpu([dot(7, 7)] * 3, [0, 3], SQ, grid=GRID)[0].tolist() == [1, 0, 0]
    assert res['succ'].tolist() == [1, -1, -1] and res['pred'].tolist() == [-1, 0, -1] and res['line'].tolist() == [0, 0, 1]


def test_extremes_keep_the_bounds():
    g = OV.GRID_MAX
    far = [0, 0] * 8 + [g - 1, g - 1] * 8                                    # no word, but the largest T - B and H there is
    p = np.asarray([far, far[::-1], [g - 1, 0] * 16, [0, g - 1] * 16, RC.to_bins(RC.word(0, 0, g - 1, g - 1)[None])[0]], dtype=np.int32)
    for asp in ([[256, 256]], [[256, 1]], [[1, 256]]):
        for v in (0, 10000):
            res = RD.lines_cpu(p, [0, len(p)], asp, v, v, v, g)               # the assertions inside hold
            assert sorted(res['rank'].tolist()) == list(range(len(p)))
    f = RD.features_cpu(p, np.repeat([[256, 256]], len(p), 0))
    assert int(f['H'].max()) * 10000 < 2 ** 63 and int(f['H'].max()) >= 8 * (4095 * 256) ** 2 // 2
    with pytest.raises(AssertionError):
        RD.features_cpu(np.full((1, 32), g), [[256, 256]])
    with pytest.raises(AssertionError):
        RD.features_cpu(np.zeros((1, 32)), [[257, 1]])


def test_blocked_links_equal_an_unblocked_evaluation():
    rng = np.random.RandomState(11)
    polys = np.concatenate([RC.page(10, 20, w=24, h=8, gap=5, pitch=14, seed=2)[0], rng.randint(0, GRID, (100, 32)).astype(np.int32)])
    gs, asp = [0, 120, 300], [[256, 200], [37, 256]]
    a = RD.links_cpu(polys, gs, asp, grid=GRID)
    b = RD.links_cpu(polys, gs, asp, grid=GRID, block=10 ** 6)
    c = RD.links_cpu(polys, gs, asp, grid=GRID, block=7)
    assert (a[0] >= 0).sum() > 100
    for x, y in ((a, b), (a, c)):
        assert (x[0] == y[0]).all() and (x[1] == y[1]).all()
    # and a plain double loop over the pairs of the second group
    f = RD.features_cpu(polys, np.repeat(asp, [120, 180], 0))
    for i in range(120, 300, 17):
        best = (-1, -1)
        for j in range(120, 300):
            v = f['L'][j] - f['R'][i]
            da, db = f['d'][i], f['d'][j]
            along, pa, pb = int(v @ da), int(v[0] * da[1] - v[1] * da[0]), int(v[0] * db[1] - v[1] * db[0])
            if (i != j and int(da @ db) > 0 and 4000 * along <= 2000 * f['H'][i] and 4000 * along >= -500 * f['H'][i]
                    and 4000 * abs(pa) <= 500 * f['H'][i] and 4000 * abs(pb) <= 500 * f['H'][j]):
                if best[0] < 0 or int(v @ v) < best[1]:
                    best = (j, int(v @ v))
        assert (a[0][i], a[1][i]) == best


# -- refusals -----------------------------------------------------------------------------------------------------------------------
def test_specification_refusals():
    p = words((100, 100, 60, 20))
    for bad in (dict(grid=4097), dict(grid=1), dict(gap=-1), dict(gap=10001), dict(back=10001), dict(offset=-1), dict(offset=0.5)):
        with pytest.raises(ValueError):
            run(p, **bad)
    for asp in ([[0, 256]], [[256, 257]], [[256, 256], [256, 256]], []):
        with pytest.raises(ValueError):
            run(p, aspect=asp)
    with pytest.raises(ValueError):
        run(np.zeros((1, 30), np.int32))
    for gs in ([0, 2], [1, 1], [0, 1, 0, 1]):
        with pytest.raises(ValueError):
            RD.lines_cpu(p, gs, [[256, 256]] * (len(gs) - 1), grid=GRID)
    with pytest.raises(ValueError):
        RD.links_cpu(np.zeros((8193, 32), np.int32), [0, 8193], SQ, grid=GRID)
    for v in (-0.1, 10.01, float('nan')):
        with pytest.raises(ValueError):
            RD.permille(v)
    assert RD.permille(2.0) == 2000 and RD.permille(0) == 0 and RD.permille(10) == 10000
    for hw in ((0, 5), (5, 0), (-1, 5)):
        with pytest.raises(ValueError):
            RD.aspect_of(*hw)
    with pytest.raises(RuntimeError):
        RD.ReadingOrder('cpu', GRID)                                         # there is no CPU stage
    res = run(np.zeros((0, 32), np.int32), aspect=[[256, 256], [3, 4]], gs=[0, 0, 0])
    assert res['n_lines'].tolist() == [0, 0] and res['rank'].size == 0


def test_entry_points_match_the_header():
    from advancedliteratemachinery_amd import _lib, build
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24
    for name in ('omp_reading_links', 'omp_reading_lines'):
        m = re.search(r'int %s\((.*?)\);' % name, text, re.S)
        want = []
        for p in (' '.join(p.split()) for p in m.group(1).split(',')):
            if '*' in p or p.startswith('omp_stream_t'):
                want.append(ctypes.c_void_p)
            else:
                assert p.startswith('int '), p
                want.append(ctypes.c_int)
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and args == want, name
        assert name in _lib.EXPORTS
    assert 'reading.hip' in build.SOURCES
    src = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'reading.hip')).read()
    assert 'RD_MAX_GRID = %d' % OV.GRID_MAX in src and 'RD_MAX_GROUP = %d' % OV.GROUP_MAX in src
    assert 'RD_MAX_ASPECT = %d' % RD.ASPECT_MAX in src and 'RD_MAX_PARAM = %d' % RD.PARAM_MAX in src


# -- routing: predict / predict_images / spot_and_recognize with the engine and the device stages stubbed out ------------------------
def _w(x, y):
    return RC.to_bins(RC.word(x, y, 60, 20)[None])[0].tolist()


class _Stub(torch.nn.Module):
    """infer() answering the same five words under every window: two lines of two, out of order, and a near-duplicate of word 1"""
    WORDS = (_w(172, 140), _w(100, 100), _w(100, 102), _w(172, 100), _w(100, 140))
    PROBS = (0.5, 0.9, 0.7, 0.6, 0.8)

    def __init__(self, rec_length):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.rec_length = rec_length

    def infer(self, img, mask, seqs, has_padding=None, ragged=False, windows=None, char_windows=None, clip_windows=False):
        out = []
        for b in range(len(img)):
            W = 1 if windows is None else len(windows[b])
            n = 5 * W
            pt = torch.arange(2 * n).reshape(1, -1)
            poly = torch.tensor([self.WORDS[k % 5] for k in range(n)], dtype=torch.long).reshape(1, -1)
            probs = torch.tensor([self.PROBS[k % 5] for k in range(n)])[:, None].repeat(1, self.rec_length)
            res = ([pt, poly, torch.full((1, n, self.rec_length), 1000)], [probs])
            out.append(res if windows is None else res + (torch.arange(W).repeat_interleave(5),))
        return out


class _HostSuppressor(object):
    def __init__(self, device, grid):
        self.grid = grid

    def __call__(self, polys, group_start, order=None, t=500, measure='iou'):
        polys = torch.as_tensor(polys).numpy()
        return OV.suppress_cpu(polys, group_start, np.arange(len(polys)) if order is None else order, t, measure, self.grid)


class _HostReader(object):
    """ReadingOrder without a device: the specification behind the same interface, and a log of its calls"""
    calls = []

    def __init__(self, device, grid):
        self.grid = grid

    def __call__(self, polys, group_start, aspect, gap=2000, back=500, offset=500):
        polys = torch.as_tensor(polys).numpy()
        type(self).calls.append(dict(polys=polys.tolist(), groups=np.asarray(group_start).tolist(), aspect=np.asarray(aspect).tolist(),
                                     params=(gap, back, offset)))
        return RD.lines_cpu(polys, group_start, aspect, gap, back, offset, self.grid)


@pytest.fixture
def stubbed(monkeypatch):
    _HostReader.calls = []
    monkeypatch.setattr(OV, 'OverlapSuppressor', _HostSuppressor)
    monkeypatch.setattr(RD, 'ReadingOrder', _HostReader)
    a = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    return a, _Stub(a.rec_length), torch.zeros(2, 3, 32, 64)


def _minus(r, keys=('line', 'line_pos')):
    return {k: v for k, v in r.items() if k not in keys}


def test_predict_without_reading_order_is_unchanged(stubbed):
    a, stub, imgs = stubbed
    plain = inf.predict(stub, imgs, a)
    assert [len(r) for r in plain] == [5, 5] and all('line' not in r and 'line_pos' not in r for recs in plain for r in recs)
    assert inf.predict(stub, imgs, a, reading_order=False, line_gap=9.0, line_back=9.0, line_offset=9.0) == plain
    assert _HostReader.calls == []
    for fn in (inf.predict, inf.predict_images, two_stage.spot_and_recognize):
        p = inspect.signature(fn).parameters
        assert p['reading_order'].default is False
        assert (p['line_gap'].default, p['line_back'].default, p['line_offset'].default) == (2.0, 0.5, 0.5)
    from advancedliteratemachinery_amd.model import omniparser as omp
    assert 'reading_order' not in inspect.signature(omp.OmniParser.infer).parameters


def test_predict_reorders_and_attaches_lines_in_one_call(stubbed):
    a, stub, imgs = stubbed
    plain = inf.predict(stub, imgs, a)
    got = inf.predict(stub, imgs, a, reading_order=True, line_offset=0.05)   # 2 bins off the line, 1 allowed: the duplicate joins no line
    assert len(_HostReader.calls) == 1                                        # both images in ONE call
    c = _HostReader.calls[0]
    assert c['groups'] == [0, 5, 10] and c['params'] == (2000, 500, 50) and c['polys'] == [list(w) for w in _Stub.WORDS] * 2
    assert c['aspect'] == [[256, 128]] * 2                                    # 32 x 64 images: x bins are twice as wide
    for recs, before in zip(got, plain):
        assert [_minus(r) for r in recs] == [before[i] for i in (1, 3, 2, 4, 0)]
        assert [(r['line'], r['line_pos']) for r in recs] == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)]
    assert RD.page_lines(got[0], field='line_pos') == ['0 1', '0', '0 1']
    assert inf.predict(stub, [imgs[0], imgs[1]], a, ragged=True, reading_order=True, line_offset=0.05) == got


def test_predict_reading_order_runs_on_the_survivors_rows(stubbed):
    a, stub, imgs = stubbed
    plain = inf.predict(stub, imgs, a, suppress=0.5)
    assert [[r['merged'] for r in recs] for recs in plain] == [[[], [2], [], []]] * 2
    got = inf.predict(stub, imgs, a, suppress=0.5, reading_order=True)
    c = _HostReader.calls[-1]
    assert c['groups'] == [0, 4, 8] and c['polys'] == [list(_Stub.WORDS[i]) for i in (0, 1, 3, 4)] * 2   # rows of the survivors only
    for recs, before in zip(got, plain):
        assert [_minus(r) for r in recs] == [before[i] for i in (1, 2, 3, 0)]
        assert [(r['line'], r['line_pos']) for r in recs] == [(0, 0), (0, 1), (1, 0), (1, 1)]
        assert recs[0]['merged'] == [2]                                       # an index before suppression
    # windows: window, window_bins and merged stay on their records
    wins = [WN.default_window(a), WN.default_window(a)]
    plain = inf.predict(stub, imgs, a, windows=wins, suppress=0.5)
    got = inf.predict(stub, imgs, a, windows=wins, suppress=0.5, reading_order=True)
    assert _HostReader.calls[-1]['groups'] == [0, 4, 8]
    for recs, before in zip(got, plain):
        assert [_minus(r) for r in recs] == [before[i] for i in (1, 2, 3, 0)]
        assert recs[0]['merged'] == [(0, 2), (1, 6), (1, 7)] and recs[0]['window'] == 0 and recs[0]['window_bins'] == list(wins[0])
    got = inf.predict(stub, imgs, a, windows=wins, reading_order=True)        # without suppress=: every window's words, duplicates included
    assert _HostReader.calls[-1]['groups'] == [0, 10, 20] and sorted(r['window'] for r in got[0]) == [0] * 5 + [1] * 5


def test_order_records_on_empty_images():
    recs = [[], [dict(rec='a')], []]
    polys = [None, torch.tensor([_w(10, 10)]), None]
    out = RD.order_records(copy.deepcopy(recs), polys, [(10, 10)] * 3, GRID, reader=_HostReader(None, GRID))
    assert out == [[], [dict(rec='a', line=0, line_pos=0)], []]
    assert RD.order_records([[], []], [None, None], [(1, 1)] * 2, GRID, reader=None) == [[], []]   # nothing to do: no device is touched
    with pytest.raises(ValueError):
        RD.order_records([[dict(rec='a')]], [torch.zeros(2, 32)], [(1, 1)], GRID, reader=_HostReader(None, GRID))


def test_entry_points_refuse(stubbed):
    a, stub, imgs = stubbed
    for kw in (dict(line_gap=-0.1), dict(line_gap=10.5), dict(line_back=-1), dict(line_back=11), dict(line_offset=-0.5), dict(line_offset=100)):
        with pytest.raises(ValueError):
            inf.predict(stub, imgs, a, reading_order=True, **kw)
        with pytest.raises(ValueError):
            inf.predict_images(stub, [], a, reading_order=True, **kw)
        with pytest.raises(ValueError):
            two_stage.spot_and_recognize(stub, None, [], a, reading_order=True, **kw)
    kie = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, infer_vie=True, vie_categories=4, val_dataset=['sroie_val'])
    for call in (lambda: inf.predict(stub, imgs, kie, reading_order=True), lambda: inf.predict_images(stub, [], kie, reading_order=True),
                 lambda: two_stage.spot_and_recognize(stub, None, [], kie, reading_order=True)):
        with pytest.raises(ValueError):
            call()


def test_page_lines():
    recs = [dict(rec='the', line=0), dict(rec='quick', line=0), dict(rec='fox', line=1), dict(rec='!', line=2, mgp_text='?')]
    assert RD.page_lines(recs) == ['the quick', 'fox', '!']
    assert RD.page_lines(recs, sep='_') == ['the_quick', 'fox', '!']
    assert RD.page_lines(recs[3:], field='mgp_text') == ['?'] and RD.page_lines([]) == []
