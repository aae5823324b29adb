"""Page text scoring on the host (no GPU): the numpy definition (utils/page_text.py) against the plain double loop of
utils/lexicon.py, the encoding, the page strings, the scores, score_page_text and sweep_reading on a two-column page with the host
scorer and a host reader, the command line on a results file written here, and the C ABI's declaration.  The kernel and the device stage
are tests/test_gpu_page_text.py."""
import ctypes
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

from advancedliteratemachinery_amd.engine import evaluate as EV
from advancedliteratemachinery_amd.utils import lexicon as LX
from advancedliteratemachinery_amd.utils import page_text as PT
from advancedliteratemachinery_amd.utils import reading as RD
from tests import blocks_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 1000


def _naive(a, b):
    """the double loop over sequences in which 255 is replaced by symbols that occur once: 255 equals nothing"""
    fresh = itertools.count(1000)
    return LX.edit_distance_cpu([next(fresh) if v == PT.NONE else int(v) for v in a], [next(fresh) if v == PT.NONE else int(v) for v in b])


# -- distance_cpu -----------------------------------------------------------------------------------------------------------------------
def test_distance_cpu_equals_the_double_loop_on_every_short_binary_string():
    strings = [list(s) for n in range(5) for s in itertools.product((0, 1), repeat=n)]
    assert len(strings) == 31
    for a in strings:
        for b in strings:
            assert PT.distance_cpu(a, b) == LX.edit_distance_cpu(a, b), (a, b)


def test_distance_cpu_equals_the_double_loop_on_random_strings():
    rng = np.random.RandomState(0)
    for _ in range(300):
        sigma = int(rng.choice([1, 2, 4, 26]))
        a = rng.randint(0, sigma, rng.randint(0, 41)).astype(np.uint8)
        b = rng.randint(0, sigma, rng.randint(0, 41)).astype(np.uint8)
        if rng.rand() < 0.3:
            b[rng.rand(b.size) < 0.2] = PT.NONE
        if rng.rand() < 0.1:
            a[rng.rand(a.size) < 0.2] = PT.NONE
        assert PT.distance_cpu(a, b) == _naive(a, b) == PT.distance_cpu(b, a)


def test_code_255_equals_nothing():
    assert PT.distance_cpu([255], [255]) == 1 and PT.distance_cpu([255, 3], [255, 3]) == 1 and PT.distance_cpu([3], [3]) == 0
    assert PT.distance_cpu([], []) == 0 and PT.distance_cpu([1, 2, 3], []) == 3 and PT.distance_cpu([], [255]) == 1
    with pytest.raises(ValueError, match='limit'):
        PT.distance_cpu(np.zeros(PT.LEN_MAX + 1, np.uint8), [1])


# -- encode_pairs, pairs_cpu --------------------------------------------------------------------------------------------------------------
def test_encode_pairs_codes_the_prediction_alphabet_and_shares_ranges():
    pred = ['abcab', 'cab', '', 'abcab']
    truth = ['abxab', 'abxab', 'q', 'abcab']
    pool, a_off, a_len, b_off, b_len, sigma = PT.encode_pairs(pred, truth)
    assert pool.dtype == np.uint8 and all(t.dtype == np.int32 for t in (a_off, a_len, b_off, b_len)) and sigma == 3
    assert a_len.tolist() == [5, 3, 0, 5] and b_len.tolist() == [5, 5, 1, 5]
    assert a_off[0] == a_off[3] and b_off[0] == b_off[1] and b_off[0] != b_off[3]          # equal strings of one side share a range
    assert pool.size == 5 + 3 + 0 + 5 + 1 + 5
    gt0 = pool[b_off[0]:b_off[0] + 5].tolist()
    assert gt0 == [0, 1, 255, 0, 1] and pool[b_off[2]] == 255                               # ground-truth-only characters
    dist = PT.pairs_cpu(pool, a_off, a_len, b_off, b_len)
    assert dist.dtype == np.int32 and dist.tolist() == [LX.edit_distance_cpu(p, t) for p, t in zip(pred, truth)] == [1, 3, 1, 0]
    assert PT.HostPageScorer().run(pool, a_off, a_len, b_off, b_len, sigma).tolist() == dist.tolist()


def test_encode_pairs_distance_equals_the_one_over_raw_code_points():
    rng = np.random.RandomState(3)
    letters = 'abcdefghijklmnopqrstuvwxyz0123456789'
    pred = [''.join(rng.choice(list(letters[:10]), rng.randint(0, 60))) for _ in range(20)]
    truth = [''.join(rng.choice(list(letters), rng.randint(0, 60))) for _ in range(20)]
    enc = PT.encode_pairs(pred, truth)
    assert enc[5] <= 10
    assert PT.pairs_cpu(*enc[:5]).tolist() == [LX.edit_distance_cpu(p, t) for p, t in zip(pred, truth)]


def test_encode_pairs_refuses():
    many = ''.join(chr(0x100 + k) for k in range(255))
    with pytest.raises(ValueError, match='edit_distance_cpu'):
        PT.encode_pairs([many], ['a'])
    assert PT.encode_pairs([many[:254]], [many])[5] == 254                                  # 254 fit; the 255th is ground truth only
    with pytest.raises(ValueError, match='limit'):
        PT.encode_pairs(['a' * (PT.LEN_MAX + 1)], ['a'])
    with pytest.raises(ValueError):
        PT.encode_pairs(['a'], ['a', 'b'])
    assert PT.encode_pairs(['a' * PT.LEN_MAX], [''])[2].tolist() == [PT.LEN_MAX]
    for bad in (dict(a_len=[2]), dict(a_len=[-1]), dict(b_off=[1]), dict(a_len=[PT.LEN_MAX + 1])):
        kw = dict(pool=np.zeros(1, np.uint8), a_off=[0], a_len=[1], b_off=[0], b_len=[1])
        kw.update(bad)
        with pytest.raises(ValueError):
            PT.pairs_cpu(**kw)


def test_encode_pairs_gives_the_recorded_pools_and_tables():
    """encode_pairs goes through page_text._encode, which encode_search shares: the outputs are the ones recorded from encode_pairs
    before the two were joined, values, dtypes and shapes"""
    many = ''.join(chr(0x100 + k) for k in range(255))
    i32 = lambda *v: np.asarray(v, dtype=np.int32).reshape(-1)               # noqa: E731
    cases = [
        # equal strings of one side share a range; x and q are ground truth only
        ((['abcab', 'cab', '', 'abcab'], ['abxab', 'abxab', 'q', 'abcab']),
         (np.asarray([0, 1, 2, 0, 1, 2, 0, 1, 0, 1, 255, 0, 1, 255, 0, 1, 2, 0, 1], np.uint8), i32(0, 5, 8, 0), i32(5, 3, 0, 5), i32(8, 8, 13, 14), i32(5, 5, 1, 5), 3)),
        # an empty side: no table, so every ground-truth character is 255
        ((['', ''], ['ab', '']), (np.asarray([255, 255], np.uint8), i32(0, 0), i32(0, 0), i32(0, 2), i32(2, 0), 0)),
        ((['', 'ba'], ['', 'ab']), (np.asarray([0, 1, 1, 0], np.uint8), i32(0, 0), i32(0, 2), i32(2, 2), i32(0, 2), 2)),
        (([], []), (np.zeros(0, np.uint8), i32(), i32(), i32(), i32(), 0)),
        # sigma at its limit: 254 codes, the 255th character is ground truth only
        (([many[:254]], [many]), (np.concatenate([np.arange(254), np.arange(254), [255]]).astype(np.uint8), i32(0), i32(254), i32(254), i32(255), 254)),
        # a string at the length limit
        ((['a' * PT.LEN_MAX], ['']), (np.zeros(PT.LEN_MAX, np.uint8), i32(0), i32(PT.LEN_MAX), i32(PT.LEN_MAX), i32(0), 1)),
    ]
    for args, want in cases:
        got = PT.encode_pairs(*args)
        assert len(got) == 6 and got[5] == want[5] and type(got[5]) is int, args
        for g, w in zip(got[:5], want[:5]):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (args, g, w)
    for args, text in ((([many], ['a']), 'the prediction strings hold 255 distinct characters; a call takes 254 -- score such pages on the host with '
                        'utils.lexicon.edit_distance_cpu'),
                       ((['a' * (PT.LEN_MAX + 1)], ['a']), 'a page string holds 65536 characters; the limit is 65535'),
                       ((['a'], ['a' * (PT.LEN_MAX + 1)]), 'a page string holds 65536 characters; the limit is 65535')):
        with pytest.raises(ValueError) as e:
            PT.encode_pairs(*args)
        assert str(e.value) == text


# -- page_string ------------------------------------------------------------------------------------------------------------------------
def test_page_string_strips_then_normalises_and_follows_the_fallbacks():
    recs = [dict(rec='Hel lo', lex=None), dict(rec='W\nx', lex='World'), dict(rec='STRASSE', lex=None)]
    assert PT.page_string(recs) == 'hellowxstrasse'
    assert PT.page_string(recs, 'lex') == 'helloworldstrasse'                               # None falls back to `rec`
    assert PT.page_string(recs, normalise=None) == 'HelloWxSTRASSE'
    assert PT.page_string(recs, strip='') == 'hel low\nxstrasse'
    assert PT.page_string(recs, strip='l', normalise=str.upper) == 'HE OW\nXSTRASSE'
    # the characters are removed BEFORE normalise runs: casefold makes 'ss' of the eszett, and stripping 's' afterwards would remove it
    assert PT.page_string(['Straße'], strip='s') == 'strasse' and PT.page_string(['Straße'], strip='S') == 'trasse'
    assert PT.page_string('A b\nC') == PT.page_string(['A', ' b', '\nC']) == PT.page_string([dict(text='A b'), dict(text='C')], 'text') == 'abc'
    assert PT.page_string([]) == ''
    with pytest.raises(KeyError):
        PT.page_string([dict(rec='a')], 'mgp_text')
    with pytest.raises(ValueError):
        PT.page_string([3])


# -- page_scores ------------------------------------------------------------------------------------------------------------------------
def test_page_scores_is_the_reference_formula():
    s = PT.page_scores([1, 3, 0, 0, 5], [5, 3, 0, 4, 0], [5, 5, 0, 4, 5])
    assert s['score'].dtype == np.float64 and s['score'].tolist() == [1 - 1 / 5, 1 - 3 / 5, 1.0, 1.0, 0.0]
    assert s['mean'] == pytest.approx((0.8 + 0.4 + 1 + 1 + 0) / 5) and s['micro'] == 1 - 9 / 19
    both_empty = PT.page_scores([0, 0], [0, 0], [0, 0])
    assert both_empty['score'].tolist() == [1.0, 1.0] and both_empty['mean'] == 1.0 and both_empty['micro'] == 1.0
    for bad in (([6], [5], [5]), ([-1], [5], [5]), ([1, 2], [5], [5])):
        with pytest.raises(ValueError):
            PT.page_scores(*bad)


# -- score_page_text and sweep_reading on a two-column page -----------------------------------------------------------------------------
class _HostReader(object):
    """ReadingOrder without a device: the two specifications behind the same interface"""

    def __init__(self, grid):
        self.grid, self.calls = grid, 0

    def __call__(self, polys, group_start, aspect, gap=2000, back=500, offset=500, blocks=None):
        self.calls += 1
        polys = torch.as_tensor(polys).numpy()
        res = RD.lines_cpu(polys, group_start, aspect, gap, back, offset, self.grid)
        if blocks is not None:
            res['blocks'] = RD.blocks_cpu(polys, group_start, aspect, res['line'], res['line_pos'], res['n_lines'], *blocks, grid=self.grid)
        return res


class _Recording(PT.HostPageScorer):
    def run(self, pool, a_off, a_len, b_off, b_len, sigma):
        self.last = dict(pool=np.asarray(pool).copy(), a_off=np.asarray(a_off).copy(), b_off=np.asarray(b_off).copy(), sigma=sigma)
        return super().run(pool, a_off, a_len, b_off, b_len, sigma)


def _word_of(name):
    return 'Head Line' if name == ('head',) else 'foot' if name == ('foot',) else 'c%dr%dk%d' % name[1:]


def two_column_page(seed=0):
    """-> (records shuffled, size, ground truth read column by column): the polygons are pixels of a 1000 x 1000 image, so they are
    their own bins on the 1000 grid"""
    pts, names = BC.column_page(cols=2, rows=5, words=2)
    order = np.random.RandomState(seed).permutation(len(pts))
    records = [dict(polys=pts[i].tolist(), rec=_word_of(names[i]), score=0.9) for i in order]
    truth = [_word_of(n) for n in [('head',)] + [('col', c, r, k) for c in range(2) for r in range(5) for k in range(2)] + [('foot',)]]
    return records, (GRID, GRID), truth


def _ordered(records, size, **kw):
    from advancedliteratemachinery_amd.utils import scoring as SC
    polys = [torch.from_numpy(SC.quantise([r['polys'] for r in records], size, GRID))]
    return RD.order_records([[dict(r) for r in records]], polys, [size], GRID, reader=_HostReader(GRID), **kw)[0]


def test_score_page_text_tells_column_order_from_line_order():
    records, size, truth = two_column_page()
    host = PT.HostPageScorer()
    by_line = _ordered(records, size)                                       # plain line order: the columns interleave
    by_block = _ordered(records, size, blocks=True)
    assert [r['rec'] for r in by_block] == truth
    assert [r['rec'] for r in by_line] != truth and sorted(r['rec'] for r in by_line) == sorted(truth)
    res = EV.score_page_text([by_line, by_block, records], [truth, ' '.join(truth), truth], scorer=host)
    assert host.calls == 1                                                  # all images in ONE call
    assert res['dist'].dtype == np.int32 and res['len_pred'].tolist() == res['len_gt'].tolist() == [len(''.join(truth).replace(' ', ''))] * 3
    assert res['score'][1] == 1.0 and res['dist'][1] == 0                   # blocks=True reads the page as the ground truth does
    assert res['score'][0] < res['score'][1] and res['dist'][0] > 0         # the interleaved columns cost
    assert res['dist'].tolist() == [LX.edit_distance_cpu(PT.page_string(r), PT.page_string(truth)) for r in (by_line, by_block, records)]
    assert res['mean'] == pytest.approx(res['score'].mean()) and res['micro'] == 1 - int(res['dist'].sum()) / (3 * int(res['len_gt'][0]))
    # case, the lexicon key with its fallback, the refusals
    assert EV.score_page_text([by_block], [[t.upper() for t in truth]], scorer=host)['dist'].tolist() == [0]
    assert EV.score_page_text([by_block], [[t.upper() for t in truth]], scorer=host, normalise=None)['dist'][0] > 0
    lex = [dict(r, lex=None if k % 2 else 'zz') for k, r in enumerate(by_block)]
    want = LX.edit_distance_cpu(''.join(r['rec'] if k % 2 else 'zz' for k, r in enumerate(by_block)).replace(' ', '').casefold(), PT.page_string(truth))
    assert EV.score_page_text([lex], [truth], text_key='lex', scorer=host)['dist'].tolist() == [want]
    empty = EV.score_page_text([[], []], ['', 'abc'], scorer=host)
    assert empty['score'].tolist() == [1.0, 0.0] and empty['dist'].tolist() == [0, 3]
    none = EV.score_page_text([], [], scorer=host)
    assert none['dist'].shape == (0,) and none['mean'] == 1.0 and none['micro'] == 1.0
    with pytest.raises(ValueError, match='text_key'):
        EV.score_page_text([by_block], [truth], text_key='nope', scorer=host)
    with pytest.raises(ValueError, match='per image'):
        EV.score_page_text([by_block], [truth, truth], scorer=host)
    with pytest.raises(ValueError, match='needs text-spotting records'):
        EV.score_page_text([[('entity', 'value')]], [truth], scorer=host)
    with pytest.raises(RuntimeError, match='MI355X'):
        PT.PageTextScorer('cpu')                                            # there is no CPU stage


def test_sweep_reading_picks_the_blocks_setting_in_one_scorer_call():
    records, size, truth = two_column_page(1)
    other, _, _ = two_column_page(2)
    before = [[dict(r) for r in records], [dict(r) for r in other]]
    scorer, reader = _Recording(), _HostReader(GRID)
    settings = [None, dict(), dict(blocks=True), dict(line_gap=0.0), dict(blocks=True, block_gap_x=10.0)]
    res = EV.sweep_reading([records, other], [size, size], GRID, [truth, truth], settings, reader=reader, scorer=scorer)
    assert scorer.calls == 1 and reader.calls == 4                          # ONE scorer.run; one reading call per setting that re-orders
    assert res['best'] == 2 and len(res['settings']) == 5
    assert res['settings'][2]['score'].tolist() == [1.0, 1.0] and res['settings'][2]['mean'] == 1.0
    assert all(s['mean'] < 1.0 for k, s in enumerate(res['settings']) if k != 2)
    assert [records, other] == before                                       # copies were re-ordered, not the records
    # a page's ground truth is stored once and shared by its settings (both pages hold the same text here: one range)
    assert len(set(scorer.last['b_off'].tolist())) == 1 and scorer.last['b_off'].size == 10
    # every entry equals score_page_text on the records ordered that way
    for st, got in zip(settings, res['settings']):
        pages = [records, other] if st is None else [_ordered(r, size, **st) for r in (records, other)]
        want = EV.score_page_text(pages, [truth, truth], scorer=PT.HostPageScorer())
        assert got['dist'].tolist() == want['dist'].tolist() and got['mean'] == want['mean'] and got['micro'] == want['micro']
    tie = EV.sweep_reading([records], [size], GRID, [truth], [dict(blocks=True), dict(blocks=True)], reader=reader, scorer=scorer)
    assert tie['best'] == 0                                                 # ties go to the lowest index
    for bad in ([], [dict(nope=1)], ['x']):
        with pytest.raises(ValueError):
            EV.sweep_reading([records], [size], GRID, [truth], bad, reader=reader, scorer=scorer)


def test_evaluate_reading_collects_the_batches_and_scores_once(monkeypatch):
    from advancedliteratemachinery_amd.engine import inference as inf
    from advancedliteratemachinery_amd.utils.parser import make_args
    a = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    pages = [two_column_page(k) for k in range(3)]
    seen = []

    def fake(model, imgs, args, file_names=None, preprocessor=None, **kw):
        seen.append((len(imgs), dict(kw)))
        lo = sum(n for n, _ in seen[:-1])
        return [[dict(r) for r in pages[lo + k][0]] for k in range(len(imgs))], preprocessor
    monkeypatch.setattr(inf, 'predict_images', fake)
    images = [np.zeros((GRID, GRID, 3), np.uint8)] * 3
    truth = [p[2] for p in pages]
    scorer = _Recording()
    res = EV.evaluate_reading(None, images, truth, a, batch=2, scorer=scorer, suppress=0.5)
    assert [n for n, _ in seen] == [2, 1] and seen[0][1] == dict(suppress=0.5) and scorer.calls == 1
    assert res['dist'].shape == (3,) and (res['score'] < 1.0).all() and [len(r) for r in res['records']] == [22] * 3
    seen.clear()
    res = EV.evaluate_reading(None, images, truth, a, batch=8, scorer=scorer, reader=_HostReader(GRID), settings=[None, dict(blocks=True)], bins=GRID)
    assert res['best'] == 1 and res['settings'][1]['mean'] == 1.0 and scorer.calls == 2
    a.infer_vie = True
    with pytest.raises(ValueError, match='infer_vie'):
        EV.evaluate_reading(None, images, truth, a, scorer=scorer)


# -- the command line ---------------------------------------------------------------------------------------------------------------
def test_eval_reading_scores_a_results_file(tmp_path, capsys):
    import sys
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import eval_reading
    pages = [two_column_page(k) for k in range(2)]
    names = ['page_%d.png' % k for k in range(2)]
    flat = [dict(r, image_id=n) for n, (recs, _, _) in zip(names, pages) for r in recs]
    (tmp_path / 'results.json').write_text(json.dumps(flat))
    gt = dict(images=[dict(file_name=n, height=GRID, width=GRID, text=(' '.join(t) if k else t)) for k, (n, (_, _, t)) in enumerate(zip(names, pages))])
    (tmp_path / 'gt.json').write_text(json.dumps(gt))
    common = ['--results', str(tmp_path / 'results.json'), '--gt', str(tmp_path / 'gt.json'), '--bins', str(GRID), '--tfm_pre_norm', '--use_fpn',
              '--use_char_window_prompt']
    doc = eval_reading.main(common, scorer=PT.HostPageScorer())
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(doc))
    want = EV.score_page_text([p[0] for p in pages], [p[2] for p in pages], scorer=PT.HostPageScorer())
    assert doc['dist'] == want['dist'].tolist() and doc['mean'] == want['mean'] and doc['images'] == 2 and doc['records'] == 44 and doc['mean'] < 1.0
    doc = eval_reading.main(common + ['--settings', json.dumps([None, dict(blocks=True), dict()])], scorer=PT.HostPageScorer(), reader=_HostReader(GRID))
    assert doc['best'] == 1 and doc['best_setting'] == dict(blocks=True) and doc['best_mean'] == 1.0
    assert [s['setting'] for s in doc['settings']] == [None, dict(blocks=True), dict()] and doc['settings'][0]['dist'] == want['dist'].tolist()


# -- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_entry_point_matches_the_header():
    from advancedliteratemachinery_amd import _lib, build, ops
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24   # the library only gains an entry point
    m = re.search(r'int omp_page_edit_distance\((.*?)\);', text, re.S)
    want = []
    for p in (' '.join(p.split()) for p in m.group(1).split(',')):
        if '*' in p or p.startswith('omp_stream_t'):
            want.append(ctypes.c_void_p)
        elif p.startswith('int64_t '):
            want.append(ctypes.c_int64)
        else:
            assert p.startswith('int '), p
            want.append(ctypes.c_int)
    res, args = _lib._SIGS['omp_page_edit_distance']
    assert res is ctypes.c_int and args == want and len(want) == 12 and 'omp_page_edit_distance' in _lib.EXPORTS
    assert 'page_text.hip' in build.SOURCES and 'page_text.hip' not in build.AUDITED
    assert callable(ops.page_edit_distance) and callable(ops.page_scratch_bytes)
    csrc = os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc')
    src = open(os.path.join(csrc, 'page_text.hip')).read()
    assert 'extern "C" int omp_page_edit_distance(' in src
    # the constants of the forward pass live in myers.h, which page_align.hip shares, and nowhere else
    hdr = open(os.path.join(csrc, 'myers.h')).read()
    assert 'myers.h' in [os.path.basename(h) for h in build.HEADERS] and '#include "myers.h"' in src
    assert 'PT_LEN_MAX = %d' % PT.LEN_MAX in hdr and 'PT_BLOCK = %d' % PT.BLOCK in hdr and 'PT_STRIPE = %d' % PT.STRIPE in hdr
    assert 'PT_SIGMA_MAX = %d' % PT.SIGMA_MAX in hdr and 'PT_NONE = %d' % PT.NONE in hdr
    assert not re.search(r'\w*(LEN_MAX|BLOCK|STRIPE|SIGMA_MAX|NONE|CARRY_WORDS)\s*=[^=]', src)
    assert 'PT_SLICE_BYTES = %d' % ops.PAGE_TEXT_SLICE_BYTES in hdr and ops.page_scratch_bytes(3) == 3 * ops.PAGE_TEXT_SLICE_BYTES
    assert PT.STRIPE == 64 * PT.BLOCK and PT.LEN_MAX == 65535
    assert PT.chunk_pairs(10, 3 * ops.PAGE_TEXT_SLICE_BYTES + 5) == [(0, 3), (3, 6), (6, 9), (9, 10)] and PT.chunk_pairs(0) == []
    with pytest.raises(ValueError):
        PT.chunk_pairs(1, ops.PAGE_TEXT_SLICE_BYTES - 1)
