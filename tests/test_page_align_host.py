"""Page text alignment on the host (no GPU): the numpy definition (utils/page_align.py) against a pure-Python table with the same
walk, the identities of the script, the worked examples, page_words, word_report_cpu and confusions on hand-made cases, align_page_text
with the host aligner on stub records, the scratch cap, the command line on a results file written here, and the C ABI's declaration.
The kernel and the device stage are tests/test_gpu_page_align.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from advancedliteratemachinery_amd.engine import evaluate as EV
from advancedliteratemachinery_amd.utils import page_align as PA
from advancedliteratemachinery_amd.utils import page_text as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(a, b):
    """the triple-min table in pure Python and the walk of the definition's three rules"""
    la, lb = len(a), len(b)
    ne = lambda i, j: 0 if (a[i - 1] == b[j - 1] and a[i - 1] != PT.NONE) else 1   # noqa: E731
    D = [[0] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        D[i][0] = i
    for j in range(lb + 1):
        D[0][j] = j
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            D[i][j] = min(D[i - 1][j - 1] + ne(i, j), D[i - 1][j] + 1, D[i][j - 1] + 1)
    a_map, b_map, counts = [-1] * la, [-1] * lb, [0, 0, 0, 0]
    i, j = la, lb
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1][j - 1] + ne(i, j) == D[i][j]:
            a_map[i - 1], b_map[j - 1] = j - 1, i - 1
            counts[ne(i, j)] += 1
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1][j] + 1 == D[i][j]:
            counts[2] += 1
            i -= 1
        else:
            counts[3] += 1
            j -= 1
    return D[la][lb], counts, a_map, b_map


def _codes(s):
    return np.asarray([ord(c) - ord('a') for c in s], dtype=np.uint8)


# -- align_cpu --------------------------------------------------------------------------------------------------------------------------
def test_align_cpu_equals_the_plain_table_and_walk_on_random_pairs():
    rng = np.random.RandomState(0)
    for _ in range(2000):
        sigma = int(rng.randint(1, 4))
        a = rng.randint(0, sigma, rng.randint(0, 10)).astype(np.uint8)
        b = rng.randint(0, sigma, rng.randint(0, 10)).astype(np.uint8)
        if rng.rand() < 0.3:
            b[rng.rand(b.size) < 0.3] = PT.NONE
        dist, counts, a_map, b_map = PA.align_cpu(a, b)
        want = _plain(a.tolist(), b.tolist())
        assert (dist, counts.tolist(), a_map.tolist(), b_map.tolist()) == want, (a, b)
        assert counts.dtype == a_map.dtype == b_map.dtype == np.int32


def test_the_identities_of_the_script():
    rng = np.random.RandomState(1)
    for _ in range(300):
        sigma = int(rng.choice([1, 2, 4, 26]))
        a = rng.randint(0, sigma, rng.randint(0, 90)).astype(np.uint8)
        b = rng.randint(0, sigma, rng.randint(0, 90)).astype(np.uint8)
        if rng.rand() < 0.3:
            b[rng.rand(b.size) < 0.2] = PT.NONE
        dist, (match, sub, ins, dele), a_map, b_map = PA.align_cpu(a, b)
        assert sub + ins + dele == dist == PT.distance_cpu(a, b)
        assert match + sub + ins == a.size and match + sub + dele == b.size
        hit = a_map[a_map >= 0]
        assert (np.diff(hit) > 0).all() and int((a_map < 0).sum()) == ins and int((b_map < 0).sum()) == dele
        at = np.flatnonzero(a_map >= 0)
        assert (b_map[hit] == at).all() and (a_map[b_map[b_map >= 0]] == np.flatnonzero(b_map >= 0)).all()   # mutual inverses
        same = (a[at] == b[hit]) & (a[at] != PT.NONE)
        assert int(same.sum()) == match


def test_the_worked_examples():
    dist, counts, a_map, b_map = PA.align_cpu(_codes('ab'), _codes('ba'))
    assert dist == 2 and counts.tolist() == [0, 2, 0, 0] and a_map.tolist() == [0, 1] and b_map.tolist() == [0, 1]
    dist, counts, a_map, b_map = PA.align_cpu(_codes('aaa'), _codes('a'))
    assert dist == 2 and counts.tolist() == [1, 0, 2, 0] and a_map.tolist() == [-1, -1, 0] and b_map.tolist() == [2]   # the LAST a matches
    dist, counts, a_map, b_map = PA.align_cpu(_codes('a'), _codes('aaa'))
    assert dist == 2 and counts.tolist() == [1, 0, 0, 2] and b_map.tolist() == [-1, -1, 0] and a_map.tolist() == [2]
    dist, counts, a_map, b_map = PA.align_cpu([], [])
    assert dist == 0 and counts.tolist() == [0, 0, 0, 0] and a_map.size == 0 and b_map.size == 0
    assert PA.align_cpu([PT.NONE], [PT.NONE])[1].tolist() == [0, 1, 0, 0]   # 255 equals nothing, itself included: a SUB
    assert PA.align_cpu([1, 2], [])[1].tolist() == [0, 0, 2, 0] and PA.align_cpu([], [1, 2])[1].tolist() == [0, 0, 0, 2]


def test_table_cpu_and_distance_cpu_share_one_row_recurrence():
    """table_cpu stacks the rows distance_cpu takes the last of (page_text._rows): the corner is the distance, the table of (b, a) is
    the transpose, and the table equals the plain triple-min one -- at lengths around one and two 64-character blocks"""
    rng = np.random.RandomState(5)
    lengths = (0, 1, 2, 64, 65)
    for kind in ('sigma 1', 'sigma 26', 'a side of 255'):
        for la in lengths:
            for lb in lengths:
                sigma = 1 if kind == 'sigma 1' else 26
                a, b = rng.randint(0, sigma, la).astype(np.uint8), rng.randint(0, sigma, lb).astype(np.uint8)
                if kind == 'a side of 255':
                    b[:] = PT.NONE
                D = PA.table_cpu(a, b)
                assert D.shape == (la + 1, lb + 1) and D.dtype == np.int32 and D.flags['C_CONTIGUOUS'], (kind, la, lb)
                assert int(D[-1, -1]) == PT.distance_cpu(a, b) == PT.distance_cpu(b, a), (kind, la, lb)
                assert np.array_equal(PA.table_cpu(b, a), D.T), (kind, la, lb)
                assert D[0].tolist() == list(range(lb + 1)) and D[:, 0].tolist() == list(range(la + 1))
                ne = ((a[:, None] != b[None, :]) | (a[:, None] == PT.NONE)).astype(np.int64)
                want = np.zeros((la + 1, lb + 1), np.int64)
                want[0], want[:, 0] = np.arange(lb + 1), np.arange(la + 1)
                for i in range(1, la + 1):
                    for j in range(1, lb + 1):
                        want[i, j] = min(want[i - 1, j - 1] + ne[i - 1, j - 1], want[i - 1, j] + 1, want[i, j - 1] + 1)
                assert np.array_equal(D, want), (kind, la, lb)
                if kind == 'a side of 255':
                    assert int(D[-1, -1]) == max(la, lb)


def test_pairs_align_cpu_lays_the_maps_out_by_map_off():
    pool = np.concatenate([_codes('abcab'), _codes('abxb'), _codes('b')])
    a_off, a_len, b_off, b_len = [0, 5, 0], [5, 4, 5], [5, 0, 9], [4, 5, 1]
    map_off = [3, 20, 40]
    counts, maps = PA.pairs_align_cpu(pool, a_off, a_len, b_off, b_len, map_off)
    assert counts.shape == (3, 4) and counts.dtype == np.int32 and maps.dtype == np.int32 and maps.size == 46
    for p in range(3):
        a, b = pool[a_off[p]:a_off[p] + a_len[p]], pool[b_off[p]:b_off[p] + b_len[p]]
        _, c, am, bm = PA.align_cpu(a, b)
        at = map_off[p]
        assert counts[p].tolist() == c.tolist() and maps[at:at + a_len[p]].tolist() == am.tolist()
        assert maps[at + a_len[p]:at + a_len[p] + b_len[p]].tolist() == bm.tolist()
    owned = np.zeros(46, bool)
    for p in range(3):
        owned[map_off[p]:map_off[p] + a_len[p] + b_len[p]] = True
    assert (maps[~owned] == PA.GAP).all()
    assert PA.dense_map_off(a_len, b_len).tolist() == [0, 9, 18]
    res = PA.HostPageAligner().run(pool, a_off, a_len, b_off, b_len, 24)
    assert res['counts'].tolist() == counts.tolist() and res['maps'].size == 24 and res['map_off'].dtype == np.int64
    assert [m.tolist() for m in PA.split_maps(res, a_len, b_len, 1)] == [maps[20:24].tolist(), maps[24:29].tolist()]
    with pytest.raises(ValueError):
        PA.pairs_align_cpu(pool, a_off, a_len, b_off, b_len, [0, -1, 2])
    with pytest.raises(ValueError):
        PA.pairs_align_cpu(pool, a_off, a_len, b_off, b_len, [0, 1])
    with pytest.raises(ValueError):
        PA.pairs_align_cpu(pool, a_off, [5, 4, 11], b_off, b_len, map_off)            # a range outside the pool


# -- words --------------------------------------------------------------------------------------------------------------------------------
def test_page_words_concatenates_to_the_page_string_under_casefold():
    recs = [dict(rec='Hel lo', lex=None), dict(rec='W\nx', lex='World'), dict(rec=' \n', lex=None), dict(rec='STRASSE', lex=None)]
    for field in ('rec', 'lex'):
        text, w_start, w_len = PA.page_words(recs, field)
        assert text == PT.page_string(recs, field) and w_start.dtype == w_len.dtype == np.int32
        assert [text[s:s + n] for s, n in zip(w_start, w_len)] == [PT.page_string([r], field) for r in recs]
    assert PA.page_words(recs)[2].tolist() == [5, 2, 0, 7]
    assert PA.page_words('A b\nC')[0] == 'abc' and PA.page_words('A b\nC')[2].tolist() == [3]          # one string = one word
    text, w_start, w_len = PA.page_words(['Ab', ' c', 'D e'], normalise=None)
    assert (text, w_start.tolist(), w_len.tolist()) == ('AbcDe', [0, 2, 3], [2, 1, 2])
    assert PA.page_words([dict(text='A b'), dict(text='C')], 'text')[0] == 'abc'
    # a normalise that is not per character: the per-word string is the one that is aligned
    rev = lambda s: s[::-1]                                                 # noqa: E731
    assert PA.page_words(['ab', 'cd'], normalise=rev)[0] == 'badc' and PT.page_string(['ab', 'cd'], normalise=rev) == 'dcba'
    empty = PA.page_words([])
    assert empty[0] == '' and empty[1].shape == (0,) and empty[2].shape == (0,)


def test_word_report_and_confusions_on_hand_made_pages():
    pred = 'helloworlzzfoo'                                                 # hello | worl | zz | '' | foo
    gt = 'hellowor1dfoobar'                                                 # hello | wor1d | foo | bar
    p_start, p_len = [0, 5, 9, 11, 11], [5, 4, 2, 0, 3]
    t_start, t_len = [0, 5, 10, 13], [5, 5, 3, 3]
    enc = PT.encode_pairs([pred], [gt])
    dist, counts, a_map, b_map = PA.align_cpu(enc[0][enc[1][0]:enc[1][0] + len(pred)], enc[0][enc[3][0]:enc[3][0] + len(gt)])
    assert dist == PT.distance_cpu(enc[0][:len(pred)], enc[0][len(pred):])
    status, span = PA.word_report_cpu(a_map, p_start, p_len, pred, gt)
    assert status.dtype == np.int8 and span.dtype == np.int32 and span.shape == (5, 2)
    assert status[0] == PA.CORRECT and span[0].tolist() == [0, 5] and status[3] == PA.EMPTY and span[3].tolist() == [-1, -1]
    assert status[4] == PA.CORRECT and span[4].tolist() == [10, 13]
    assert status[1] == PA.WRONG                                            # worl against wor1d
    t_status, t_span = PA.word_report_cpu(b_map, t_start, t_len, gt, pred)
    assert t_status.tolist() == [PA.CORRECT, PA.WRONG, PA.CORRECT, PA.ABSENT] and t_span[3].tolist() == [-1, -1] and t_span[2].tolist() == [11, 14]
    # a word split by a deleted character is WRONG although every mapped pair is equal; an absent word; hand-made maps
    x_map = np.asarray([0, 1, 3, 4, -1, -1, 5])                             # x = abde | zz | f, y = abcdef
    status, span = PA.word_report_cpu(x_map, [0, 4, 6, 7], [4, 2, 1, 0], 'abdezzf', 'abcdef')
    assert status.tolist() == [PA.WRONG, PA.ABSENT, PA.CORRECT, PA.EMPTY] and span.tolist() == [[0, 5], [-1, -1], [5, 6], [-1, -1]]
    y_map = np.asarray([0, 1, -1, 2, 3, 6])
    status, span = PA.word_report_cpu(y_map, [0, 2, 3], [2, 1, 3], 'abcdef', 'abdezzf')
    assert status.tolist() == [PA.CORRECT, PA.ABSENT, PA.WRONG] and span.tolist() == [[0, 2], [-1, -1], [2, 7]]
    assert PA.word_report_cpu([0, 1], [0], [2], 'ab', 'ax')[0].tolist() == [PA.WRONG]     # a substituted character
    with pytest.raises(ValueError):
        PA.word_report_cpu([0], [0], [2], 'ab', 'ab')
    conf = PA.confusions('abdezzf', 'abcdef', x_map, y_map)
    assert conf == dict(sub={}, ins={'z': 2}, dele={'c': 1})
    conf = PA.confusions('hel1o', 'hello', [0, 1, 2, 3, 4], [0, 1, 2, 3, 4])
    assert conf == dict(sub={('1', 'l'): 1}, ins={}, dele={})


# -- align_page_text ------------------------------------------------------------------------------------------------------------------
def _box(x0, y0, x1, y1):
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


def _stub_pages():
    words = ['Invoice', 'No', '12345', 'EUR', 'EUR', 'Tota1', '99']
    recs = [dict(polys=_box(10 + 100 * k, 20, 90 + 100 * k, 50), rec=w, score=0.9) for k, w in enumerate(words)]
    truth = ['Thanks', 'Invoice', 'No.', '12345', 'EUR', 'Total', '99']
    other = [dict(polys=_box(5, 5, 50, 30), rec='in voice', score=0.9), dict(polys=_box(60, 5, 90, 30), rec='x', score=0.9)]
    return [recs, other, []], [truth, 'In\nvoice', ['lost']]


def test_align_page_text_with_the_host_aligner_on_stub_records():
    records, truth = _stub_pages()
    host = PA.HostPageAligner()
    res = EV.align_page_text(records, truth, aligner=host)
    assert host.calls == 1                                                  # all images in ONE call
    want = EV.score_page_text(records, truth, scorer=PT.HostPageScorer())
    for k in ('dist', 'len_pred', 'len_gt'):
        assert res[k].tolist() == want[k].tolist() and res[k].dtype == np.int32
    assert (res['score'] == want['score']).all() and res['mean'] == want['mean'] and res['micro'] == want['micro']
    assert (res['sub'] + res['ins'] + res['dele']).tolist() == res['dist'].tolist()
    assert (res['match'] + res['sub'] + res['ins']).tolist() == res['len_pred'].tolist()
    assert (res['match'] + res['sub'] + res['dele']).tolist() == res['len_gt'].tolist()
    assert res['cer'] == [int(d) / int(n) for d, n in zip(res['dist'], res['len_gt'])] and res['cer_micro'] == int(res['dist'].sum()) / int(res['len_gt'].sum())
    page = res['pages'][0]
    assert page['pred'] == 'invoiceno12345eureurtota1' + '99' and page['gt'] == 'thanksinvoiceno.12345eurtotal99'
    assert page['pred_to_gt'].dtype == np.int32 and len(page['pred_to_gt']) == len(page['pred']) and len(page['gt_to_pred']) == len(page['gt'])
    assert [w['status'] for w in page['words']] == ['correct', 'correct', 'correct', 'absent', 'correct', 'wrong', 'correct']
    assert page['words'][0]['chars'] == (0, 7) and page['words'][0]['span'] == (6, 13) and page['words'][3]['span'] == (-1, -1)
    gw = {w['text']: w for w in page['gt_words']}
    assert [w['status'] for w in page['gt_words']] == ['absent', 'correct', 'wrong', 'correct', 'correct', 'wrong', 'correct']
    assert gw['invoice']['records'] == (0, 0) and gw['invoice']['box'] == (10.0, 20.0, 90.0, 50.0)
    assert gw['no.']['records'] == (1, 1) and gw['no.']['box'] == (110.0, 20.0, 190.0, 50.0)
    assert gw['total']['records'] == (5, 5) and gw['total']['box'] == (510.0, 20.0, 590.0, 50.0)
    assert gw['eur']['records'] == (4, 4) and gw['eur']['span'] == (17, 20)     # the walk starts at the end: the LAST of the two EURs
    assert gw['99']['box'] == (610.0, 20.0, 690.0, 50.0)
    assert gw['thanks']['box'] is None and gw['thanks']['records'] is None and gw['thanks']['span'] == (-1, -1)
    # a ground-truth word carried by two records gets the union of their polygons
    two = res['pages'][1]['gt_words']
    assert len(two) == 1 and two[0]['text'] == 'invoice' and two[0]['status'] == 'correct' and two[0]['records'] == (0, 0)
    split = EV.align_page_text([[dict(polys=_box(0, 0, 10, 10), rec='in'), dict(polys=_box(20, 5, 40, 30), rec='voice')]], [['Invoice']], aligner=host)
    w = split['pages'][0]['gt_words'][0]
    assert w['status'] == 'correct' and w['records'] == (0, 1) and w['box'] == (0.0, 0.0, 40.0, 30.0)
    assert [x['status'] for x in split['pages'][0]['words']] == ['correct', 'correct'] and split['word_precision'] == 1.0 and split['word_recall'] == 1.0
    # the totals
    assert res['word_precision'] == (5 + 1 + 0) / (7 + 2 + 0) and res['word_recall'] == (4 + 1 + 0) / (7 + 1 + 1)
    conf = res['confusions']
    assert dict(conf['sub']) == {('1', 'l'): 1} and dict(conf['ins'])['x'] == 1 and dict(conf['ins'])['e'] == 1 and dict(conf['dele'])['.'] == 1
    assert [n for _, n in conf['dele']] == sorted((n for _, n in conf['dele']), reverse=True)
    assert len(EV.align_page_text(records, truth, aligner=host, top=1)['confusions']['dele']) == 1
    # one string per page: no word recall; an empty ground truth: no CER
    one = EV.align_page_text([records[0], []], ['Invoice No', ''], aligner=host)
    assert one['word_recall'] is None and one['cer'][1] is None and one['cer'][0] > 0 and one['score'][1] == 1.0
    none = EV.align_page_text([], [], aligner=host)
    assert none['dist'].shape == (0,) and none['pages'] == [] and none['cer_micro'] is None and none['word_precision'] is None
    with pytest.raises(ValueError, match='text_key'):
        EV.align_page_text(records, truth, text_key='nope', aligner=host)
    with pytest.raises(ValueError, match='per image'):
        EV.align_page_text(records, truth[:2], aligner=host)
    with pytest.raises(RuntimeError, match='MI355X'):
        PA.PageAligner('cpu')                                               # there is no CPU stage


def test_a_pair_above_the_scratch_cap_is_refused_with_its_size():
    from advancedliteratemachinery_amd import ops
    need = ops.page_align_scratch_bytes(PT.LEN_MAX, PT.LEN_MAX)
    assert need > PA.SCRATCH_CAP == 1 << 30
    with pytest.raises(ValueError, match=str(need)):
        PA.chunk_pairs([10, PT.LEN_MAX], [10, PT.LEN_MAX])
    one = ops.page_align_scratch_bytes(100, 100)
    with pytest.raises(ValueError, match=str(one)):
        PA.chunk_pairs([100], [100], scratch_cap=one - 1)
    assert PA.chunk_pairs([100] * 5, [100] * 5, scratch_cap=2 * one) == [(0, 2), (2, 4), (4, 5)]
    assert PA.chunk_pairs([100] * 5, [100] * 5, scratch_cap=one) == [(k, k + 1) for k in range(5)]
    assert PA.chunk_pairs([100] * 5, [100] * 5) == [(0, 5)] and PA.chunk_pairs([], []) == []
    assert PA.chunk_pairs([100] * 3, [100] * 3, maps_cap=450) == [(0, 2), (2, 3)]


# -- the command line -----------------------------------------------------------------------------------------------------------------
def test_align_text_reports_a_results_file(tmp_path, capsys):
    import sys
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import align_text
    records, truth = _stub_pages()
    names = ['page_%d.png' % k for k in range(3)]
    flat = [dict(r, image_id=n) for n, recs in zip(names, records) for r in recs]
    (tmp_path / 'results.json').write_text(json.dumps(flat))
    (tmp_path / 'gt.json').write_text(json.dumps(dict(images=[dict(file_name=n, text=t) for n, t in zip(names, truth)])))
    doc = align_text.main(['--results', str(tmp_path / 'results.json'), '--gt', str(tmp_path / 'gt.json'), '--host', '--top', '3'])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(doc))
    want = EV.align_page_text(records, truth, aligner=PA.HostPageAligner(), top=3)
    assert [p['dist'] for p in doc['pages']] == want['dist'].tolist() and doc['mean'] == want['mean'] and doc['images'] == 3 and doc['records'] == 9
    assert doc['sub'] == int(want['sub'].sum()) and doc['ins'] == int(want['ins'].sum()) and doc['dele'] == int(want['dele'].sum())
    assert doc['word_precision'] == want['word_precision'] and doc['word_recall'] == want['word_recall'] and doc['host'] is True
    assert doc['confusions']['sub'] == [['1', 'l', 1]] and len(doc['confusions']['dele']) == 3
    assert doc['pages'][0]['gt_words'][5] == dict(text='total', status='wrong', chars=[24, 29], span=[20, 25], records=[5, 5], box=[510.0, 20.0, 590.0, 50.0])
    assert doc['pages'][0]['gt_words'][0]['box'] is None and doc['pages'][2]['cer'] == 1.0


# -- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_point_matches_the_header():
    from advancedliteratemachinery_amd import _lib, build, ops
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24   # the library only gains an entry point
    m = re.search(r'int omp_page_align\((.*?)\);', text, re.S)
    want = []
    for p in (' '.join(p.split()) for p in m.group(1).split(',')):
        if '*' in p or p.startswith('omp_stream_t'):
            want.append(ctypes.c_void_p)
        elif p.startswith('int64_t '):
            want.append(ctypes.c_int64)
        else:
            assert p.startswith('int '), p
            want.append(ctypes.c_int)
    res, args = _lib._SIGS['omp_page_align']
    assert res is ctypes.c_int and args == want and len(want) == 16 and 'omp_page_align' in _lib.EXPORTS
    assert 'page_align.hip' in build.SOURCES and 'page_align.hip' not in build.AUDITED
    assert callable(ops.page_align) and callable(ops.page_align_scratch_bytes)
    csrc = os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc')
    src = open(os.path.join(csrc, 'page_align.hip')).read()
    assert 'extern "C" int omp_page_align(' in src
    # the forward pass and its constants are page_text.hip's: both take them from myers.h, and neither keeps a copy
    hdr = open(os.path.join(csrc, 'myers.h')).read()
    assert 'myers.h' in [os.path.basename(h) for h in build.HEADERS] and '#include "myers.h"' in src
    assert 'PT_LEN_MAX = %d' % PT.LEN_MAX in hdr and 'PT_BLOCK = %d' % PT.BLOCK in hdr and 'PT_STRIPE = %d' % PT.STRIPE in hdr
    assert 'PT_SIGMA_MAX = %d' % PT.SIGMA_MAX in hdr and 'PT_NONE = %d' % PT.NONE in hdr
    for unit in (src, open(os.path.join(csrc, 'page_text.hip')).read()):
        assert not re.search(r'\w*(LEN_MAX|BLOCK|STRIPE|SIGMA_MAX|NONE|CARRY_WORDS)\s*=[^=]', unit)
    assert 'PA_CARRY_BYTES = %d' % ops.PAGE_ALIGN_CARRY_BYTES in src and 'PA_CELL_BYTES = %d' % ops.PAGE_ALIGN_CELL_BYTES in src
    for la, lb in ((64, 65535), (65535, 64), (4097, 4097), (0, 0), (1, 1), (65535, 65535)):
        need = ops.page_align_scratch_bytes(la, lb)
        assert 0 < need <= 32 * ((la + 63) // 64) * lb + 65536 and need % 8 == 0, (la, lb)
        assert need == ops.PAGE_ALIGN_CARRY_BYTES + ops.PAGE_ALIGN_CELL_BYTES * ((la + 63) // 64) * lb
