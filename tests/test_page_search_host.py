"""Page search on the host (no GPU): the numpy definition (utils/page_search.py) against the plain double loop, the warm-up fact the
kernel rests on, the hits against a literal restatement of the rule and the starts against brute force, the fixed cases, the tolerance,
the queries and the encoding, find_text on a hand-made page with the host searcher, the command line on a results file written here, and
the C ABI's declaration.  The kernel and the device stage are tests/test_gpu_page_search.py."""
import ctypes
import itertools
import json
import os
import re

import numpy as np
import pytest

from advancedliteratemachinery_amd.engine.search import find_text
from advancedliteratemachinery_amd.utils import lexicon as LX
from advancedliteratemachinery_amd.utils import page_search as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plant(rng, m, n, sigma):
    """a random query and text; half of the pairs have the query planted, and half of those one planted character set to 255"""
    q = rng.randint(0, sigma, m).astype(np.uint8)
    t = rng.randint(0, sigma, n).astype(np.uint8)
    kind = 'random'
    if n >= m and rng.rand() < 0.5:
        at = int(rng.randint(0, n - m + 1))
        t[at:at + m] = q
        kind = 'planted'
        if rng.rand() < 0.5:
            t[at + int(rng.randint(0, m))] = PS.NONE
            kind = 'planted, one 255'
    return q, t, kind


_CASES = {}


def random_cases():
    """300 pairs: m in 1 .. 12, n in 0 .. 60, sigma in {1, 2, 3, 26}; made once and shared, never changed"""
    if not _CASES:
        rng = np.random.RandomState(0)
        cases = []
        for i in range(300):
            sigma = (1, 2, 3, 26)[i % 4]
            q, t, kind = _plant(rng, int(rng.randint(1, 13)), int(rng.randint(0, 61)), sigma)
            cases.append((q, t, kind, PS.row_cpu(q, t)))
        _CASES['cases'] = cases
    return _CASES['cases']


def _distance(q, s):
    """the plain edit distance in which 255 is replaced by symbols that occur once: 255 equals nothing"""
    fresh = itertools.count(1000)
    return LX.edit_distance_cpu([next(fresh) if v == PS.NONE else int(v) for v in q], [next(fresh) if v == PS.NONE else int(v) for v in s])


def _search1(q, t, k, H=16):
    q, t = np.asarray(q, np.uint8), np.asarray(t, np.uint8)
    res = PS.search_cpu(np.concatenate([t, q]), [0], [t.size], [t.size], [q.size], [[0, 0]], [k], H)
    return tuple(res['best'][0].tolist()), int(res['n_hits'][0]), [tuple(h) for h in res['hits'][0].tolist() if h[0] >= 0]


def _codes(query, text):
    pool, po, pl, qo, ql, _ = PS.encode_search([text], [query])
    return pool[qo[0]:qo[0] + ql[0]], pool[po[0]:po[0] + pl[0]]


# -- the row ----------------------------------------------------------------------------------------------------------------------------
def test_row_cpu_equals_the_double_loop_on_every_short_binary_string():
    strings = [list(s) for n in range(5) for s in itertools.product((0, 1), repeat=n)]
    assert len(strings) == 31
    for q in strings[1:]:
        for t in strings:
            assert PS.row_cpu(q, t).tolist() == PS.row_py(q, t).tolist(), (q, t)


def test_row_cpu_equals_the_double_loop_on_random_pairs():
    kinds = {}
    for q, t, kind, v in random_cases():
        kinds[kind] = kinds.get(kind, 0) + 1
        assert v.dtype == np.int32 and v.tolist() == PS.row_py(q, t).tolist(), (q, t)
        assert v[0] == q.size and (np.abs(np.diff(v)) <= 1).all()           # adjacent v differ by at most 1
    assert min(kinds.get(k, 0) for k in ('random', 'planted', 'planted, one 255')) >= 30, kinds


def test_a_255_equals_nothing_itself_included():
    assert PS.row_cpu([255], [255, 255]).tolist() == [1, 1, 1] and PS.row_cpu([3], [255, 3]).tolist() == [1, 1, 0]
    assert PS.row_py([255], [255]).tolist() == [1, 1]


def test_the_warm_up_fact_on_every_column():
    """v_j computed on t[max(0, j - 2m) : j] from a fresh column equals v_j of the whole text: what lets a lane start in mid-text"""
    checked = 0
    for q, t, _, v in random_cases():
        for j in range(t.size + 1):
            assert PS.row_cpu(q, t[max(0, j - 2 * q.size):j])[-1] == v[j], (q, t, j)
            checked += 1
    assert checked > 5000


# -- the hits ---------------------------------------------------------------------------------------------------------------------------
def _literal_hits(v, k):
    n = len(v) - 1
    return [j for j in range(1, n + 1) if v[j] <= k and v[j] <= v[j - 1] and (j == n or v[j] < v[j + 1])]


def test_search_cpu_hits_and_starts_against_the_rule_and_brute_force():
    rng = np.random.RandomState(1)
    total, over = 0, 0
    jobs = []
    for q, t, _, v in random_cases():
        jobs.append((q, t, int(rng.randint(0, q.size)), 16, v))
    for _ in range(60):                                                       # a phrase planted 5 times, 2 hits kept
        q = rng.randint(0, 26, int(rng.randint(3, 9))).astype(np.uint8)
        t = np.concatenate([np.concatenate([rng.randint(0, 26, int(rng.randint(4, 12))).astype(np.uint8), q]) for _ in range(5)])
        jobs.append((q, t, 1, 2, PS.row_cpu(q, t)))
    for q, t, k, H, v in jobs:
        best, n_hits, hits = _search1(q, t, k, H)
        v = v.tolist()
        want = _literal_hits(v, k)
        assert best == (min(v), v.index(min(v)))
        assert n_hits == len(want) and [h[0] for h in hits] == want[:H] and all(h[1] == v[h[0]] for h in hits)
        for end, dist, start in hits:
            fits = [s for s in range(end + 1) if _distance(q, t[s:end]) == dist]
            assert start == max(fits) and end - start <= q.size + dist, (q, t, end, dist, start)
        total += n_hits
        over += n_hits > H
    assert total >= 1000 and over >= 20, (total, over)


def test_fixed_cases():
    assert _search1(*_codes('total', 'sub total 12 totai amount total'), 1) == ((0, 9), 3, [(9, 0, 4), (18, 1, 13), (31, 0, 26)])
    assert _search1(*_codes('aa', 'aaaa'), 0) == ((0, 2), 1, [(4, 0, 2)])   # a run yields its last occurrence only
    assert _search1(*_codes('invoice no', 'lnvoice n0: 1234'), 2)[1:] == (1, [(10, 2, 1)])
    assert _search1(*_codes('abc', ''), 2) == ((3, 0), 0, [])               # n = 0: the empty match
    assert _search1([0, 1, 0], [255] * 9, 2) == ((3, 0), 0, [])             # a page of only 255 codes
    rng = np.random.RandomState(2)
    q = rng.randint(0, 26, 64).astype(np.uint8)
    t = np.concatenate([rng.randint(0, 26, 50), q, rng.randint(0, 26, 50)]).astype(np.uint8)
    assert _search1(q, t, 0) == ((0, 114), 1, [(114, 0, 50)])               # m = 64
    t[70] = 255
    assert _search1(q, t, 63, 64)[0] == (1, 114) and (114, 1, 50) in _search1(q, t, 63, 64)[2]


def test_search_cpu_refuses_what_the_limits_exclude():
    pool = np.zeros(10, np.uint8)
    ok = dict(pool=pool, page_off=[0], page_len=[6], query_off=[6], query_len=[4], jobs=[[0, 0]], k=[1], max_hits=4)
    PS.search_cpu(**ok)
    for kw in (dict(k=[4]), dict(k=[-1]), dict(query_len=[0]), dict(query_len=[65]), dict(page_len=[11]), dict(query_off=[7]), dict(max_hits=0),
               dict(max_hits=65), dict(jobs=[[1, 0]]), dict(jobs=[[0, 1]]), dict(page_len=[PS.LEN_MAX + 1])):
        with pytest.raises(ValueError):
            PS.search_cpu(**dict(ok, **kw))


# -- tolerance, queries, codes ----------------------------------------------------------------------------------------------------------
def test_tolerance():
    assert [PS.tolerance(m) for m in (1, 4, 5, 9, 10, 64)] == [0, 0, 1, 1, 2, 12]
    assert PS.tolerance(10, max_dist=1) == 1 and PS.tolerance(10, max_dist=5) == 2 and PS.tolerance(10, max_ratio=None) == 9
    assert PS.tolerance(3, max_ratio=1.0) == 2 and PS.tolerance(10, max_ratio=0.0) == 0 and PS.tolerance(10, max_dist=0, max_ratio=None) == 0
    for bad in (dict(m=0), dict(m=65), dict(m=5, max_ratio=1.5), dict(m=5, max_dist=-1)):
        with pytest.raises(ValueError):
            PS.tolerance(**bad)


def test_normalise_query():
    assert PS.normalise_query('  Invoice \t No ') == 'invoice no' and PS.normalise_query('Straße') == 'strasse'
    assert PS.normalise_query('A  b', sep='', normalise=None) == 'Ab'
    assert PS.normalise_query('x' * 64) == 'x' * 64
    for bad in ('x' * 65, '', '   '):
        with pytest.raises(ValueError) as e:
            PS.normalise_query(bad)
        assert repr(bad) in str(e.value)


def test_encode_search_shares_ranges_and_keeps_the_limits():
    pool, po, pl, qo, ql, sigma = PS.encode_search(['ab cd', 'xyz', 'ab cd', ''], ['cd', 'b c', 'cd'])
    assert sigma == 4 and pool.dtype == np.uint8                           # c, d, b and the blank
    assert po.tolist() == [0, 5, 0, 8] and pl.tolist() == [5, 3, 5, 0] and qo.tolist() == [8, 10, 8] and ql.tolist() == [2, 3, 2]
    assert pool.tolist() == [255, 2, 3, 0, 1, 255, 255, 255, 0, 1, 2, 3, 0]
    with pytest.raises(ValueError):
        PS.encode_search(['a'], ['x' * 65])
    with pytest.raises(ValueError):
        PS.encode_search(['a' * (PS.LEN_MAX + 1)], ['a'])
    chars = [chr(0x4e00 + i) for i in range(255)]
    assert PS.encode_search([''], [''.join(chars[:254][i:i + 64]) for i in range(0, 254, 64)])[5] == 254
    with pytest.raises(ValueError):
        PS.encode_search([''], [''.join(chars[i:i + 64]) for i in range(0, 255, 64)])


def test_encode_search_gives_the_recorded_pools_and_tables():
    """encode_search goes through page_text._encode, which encode_pairs shares: the outputs are the ones recorded from encode_search
    before the two were joined, values, dtypes and shapes"""
    chars = [chr(0x4e00 + i) for i in range(255)]
    i32 = lambda *v: np.asarray(v, dtype=np.int32).reshape(-1)               # noqa: E731
    cases = [
        # equal strings of one side share a range; a, x, y and z are page characters only
        ((['ab cd', 'xyz', 'ab cd', ''], ['cd', 'b c', 'cd']),
         (np.asarray([255, 2, 3, 0, 1, 255, 255, 255, 0, 1, 2, 3, 0], np.uint8), i32(0, 5, 0, 8), i32(5, 3, 5, 0), i32(8, 10, 8), i32(2, 3, 2), 4)),
        # sigma at its limit, against one empty page
        (([''], [''.join(chars[:254][i:i + 64]) for i in range(0, 254, 64)]),
         (np.arange(254).astype(np.uint8), i32(0), i32(0), i32(0, 64, 128, 192), i32(64, 64, 64, 62), 254)),
        # a page at the length limit, none of its characters in a query
        ((['z' * PS.LEN_MAX, ''], ['a']),
         (np.concatenate([np.full(PS.LEN_MAX, 255), [0]]).astype(np.uint8), i32(0, PS.LEN_MAX), i32(PS.LEN_MAX, 0), i32(PS.LEN_MAX), i32(1), 1)),
        # an empty side: no pages
        (([], ['ab', 'ab']), (np.asarray([0, 1], np.uint8), i32(), i32(), i32(0, 0), i32(2, 2), 2)),
    ]
    for args, want in cases:
        got = PS.encode_search(*args)
        assert len(got) == 6 and got[5] == want[5] and type(got[5]) is int, args
        for g, w in zip(got[:5], want[:5]):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (args, g, w)
    for args, text in ((([''], [''.join(chars[i:i + 64]) for i in range(0, 255, 64)]), 'the queries hold 255 distinct characters; a call takes 254'),
                       ((['a' * (PS.LEN_MAX + 1)], ['a']), 'a page text holds 65536 characters; the limit is 65535'),
                       ((['a'], ['']), "query '' holds 0 characters; a query takes 1 .. 64")):
        with pytest.raises(ValueError) as e:
            PS.encode_search(*args)
        assert str(e.value) == text


def test_page_index_normalises_per_word():
    recs = [dict(rec='Straße', polys=[]), dict(rec='', polys=[]), dict(lex=None, rec='No', polys=[])]
    text, start, ln = PS.page_index(recs, field='lex')
    assert text == 'strasse  no' and start.tolist() == [0, 8, 9] and ln.tolist() == [7, 0, 2] and start.dtype == ln.dtype == np.int32
    assert PS.page_index([], 'rec')[0] == '' and PS.page_index(recs, 'rec', sep='', normalise=None)[0] == 'StraßeNo'
    with pytest.raises(ValueError):
        PS.page_index([('a', 'b')])


# -- find_text --------------------------------------------------------------------------------------------------------------------------
def _word(text, x, y, w=40, h=10, **kw):
    return dict(rec=text, polys=[[x, y], [x + w, y], [x + w, y + h], [x, y + h]], **kw)


def _page():
    """two lines: `Invoice No 1234 Straße` / `Total amount 99`"""
    return [_word('Invoice', 0, 0), _word('No', 50, 0), _word('1234', 100, 0), _word('Straße', 150, 0),
            _word('Total', 0, 20), _word('amount', 50, 20), _word('99', 100, 20)]


def test_find_text_on_a_two_line_page():
    page = _page()
    host = PS.HostSearcher()
    res = find_text([page], ['invoice no', 'STRASSE total', 'amount', 'lnvoice', 'zzzz'], searcher=host)
    assert host.calls == 1 and len(res) == 1 and [d['query'] for d in res[0]] == ['invoice no', 'STRASSE total', 'amount', 'lnvoice', 'zzzz']
    two, across, one, fuzzy, none = res[0]
    text = PS.page_index(page)[0]
    assert text == 'invoice no 1234 strasse total amount 99'
    h = two['hits'][0]                                                      # a phrase that spans two words
    assert two['best'] == 0 and two['n_hits'] == 1 and h['dist'] == 0 and h['chars'] == (0, 10) and h['text'] == 'invoice no' and h['words'] == (0, 1)
    assert h['records'] == page[0:2] and h['box'] == (0.0, 0.0, 90.0, 10.0)
    h = across['hits'][0]                                                   # a phrase that spans the line break; ß moved the offsets
    assert across['normalised'] == 'strasse total' and h['chars'] == (16, 29) and h['words'] == (3, 4) and h['box'] == (0.0, 0.0, 190.0, 30.0)
    assert one['hits'][0]['words'] == (5, 5) and one['hits'][0]['records'] == [page[5]] and one['k'] == 1
    assert fuzzy['best'] == 1 and fuzzy['hits'][0]['dist'] == 1 and fuzzy['hits'][0]['words'] == (0, 0) and fuzzy['hits'][0]['text'] == 'nvoice'   # the shortest match
    assert none['hits'] == [] and none['n_hits'] == 0 and none['dropped'] == 0 and none['best'] is None
    assert all(text[h['chars'][0]:h['chars'][1]] == h['text'] for d in res[0] for h in d['hits'])


def test_find_text_per_image_lists_drops_and_refusals():
    page = _page()
    host = PS.HostSearcher()
    res = find_text([page, page[4:], []], [['total'], ['total', '99'], ['total']], searcher=host)
    assert host.calls == 1 and [len(r) for r in res] == [1, 2, 1]
    assert res[0][0]['hits'][0]['words'] == (4, 4) and res[1][0]['hits'][0]['words'] == (0, 0) and res[1][1]['hits'][0]['words'] == (2, 2)
    assert res[2][0]['best'] is None and res[2][0]['hits'] == []              # an empty page: nothing beats the empty match
    assert find_text([page], [], searcher=host) == [[]] and host.calls == 1
    with pytest.raises(ValueError):                                         # a blank query
        find_text([page], [' '], searcher=host)
    res = find_text([[_word('ab', 0, 0), _word('', 50, 0), _word('cd', 100, 0)]], ['b  c'], sep=' ', max_dist=1, max_ratio=None, searcher=host)
    h = res[0][0]['hits'][0]                                                # `ab  cd` with an empty word in the middle: the shortest match of
    assert h['chars'] == (3, 5) and h['dist'] == 1 and h['words'] == (2, 2)   # `b c` at distance 1 is ` c`, carried by the last word alone
    with pytest.raises(ValueError):
        find_text([[('entity', 'value')]], ['x'], searcher=host)
    with pytest.raises(ValueError):
        find_text([page, page], [['a'], ['b'], ['c']], searcher=host)
    with pytest.raises(ValueError) as e:
        find_text([page], ['y' * 65], searcher=host)
    assert 'yyyy' in str(e.value)


def test_a_hit_inside_a_separator_is_dropped():
    host = PS.HostSearcher()
    res = find_text([[_word('ab', 0, 0), _word('cd', 50, 0)]], ['-'], sep=' - ', normalise=None, searcher=host)
    assert res[0][0]['n_hits'] == 1 and res[0][0]['dropped'] == 1 and res[0][0]['hits'] == []


def test_the_command_line_on_a_results_file(tmp_path, capsys):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import find_text as tool
    flat = [dict(r, image_id='a.jpg', score=0.9) for r in _page()] + [dict(r, image_id='b.jpg', score=0.8) for r in _page()[4:]]
    results, queries = tmp_path / 'results.json', tmp_path / 'queries.json'
    results.write_text(json.dumps(flat))
    queries.write_text(json.dumps(['Invoice No', 'totai']))
    doc = tool.main(['--results', str(results), '--queries', str(queries), '--host'])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(doc))
    want = find_text([_page(), _page()[4:]], ['Invoice No', 'totai'], searcher=PS.HostSearcher())
    assert [im['image_id'] for im in doc['images']] == ['a.jpg', 'b.jpg'] and doc['records'] == 10 and doc['searcher'] == 'host'
    for im, per in zip(doc['images'], want):
        for got, w in zip(im['queries'], per):
            assert got['best'] == w['best'] and got['n_hits'] == w['n_hits']
            assert [(h['chars'], h['words'], h['dist'], h['box']) for h in got['hits']] == [(h['chars'], h['words'], h['dist'], h['box']) for h in w['hits']]
    assert doc['images'][0]['queries'][0]['hits'][0]['words'] == (0, 1) and doc['images'][1]['queries'][1]['hits'][0]['dist'] == 1
    queries.write_text(json.dumps({'b': ['amount'], 'a.jpg': ['1234']}))
    doc = tool.main(['--results', str(results), '--queries', str(queries), '--host', '--max-dist', '0', '--max-hits', '2'])
    assert [[q['query'] for q in im['queries']] for im in doc['images']] == [['1234'], ['amount']]
    assert doc['images'][0]['queries'][0]['hits'][0]['words'] == (2, 2) and doc['images'][1]['queries'][0]['hits'][0]['words'] == (1, 1)


# -- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_entry_point_matches_the_header():
    from advancedliteratemachinery_amd import _lib, build, ops
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24   # the library only gains an entry point
    m = re.search(r'int omp_page_search\((.*?)\);', text, re.S)
    want = []
    for p in (' '.join(p.split()) for p in m.group(1).split(',')):
        if '*' in p or p.startswith('omp_stream_t'):
            want.append(ctypes.c_void_p)
        elif p.startswith('int64_t '):
            want.append(ctypes.c_int64)
        else:
            assert p.startswith('int '), p
            want.append(ctypes.c_int)
    res, args = _lib._SIGS['omp_page_search']
    assert res is ctypes.c_int and args == want and len(want) == 19 and 'omp_page_search' in _lib.EXPORTS
    assert 'page_search.hip' in build.SOURCES and 'page_search.hip' not in build.AUDITED
    assert callable(ops.page_search) and callable(ops.page_search_scratch_bytes)
    csrc = os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc')
    src = open(os.path.join(csrc, 'page_search.hip')).read()
    assert 'extern "C" int omp_page_search(' in src
    # the frame and its constants are page_frame.h's: the four page-search units take them from there, and none keeps a copy
    hdr = open(os.path.join(csrc, 'page_frame.h')).read()
    assert 'page_frame.h' in [os.path.basename(h) for h in build.HEADERS] and '#include "page_frame.h"' in src
    assert 'PG_LEN_MAX = %d' % PS.LEN_MAX in hdr and 'PS_QUERY_MAX = %d' % PS.QUERY_MAX in src and 'PG_CHUNK = %d' % PS.CHUNK in hdr
    assert 'PG_HITS_MAX = %d' % PS.HITS_MAX in hdr and 'PG_SIGMA_MAX = %d' % PS.SIGMA_MAX in hdr and 'PS_NONE = %d' % PS.NONE in src
    assert 'PG_POS_MAX = %d' % PS.QUERY_MAX in hdr and 'PS_QUERY_MAX == PG_POS_MAX' in src
    assert 'PG_JOBS_MAX = 1 << 20' in hdr and PS.JOBS_MAX == 1 << 20 and ops.PAGE_SEARCH_CHUNK == PS.CHUNK
    assert 'PG_ROUND = 64 * PG_CHUNK' in hdr
    for unit in ('page_search.hip', 'page_pattern.hip', 'page_regex.hip'):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "page_frame.h"' in text and unit in build.SOURCES
        assert not re.search(r'\bPG_\w+\s*=[^=]', text), unit                                         # no unit redefines a shared constant
        assert not re.search(r'\bP[SPRF]_(LEN_MAX|POS_MAX|CHUNK|HITS_MAX|SIGMA_MAX|JOBS_MAX|ROUND)\b', text), unit   # nor keeps its own copy
    # the search with errors is the exact search's unit: one source, both entry points
    assert 'page_regex_fuzzy.hip' not in build.SOURCES and not os.path.exists(os.path.join(csrc, 'page_regex_fuzzy.hip'))
    regex = open(os.path.join(csrc, 'page_regex.hip')).read()
    assert 'extern "C" int omp_page_regex_search(' in regex and 'extern "C" int omp_page_regex_fuzzy_search(' in regex
    assert ops.page_search_scratch_bytes(3, 16) == 3 * 16 * 64 * 8 == 3 * 16 * ops.PAGE_SEARCH_HIT_BYTES
    assert PS.chunk_jobs(10, 16, 3 * 16 * 512 + 5) == [(0, 3), (3, 6), (6, 9), (9, 10)] and PS.chunk_jobs(0, 16) == []
    with pytest.raises(ValueError):
        PS.chunk_jobs(1, 16, 16 * 512 - 1)
