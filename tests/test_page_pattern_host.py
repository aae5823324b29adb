"""Page patterns on the host (no GPU): the parser, the encoding, the numpy definition (utils/page_pattern.py) against the plain double loop
and against the bit-parallel rows the kernel runs, an independent oracle at k = 0 (Python's re), literals pinned to page search, the
tolerance, find_pattern on a hand-made page with the host searcher, find_text unchanged by the shared helper, the command line on a
results file written here, and the C ABI's declaration.  The kernel and the device stage are tests/test_gpu_page_pattern.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from advancedliteratemachinery_amd.engine.search import find_pattern, find_text
from advancedliteratemachinery_amd.utils import page_pattern as PP
from advancedliteratemachinery_amd.utils import page_search as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the parser -------------------------------------------------------------------------------------------------------------------------
def test_parser_accepts_every_form_and_expands_repetition():
    p = PP.parse_pattern(r'a\.[0-9x][^a-c].\d\D\w\W\s\S')
    assert p.atoms == ('a', r'\.', '[0-9x]', '[^a-c]', '.', r'\d', r'\D', r'\w', r'\W', r'\s', r'\S') and p.P == p.Mand == 11 and p.opt == 0
    p = PP.parse_pattern(r'\d{2}[./-]?x{1,3}y{0,2}z{2}')
    assert p.atoms == (r'\d', r'\d', '[./-]', 'x', 'x', 'x', 'y', 'y', 'z', 'z')
    assert p.optional == (False, False, True, False, True, True, True, True, False, False) and p.P == 10 and p.Mand == 5 and p.opt == 0b0011110100
    assert PP.parse_pattern(r'a{,2}b').optional == (True, True, False) and PP.parse_pattern('a{0}b').atoms == ('b',)
    assert PP.parse_pattern(r'[]a]\]\\ \n').atoms == ('[]a]', r'\]', '\\\\', ' ', r'\n') and PP.parse_pattern('[^]]]').atoms == ('[^]]', r'\]')
    assert PP.parse_pattern(r'[\]a-c]x').atoms == (r'[\]a-c]', 'x')
    assert PP.parse_pattern(p) is p
    star = PP.parse_pattern(r'a*b+', rep_max=3)
    assert star.atoms == ('a', 'a', 'a', 'b', 'b', 'b') and star.optional == (True, True, True, False, True, True)
    assert PP.parse_pattern(r'a{2,}', rep_max=4).optional == (False, False, True, True) and PP.parse_pattern(r'a{5,}', rep_max=4).P == 5
    assert PP.parse_pattern('a' * 64).P == 64 and PP.parse_pattern(r'\d{32}x{0,32}').P == 64


def test_parser_refuses_with_the_pattern_and_the_offset():
    for src, at, word in ((r'ab(c)', 2, 'groups'), (r'ab)', 2, 'groups'), (r'a|b', 1, 'alternation'), (r'^ab', 0, 'anchors'), (r'ab$', 2, 'anchors'),
                          (r'a\b', 1, 'anchors'), (r'a\Z', 1, 'anchors'), (r'(a)\1', 0, 'groups'), (r'a\1', 1, 'back-references'), (r'ab??', 3, 'lazy'),
                          (r'a{2}?', 4, 'lazy'), (r'a{1,2}+', 6, 'lazy'), (r'a?{2}', 2, 'quantifier on a quantifier'), (r'?a', 0, 'nothing to repeat'),
                          (r'a{', 1, 'brace'), (r'a{x}', 1, 'brace'), (r'a{}', 1, 'brace'), (r'a}', 1, 'brace'), (r'a{3,2}', 1, 'b < a'), ('a[bc', 1, 'not closed'),
                          ('ab\\', 2, 'backslash'), (r'a\q', 1, 'escape'), (r'a\x41', 1, 'escape'), ('a[z-a]', 1, 'refused by re'), ('', 0, 'no position'),
                          (r'a?b{0,3}', 0, 'optional'), ('a' * 65, 64, '64 positions'), (r'a{40}b{25}', 5, '64 positions'), (r'a{0}', 0, 'no position')):
        with pytest.raises(ValueError) as e:
            PP.parse_pattern(src)
        assert 'pattern %r, offset %d:' % (src, at) in str(e.value) and word in str(e.value), (src, str(e.value))
    for src, at in ((r'a*', 1), (r'ab+', 2), (r'a{2,}', 1)):
        with pytest.raises(ValueError) as e:
            PP.parse_pattern(src)
        assert 'offset %d' % at in str(e.value) and 'rep_max' in str(e.value) and 'unbounded' in str(e.value)
    with pytest.raises(ValueError) as e:
        PP.parse_pattern(r'a*b*', rep_max=33)
    assert '64 positions' in str(e.value)
    with pytest.raises(ValueError):
        PP.parse_pattern(r'a*', rep_max=3)                                    # every position optional
    with pytest.raises(ValueError):
        PP.parse_pattern(r'a+', rep_max=0)
    with pytest.raises(ValueError):
        PP.parse_pattern(12)


# -- the encoding -----------------------------------------------------------------------------------------------------------------------
def test_encoding_gives_one_code_per_signature():
    pats = [PP.parse_pattern(r'\d[a-c]?x'), PP.parse_pattern(r'[^x].')]
    pool, po, pl, masks, opt, P, sigma = PP.encode_patterns(['a1 x', 'b27z\n', 'a1 x', ''], pats)
    # atoms \d [a-c] x [^x] . ; signatures in order of first appearance: a, 1, ' ', x; b = a, 2 = 7 = 1, z = '\n' = ' '
    assert sigma == 4 and pool.tolist() == [0, 1, 2, 3, 0, 1, 1, 2, 2] and po.tolist() == [0, 4, 0, 9] and pl.tolist() == [4, 5, 4, 0]
    assert pool.dtype == np.uint8 and po.dtype == pl.dtype == P.dtype == np.int32 and masks.dtype == opt.dtype == np.uint64 and masks.shape == (2, 5)
    assert masks[0].tolist() == [0b010, 0b001, 0, 0b100, 0] and opt.tolist() == [0b010, 0] and P.tolist() == [3, 2]
    assert masks[1].tolist() == [0b11, 0b11, 0b11, 0b10, 0]                   # a negated class and `.` hold characters no atom names, `\n` among them
    assert PP.encode_patterns([''], pats)[6] == 0 and PP.encode_patterns([''], pats)[3].shape == (2, 1)
    strings = PP.encode_patterns(['a1'], [r'\d[a-c]?x'])                      # strings are parsed without rep_max
    assert strings[3].tolist() == [[0b010, 0b001, 0]] and strings[6] == 2


def test_encoding_limits():
    letters = [chr(0x4e00 + i) for i in range(255)]
    one_each = ['[%s]' % c for c in letters]                                  # 255 atoms, every character its own signature
    pats = [PP.Pattern('x', one_each[i:i + 64], [False] * len(one_each[i:i + 64])) for i in range(0, 255, 64)]
    assert PP.encode_patterns([''.join(letters[:254])], pats)[6] == 254
    with pytest.raises(ValueError) as e:
        PP.encode_patterns([''.join(letters)], pats)
    assert '255 classes' in str(e.value) and '254' in str(e.value)
    assert PP.encode_patterns([''.join(letters) * 3], ['a'])[6] == 1         # 255 characters, one signature
    with pytest.raises(ValueError):
        PP.encode_patterns(['a' * (PP.LEN_MAX + 1)], ['a'])
    with pytest.raises(ValueError):
        PP.encode_patterns(['a'], ['a*'])


# -- the table --------------------------------------------------------------------------------------------------------------------------
def _random_pattern(rng, P, sigma, shape):
    optional = rng.rand(P) < (0.0, 0.2, 0.5, 0.9)[shape % 4]
    if shape % 5 == 0:
        optional[:int(rng.randint(0, P + 1))] = True                         # a leading run
    if shape % 7 == 0:
        optional[P - int(rng.randint(0, P + 1)):] = True                     # a trailing run
    if shape % 3 == 0 and P >= 34:
        optional[29:34] = True                                               # a run across bit 31 / 32
    if optional.all():
        optional[int(rng.randint(0, P))] = False
    mask = np.zeros(sigma + 1, dtype=np.uint64)
    for c in range(sigma):
        mask[c] = sum(1 << i for i in range(P) if rng.rand() < 0.6)
    return mask, sum(1 << i for i in range(P) if optional[i]), P - int(optional.sum())


_CASES = []


def random_cases():
    """400 cases: P in 1 .. 64, sigma in {1, 2, 3, 5}, texts of 0 .. 90 codes, some at or above sigma; made once and shared"""
    if not _CASES:
        rng = np.random.RandomState(0)
        for i in range(400):
            P = int(rng.randint(1, 65)) if i % 3 else (1, 2, 31, 32, 33, 63, 64)[i // 3 % 7]
            sigma = (1, 2, 3, 5)[i % 4]
            mask, opt, mand = _random_pattern(rng, P, sigma, i)
            t = rng.randint(0, sigma + (i % 2), int(rng.randint(0, 91))).astype(np.uint8)
            _CASES.append((mask, opt, P, mand, t, PP.row_py(mask, opt, P, t)))
    return _CASES


def test_row_cpu_equals_the_double_loop():
    shapes = set()
    for mask, opt, P, mand, t, want in random_cases():
        assert np.array_equal(PP.row_cpu(mask, opt, P, t), want) and want.dtype == np.int32 and want[0] == mand
        assert np.array_equal(PP.row_cpu(mask, opt, P, t, anchored=True), PP.row_py(mask, opt, P, t, anchored=True))
        shapes |= {('lead', bool(opt & 1)), ('trail', bool(opt >> (P - 1))), ('32', bool(opt >> 31 & 1 and opt >> 32 & 1)), ('none', opt == 0)}
    assert len(shapes) == 8


def test_the_bit_parallel_rows_equal_the_table_and_the_start_walk_equals_match_start():
    """row_bits and start_bits are the column step and the start walk of csrc/page_pattern.hip in Python integers"""
    hits = 0
    for i, (mask, opt, P, mand, t, want) in enumerate(random_cases()):
        for k in {0, min(mand - 1, PP.K_MAX), i % (min(mand - 1, PP.K_MAX) + 1)}:
            v = np.minimum(want, k + 1)
            assert np.array_equal(PP.row_bits(mask, opt, P, t, k), v), (P, bin(opt), k)
            for e in PS.hit_ends(v, k).tolist()[:6]:
                assert PP.start_bits(mask, opt, P, t, e, int(v[e])) == PP.match_start(mask, opt, P, t, e, int(v[e])), (P, bin(opt), k, e)
                hits += 1
    assert hits > 500


def test_a_fresh_start_P_plus_k_columns_early_reproduces_every_later_value():
    """the warm-up fact the kernel's chunks rest on"""
    for i, (mask, opt, P, mand, t, want) in enumerate(random_cases()):
        k = min(mand - 1, PP.K_MAX, i % 4)
        v = np.minimum(want, k + 1)
        for cs in range(P + k, t.size + 1, 7):
            part = np.minimum(PP.row_cpu(mask, opt, P, t[cs - (P + k):]), k + 1)
            assert np.array_equal(part[P + k:], v[cs:]), (P, k, cs)


def _search1(src, text, k, H=16, rep_max=None):
    pool, po, pl, masks, opt, P, sigma = PP.encode_patterns([text], [PP.parse_pattern(src, rep_max)])
    res = PP.search_cpu(pool, po, pl, masks, opt, P, [[0, 0]], [k], H)
    return res['best'][0].tolist(), int(res['n_hits'][0]), [r for r in res['hits'][0].tolist() if r[0] >= 0]


def test_hand_cases():
    assert _search1(r'\d{1,4}', '12345', 0) == ([0, 1], 1, [[5, 0, 1]])         # the longest match; page search would report (5, 0, 4)
    assert _search1('ab?c', 'ac', 0) == ([0, 2], 1, [[2, 0, 0]])
    assert _search1('ab?c', 'abc', 0) == ([0, 3], 1, [[3, 0, 0]])
    assert _search1('ab?c', 'abbc', 0) == ([1, 0], 0, [])
    assert _search1('ab?c', 'abbc', 1) == ([1, 1], 1, [[4, 1, 0]])              # v = 2, 1, 1, 1, 1: the floor's last column, from its least start
    assert _search1('ab?c', '', 1) == ([2, 0], 0, []) and _search1('ab?c', 'zzzz', 1) == ([2, 0], 0, [])
    assert _search1(r'\d{2}[./-]\d{2}[./-]\d{4}', 'due 03.O4.2024 or 1.1.24', 2) == ([1, 14], 1, [[14, 1, 4]])
    hits = _search1('aa', 'aaaa', 0, H=2)
    assert hits == ([0, 2], 1, [[4, 0, 2]])                                   # a run: only the last occurrence, as in page search


# -- an independent oracle at k = 0 -------------------------------------------------------------------------------------------------
def test_at_k_0_the_ends_and_starts_are_those_of_re_fullmatch():
    rng = np.random.RandomState(3)
    atoms = ['a', 'b', '[ab]', '[^a]', '.', '[c-d]', r'\w']
    checked = ends = 0
    for _ in range(250):
        parts = []
        for _ in range(int(rng.randint(1, 6))):
            q = ('', '', '?', '{2}', '{1,3}', '{0,2}')[int(rng.randint(0, 6))]
            parts.append(atoms[int(rng.randint(0, len(atoms)))] + q)
        src = ''.join(parts)
        try:
            pat = PP.parse_pattern(src)
        except ValueError:
            continue                                                         # every position optional
        rx = re.compile(src, re.DOTALL)
        text = ''.join('abcd'[c] for c in rng.randint(0, 4, int(rng.randint(0, 25))))
        pool, po, pl, masks, opt, P, sigma = PP.encode_patterns([text], [pat])
        v = PP.row_cpu(masks[0], opt[0], P[0], pool)
        for j in range(1, len(text) + 1):
            starts = [s for s in range(j) if rx.fullmatch(text, s, j)]
            assert (v[j] == 0) == bool(starts), (src, text, j)
            if starts:
                assert PP.match_start(masks[0], opt[0], P[0], pool, j, 0) == starts[0], (src, text, j)
                ends += 1
        checked += 1
    assert checked > 150 and ends > 300


# -- pinned to page search ----------------------------------------------------------------------------------------------------------
def test_literal_patterns_equal_page_search():
    rng = np.random.RandomState(5)
    jobs = 0
    for i in range(120):
        m, sigma = int(rng.randint(1, 20)), (2, 3, 26)[i % 3]
        q = ''.join(chr(97 + c) for c in rng.randint(0, sigma, m))
        text = ''.join(chr(97 + c) for c in rng.randint(0, sigma, int(rng.randint(0, 80))))
        if i % 2 and len(text) >= m:
            at = int(rng.randint(0, len(text) - m + 1))
            text = text[:at] + q + text[at + m:]
        k = min(int(rng.randint(0, m)), PP.K_MAX)
        pool, po, pl, qo, ql, _ = PS.encode_search([text], [q])
        old = PS.search_cpu(pool, po, pl, qo, ql, [[0, 0]], [k], 64)
        pool, po, pl, masks, opt, P, _ = PP.encode_patterns([text], [re.escape(q)])
        new = PP.search_cpu(pool, po, pl, masks, opt, P, [[0, 0]], [k], 64)
        assert new['n_hits'][0] == old['n_hits'][0] and np.array_equal(new['hits'][0][:, :2], old['hits'][0][:, :2]), (q, text, k)
        assert (new['hits'][0][:, 2] <= old['hits'][0][:, 2]).all()
        if old['best'][0][0] <= k:
            assert new['best'][0].tolist() == old['best'][0].tolist()
        else:
            assert new['best'][0].tolist() == [k + 1, 0]
        jobs += int(old['n_hits'][0] > 0)
    assert jobs > 40


# -- the tolerance ------------------------------------------------------------------------------------------------------------------
def test_every_bound_of_the_tolerance():
    assert PP.tolerance(10) == 0 and PP.tolerance(10, max_ratio=None) == 8 and PP.tolerance(5, max_ratio=None) == 4 and PP.tolerance(1, max_ratio=1.0) == 0
    assert PP.tolerance(10, max_ratio=0.25) == 2 and PP.tolerance(64, max_ratio=0.2) == 8 and PP.tolerance(64, max_ratio=0.1) == 6
    assert PP.tolerance(10, max_dist=1, max_ratio=0.5) == 1 and PP.tolerance(10, max_dist=7, max_ratio=0.5) == 5 and PP.tolerance(3, max_dist=9, max_ratio=1.0) == 2
    assert PP.tolerance(7, max_ratio=0.143) == 1 and PP.tolerance(7, max_ratio=0.142) == 0 and PP.K_MAX == 8
    for bad in (dict(mand=0), dict(mand=65), dict(mand=4, max_ratio=1.5), dict(mand=4, max_ratio=-0.1), dict(mand=4, max_dist=-1)):
        with pytest.raises(ValueError):
            PP.tolerance(**bad)


def test_search_cpu_refuses_what_the_device_refuses():
    ok = dict(pool=np.asarray([0, 1, 2], np.uint8), page_off=[0], page_len=[3], masks=np.asarray([[1, 2, 3, 0]], np.uint64), opt=[0], pat_len=[2], jobs=[[0, 0]], k=[1],
              max_hits=4)
    assert PP.search_cpu(**ok)['n_hits'].tolist() == [1]
    for kw in (dict(page_len=[PP.LEN_MAX + 1]), dict(page_off=[1]), dict(page_off=[-1]), dict(k=[2]), dict(k=[-1]), dict(pat_len=[0]), dict(pat_len=[65]),
               dict(max_hits=0), dict(max_hits=65), dict(opt=[4]), dict(opt=[3]), dict(jobs=[[1, 0]]), dict(jobs=[[0, 1]]), dict(jobs=[[0, -1]]),
               dict(masks=np.zeros((1, 256), np.uint64)), dict(masks=np.zeros((2, 4), np.uint64)), dict(page_len=[3, 3])):
        with pytest.raises(ValueError):
            PP.search_cpu(**dict(ok, **kw))
    many = dict(ok, masks=np.asarray([[(1 << 12) - 1, 0]], np.uint64), pat_len=[12])
    assert PP.search_cpu(**dict(many, k=[8]))['best'].tolist() == [[9, 0]]
    with pytest.raises(ValueError):
        PP.search_cpu(**dict(many, k=[9]))                                    # Mand - 1 = 11 allows it, K_MAX does not


# -- find_pattern ---------------------------------------------------------------------------------------------------------------------
def _word(text, x, y, w=40, h=10, **kw):
    return dict(rec=text, polys=[[x, y], [x + w, y], [x + w, y + h], [x, y + h]], **kw)


def _page():
    """two lines: `Invoice No 1234 Straße` / `Total amount 99` / `Date 03.O4.2024 IBAN DE12 3456 7890`"""
    return [_word('Invoice', 0, 0), _word('No', 50, 0), _word('1234', 100, 0), _word('Straße', 150, 0),
            _word('Total', 0, 20), _word('amount', 50, 20), _word('99', 100, 20),
            _word('Date', 0, 40), _word('03.O4.2024', 50, 40), _word('IBAN', 100, 40), _word('DE12', 150, 40), _word('3456', 200, 40), _word('7890', 250, 40)]


def test_find_pattern_on_a_three_line_page():
    page = _page()
    host = PP.HostPatternSearcher()
    pats = [('date', r'\d{2}[./-]\d{2}[./-]\d{4}'), r'[A-Z]{2}\d{2} ?\d{4} ?\d{4}', ('number', r'\d{1,4}'), r'Stra[sß]{1,2}e', 'zzzz']
    res = find_pattern([page], pats, max_ratio=0.15, searcher=host)
    assert host.calls == 1 and len(res) == 1 and [d['name'] for d in res[0]] == ['date', None, 'number', None, None]
    assert [d['pattern'] for d in res[0]] == [p if isinstance(p, str) else p[1] for p in pats]
    date, iban, number, street, none = res[0]
    text = PS.page_index(page, normalise=None)[0]
    assert text == 'Invoice No 1234 Straße Total amount 99 Date 03.O4.2024 IBAN DE12 3456 7890'
    assert date['P'] == 10 and date['k'] == 1 and date['best'] == 1 and date['n_hits'] == 1                  # O for 0: one substitution
    h = date['hits'][0]
    assert h['dist'] == 1 and h['text'] == '03.O4.2024' and h['chars'] == (44, 54) and h['words'] == (8, 8) and h['records'] == [page[8]]
    assert h['box'] == (50.0, 40.0, 90.0, 50.0)
    h = iban['hits'][0]                                                       # a shape that spans three words
    assert iban['P'] == 14 and iban['k'] == 1 and iban['best'] == 0 and h['text'] == 'DE12 3456 7890' and h['words'] == (10, 12) and h['box'] == (150.0, 40.0, 290.0, 50.0)
    assert h['records'] == page[10:13]
    assert number['k'] == 0 and [h['text'] for h in number['hits']] == ['1234', '99', '03', '4', '2024', '12', '3456', '7890'] and number['n_hits'] == 8
    assert [h['words'] for h in number['hits']] == [(2, 2), (6, 6), (8, 8), (8, 8), (8, 8), (10, 10), (11, 11), (12, 12)]
    assert street['hits'][0]['text'] == 'Straße' and street['hits'][0]['words'] == (3, 3)
    assert none['hits'] == [] and none['n_hits'] == 0 and none['dropped'] == 0 and none['best'] is None and none['k'] == 0
    assert all(text[h['chars'][0]:h['chars'][1]] == h['text'] for d in res[0] for h in d['hits'])
    # exact shapes by default: the misread date is not found; normalise touches the page, never the pattern
    assert find_pattern([page], [pats[0]], searcher=host)[0][0]['hits'] == []
    assert find_pattern([page], ['invoice', 'Invoice'], normalise=str.casefold, searcher=host)[0][0]['hits'][0]['words'] == (0, 0)
    assert find_pattern([page], ['invoice', 'Invoice'], normalise=str.casefold, searcher=host)[0][1]['hits'] == []
    assert find_pattern([page], [r'\d+'], rep_max=4, searcher=host)[0][0]['n_hits'] == 8


def test_find_pattern_per_image_lists_drops_and_refusals():
    page = _page()
    host = PP.HostPatternSearcher()
    res = find_pattern([page, page[4:7], []], [[r'\d{4}'], [('n', r'\d{2}'), 'Total'], ['Total']], searcher=host)
    assert host.calls == 1 and [len(r) for r in res] == [1, 2, 1]
    assert [h['words'] for h in res[0][0]['hits']] == [(2, 2), (8, 8), (11, 11), (12, 12)]
    assert res[1][0]['name'] == 'n' and res[1][0]['hits'][0]['words'] == (2, 2) and res[1][1]['hits'][0]['words'] == (0, 0)
    assert res[2][0]['best'] is None and res[2][0]['hits'] == []              # an empty page
    assert find_pattern([page], [], searcher=host) == [[]] and host.calls == 1
    res = find_pattern([[_word('ab', 0, 0), _word('cd', 50, 0)]], ['-', ' ?-'], sep=' - ', searcher=host)
    assert res[0][0]['n_hits'] == 1 and res[0][0]['dropped'] == 1 and res[0][0]['hits'] == []      # a hit inside a separator
    assert res[0][1]['dropped'] == 1
    res = find_pattern([page], [r'\d{1,4}'], max_hits=3, searcher=host)
    assert res[0][0]['n_hits'] == 8 and len(res[0][0]['hits']) == 3
    for bad in (dict(patterns=['a(b)']), dict(patterns=['a*']), dict(patterns=[('n', 'a', 'b')]), dict(patterns=[7]), dict(patterns=[['a'], ['b']]),
                dict(records=[[('entity', 'value')]], patterns=['a'])):
        with pytest.raises(ValueError):
            find_pattern(**dict(dict(records=[page], searcher=host), **bad))


def test_find_text_returns_what_it_returned_before_the_helper_was_shared():
    page = _page()[:7]
    res = find_text([page, page[4:]], ['invoice no', 'lnvoice', 'zzzz'], searcher=PS.HostSearcher())
    want0 = [
        dict(query='invoice no', normalised='invoice no', k=2, best=0, n_hits=1, dropped=0,
             hits=[dict(dist=0, chars=(0, 10), text='invoice no', words=(0, 1), records=page[0:2], box=(0.0, 0.0, 90.0, 10.0))]),
        dict(query='lnvoice', normalised='lnvoice', k=1, best=1, n_hits=1, dropped=0,
             hits=[dict(dist=1, chars=(1, 7), text='nvoice', words=(0, 0), records=page[0:1], box=(0.0, 0.0, 40.0, 10.0))]),
        dict(query='zzzz', normalised='zzzz', k=0, best=None, n_hits=0, dropped=0, hits=[])]
    want1 = [dict(query='invoice no', normalised='invoice no', k=2, best=8, n_hits=0, dropped=0, hits=[]),
             dict(query='lnvoice', normalised='lnvoice', k=1, best=6, n_hits=0, dropped=0, hits=[]),
             dict(query='zzzz', normalised='zzzz', k=0, best=None, n_hits=0, dropped=0, hits=[])]
    assert res == [want0, want1]
    assert [type(v) for v in res[0][0]['hits'][0]['chars']] == [int, int] and type(res[0][0]['hits'][0]['dist']) is int
    res = find_text([[_word('ab', 0, 0), _word('cd', 50, 0)]], ['-'], sep=' - ', normalise=None, searcher=PS.HostSearcher())
    assert res == [[dict(query='-', normalised='-', k=0, best=0, n_hits=1, dropped=1, hits=[])]]


def test_the_command_line_on_a_results_file(tmp_path, capsys):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import find_pattern as tool
    flat = [dict(r, image_id='a.jpg', score=0.9) for r in _page()] + [dict(r, image_id='b.jpg', score=0.8) for r in _page()[4:7]]
    results, patterns = tmp_path / 'results.json', tmp_path / 'patterns.json'
    results.write_text(json.dumps(flat))
    pats = [dict(name='date', pattern=r'\d{2}[./-]\d{2}[./-]\d{4}'), r'\d{2,4}']
    patterns.write_text(json.dumps(pats))
    doc = tool.main(['--results', str(results), '--patterns', str(patterns), '--host', '--max-ratio', '0.15'])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(doc))
    want = find_pattern([_page(), _page()[4:7]], [('date', pats[0]['pattern']), pats[1]], max_ratio=0.15, searcher=PP.HostPatternSearcher())
    assert [im['image_id'] for im in doc['images']] == ['a.jpg', 'b.jpg'] and doc['records'] == 16 and doc['searcher'] == 'host' and doc['rep_max'] is None
    for im, per in zip(doc['images'], want):
        for got, w in zip(im['patterns'], per):
            assert (got['pattern'], got['name'], got['P'], got['k'], got['best'], got['n_hits']) == (w['pattern'], w['name'], w['P'], w['k'], w['best'], w['n_hits'])
            assert [(h['chars'], h['words'], h['dist'], h['box'], h['text']) for h in got['hits']] == [(h['chars'], h['words'], h['dist'], h['box'], h['text']) for h in w['hits']]
            assert all('records' not in h for h in got['hits'])
    assert doc['images'][0]['patterns'][0]['hits'][0]['words'] == (8, 8) and doc['images'][1]['patterns'][1]['hits'][0]['text'] == '99'
    patterns.write_text(json.dumps({'b': [r'\d+'], 'a.jpg': ['IBAN']}))
    doc = tool.main(['--results', str(results), '--patterns', str(patterns), '--host', '--rep-max', '3', '--max-hits', '2'])
    assert [[q['pattern'] for q in im['patterns']] for im in doc['images']] == [['IBAN'], [r'\d+']]
    assert doc['images'][0]['patterns'][0]['hits'][0]['words'] == (9, 9) and doc['images'][1]['patterns'][0]['hits'][0]['words'] == (2, 2)
    with pytest.raises(ValueError):
        tool.main(['--results', str(results), '--patterns', str(patterns), '--host'])   # `+` without --rep-max


# -- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_entry_point_matches_the_header():
    from advancedliteratemachinery_amd import _lib, build, ops
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24   # the library only gains an entry point
    m = re.search(r'int omp_page_pattern_search\((.*?)\);', text, re.S)
    want = []
    for p in (' '.join(p.split()) for p in m.group(1).split(',')):
        if '*' in p or p.startswith('omp_stream_t'):
            want.append(ctypes.c_void_p)
        elif p.startswith('int64_t '):
            want.append(ctypes.c_int64)
        else:
            assert p.startswith('int '), p
            want.append(ctypes.c_int)
    res, args = _lib._SIGS['omp_page_pattern_search']
    assert res is ctypes.c_int and args == want and len(want) == 20 and 'omp_page_pattern_search' in _lib.EXPORTS
    assert 'page_pattern.hip' in build.SOURCES and 'page_pattern.hip' not in build.AUDITED
    assert callable(ops.page_pattern_search) and callable(ops.page_pattern_scratch_bytes)
    src = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'page_pattern.hip')).read()
    hdr = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'page_frame.h')).read()       # the shared constants: test_page_search_host.py
    assert 'extern "C" int omp_page_pattern_search(' in src and '#include "page_frame.h"' in src
    assert 'PG_LEN_MAX = %d' % PP.LEN_MAX in hdr and 'PG_POS_MAX = %d' % PP.POS_MAX in hdr and 'PG_CHUNK = %d' % PP.CHUNK in hdr and 'PP_K_MAX = %d' % PP.K_MAX in src
    assert 'PG_HITS_MAX = %d' % PS.HITS_MAX in hdr and 'PG_SIGMA_MAX = %d' % PP.SIGMA_MAX in hdr
    assert 'PG_JOBS_MAX = 1 << 20' in hdr and PS.JOBS_MAX == 1 << 20 and ops.PAGE_PATTERN_CHUNK == PP.CHUNK
    assert ops.page_pattern_scratch_bytes(3, 16) == 3 * 16 * 64 * 8 == 3 * 16 * ops.PAGE_PATTERN_HIT_BYTES
    assert PP.chunk_jobs(10, 16, 3 * 16 * 512 + 5) == [(0, 3), (3, 6), (6, 9), (9, 10)] and PP.chunk_jobs(0, 16) == []
    with pytest.raises(ValueError):
        PP.chunk_jobs(1, 16, 16 * 512 - 1)
    with pytest.raises(RuntimeError):
        PP.PatternSearcher('cpu')
