"""Page expressions on the host (no GPU): the parser and the position automaton (utils/page_regex.py) against Python's re alone, the set
form, the word form and the chunk-and-carry split against each other, flat patterns pinned to page patterns at k = 0, the hit rule, every
refusal, find_regex on a hand-made page with the host searcher, the command line on a results file written here, and the C ABI's
declaration.  The kernel and the device stage are tests/test_gpu_page_regex.py."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest

from advancedliteratemachinery_amd.engine.search import find_pattern, find_regex
from advancedliteratemachinery_amd.utils import page_pattern as PP
from advancedliteratemachinery_amd.utils import page_regex as PR
from advancedliteratemachinery_amd.utils import page_search as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the twelve expressions the scheme was first checked on, then a (?: ) group, a class inside a group and one of exactly 64 positions
EXPRESSIONS = [r'a(b|c)*a', r'(ab|ba)+', r'\d{1,3}(,\d{3})*\.\d{2}', r'(a|bc){2,3}c', r'a.*b', r'(EUR|USD) ?\d+', r'a+b?c{2,}', r'(a|b)?c', r'((ab)?c)+',
               r'a{0,2}b', r'(a*b)+', r'x|yz|a(b)', r'(?:ab|c)+d', r'([a-c]\d)+x', r'(ab){30}(c|d)(e|f)']
ALPHABET = {r'\d{1,3}(,\d{3})*\.\d{2}': '12,.', r'(EUR|USD) ?\d+': ('EUR', 'USD', 'UR', ' ', '1', '22', 'E'), r'x|yz|a(b)': 'xyzab', r'([a-c]\d)+x': ('a1', 'b2', 'x', 'c', '1'),
            r'(?:ab|c)+d': 'abcd'}
SPLITS = ((4, 4), (3, 2), (1, 5), (128, 64))


def _texts(src, count=200, seed=1):
    """seeded random texts of 0 to 40 characters over an alphabet that makes matches frequent; the 64-position expression gets texts that
    hold it whole"""
    rng = random.Random('%s/%d' % (src, seed))
    out = []
    for _ in range(count):
        if src == EXPRESSIONS[-1]:
            body = 'ab' * rng.choice((29, 30, 30, 31)) + rng.choice('cd') + rng.choice('efa')
            out.append(''.join(rng.choice('ab') for _ in range(rng.randint(0, 3))) + body + ''.join(rng.choice('abce') for _ in range(rng.randint(0, 3))))
        else:
            out.append(''.join(rng.choice(ALPHABET.get(src, 'abc')) for _ in range(40))[:rng.randint(0, 40)])
    return out


def _tab(src, text):
    enc = PR.encode_regex([text], [src])
    return PR.tables(*enc[3:9]), enc[0]


# -- the parser and the automaton against re -------------------------------------------------------------------------------------------
def test_the_automaton():
    r = PR.parse_regex(r'a(b|c)*a')
    assert r.atoms == ('a', 'b', 'c', 'a') and r.P == 4 and r.first == 0b0001 and r.last == 0b1000
    assert r.follow[:4].tolist() == [0b1110, 0b1110, 0b1110, 0] and not r.follow[4:].any() and r.follow.shape == r.pred.shape == (64,)
    assert r.pred[:4].tolist() == [0, 0b0111, 0b0111, 0b0111] and r.follow.dtype == r.pred.dtype == np.uint64
    r = PR.parse_regex(r'x{2,}(?:y|[0-9]z)?')                                 # a copies, the loop on the last one
    assert r.atoms == ('x', 'x', 'y', '[0-9]', 'z') and r.first == 1 and r.last == 0b10110 and r.follow[:5].tolist() == [0b10, 0b1110, 0, 0b10000, 0]
    assert PR.parse_regex(r'a{2,3}').follow[:3].tolist() == [0b10, 0b100, 0] and PR.parse_regex(r'a{2,3}').last == 0b110
    assert PR.parse_regex(r'a{0,}b').follow[:2].tolist() == [0b11, 0] and PR.parse_regex(r'a{0,}b').first == 0b11
    assert PR.parse_regex(r'(a+)*b').P == 2 and PR.parse_regex(r'((a|b)+c?)+').P == 3      # a quantifier on a group that holds one is fine
    assert PR.parse_regex(r'[]a]\]\\ \n').atoms == ('[]a]', r'\]', '\\\\', ' ', r'\n') and PR.parse_regex(r'(\))').atoms == (r'\)',)
    assert PR.parse_regex('a' * 64).P == 64 and PR.parse_regex(r'(ab|cd){16}').P == 64 and PR.parse_regex(r'(a{8}|b{8}){4}').P == 64
    assert PR.parse_regex(EXPRESSIONS[-1]).P == 64 and PR.parse_regex(r) is r
    assert all(int(f) >> r.P == 0 for r in map(PR.parse_regex, EXPRESSIONS) for f in list(r.follow) + list(r.pred) + [r.first, r.last])


@pytest.mark.parametrize('src', EXPRESSIONS)
def test_the_ends_and_starts_are_those_of_re_fullmatch(src):
    """the ends equal {j : some s < j has re.fullmatch(src, text, s, j)} and every end's match_start the least such s; ends_py, ends_cpu and
    the split at every (chunk, lanes) agree"""
    cre = re.compile(src, re.DOTALL)
    some, carried = 0, 0
    for text in _texts(src):
        tab, t = _tab(src, text)
        starts = {j: [s for s in range(j) if cre.fullmatch(text, s, j)] for j in range(1, len(text) + 1)}
        want = [j for j, ss in starts.items() if ss]
        assert PR.ends_cpu(tab, t).tolist() == want, (src, text)
        assert PR.ends_py(tab, t).tolist() == want, (src, text)
        for j in want:
            assert PR.match_start(tab, t, j) == min(starts[j]), (src, text, j)
        for chunk, lanes in SPLITS:
            ends, rounds = PR.ends_chunked(tab, t, chunk, lanes)
            assert ends.tolist() == want, (src, text, chunk, lanes)
            carried += sum(rounds)
        some += len(want)
    assert some >= 100 and carried >= 1, (src, some, carried)                  # the alphabet makes matches frequent, and carries cross chunks


def test_the_split_over_more_than_one_round_of_the_wave():
    rng = random.Random(5)
    for src, alphabet, n in ((r'a.*b', 'abc', 300), (r'\d+', '1111 ', 200), (r'(ab|ba)+', 'ab', 150), (r'a(b|c)*a', 'abc', 100), (r'\d{1,3}(,\d{3})*\.\d{2}', '12,.', 200)):
        text = ''.join(rng.choice(alphabet) for _ in range(n))
        tab, t = _tab(src, text)
        want = PR.ends_cpu(tab, t).tolist()
        assert want == PR.ends_py(tab, t).tolist() and want
        for chunk, lanes in SPLITS[:3] + ((8, 8),):
            ends, rounds = PR.ends_chunked(tab, t, chunk, lanes)
            assert ends.tolist() == want and len(rounds) == -(-n // (chunk * lanes)) >= 2, (src, chunk, lanes)
    # the never-dying carry degenerates to the serial run: one carry round per lane; a bounded one dies within two rounds
    tab, t = _tab(r'a.*b', 'a' + 'c' * 62 + 'b')
    ends, rounds = PR.ends_chunked(tab, t, 4, 16)
    assert ends.tolist() == PR.ends_cpu(tab, t).tolist() == [64] and rounds == [15]
    tab, t = _tab(r'abcab', 'xabcab' * 10)
    ends, rounds = PR.ends_chunked(tab, t, 4, 5)
    assert ends.tolist() == PR.ends_cpu(tab, t).tolist() == list(range(6, 61, 6)) and 1 <= max(rounds) <= 2
    tab, t = _tab(r'a+', 'a' * 20000 + 'b')                                   # the kernel's own split: 128 columns a lane, 64 lanes, three rounds
    ends, rounds = PR.ends_chunked(tab, t)
    assert ends.tolist() == list(range(1, 20001)) and rounds == [1, 1, 1]     # the carried state is a subset of the speculative one: one round, no new bit after it


# -- the subset page patterns also takes ------------------------------------------------------------------------------------------------
FLAT = [r'\d{2}[./-]\d{2}[./-]\d{4}', r'[A-Z]{2}\d{2} ?\d{4}', r'\d{1,4}', r'a?b{2}c{0,2}', r'x{2,3}y?z', r'[ab]{1,3}c?']


def test_flat_patterns_equal_page_patterns_at_k_0():
    rng = random.Random(11)
    pages = [''.join(rng.choice('ab c12./-xyzDE') for _ in range(rng.choice((0, 1, 7, 60, 300)))) for _ in range(12)]
    pages += ['12.04.2024 DE12 3456 xxyz abbcc 1234567', 'abbc' * 40]
    jobs = np.asarray([(p, q) for p in range(len(pages)) for q in range(len(FLAT))], dtype=np.int32)
    pool, po, pl, masks, opt, P, sigma = PP.encode_patterns(pages, FLAT)
    want = PP.search_cpu(pool, po, pl, masks, opt, P, jobs, np.zeros(len(FLAT), np.int32), 8)
    enc = PR.encode_regex(pages, FLAT)
    assert enc[0].tolist() == pool.tolist() and enc[3].tolist() == masks.tolist() and enc[8].tolist() == P.tolist() and enc[9] == sigma
    got = PR.search_cpu(*enc[:9], jobs, 8)
    hit = want['best'][:, 1] > 0
    assert hit.sum() >= 20 and (want['n_hits'] > 8).any()
    assert got['n_hits'].tolist() == want['n_hits'].tolist() and got['hits'].tolist() == want['hits'].tolist()
    assert got['best'].tolist() == want['best'].tolist() and want['best'][~hit].tolist() == [[1, 0]] * int((~hit).sum())
    assert all(got[k].dtype == np.int32 for k in got)


# -- the hit rule ---------------------------------------------------------------------------------------------------------------------
def _search(texts, exprs, jobs, H):
    enc = PR.encode_regex(texts, exprs)
    return PR.search_cpu(*enc[:9], np.asarray(jobs, dtype=np.int32), H)


def test_a_hit_is_the_last_column_of_a_run_of_ends():
    res = _search(['12345 ', '12 345', 'ab', ''], [r'\d+', r'\d'], [(0, 0), (1, 0), (1, 1), (2, 0), (3, 0)], 4)
    assert res['n_hits'].tolist() == [1, 2, 2, 0, 0] and res['best'].tolist() == [[0, 1], [0, 1], [0, 1], [1, 0], [1, 0]]
    assert res['hits'][0].tolist() == [[5, 0, 0]] + [[-1, -1, -1]] * 3
    assert res['hits'][1].tolist() == [[2, 0, 0], [6, 0, 3], [-1, -1, -1], [-1, -1, -1]]       # a run of ends that reaches n
    assert res['hits'][2].tolist() == [[2, 0, 1], [6, 0, 5], [-1, -1, -1], [-1, -1, -1]]
    assert (res['hits'][3:] == -1).all()
    one = _search(['1 22 333'], [r'\d+'], [(0, 0)], 1)                                          # more hits than are kept
    assert one['n_hits'].tolist() == [3] and one['hits'].tolist() == [[[1, 0, 0]]] and one['best'].tolist() == [[0, 1]]
    amb = _search(['xab abcd ac', 'abc xbc'], [r'(a|ab)(c|bcd)?', r'(b|ab)c'], [(0, 0), (1, 1)], 4)  # the longest of several
    assert amb['hits'][0].tolist() == [[3, 0, 1], [8, 0, 4], [11, 0, 9], [-1, -1, -1]] and amb['n_hits'].tolist() == [3, 2]
    assert amb['hits'][1][:2].tolist() == [[3, 0, 0], [7, 0, 5]]
    loop = _search(['a' + 'x' * 500 + 'b' + 'x' * 9 + 'b'], [r'a.*b'], [(0, 0)], 4)            # no span cap on the reverse walk
    assert loop['hits'][0][:2].tolist() == [[502, 0, 0], [512, 0, 0]]


# -- refusals -------------------------------------------------------------------------------------------------------------------------
def test_parser_refuses_with_the_expression_and_the_offset():
    for src, at, word in ((r'^ab', 0, 'anchors'), (r'ab$', 2, 'anchors'), (r'(a|^b)', 3, 'anchors'), (r'a\b', 1, 'anchors'), (r'a\B', 1, 'anchors'),
                          (r'\Aa', 0, 'anchors'), (r'a\Z', 1, 'anchors'), (r'(a)\1', 3, 'back-references'), (r'ab??', 3, 'lazy'), (r'a*?', 2, 'lazy'),
                          (r'a+?', 2, 'lazy'), (r'a{2}?', 4, 'lazy'), (r'(ab)*+', 5, 'possessive'), (r'a{1,2}+', 6, 'possessive'), (r'a**', 2, 'quantifier on a quantifier'),
                          (r'a?{2}', 2, 'quantifier on a quantifier'), (r'(a)+*', 4, 'quantifier on a quantifier'), (r'a{2}{3}', 4, 'quantifier on a quantifier'),
                          (r'()', 1, 'empty'), (r'a()', 2, 'empty'), (r'(a|)', 3, 'empty'), (r'(|a)', 1, 'empty'), (r'a||b', 2, 'empty'), (r'a|', 2, 'empty'),
                          (r'|a', 0, 'empty'), (r'(?:)', 3, 'empty'), (r'(?=a)b', 0, 'extension'), (r'(?!a)b', 0, 'extension'), (r'(?P<n>a)', 0, 'extension'),
                          (r'a(?i)b', 1, 'extension'), (r'(?<=a)b', 0, 'extension'), (r'(?#c)a', 0, 'extension'), (r'(ab', 0, 'not closed'), (r'a(b(c)', 1, 'not closed'),
                          (r'ab)', 2, 'closes nothing'), (r'?a', 0, 'nothing to repeat'), (r'(*a)', 1, 'nothing to repeat'), (r'a|+', 2, 'nothing to repeat'),
                          (r'a{', 1, 'brace'), (r'a{x}', 1, 'brace'), (r'a{}', 1, 'brace'), (r'a}', 1, 'brace'), (r'a{3,2}', 1, 'b < a'), (r'a{0}b', 1, 'repeats nothing'),
                          (r'(a){0,0}b', 3, 'repeats nothing'), ('a[bc', 1, 'not closed'), ('ab\\', 2, 'backslash'), (r'a\q', 1, 'escape'), ('a[z-a]', 1, 'refused by re'),
                          ('', 0, 'no position'), ('a' * 65, 0, '64 positions'), (r'a{40}b{25}', 0, '64 positions'), (r'x(ab){33}', 1, '64 positions'),
                          (r'(a{33}){2}', 0, '64 positions'), (r'a{40}|b{25}', 0, '64 positions'), (r'(ab|cd){17}', 0, '64 positions'), (r'a{65,}', 0, '64 positions'),
                          (r'a*', 0, 'empty string'), (r'a?b{0,3}', 0, 'empty string'), (r'(a|b?)', 0, 'empty string'), (r'(a*)+', 0, 'empty string'),
                          (r'a|b*', 0, 'empty string'), (r'(ab)?(c|d*)', 0, 'empty string')):
        with pytest.raises(ValueError) as e:
            PR.parse_regex(src)
        assert 'expression %r, offset %d:' % (src, at) in str(e.value) and word in str(e.value), (src, str(e.value))
    with pytest.raises(ValueError):
        PR.parse_regex(12)
    for src in (r'a*', r'(a', r'a\1'):                                         # what re accepts or refuses does not matter: the refusal is ours
        with pytest.raises(ValueError):
            PR.encode_regex(['abc'], [src])


def test_search_cpu_refuses_what_the_device_refuses():
    enc = list(PR.encode_regex(['ab1', 'b'], [r'a(b|c)+', r'\d']))
    ok = dict(zip('pool page_off page_len masks first last follow pred pat_len'.split(), enc[:9]), jobs=[[0, 0], [1, 1]], max_hits=4)
    assert PR.search_cpu(**ok)['n_hits'].tolist() == [1, 0]
    u64 = lambda v: np.asarray(v, dtype=np.uint64)                            # noqa: E731

    def row(name, q, i, v):
        a = ok[name].copy()
        a[q, i] = v
        return {name: a}
    cases = [dict(page_len=[PS.JOBS_MAX, 1]), dict(page_len=[PP.LEN_MAX + 1, 1]), dict(page_len=[-1, 1]), dict(page_off=[2, 0]), dict(page_off=[-1, 0]), dict(page_off=[0]),
             dict(pat_len=[0, 1]), dict(pat_len=[65, 1]), dict(pat_len=[3]), dict(pat_len=[2, 1]), dict(first=u64([8, 1])), dict(last=u64([6, 2])),
             dict(first=u64([0, 1])), dict(last=u64([6, 0])), dict(first=u64([1])), row('follow', 0, 0, 14), row('follow', 1, 1, 1), row('follow', 0, 3, 1),
             row('pred', 0, 1, 15), row('pred', 0, 5, 1), row('follow', 0, 0, 2), row('pred', 0, 2, 0), dict(follow=ok['follow'][:, :63]), dict(pred=ok['pred'][:1]),
             dict(max_hits=0), dict(max_hits=65), dict(jobs=[[2, 0]]), dict(jobs=[[0, 2]]), dict(jobs=[[-1, 0]]), dict(jobs=[[0, -1]]),
             dict(masks=np.zeros((2, 256), np.uint64)), dict(masks=np.zeros((2, 0), np.uint64)), dict(masks=np.zeros((1, 3), np.uint64)), dict(masks=np.zeros(6, np.uint64))]
    for kw in cases:
        with pytest.raises(ValueError):
            PR.search_cpu(**dict(ok, **kw))
        with pytest.raises(ValueError):
            PR.HostRegexSearcher().run(**dict(ok, **kw))
    with pytest.raises(ValueError):
        PR.tables(ok['masks'], u64([16, 1]), ok['last'], ok['follow'], ok['pred'], ok['pat_len'])
    with pytest.raises(ValueError):
        PR.encode_regex(['a' * (PP.LEN_MAX + 1)], ['a'])
    assert PR.search_cpu(**dict(ok, jobs=np.zeros((0, 2), np.int32)))['hits'].shape == (0, 4, 3)


# -- find_regex -----------------------------------------------------------------------------------------------------------------------
def _word(text, x, y, w=40, h=10, **kw):
    return dict(rec=text, polys=[[x, y], [x + w, y], [x + w, y + h], [x, y + h]], **kw)


def _page():
    """`Rechnung Nr. 12345 Total EUR 1,234,567.89` / `Invoice no 77 CHF 5 Date 3 Feb 2024 id AB123456789`"""
    return [_word('Rechnung', 0, 0), _word('Nr.', 50, 0), _word('12345', 100, 0), _word('Total', 150, 0), _word('EUR', 200, 0), _word('1,234,567.89', 250, 0),
            _word('Invoice', 0, 20), _word('no', 50, 20), _word('77', 100, 20), _word('CHF', 150, 20), _word('5', 200, 20),
            _word('Date', 0, 40), _word('3', 50, 40), _word('Feb', 100, 40), _word('2024', 150, 40), _word('id', 200, 40), _word('AB123456789', 250, 40)]


def test_find_regex_on_a_three_line_page():
    page = _page()
    host = PR.HostRegexSearcher()
    exprs = [('amount', r'\d{1,3}(,\d{3})*\.\d{2}'), r'(EUR|USD|CHF) ?\d+', ('date', r'\d{1,2} (Jan|Feb|Mar) \d{4}'), ('label', r'(invoice|rechnung) ?(no|nr)\.?'),
             r'[A-Z]{2}\d+', 'zzzz']
    res = find_regex([page], exprs, searcher=host)
    assert host.calls == 1 and len(res) == 1 and [d['name'] for d in res[0]] == ['amount', None, 'date', 'label', None, None]
    assert [d['pattern'] for d in res[0]] == [p if isinstance(p, str) else p[1] for p in exprs] and [d['P'] for d in res[0]] == [10, 11, 17, 21, 3, 4]
    assert all(set(d) == {'pattern', 'name', 'P', 'best', 'n_hits', 'dropped', 'hits'} for d in res[0])
    amount, currency, date, label, ident, none = res[0]
    text = PS.page_index(page, normalise=None)[0]
    h = amount['hits'][0]
    assert amount['n_hits'] == 1 and amount['best'] == 0 and h['text'] == '1,234,567.89' and h['words'] == (5, 5) and h['records'] == [page[5]] and h['dist'] == 0
    assert h['box'] == (250.0, 0.0, 290.0, 10.0) and h['chars'] == (text.index('1,234'), text.index('1,234') + 12)
    assert [(h['text'], h['words']) for h in currency['hits']] == [('EUR 1', (4, 5)), ('CHF 5', (9, 10))] and currency['hits'][0]['box'] == (200.0, 0.0, 290.0, 10.0)
    assert [(h['text'], h['words']) for h in date['hits']] == [('3 Feb 2024', (12, 14))] and date['hits'][0]['records'] == page[12:15]
    assert label['hits'] == [] and label['best'] is None and label['n_hits'] == 0                          # expressions are case-sensitive
    assert [(h['text'], h['words']) for h in ident['hits']] == [('AB123456789', (16, 16))]                # one hit for the whole run, the longest match
    assert none['hits'] == [] and none['n_hits'] == 0 and none['dropped'] == 0 and none['best'] is None
    assert all(text[h['chars'][0]:h['chars'][1]] == h['text'] for d in res[0] for h in d['hits'])
    folded = find_regex([page], [exprs[3]], normalise=str.casefold, searcher=host)[0][0]                    # normalise touches the page, never the expression
    assert [(h['text'], h['words']) for h in folded['hits']] == [('rechnung nr.', (0, 1)), ('invoice no', (6, 7))]
    assert [type(v) for v in folded['hits'][0]['chars']] == [int, int] and type(folded['hits'][0]['dist']) is int


def test_find_regex_per_image_lists_drops_and_refusals():
    page = _page()
    host = PR.HostRegexSearcher()
    res = find_regex([page, page[6:11], []], [[r'\d+'], [('n', r'(no|nr) \d+'), 'CHF|EUR'], ['Total']], searcher=host)
    assert host.calls == 1 and [len(r) for r in res] == [1, 2, 1]
    assert [h['words'] for h in res[0][0]['hits']] == [(2, 2), (5, 5), (5, 5), (5, 5), (5, 5), (8, 8), (10, 10), (12, 12), (14, 14), (16, 16)]
    assert res[1][0]['name'] == 'n' and res[1][0]['hits'][0]['words'] == (1, 2) and res[1][1]['hits'][0]['words'] == (3, 3)
    assert res[2][0]['best'] is None and res[2][0]['hits'] == []              # an empty page
    assert find_regex([page], [], searcher=host) == [[]] and host.calls == 1
    res = find_regex([[_word('ab', 0, 0), _word('cd', 50, 0)]], ['-+', '( |-)+'], sep=' - ', searcher=host)
    assert res[0][0]['n_hits'] == 1 and res[0][0]['dropped'] == 1 and res[0][0]['hits'] == []      # a hit inside a separator
    assert res[0][1]['dropped'] == 1 and res[0][1]['n_hits'] == 1
    res = find_regex([page], [r'\d+'], max_hits=3, searcher=host)
    assert res[0][0]['n_hits'] == 10 and len(res[0][0]['hits']) == 3
    for bad in (dict(expressions=['a(b']), dict(expressions=['a*']), dict(expressions=[('n', 'a', 'b')]), dict(expressions=[7]), dict(expressions=[['a'], ['b']]),
                dict(records=[[('entity', 'value')]], expressions=['a'])):
        with pytest.raises(ValueError):
            find_regex(**dict(dict(records=[page], searcher=host), **bad))
    with pytest.raises(RuntimeError):
        find_regex([page], ['a'], device='cpu')                                # no CPU fallback behind the device stage


def test_find_regex_equals_find_pattern_on_the_shared_subset():
    pages = [_page(), _page()[6:], [_word('12.04.2024', 0, 0), _word('1', 50, 0), _word('22', 100, 0), _word('4444', 150, 0), _word('55555', 200, 0)]]
    shared = [('number', r'\d{1,4}'), r'[A-Z]{2}\d{2}', r'\d{2}[./-]\d{2}[./-]\d{4}', r'no ?\d{2}', 'Total']
    got = find_regex(pages, shared, max_hits=32, searcher=PR.HostRegexSearcher())
    want = find_pattern(pages, shared, max_hits=32, searcher=PP.HostPatternSearcher())
    assert sum(len(d['hits']) for per in want for d in per) >= 20
    for g_img, w_img in zip(got, want):
        for g, w in zip(g_img, w_img):
            assert {k: g[k] for k in g} == {k: w[k] for k in g} and w['k'] == 0
            assert g['hits'] == w['hits']                                      # hit by hit, records and boxes included


def test_the_command_line_on_a_results_file(tmp_path, capsys):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import find_regex as tool
    flat = [dict(r, image_id='a.jpg', score=0.9) for r in _page()] + [dict(r, image_id='b.jpg', score=0.8) for r in _page()[6:11]]
    results, expressions = tmp_path / 'results.json', tmp_path / 'expressions.json'
    results.write_text(json.dumps(flat))
    exprs = [dict(name='amount', expression=r'\d{1,3}(,\d{3})*\.\d{2}'), r'(EUR|CHF) ?\d+']
    expressions.write_text(json.dumps(exprs))
    doc = tool.main(['--results', str(results), '--expressions', str(expressions), '--host'])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(doc))
    want = find_regex([_page(), _page()[6:11]], [('amount', exprs[0]['expression']), exprs[1]], searcher=PR.HostRegexSearcher())
    assert [im['image_id'] for im in doc['images']] == ['a.jpg', 'b.jpg'] and doc['records'] == 22 and doc['searcher'] == 'host' and doc['max_hits'] == 16
    for im, per in zip(doc['images'], want):
        for got, w in zip(im['expressions'], per):
            assert (got['pattern'], got['name'], got['P'], got['best'], got['n_hits']) == (w['pattern'], w['name'], w['P'], w['best'], w['n_hits'])
            assert [(h['chars'], h['words'], h['dist'], h['box'], h['text']) for h in got['hits']] == [(h['chars'], h['words'], h['dist'], h['box'], h['text']) for h in w['hits']]
            assert all('records' not in h for h in got['hits'])
    assert doc['images'][0]['expressions'][0]['hits'][0]['words'] == (5, 5) and doc['images'][1]['expressions'][1]['hits'][0]['text'] == 'CHF 5'
    expressions.write_text(json.dumps({'b': [r'\d+'], 'a.jpg': ['Feb|Mar']}))
    doc = tool.main(['--results', str(results), '--expressions', str(expressions), '--host', '--max-hits', '1'])
    assert [[q['pattern'] for q in im['expressions']] for im in doc['images']] == [['Feb|Mar'], [r'\d+']]
    assert doc['images'][0]['expressions'][0]['hits'][0]['words'] == (13, 13) and doc['images'][1]['expressions'][0]['hits'][0]['words'] == (2, 2)
    assert doc['images'][1]['expressions'][0]['n_hits'] == 2 and len(doc['images'][1]['expressions'][0]['hits']) == 1
    expressions.write_text(json.dumps(['a(b']))
    with pytest.raises(ValueError):
        tool.main(['--results', str(results), '--expressions', str(expressions), '--host'])


# -- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_entry_point_matches_the_header():
    from advancedliteratemachinery_amd import _lib, build, ops
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24   # the library only gains an entry point
    m = re.search(r'int omp_page_regex_search\((.*?)\);', text, re.S)
    want = []
    for p in (' '.join(p.split()) for p in m.group(1).split(',')):
        if '*' in p or p.startswith('omp_stream_t'):
            want.append(ctypes.c_void_p)
        elif p.startswith('int64_t '):
            want.append(ctypes.c_int64)
        else:
            assert p.startswith('int '), p
            want.append(ctypes.c_int)
    res, args = _lib._SIGS['omp_page_regex_search']
    assert res is ctypes.c_int and args == want and len(want) == 20 and 'omp_page_regex_search' in _lib.EXPORTS
    assert 'page_regex.hip' in build.SOURCES and 'page_regex.hip' not in build.AUDITED
    assert callable(ops.page_regex_search) and not hasattr(ops, 'page_regex_scratch_bytes')         # the kernel needs no scratch
    src = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'page_regex.hip')).read()
    hdr = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'page_frame.h')).read()       # the shared constants: test_page_search_host.py
    assert 'extern "C" int omp_page_regex_search(' in src and '#include "page_frame.h"' in src
    assert 'PG_LEN_MAX = %d' % PP.LEN_MAX in hdr and 'PG_POS_MAX = %d' % PR.POS_MAX in hdr and 'PG_CHUNK = %d' % PR.CHUNK in hdr
    assert 'PG_HITS_MAX = %d' % PS.HITS_MAX in hdr and 'PG_SIGMA_MAX = %d' % PP.SIGMA_MAX in hdr and 'PG_JOBS_MAX = 1 << 20' in hdr
    assert PR.ROUND == 64 * PR.CHUNK == 8192 and PR.LANES == 64 and ops.PAGE_REGEX_CHUNK == PR.CHUNK
    with pytest.raises(RuntimeError):
        PR.RegexSearcher('cpu')
