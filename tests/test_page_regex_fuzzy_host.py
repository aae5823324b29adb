"""Page expressions with errors on the host (no GPU): the set form, the word form and the chunk-and-carry split of the step
(utils/page_regex.py: dist_py, dist_cpu, dist_chunked) against each other, rows, distances and starts against a brute force that walks
every path of the automaton with a plain Levenshtein table, k = 0 pinned to the exact search, flat expressions pinned to page patterns at
k = 1 .. 3, min_len and the tolerance at their edges, the refusals, and find_regex with and without max_dist on hand-made pages.  The
kernel and the device stage are tests/test_gpu_page_regex_fuzzy.py."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest

from advancedliteratemachinery_amd.engine.search import find_regex
from advancedliteratemachinery_amd.utils import page_pattern as PP
from advancedliteratemachinery_amd.utils import page_regex as PR
from advancedliteratemachinery_amd.utils import page_search as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 1 << 20


def _bits(x):
    return [i for i in range(64) if (int(x) >> i) & 1]


def _automaton(rng, P, sigma, fan=2):
    """a random automaton of P positions whose last is reachable: position i goes on to i + 1 mostly, and to at most `fan` positions"""
    while True:
        follow = []
        for i in range(P):
            f = (1 << (i + 1)) if i + 1 < P and rng.random() < 0.85 else 0
            if rng.random() < 0.4 and bin(f).count('1') < fan:
                f |= 1 << rng.randrange(P)
            follow.append(f)
        first = 1 | ((1 << rng.randrange(P)) if rng.random() < 0.3 else 0)
        last = (1 << (P - 1)) | ((1 << rng.randrange(P)) if rng.random() < 0.3 else 0)
        if PR.min_len(first, last, follow) <= P:
            break
    mask = np.zeros(sigma + 1, dtype=np.uint64)
    for i in range(P):
        for c in set([rng.randrange(sigma)] + [c for c in range(sigma) if rng.random() < 0.3]):
            mask[c] |= np.uint64(1 << i)
    rows = follow + [0] * (PR.POS_MAX - P)
    return PR.Tables(mask, first, last, rows, PR._transpose(rows), P)


# -- the brute force: every path of the automaton, a plain Levenshtein table; nothing of the module --------------------------------
def _next_row(prev, member):
    """the table's row of one more position: member[j - 1] says that character j is in its class"""
    cur = [prev[0] + 1]
    for j in range(1, len(prev)):
        cur.append(min(prev[j - 1] + (0 if member[j - 1] else 1), prev[j] + 1, cur[j - 1] + 1))
    return cur


def brute_costs(tab, t, k):
    """cost[j][p]: the least edit distance of some t[s:j] to some path from first that ends at p, exact wherever it is <= k"""
    n, P = len(t), tab.P
    member = [[bool((int(tab.mask[min(c, len(tab.mask) - 1)]) >> p) & 1) for c in t] for p in range(P)]
    cost = [[INF] * P for _ in range(n + 1)]

    def walk(p, row, depth):
        for j in range(n + 1):
            cost[j][p] = min(cost[j][p], row[j])
        if depth >= n + k or min(row) > k:                                   # a longer path costs more than k against any stretch
            return
        for q in _bits(tab.follow[p]):
            walk(q, _next_row(row, member[q]), depth + 1)
    for p in _bits(tab.first):
        walk(p, _next_row([0] * (n + 1), member[p]), 1)                       # row 0 of zeros: the stretch may start anywhere
    return cost


def brute_start(tab, t, end, dist):
    """the least s whose anchored distance of t[s:end] to the language equals dist: the paths backwards from last to first against the
    reversed stretch, row 0 = 0, 1, 2, ..."""
    u = list(t[:end])[::-1]
    member = [[bool((int(tab.mask[min(c, len(tab.mask) - 1)]) >> p) & 1) for c in u] for p in range(tab.P)]
    best = [INF] * (end + 1)                                                 # best[l]: the anchored distance of t[end - l:end]

    def walk(p, row, depth):
        if (tab.first >> p) & 1:
            for l in range(end + 1):
                best[l] = min(best[l], row[l])
        if depth >= end + dist or min(row) > dist:
            return
        for q in _bits(tab.pred[p]):
            walk(q, _next_row(row, member[q]), depth + 1)
    for p in _bits(tab.last):
        walk(p, _next_row(list(range(end + 1)), member[p]), 1)
    return end - max(l for l in range(end + 1) if best[l] == dist)


def _tiny_cases(count, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        P, sigma = rng.randint(1, 6), rng.randint(1, 3)
        tab = _automaton(rng, P, sigma)
        k = rng.randint(0, min(2, PR.min_len(tab.first, tab.last, tab.follow) - 1))
        t = np.asarray([rng.randrange(sigma + 1) for _ in range(rng.randint(0, 7))], dtype=np.uint8)     # code sigma: in no class
        out.append((tab, t, k))
    return out


def test_rows_distances_and_starts_equal_the_brute_force():
    cases = _tiny_cases(400, 11)
    hits = with_errors = loops = 0
    for tab, t, k in cases:
        cost = brute_costs(tab, t.tolist(), k)
        v, rows = PR.dist_py(tab, t, k, rows=True)
        for j in range(len(t) + 1):
            for i in range(k + 1):
                assert rows[j][i] == frozenset(p for p in range(tab.P) if cost[j][p] <= i), (tab, t, k, j, i)
        want = [k + 1] + [min(k + 1, min(cost[j][p] for p in _bits(tab.last))) for j in range(1, len(t) + 1)]
        assert v.tolist() == want and PR.dist_cpu(tab, t, k).tolist() == want
        loops += any((int(f) >> i) & 1 for i, f in enumerate(tab.follow[:tab.P]))
        for e in PS.hit_ends(v, k).tolist():
            assert PR.fuzzy_start(tab, t, e, int(v[e])) == brute_start(tab, t.tolist(), e, int(v[e])), (tab, t, k, e)
            hits += 1
            with_errors += int(v[e]) > 0
    assert hits >= 150 and with_errors >= 60 and loops >= 20 and sum(k == 2 for _, _, k in cases) >= 30


def test_the_set_form_the_word_form_and_the_split_agree():
    rng = random.Random(5)
    carried = 0
    for _ in range(120):
        P = rng.choice((1, 2, 5, 8, 9, 17, 40, 64))
        sigma = rng.randint(1, 4)
        tab = _automaton(rng, P, sigma, fan=3)
        k = rng.randint(0, min(PR.K_MAX, PR.min_len(tab.first, tab.last, tab.follow) - 1))
        t = np.asarray([rng.randrange(sigma + 1) for _ in range(rng.randint(0, 60))], dtype=np.uint8)
        v = PR.dist_cpu(tab, t, k)
        assert PR.dist_py(tab, t, k).tolist() == v.tolist() and v[0] == k + 1 and v.dtype == np.int32
        for chunk, lanes in ((4, 4), (3, 2), (1, 5), (128, 64)):
            got, rounds = PR.dist_chunked(tab, t, k, chunk, lanes)
            assert got.tolist() == v.tolist(), (tab, t, k, chunk, lanes)
            carried += sum(rounds) > 0
    assert carried >= 100


def test_a_carry_that_never_dies_and_one_that_climbs_the_rows():
    tab, pool = _tab(r'a.*b', 'xaxxxxxxxxxxxxb')
    for k in (0, 1):
        v = PR.dist_cpu(tab, pool, k)
        got, rounds = PR.dist_chunked(tab, pool, k, 2, 4)
        assert got.tolist() == v.tolist() and v[-1] == 0 and max(rounds) >= 3     # the state of `.*` crosses every lane of a round
    tab, pool = _tab(r'abcdef', 'xxabXdefxx')                                    # the substituted c lies in another chunk than the end
    got, _ = PR.dist_chunked(tab, pool, 1, 3, 2)
    assert got.tolist() == PR.dist_cpu(tab, pool, 1).tolist() and got[8] == 1 and PR.fuzzy_start(tab, pool, 8, 1) == 2


EXPRESSIONS = [r'a(b|c)*a', r'(ab|ba)+', r'(a|bc){2,3}c', r'a.*b', r'a+b?c{2,}', r'((ab)?c)+', r'a{0,2}b', r'(a*b)+', r'(?:ab|c)+a']


def _tab(src, text):
    enc = PR.encode_regex([text], [src])
    return PR.tables(*enc[3:9]), enc[0]


def test_k_0_is_the_exact_search_on_every_integer():
    rng = random.Random(3)
    texts = [''.join(rng.choice('abc') for _ in range(rng.randint(0, 40))) for _ in range(60)]
    enc = PR.encode_regex(texts, EXPRESSIONS)
    jobs = [(p, q) for p in range(len(texts)) for q in range(len(EXPRESSIONS))]
    want = PR.search_cpu(*enc[:9], jobs, 8)
    got = PR.fuzzy_search_cpu(*enc[:9], jobs, np.zeros(len(EXPRESSIONS), np.int32), 8)
    assert set(got) == set(want) == {'best', 'n_hits', 'hits'} and want['n_hits'].sum() > 300
    for key in want:
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key])
    for p, q in jobs[::7]:
        tab = PR.tables(*enc[3:9], q)
        t = enc[0][enc[1][p]:enc[1][p] + enc[2][p]]
        assert np.flatnonzero(PR.dist_cpu(tab, t, 0) == 0).tolist() == PR.ends_cpu(tab, t).tolist()
        for e in PR.ends_cpu(tab, t).tolist():
            assert PR.fuzzy_start(tab, t, e, 0) == PR.match_start(tab, t, e)


FLAT = [(r'\d{2}[./-]\d{2}[./-]\d{4}', '0123./- a'), (r'[A-Z]{3} ?\d{1,3}', 'EURX 12a'), ('abcab', 'abc'), (r'a?bc{1,3}d', 'abcd'), (r'ab{0,2}c?a.b', 'abcx'),
        (r'\d{1,3},\d{3}', '12,a'), (r'id ?\d{4}', 'id 12x')]


@pytest.mark.parametrize('k', [1, 2, 3])
def test_flat_expressions_equal_page_patterns(k):
    """an expression in find_pattern's subset gets find_pattern's best, hits, distances and starts at equal k"""
    rng = random.Random(k)
    total = errors = 0
    for src, alphabet in FLAT:
        texts = [''.join(rng.choice(alphabet) for _ in range(rng.randint(0, 50))) for _ in range(20)]
        pat, rx = PP.parse_pattern(src), PR.parse_regex(src)
        assert rx.min_len == pat.Mand
        kk = min(k, pat.Mand - 1)
        jobs = [(p, 0) for p in range(len(texts))]
        e1 = PP.encode_patterns(texts, [pat])
        want = PP.search_cpu(*e1[:6], jobs, [kk], 16)
        e2 = PR.encode_regex(texts, [rx])
        got = PR.fuzzy_search_cpu(*e2[:9], jobs, [kk], 16)
        for key in want:
            assert np.array_equal(got[key], want[key]), (src, key)
        total += int(want['n_hits'].sum())
        errors += int((want['hits'][:, :, 1] > 0).sum())
    assert total >= 100 and errors >= 50


def test_min_len_and_the_tolerance_at_their_edges():
    for src, want in ((r'a', 1), (r'a|bcd', 1), (r'ab?c', 2), (r'(ab|cde)+f', 3), (r'a{3,5}', 3), (r'a.*b', 2), (r'(EUR|USD) ?\d+', 4), ('a' * 64, 64),
                      (r'\d{1,3}(,\d{3})*\.\d{2}', 4), (r'\d{1,2} (Jan|Feb|Mar) \d{4}', 10)):
        assert PR.parse_regex(src).min_len == want, src
    assert PR.min_len(1, 4, [2, 0, 0]) == PR.POS_MAX + 1                          # last cannot be reached
    assert PR.K_MAX == 4
    assert PR.regex_tolerance(1, 5, 1.0) == 0                                   # min_len = 1: nothing may be deleted
    assert PR.regex_tolerance(2, 5, None) == 1 and PR.regex_tolerance(4, None, None) == 3 and PR.regex_tolerance(5, None, None) == 4
    assert PR.regex_tolerance(64, None, None) == 4 and PR.regex_tolerance(64, 9, 1.0) == 4         # the cap
    assert PR.regex_tolerance(10, None, 0.2) == 2 and PR.regex_tolerance(10, 1, 0.2) == 1 and PR.regex_tolerance(10) == 0
    assert PR.regex_tolerance(10, 0, 1.0) == 0
    with pytest.raises(ValueError):
        PR.regex_tolerance(10, -1)
    with pytest.raises(ValueError):
        PR.regex_tolerance(10, None, 1.5)


def test_the_refusals():
    enc = PR.encode_regex(['abcabc', 'xx'], ['abc', 'a|bcd'])
    ok = dict(zip('pool page_off page_len masks first last follow pred pat_len'.split(), enc[:9]), jobs=[(0, 0), (1, 1)], k=[2, 0], max_hits=4)
    assert PR.fuzzy_search_cpu(**ok)['n_hits'].tolist() == [2, 0]
    for what, kw in (('k = -1', dict(k=[-1, 0])), ('k above K_MAX', dict(k=[5, 0])), ('k = min_len', dict(k=[3, 0])), ('k = min_len = 1', dict(k=[0, 1])),
                     ('one k for two expressions', dict(k=[1])), ('max_hits 65', dict(max_hits=65)), ('a page that is not there', dict(jobs=[(2, 0)])),
                     ('first == 0', dict(first=[0, 1])), ('a range outside the pool', dict(page_off=[0, 7]))):
        with pytest.raises(ValueError):
            PR.fuzzy_search_cpu(**dict(ok, **kw))
        with pytest.raises(ValueError):
            PR.HostFuzzyRegexSearcher().run(**dict(ok, **kw))
    tab = PR.tables(*enc[3:9], 0)
    for fn in (PR.dist_py, PR.dist_cpu, PR.dist_chunked):
        with pytest.raises(ValueError):
            fn(tab, enc[0][:6], 5)
    assert PR.fuzzy_search_cpu(**dict(ok, jobs=np.zeros((0, 2), np.int32)))['hits'].shape == (0, 4, 3)


# -- find_regex -----------------------------------------------------------------------------------------------------------------------
def _word(text, x, y, w=40, h=10):
    return dict(rec=text, polys=[[x, y], [x + w, y], [x + w, y + h], [x, y + h]])


def _page():
    """`Total EUP 120 net 1,2O0.00 due 12 Jau 2024 sum 12O.50`"""
    return [_word(w, 50 * i, 0) for i, w in enumerate('Total EUP 120 net 1,2O0.00 due 12 Jau 2024 sum 12O.50'.split())]


class _Plain(PR.HostRegexSearcher):
    """a HostRegexSearcher that records what it was called with"""

    def run(self, *a, **kw):
        self.seen = (len(a), sorted(kw))
        return super().run(*a, **kw)


def test_find_regex_with_the_defaults_is_the_exact_search():
    page = _page()
    host = _Plain()
    exprs = [('currency', r'(EUR|USD) ?\d+'), r'\d{1,2} (Jan|Feb|Mar) \d{4}', r'\d+']
    res = find_regex([page], exprs, searcher=host)
    assert host.calls == 1 and host.seen == (11, [])                           # no k: the exact searcher's own arguments
    assert all(set(d) == {'pattern', 'name', 'P', 'best', 'n_hits', 'dropped', 'hits'} for d in res[0])
    assert res[0][0]['best'] is None and res[0][0]['hits'] == [] and res[0][1]['best'] is None     # one misread character: absent
    assert [h['text'] for h in res[0][2]['hits']] == ['120', '1', '2', '0', '00', '12', '2024', '12', '50'] and all(h['dist'] == 0 for h in res[0][2]['hits'])
    assert find_regex([page], exprs, searcher=PR.HostRegexSearcher(), max_dist=None, max_ratio=0.0) == res


def test_find_regex_with_errors_finds_the_misread_fields():
    page = _page()
    text = PS.page_index(page, normalise=None)[0]
    host = PR.HostFuzzyRegexSearcher()
    exprs = [('currency', r'(EUR|USD) ?\d+'), ('amount', r'\d{1,3}(,\d{3})*\.\d{2}'), ('date', r'\d{1,2} (Jan|Feb|Mar) \d{4}'), 'Total', 'x']
    res = find_regex([page], exprs, max_dist=1, searcher=host)
    assert host.calls == 1 and len(res) == 1 and [d['name'] for d in res[0]] == ['currency', 'amount', 'date', None, None]
    assert all(set(d) == {'pattern', 'name', 'P', 'k', 'best', 'n_hits', 'dropped', 'hits'} for d in res[0])
    assert [d['k'] for d in res[0]] == [1, 1, 1, 1, 0]                        # `x`: min_len 1, nothing may be deleted
    currency, amount, date, total, x = res[0]
    h = currency['hits'][0]
    at = text.index('EUP')
    assert currency['best'] == 1 and currency['n_hits'] == 1 and h['dist'] == 1 and h['text'] == 'EUP 120' and h['chars'] == (at, at + 7)
    assert h['words'] == (1, 2) and h['records'] == page[1:3] and h['box'] == (50.0, 0.0, 140.0, 10.0)
    # the amount shape: `0.00` stands exactly inside `1,2O0.00` and is the hit there; `12O.50` is found whole at distance 1; `120` and
    # `2024` are `1.20` and `20.24` with the point deleted
    got = [(h['text'], h['dist'], h['words']) for h in amount['hits']]
    assert got == [('120', 1, (2, 2)), ('0.00', 0, (4, 4)), ('2024', 1, (8, 8)), ('12O.50', 1, (10, 10))] and amount['best'] == 0 and amount['n_hits'] == 4
    at = text.index('12O.50')
    assert amount['hits'][1]['records'] == [page[4]] and amount['hits'][3]['chars'] == (at, at + 6) and amount['hits'][3]['records'] == [page[10]]
    wide = find_regex([page], [r'\d,\d{3}\.\d{2}'], max_dist=1, searcher=host)[0][0]           # a shape that holds the whole field
    at = text.index('1,2O0.00')
    assert [(h['text'], h['dist'], h['chars'], h['records']) for h in wide['hits']] == [('1,2O0.00', 1, (at, at + 8), [page[4]])]
    h = date['hits'][0]
    assert date['n_hits'] == 1 and (h['text'], h['dist'], h['words']) == ('12 Jau 2024', 1, (6, 8)) and h['records'] == page[6:9]
    assert total['best'] == 0 and total['hits'][0]['text'] == 'Total' and x['best'] is None and x['k'] == 0
    # max_ratio alone switches the mode on as well; max_dist = 0 is the fuzzy mode with k = 0 everywhere: the exact hits, plus `k`
    ratio = find_regex([page], exprs, max_ratio=0.25, searcher=host)
    assert [d['k'] for d in ratio[0]] == [1, 1, 2, 1, 0] and ratio[0][0]['hits'] == currency['hits']
    zero = find_regex([page], exprs, max_dist=0, searcher=host)
    exact = find_regex([page], exprs, searcher=PR.HostRegexSearcher())
    assert [dict(d, k=0) for d in exact[0]] == zero[0] and host.calls == 4
    with pytest.raises(TypeError):
        find_regex([page], exprs, max_dist=1, searcher=PR.HostRegexSearcher())     # the exact searcher takes no k


def test_the_command_line_with_errors(tmp_path, capsys):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import find_regex as tool
    results, expressions = tmp_path / 'results.json', tmp_path / 'expressions.json'
    results.write_text(json.dumps([dict(r, image_id='a.jpg') for r in _page()]))
    exprs = [{'name': 'currency', 'expression': r'(EUR|USD) ?\d+'}, r'\d{1,2} (Jan|Feb|Mar) \d{4}']
    expressions.write_text(json.dumps(exprs))
    doc = tool.main(['--results', str(results), '--expressions', str(expressions), '--host', '--max-dist', '1'])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])['max_dist'] == 1 and doc['max_ratio'] == 0.0
    got = doc['images'][0]['expressions']
    assert [(q['name'], q['k'], q['best'], [(h['text'], h['dist'], h['words']) for h in q['hits']]) for q in got] == [
        ('currency', 1, 1, [('EUP 120', 1, (1, 2))]), (None, 1, 1, [('12 Jau 2024', 1, (6, 8))])]
    doc = tool.main(['--results', str(results), '--expressions', str(expressions), '--host', '--max-ratio', '0.2'])
    assert [q['k'] for q in doc['images'][0]['expressions']] == [0, 2] and doc['images'][0]['expressions'][0]['hits'] == []
    doc = tool.main(['--results', str(results), '--expressions', str(expressions), '--host'])
    assert 'max_dist' not in doc and all('k' not in q and q['hits'] == [] for q in doc['images'][0]['expressions'])     # exact, as before


# -- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_entry_point_matches_the_header():
    from advancedliteratemachinery_amd import _lib, build, ops
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    m = re.search(r'int omp_page_regex_fuzzy_search\((.*?)\);', text, re.S)
    want = []
    for p in (' '.join(p.split()) for p in m.group(1).split(',')):
        if '*' in p or p.startswith('omp_stream_t'):
            want.append(ctypes.c_void_p)
        elif p.startswith('int64_t '):
            want.append(ctypes.c_int64)
        else:
            assert p.startswith('int '), p
            want.append(ctypes.c_int)
    res, args = _lib._SIGS['omp_page_regex_fuzzy_search']
    assert res is ctypes.c_int and args == want and len(want) == 21 and 'omp_page_regex_fuzzy_search' in _lib.EXPORTS
    exact = _lib._SIGS['omp_page_regex_search'][1]
    assert args == exact[:11] + [ctypes.c_void_p] + exact[11:]                 # omp_page_regex_search's arguments plus k
    # the unit is the exact search's: the kernel at k = 0 is the exact kernel
    assert 'page_regex.hip' in build.SOURCES and 'page_regex.hip' not in build.AUDITED and callable(ops.page_regex_fuzzy_search)
    src = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'page_regex.hip')).read()
    hdr = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'page_frame.h')).read()       # the shared constants: test_page_search_host.py
    assert 'extern "C" int omp_page_regex_fuzzy_search(' in src and 'PR_K_MAX = %d' % PR.K_MAX in src and 'pr_launch<PR_K_MAX + 1>' in src
    assert 'PG_LEN_MAX = %d' % PP.LEN_MAX in hdr and 'PG_POS_MAX = %d' % PR.POS_MAX in hdr and 'PG_CHUNK = %d' % PR.CHUNK in hdr
    assert 'PG_HITS_MAX = %d' % PS.HITS_MAX in hdr and 'PG_SIGMA_MAX = %d' % PP.SIGMA_MAX in hdr and 'PG_JOBS_MAX = 1 << 20' in hdr
    with pytest.raises(RuntimeError):
        PR.FuzzyRegexSearcher('cpu')
