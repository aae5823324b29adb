"""Lexicon correction, CPU side: the distance (edit_distance_cpu, the definition), the bit-parallel
specification the kernel is held to on the GPU (nearest_cpu), the length grid and the damaged tables of the GPU checks
(their coverage, closed forms and hand-worked clamping), encoding, ranges, ties, acceptance, the entry point's
arguments against the header, and the routing of `lexicon=` through predict / predict_images / spot_and_recognize with a
stub matcher."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

from advancedliteratemachinery_amd.utils import lexicon as LX
from advancedliteratemachinery_amd.utils.parser import DEFAULT_CHARS, make_args
from tests import gpu_checks_lexicon as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------
# the distance
# ---------------------------------------------------------------------------------------------
def test_edit_distance_hand_worked():
    d = LX.edit_distance_cpu
    assert d('kitten', 'sitting') == 3
    assert d('', '') == 0 and d('', 'abc') == 3 and d('abcd', '') == 4
    assert d('omniparser', 'omniparser') == 0
    assert d('flaw', 'lawn') == 2 and d('ab', 'ba') == 2              # no transpositions
    assert d('saturday', 'sunday') == 3
    assert d([1, 2, 3], [1, 3]) == 1                                  # any sequence of code units
    rng = np.random.RandomState(0)
    for _ in range(200):
        a, b = K.random_word(rng, 0, 12, 'abc'), K.random_word(rng, 0, 12, 'abc')
        assert d(a, b) == d(b, a)


def _recursive(a, b, memo):
    key = (a, b)
    if key not in memo:
        if not a or not b:
            memo[key] = len(a) + len(b)
        else:
            memo[key] = min(_recursive(a[1:], b, memo) + 1, _recursive(a, b[1:], memo) + 1,
                            _recursive(a[1:], b[1:], memo) + (a[0] != b[0]))
    return memo[key]


def test_edit_distance_equals_the_recursive_definition():
    """all pairs of strings up to length 4 over a 3-letter alphabet (121 x 121)"""
    strings = [''.join(t) for n in range(5) for t in itertools.product('abc', repeat=n)]
    assert len(strings) == 121
    memo = {}
    for a in strings:
        for b in strings:
            assert LX.edit_distance_cpu(a, b) == _recursive(a, b, memo), (a, b)


# ---------------------------------------------------------------------------------------------
# the bit-parallel specification against the definition
# ---------------------------------------------------------------------------------------------
def _pairs_case(rng, q_lens, n_words, chars, word_len, fold_case, foreign):
    """-> mismatches, pairs: every query of the given lengths against n_words words, nearest_encoded_cpu's distances (all of
    them, not only the least) against edit_distance_cpu on the same codes"""
    words = []
    for i in range(n_words):
        w = K.random_word(rng, word_len[0], word_len[1], chars if i % 3 else chars[:2])
        if foreign and i % 4 == 0 and w:
            w = w[:len(w) // 2] + 'é' + w[len(w) // 2 + 1:]
        words.append(w)
    queries = []
    for m in q_lens:
        q = K.random_word(rng, m, m, chars if m % 2 else chars[:2])
        if foreign and m > 0:
            q = 'é' + q[1:]
        queries.append(q)
    pool, offsets = LX.encode_words(words, chars, fold_case)
    codes, q_len = LX.encode_queries(queries, chars, fold_case)
    assert q_len.tolist() == list(q_lens)
    idx, dist, every = LX.nearest_encoded_cpu(codes, q_len, pool, offsets, with_distances=True)
    bad = 0
    for i in range(len(queries)):
        q = codes[i][:q_len[i]].tolist()
        want = [LX.edit_distance_cpu(q, pool[offsets[w]:offsets[w + 1]].tolist()) for w in range(n_words)]
        bad += int((np.asarray(want) != every[i]).sum())
        bad += int(dist[i] != min(want) or idx[i] != want.index(min(want)))
    return bad, len(queries) * n_words


def test_nearest_cpu_distances_equal_edit_distance_cpu():
    """more than 20 000 random and periodic pairs: query lengths 0, 1, 31, 32, 33, 63, 64 (and 2, 5, 25), word lengths 1 to
    255, case folding on and off, characters outside the alphabet on both sides"""
    rng = np.random.RandomState(1)
    q_lens = (0, 1, 2, 5, 25, 31, 32, 33, 63, 64)
    total = bad = 0
    for fold_case, foreign, n_words, word_len, chars in (
            (True, False, 400, (1, 40), DEFAULT_CHARS), (False, False, 400, (1, 40), DEFAULT_CHARS),
            (True, True, 400, (1, 40), DEFAULT_CHARS), (False, True, 300, (1, 64), 'abAB'),
            (True, False, 300, (60, 70), 'ab'), (True, False, 255, (1, 255), 'abc')):
        if word_len == (1, 255):                                   # every word length once
            words = [K.random_word(rng, n, n, chars) for n in range(1, 256)]
            queries = [K.random_word(rng, m, m, chars) for m in q_lens]
            pool, offsets = LX.encode_words(words, chars, fold_case)
            codes, q_len = LX.encode_queries(queries, chars, fold_case)
            every = LX.nearest_encoded_cpu(codes, q_len, pool, offsets, with_distances=True)[2]
            for i, q in enumerate(queries):
                want = [LX.edit_distance_cpu(q.upper(), w.upper()) for w in words]
                bad += int((np.asarray(want) != every[i]).sum())
            total += len(queries) * len(words)
            continue
        b, n = _pairs_case(rng, q_lens, n_words, chars, word_len, fold_case, foreign)
        bad, total = bad + b, total + n
    assert total >= 20000, total
    assert bad == 0, '%d of %d distances differ' % (bad, total)


def test_length_grid_holds_every_pair_and_its_closed_forms():
    g = K.length_grid_cases()
    want = K.length_grid_expected()
    assert len(K.GRID_M) == 12 and len(K.GRID_NW) == 23 and len(K.GRID_VARIANTS) == 6
    N = len(g['q_len'])
    assert N == 12 * 23 * 6 == 1656 and g['offsets'].shape == (N + 1,) and g['q_codes'].shape == (N, 64)
    assert g['pool'].dtype == np.uint8 and g['offsets'].dtype == np.int32 and g['q_len'].dtype == np.int32
    assert g['offsets'][0] == 0 and g['offsets'][-1] == g['pool'].size == 6 * 12 * sum(K.GRID_NW)
    seen = sorted(zip(g['m'].tolist(), g['n'].tolist(), g['variant'].tolist()))
    assert seen == sorted(itertools.product(K.GRID_M, K.GRID_NW, range(6)))
    assert g['q_len'].tolist() == g['m'].tolist() and np.diff(g['offsets']).tolist() == g['n'].tolist()
    m, n, v = g['m'], g['n'], g['variant']
    assert (want[v == 0] == np.abs(m - n)[v == 0]).all()                       # one repeated code
    assert (want[v == 4] == np.maximum(m, n)[v == 4]).all()                    # no common symbol
    allu = (v == 5) & ((m + n) % 2 == 0)
    assert (want[allu] == np.maximum(m, n)[allu]).all()                        # 254 against 255
    assert (g['closed'][(v == 0) | (v == 4) | allu] >= 0).all() and (g['closed'][~((v == 0) | (v == 4) | allu)] == -1).all()
    assert (want[g['closed'] >= 0] == g['closed'][g['closed'] >= 0]).all()
    # the near matches are near: at most two substitutions and the difference in length (m > 0)
    near = (v == 3) & (m > 0) & (n <= m)
    assert (want[near] <= (m - n)[near] + 2).all()
    # the unknown at the column's top bit: the query is the word's head but for its last position, which matches nothing
    top = (v == 5) & ((m + n) % 2 == 1) & (m <= n) & (m > 0)
    assert top.sum() > 50 and (want[top] == (n - m)[top] + 1).all()
    for i in np.nonzero(top)[0][:20]:
        assert g['q_codes'][i, m[i] - 1] == LX.UNKNOWN_QUERY and g['pool'][g['offsets'][i] + m[i] - 1] == LX.UNKNOWN_WORD
    assert (want >= np.abs(m - n)).all() and (want <= np.maximum(m, n)).all()
    u = K.unknown_self_cases()
    assert len(u['q_len']) == 12 * 23 * 3 and (K.pair_definition(u, 'unknown definition') == u['closed']).all()
    assert {(int(u['q_codes'][i, 0]), int(u['pool'][u['offsets'][i]])) for i in range(len(u['q_len'])) if u['m'][i] and u['n'][i]} == {
        (254, 254), (255, 255), (255, 254)}


def test_nearest_cpu_equals_the_definition_on_the_length_grid():
    """the Myers specification against the definition on every pair of the grid, word lengths 0 and 65 .. 255 included, and
    on whole queries and words of one unknown code"""
    for g, key in ((K.length_grid_cases(), 'grid definition'), (K.unknown_self_cases(), 'unknown definition')):
        N = len(g['q_len'])
        idx, dist = LX.nearest_encoded_cpu(g['q_codes'], g['q_len'], g['pool'], g['offsets'], ranges=[(w, w + 1) for w in range(N)])
        want = K.pair_definition(g, key)
        bad = np.nonzero(dist != want)[0]
        assert not bad.size, 'pair %d (m %d, n %d, variant %d): %d, the definition gives %d' % (
            bad[0], g['m'][bad[0]], g['n'][bad[0]], g['variant'][bad[0]], dist[bad[0]], want[bad[0]])
        assert idx.tolist() == list(range(N))


def test_materialise():
    pool = np.arange(10, 30, dtype=np.uint8)                           # 20 bytes
    clean = np.asarray([0, 3, 3, 9, 20], dtype=np.int32)               # words of 3, 0, 6 and 11 bytes
    p, o = K.materialise(pool, clean, 20)
    assert p.dtype == np.uint8 and o.dtype == np.int32 and p.tolist() == pool.tolist() and o.tolist() == clean.tolist()
    # a falling offset: word 1 runs from 9 to max(3, 9) = 9 and is empty, word 2 from 3 to 12
    p, o = K.materialise(pool, np.asarray([0, 9, 3, 12, 20], dtype=np.int32), 20)
    assert o.tolist() == [0, 9, 9, 18, 26] and p.tolist() == list(range(10, 19)) + list(range(13, 22)) + list(range(22, 30))
    # a negative offset starts at 0: word 1 is pool[0:9], word 0 is pool[0:max(-5, 0)] and empty
    p, o = K.materialise(pool, np.asarray([0, -5, 9, 9, 20], dtype=np.int32), 20)
    assert o.tolist() == [0, 0, 9, 9, 20] and p.tolist() == list(range(10, 19)) + list(range(19, 30))
    # overlong: offsets past pool_bytes = 12 are cut there; a start past it gives an empty word at 12
    p, o = K.materialise(pool, np.asarray([0, 3, 15, 18, 20], dtype=np.int32), 12)
    assert o.tolist() == [0, 3, 12, 12, 12] and p.tolist() == list(range(10, 22))
    # 2^31 - 1: word 1 runs to the pool's end, word 2 starts at the clamped 20 and is empty, word 3 is pool[9:20] as before
    p, o = K.materialise(pool, np.asarray([0, 3, 2 ** 31 - 1, 9, 20], dtype=np.int32), 20)
    assert o.tolist() == [0, 3, 20, 20, 31] and p.tolist() == pool.tolist() + list(range(19, 30))
    # pool_bytes 0: every word is empty
    p, o = K.materialise(pool, clean, 0)
    assert o.tolist() == [0, 0, 0, 0, 0] and p.size == 0 and p.dtype == np.uint8
    # a word of 300 is cut at 255
    long_pool = (np.arange(310) % 251).astype(np.uint8)
    p, o = K.materialise(long_pool, np.asarray([0, 5, 305, 310], dtype=np.int32), 310)
    assert o.tolist() == [0, 5, 260, 265] and p.tolist() == long_pool[:260].tolist() + long_pool[305:].tolist()
    # the specification applies to the result
    idx, dist = LX.nearest_encoded_cpu(np.zeros((1, 64), dtype=np.uint8), np.zeros(1, dtype=np.int32), *K.materialise(long_pool, np.asarray([0, 300, 310]), 310))
    assert (idx.tolist(), dist.tolist()) == ([1], [10])


def test_device_case_builders():
    """the operands of the pool-tail and damaged-table checks are what their docstrings say"""
    words, queries = K.pool_tail_case()
    assert len(words) == 40 and [len(w) for w in words[-3:]] == [15, 14, 15] and all(1 <= len(w) <= 15 for w in words)
    assert queries[:3] == [words[39], words[38], words[37]] and not set(words[39]) & set(c for w in words[:39] for c in w)
    pool, offsets, codes, q_len = K._pack_codes(words, queries)
    P = int(pool.size)
    for pb in range(P - 16, P + 1):                                    # the cut word answers its own spelling while it is not empty
        idx, dist = LX.nearest_encoded_cpu(codes, q_len, *K.materialise(pool, offsets, pb))
        k = max(15 - (P - pb), 0)
        assert dist[0] == 15 - k and (idx[0] == 39 if k else idx[0] < 39)
    pool, offsets, L, codes, q_len, cases = K.damaged_table_cases()
    assert L == 300 and offsets[101] - offsets[100] == 300 and len(cases) == 6
    with pytest.raises(ValueError):
        LX.encode_words(['x' * 300], DEFAULT_CHARS)
    for name, off, pb, ranges in cases:
        p, o = K.materialise(pool, off, pb)
        n = np.diff(o)
        assert o.size == L + 1 and n.min() >= 0 and n.max() <= 255 and o[-1] == p.size, name
    falling = cases[0][1]
    assert (np.diff(falling.astype(np.int64)) < 0).sum() > 30 and falling.min() < 0
    assert cases[1][1].max() > cases[1][2] and cases[2][1].max() == 2 ** 31 - 1 and cases[3][2] == 0


def test_case_folding_and_unknown_characters():
    # folded: 'a' and 'A' are one symbol; unfolded they differ
    assert LX.nearest_cpu(['hello'], ['HELLO'], alphabet=DEFAULT_CHARS)[1].tolist() == [0]
    assert LX.nearest_cpu(['hello'], ['HELLO'], fold_case=False, alphabet=DEFAULT_CHARS)[1].tolist() == [5]
    # a character outside the alphabet matches nothing, not even itself on the other side
    assert LX.nearest_cpu(['café'], ['café'], alphabet=DEFAULT_CHARS)[1].tolist() == [1]
    assert LX.nearest_cpu(['café'], ['café'])[1].tolist() == [0]           # no alphabet: every character is a symbol
    pool, _ = LX.encode_words(['éa'], 'ab')
    codes, q_len = LX.encode_queries(['éa'], 'ab')
    assert pool.tolist() == [LX.UNKNOWN_WORD, 0] and codes[0, :2].tolist() == [LX.UNKNOWN_QUERY, 0] and q_len.tolist() == [2]
    # first occurrence wins
    assert LX.code_table('abAc', True) == {'A': 0, 'B': 1, 'C': 2}
    assert LX.code_table('abAc', False) == {'a': 0, 'b': 1, 'A': 2, 'c': 3}


def test_ties_go_to_the_lowest_index():
    lex = ['cat', 'bat', 'cat', 'rat', 'bat', 'ca']
    idx, dist = LX.nearest_cpu(['cat', 'bat', 'hat', 'c', ''], lex)
    assert idx.tolist() == [0, 1, 0, 5, 5] and dist.tolist() == [0, 0, 1, 1, 2]
    idx, dist = LX.nearest_cpu(['cat', 'bat'], lex, ranges=[(1, 6), (2, 6)])
    assert idx.tolist() == [2, 4] and dist.tolist() == [0, 0]


def test_ranges():
    lex = ['alpha', 'beta', 'gamma', 'delta', 'epsilon', 'zeta']
    q = ['beta', 'beta', 'beta', 'beta', 'zeta', 'gamma']
    idx, dist = LX.nearest_cpu(q, lex, ranges=[(0, 6), (2, 3), (3, 3), (4, 2), (0, 3), (3, 6)])
    assert idx.tolist() == [1, 2, -1, -1, 1, 3]
    assert dist.tolist() == [0, LX.edit_distance_cpu('beta', 'gamma'), -1, -1, 1, LX.edit_distance_cpu('gamma', 'delta')]
    # adjacent per-image ranges: each query sees its own image's list only
    lists = [['alpha', 'beta'], ['gamma'], ['delta', 'epsilon', 'zeta']]
    r = LX.list_ranges(lists)
    assert r == [(0, 2), (2, 3), (3, 6)]
    idx, _ = LX.nearest_cpu(['zeta', 'zeta', 'zeta'], lex, ranges=r)
    assert idx.tolist() == [1, 2, 5]
    with pytest.raises(ValueError):
        LX.nearest_cpu(['a', 'b'], lex, ranges=[(0, 1)])
    assert LX.nearest_cpu([], lex)[0].shape == (0,)
    # an empty query: the distance is the word's length, so the shortest word wins
    assert [v.tolist() for v in LX.nearest_cpu([''], lex)] == [[1], [4]]


def test_acceptance():
    assert LX.accept(2, 10) and LX.accept(2, 10, max_dist=2) and not LX.accept(3, 10, max_dist=2)
    assert LX.accept(2, 10, max_ratio=0.2) and not LX.accept(3, 10, max_ratio=0.2)
    assert not LX.accept(1, 3, max_ratio=0.3) and LX.accept(0, 3, max_ratio=0.3)       # floor(0.9) = 0
    assert not LX.accept(2, 10, max_dist=5, max_ratio=0.1) and not LX.accept(2, 10, max_dist=1, max_ratio=0.5)
    assert not LX.accept(-1, 10)


def test_limits():
    with pytest.raises(ValueError):
        LX.encode_queries(['x' * 65], DEFAULT_CHARS)
    with pytest.raises(ValueError):
        LX.nearest_cpu(['x' * 65], ['x'])
    assert LX.encode_queries(['x' * 64], DEFAULT_CHARS)[1].tolist() == [64]
    with pytest.raises(ValueError):
        LX.encode_words(['x' * 256], DEFAULT_CHARS)
    assert LX.encode_words(['x' * 255], DEFAULT_CHARS)[1].tolist() == [0, 255]
    big = ''.join(chr(0x4e00 + i) for i in range(255))
    with pytest.raises(ValueError):
        LX.encode_words(['a'], big)
    with pytest.raises(ValueError):
        LX.code_table(big, False)
    assert len(LX.code_table(big[:254], False)) == 254


def test_packed_layout():
    pool, offsets = LX.encode_words(['ab', '', 'C!'], ' !abc', fold_case=True)
    assert pool.dtype == np.uint8 and offsets.dtype == np.int32
    assert offsets.tolist() == [0, 2, 2, 4] and pool.tolist() == [2, 3, 4, 1]
    codes, q_len = LX.encode_queries(['ba', ''], ' !abc')
    assert codes.dtype == np.uint8 and codes.shape == (2, 64) and q_len.dtype == np.int32
    assert codes[0, :3].tolist() == [3, 2, 0] and q_len.tolist() == [2, 0]
    keys = np.asarray([(3 << 32) | 7, LX.NONE_KEY, 5], dtype=np.uint64)
    idx, dist = LX.unpack_best(keys.view(np.int64))
    assert idx.tolist() == [7, -1, 5] and dist.tolist() == [3, -1, 0] and idx.dtype == np.int32


def test_entry_point_matches_the_header():
    import ctypes
    from advancedliteratemachinery_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24
    m = re.search(r'int omp_lexicon_nearest\((.*?)\);', text, re.S)
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    names = [p.split()[-1].lstrip('*') for p in params]
    assert names == ['q_codes', 'q_len', 'q_lo', 'q_hi', 'n', 'pool', 'pool_bytes', 'offsets', 'L', 'range_hint', 'best', 's']
    want = []
    for p in params:
        if '*' in p or p.startswith('omp_stream_t'):
            want.append(ctypes.c_void_p)
        elif p.startswith('int64_t'):
            want.append(ctypes.c_int64)
        else:
            assert p.startswith('int '), p
            want.append(ctypes.c_int)
    res, args = _lib._SIGS['omp_lexicon_nearest']
    assert res is ctypes.c_int and args == want
    assert 'uint64_t* best' in m.group(1) and 'const uint8_t* q_codes' in m.group(1) and 'const int32_t* offsets' in m.group(1)
    comment = text[:m.start()].rsplit('/*', 1)[1]
    assert 'test_final.py:14' in comment
    assert LX.QUERY_MAX == 64 and '[n][64]' in comment
    from advancedliteratemachinery_amd import build
    assert 'lexicon.hip' in build.SOURCES


def test_there_is_no_cpu_matcher():
    with pytest.raises(RuntimeError):
        LX.LexiconMatcher('cpu', ['word'], DEFAULT_CHARS)
    with pytest.raises(RuntimeError):
        LX.LexiconMatcher.from_lists('cpu', [['word']], DEFAULT_CHARS)


# ---------------------------------------------------------------------------------------------
# the engine's `lexicon=`
# ---------------------------------------------------------------------------------------------
def test_entry_points_take_lexicon():
    from advancedliteratemachinery_amd.engine import inference, two_stage
    for fn in (inference.predict, inference.predict_images, two_stage.spot_and_recognize):
        sig = inspect.signature(fn).parameters
        for name in ('lexicon', 'lexicon_max_dist', 'lexicon_max_ratio'):
            assert name in sig and sig[name].default is None, (fn.__name__, name)
    assert 'lexicon' not in inspect.signature(inference.validate).parameters


class StubMatcher(object):
    """LexiconMatcher without a device: nearest_cpu behind the same interface, and a log of its calls"""
    calls = []

    def __init__(self, device, words, alphabet=None, fold_case=True, chunk=65536):
        self.device, self.words, self.alphabet, self.fold_case = device, list(words), alphabet, fold_case
        self._ranges = None

    @classmethod
    def from_lists(cls, device, lists, alphabet=None, fold_case=True, chunk=65536):
        m = cls(device, [w for ws in lists for w in ws], alphabet, fold_case)
        m._ranges = LX.list_ranges(lists)
        return m

    n_lists = LX.LexiconMatcher.n_lists
    range_of = LX.LexiconMatcher.range_of

    def __call__(self, queries, ranges=None, max_dist=None, max_ratio=None):
        StubMatcher.calls.append(dict(matcher=self, queries=list(queries), ranges=ranges, max_dist=max_dist, max_ratio=max_ratio))
        idx, dist = LX.nearest_cpu(queries, self.words, ranges, self.fold_case, alphabet=self.alphabet)
        q_len = LX.encode_queries(queries, self.alphabet, self.fold_case)[1]
        return [(self.words[i] if LX.accept(d, m, max_dist, max_ratio) else None, i, d)
                for i, d, m in zip(idx.tolist(), dist.tolist(), q_len.tolist())]


RECS = [['HELLO', 'wrld'], [], ['Paris!', 'hello', 'zzzzzzzz']]


class _FakeModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


@pytest.fixture
def engine(monkeypatch):
    """predict with the device taken out: predict_raw answers one marker per image, decode_pred_seq turns the marker into
    that image's records; LexiconMatcher is the stub"""
    from advancedliteratemachinery_amd.engine import inference
    StubMatcher.calls = []
    monkeypatch.setattr(LX, 'LexiconMatcher', StubMatcher)

    def fake_raw(model, images, args, orig_sizes=None, ragged=False):
        raw = [([torch.tensor([[b]])] * 3, [torch.tensor([[0.0]])]) if RECS[b] else None for b in range(len(RECS))]
        return raw, type('NT', (), {'tensors': torch.zeros(len(RECS), 3, 8, 8)})()

    def fake_decode(seqs, probs, target, args):
        b = int(seqs[0][0])
        return [{'image_id': target['file_name'], 'pts': [[0.0, 0.0]], 'score': 1.0, 'polys': [[0.0, 0.0]] * 16, 'rec': w} for w in RECS[b]]

    monkeypatch.setattr(inference, 'predict_raw', fake_raw)
    monkeypatch.setattr(inference, 'decode_pred_seq', fake_decode)
    return inference


def test_routing_of_a_shared_list(engine):
    args = make_args()
    model = _FakeModel()
    plain = engine.predict(model, None, args)
    assert [[r['rec'] for r in recs] for recs in plain] == RECS and not StubMatcher.calls
    assert all(set(r) == {'image_id', 'pts', 'score', 'polys', 'rec'} for recs in plain for r in recs)
    words = ['hello', 'world', 'paris']
    got = engine.predict(model, None, args, lexicon=words, lexicon_max_dist=1)
    assert len(StubMatcher.calls) == 1                                 # all words of the call in ONE matcher call
    call = StubMatcher.calls[0]
    assert call['queries'] == ['HELLO', 'wrld', 'Paris!', 'hello', 'zzzzzzzz'] and call['ranges'] is None and call['max_dist'] == 1
    assert call['matcher'].alphabet == args.chars and call['matcher'].device == model.p.device
    flat = [r for recs in got for r in recs]
    assert [r['lex'] for r in flat] == ['hello', 'world', 'paris', 'hello', None]
    assert [r['lex_index'] for r in flat] == [0, 1, 2, 0, 0] and [r['lex_dist'] for r in flat] == [0, 1, 1, 0, 8]
    assert [r['rec'] for r in flat] == ['HELLO', 'wrld', 'Paris!', 'hello', 'zzzzzzzz']                  # never overwritten
    assert [[{k: v for k, v in r.items() if not k.startswith('lex')} for r in recs] for recs in got] == plain


def test_routing_of_per_image_lists(engine):
    args = make_args()
    lists = [['help', 'world'], ['unused'], ['hello', 'pairs']]
    got = engine.predict(_FakeModel(), None, args, lexicon=lists, lexicon_max_ratio=0.5)
    assert len(StubMatcher.calls) == 1
    call = StubMatcher.calls[0]
    assert call['ranges'] == [(0, 2), (0, 2), (3, 5), (3, 5), (3, 5)] and call['max_ratio'] == 0.5 and call['max_dist'] is None
    flat = [r for recs in got for r in recs]
    assert [r['lex'] for r in flat] == ['help', 'world', 'pairs', 'hello', None]
    assert [r['lex_index'] for r in flat] == [0, 1, 1, 0, 0]          # the index in the image's OWN list
    assert [r['lex_dist'] for r in flat] == [2, 1, 3, 0, 8]             # 'zzzzzzzz' shares nothing with 5 letters: 5 + 3
    with pytest.raises(ValueError):
        engine.predict(_FakeModel(), None, args, lexicon=[['a'], ['b']])            # two lists, three images
    with pytest.raises(ValueError):
        engine.predict(_FakeModel(), None, args, lexicon=['a', ['b'], 'c'])


def test_routing_of_a_prebuilt_matcher(engine):
    args = make_args()
    m = StubMatcher('anywhere', ['hello', 'world'], 'helowrd')
    got = engine.predict(_FakeModel(), None, args, lexicon=m)
    assert len(StubMatcher.calls) == 1 and StubMatcher.calls[0]['matcher'] is m
    assert [r['lex'] for recs in got for r in recs] == ['hello', 'world', 'world', 'hello', 'hello']     # no threshold: always the nearest ('Paris!' shares its R with 'world')
    per = StubMatcher.from_lists('anywhere', [['hello'], ['x'], ['world']], DEFAULT_CHARS)
    got = engine.predict(_FakeModel(), None, args, lexicon=per)
    assert StubMatcher.calls[1]['ranges'] == [(0, 1), (0, 1), (2, 3), (2, 3), (2, 3)]
    assert [r['lex_index'] for recs in got for r in recs] == [0] * 5


def test_predict_images_and_two_stage_pass_the_lexicon_on(engine, monkeypatch):
    from advancedliteratemachinery_amd.engine import two_stage
    from advancedliteratemachinery_amd.model.mgp_str import CHARACTER
    args = make_args()

    class FakePre(object):
        def __call__(self, imgs):
            return torch.zeros(len(imgs), 3, 8, 8), None

    images = [torch.zeros(8, 8, 3, dtype=torch.uint8)] * 3
    got, _ = engine.predict_images(_FakeModel(), images, args, preprocessor=FakePre(), lexicon=['hello'], lexicon_max_dist=0)
    assert len(StubMatcher.calls) == 1
    assert [r['lex'] for recs in got for r in recs] == ['hello', None, None, 'hello', None]

    StubMatcher.calls = []
    reads = iter(['hell0', 'w0rld', 'par1s', 'hello', 'zzz'])

    def fake_recognize(mgp_model, imgs, boxes, resizer=None, chunk=512, polys=None):
        return [dict(char_text=next(reads), conf=[1.0, 0.0, 0.0], choice=0, char_ids=[], bpe_ids=[], wp_ids=[]) for _ in boxes], resizer

    monkeypatch.setattr(two_stage, 'recognize_crops', fake_recognize)
    got, _, _ = two_stage.spot_and_recognize(_FakeModel(), None, images, args, preprocessor=FakePre(),
                                             lexicon=(w for w in ['hello', 'world', 'paris']), lexicon_max_dist=1)
    assert len(StubMatcher.calls) == 2                                 # one matcher call per source string per engine call
    assert StubMatcher.calls[0]['queries'] == ['HELLO', 'wrld', 'Paris!', 'hello', 'zzzzzzzz']
    assert StubMatcher.calls[1]['queries'] == ['hell0', 'w0rld', 'par1s', 'hello', 'zzz']
    assert StubMatcher.calls[0]['matcher'].alphabet == args.chars and StubMatcher.calls[1]['matcher'].alphabet == CHARACTER
    flat = [r for recs in got for r in recs]
    assert [r['mgp_lex'] for r in flat] == ['hello', 'world', 'paris', 'hello', None]
    assert [r['mgp_lex_dist'] for r in flat] == [1, 1, 1, 0, 5] and [r['mgp_lex_index'] for r in flat] == [0, 1, 2, 0, 0]
    assert [r['lex'] for r in flat] == ['hello', 'world', 'paris', 'hello', None]
    assert [r['mgp_text'] for r in flat] == ['hell0', 'w0rld', 'par1s', 'hello', 'zzz']

    # without a lexicon: today's keys, and no matcher
    StubMatcher.calls = []
    reads = iter(['a'] * 5)
    got, _, _ = two_stage.spot_and_recognize(_FakeModel(), None, images, args, preprocessor=FakePre())
    assert not StubMatcher.calls
    assert all(set(r) == {'image_id', 'pts', 'score', 'polys', 'rec', 'box', 'mgp_text', 'mgp_conf', 'mgp_choice', 'mgp_ids'}
               for recs in got for r in recs)


def test_kie_refuses_a_lexicon(engine):
    from advancedliteratemachinery_amd.engine import two_stage
    args = make_args()
    args.infer_vie = True
    for call in (lambda: engine.predict(_FakeModel(), None, args, lexicon=['a']),
                 lambda: engine.predict_images(_FakeModel(), [], args, lexicon=['a']),
                 lambda: two_stage.spot_and_recognize(_FakeModel(), None, [], args, lexicon=['a'])):
        with pytest.raises(ValueError, match='infer_vie'):
            call()
    assert not StubMatcher.calls
