"""Posterior lexicon decoding, CPU side: the costs, the class table, the numpy specification against the
pure-Python definition, the greedy path against the reference's confidence, the acceptance rule, the entry points' arguments against
the header, and the routing of lexicon_mode='posterior' through spot_and_recognize with stub matchers."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from advancedliteratemachinery_amd.utils import lexicon as LX
from advancedliteratemachinery_amd.utils import lexicon_post as LP
from advancedliteratemachinery_amd.utils.parser import DEFAULT_CHARS, make_args
from tests import gpu_checks_lexicon_post as K
from tests.gpu_checks_lexicon import MGP_CHARS, image_ranges, random_ranges, random_word
from tests.test_lexicon_host import RECS, StubMatcher, _FakeModel, engine  # noqa: F401  (engine is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = np.uint64(LX.NONE_KEY)


# ---------------------------------------------------------------------------------------------
# costs
# ---------------------------------------------------------------------------------------------
def test_costs_worked_rows():
    x = K.worked_logits()
    c = LP.costs_cpu(x)
    assert c.shape == (2, 26, 38) and c.dtype == np.int32                # position 0 is dropped
    assert (c[0] == 3725).all() and 3725 == math.floor(math.log(38) * 1024 + 0.5)
    for p in range(26):                                                  # cost row p is logits position p + 1
        peak = (p + 1) % 38
        assert c[1, p, peak] == 0 and (np.delete(c[1, p], peak) == 20480).all()
    assert LP.COST_CAP == 2 ** 20 - 1 and 26 * LP.COST_CAP < 2 ** 31


def test_costs_cap_and_shape():
    x = np.zeros((3, 27, 38), dtype=np.float32)
    x[1, 7] = np.linspace(-1e4, 1e4, 38)
    x[2, 0] = 1e9                                                        # position 0 never reaches the costs
    c = LP.costs_cpu(x)
    assert c[1, 6, 0] == LP.COST_CAP and c[1, 6, 37] == 0 and c.min() >= 0 and c.max() == LP.COST_CAP
    assert (c[2] == 3725).all()
    for shape in ((2, 26, 38), (2, 27, 37), (27, 38)):
        with pytest.raises(ValueError):
            LP.costs_cpu(np.zeros(shape, dtype=np.float32))
    # float64 from the fp32 logits: a float64 input is rounded to fp32 first
    y = np.random.RandomState(0).randn(4, 27, 38) * 8
    assert (LP.costs_cpu(y) == LP.costs_cpu(y.astype(np.float32))).all()


# ---------------------------------------------------------------------------------------------
# classes
# ---------------------------------------------------------------------------------------------
def test_class_table():
    from advancedliteratemachinery_amd.model.mgp_str import CHAR_TABLE, CHARACTER
    assert CHARACTER == MGP_CHARS and CHAR_TABLE[1] == '[s]' and LP.EOS_CLASS == 1 and len(CHAR_TABLE) == LP.CLASSES
    t = LP.class_table(CHARACTER, True)
    assert t.dtype == np.uint8 and t.shape == (256,)
    assert t[:36].tolist() == list(range(2, 38)) and (t[36:] == 255).all()
    for fold in (True, False):
        t = LP.class_table(DEFAULT_CHARS, fold)
        codes = LX.code_table(DEFAULT_CHARS, fold)
        assert t[254] == 255 and t[255] == 255
        seen = 0
        for ch, code in codes.items():
            low = ch.lower() if fold else ch
            if low in CHARACTER and len(low) == 1:
                assert CHAR_TABLE[t[code]] == low
                seen += 1
            else:
                assert t[code] == 255, ch                                # punctuation, space; upper case when unfolded
        assert seen == 36
        assert t[codes[' ']] == 255 and t[codes['!']] == 255
        assert (t[len(codes):] == 255).all()
    assert LP.class_table(DEFAULT_CHARS, False)[LX.code_table(DEFAULT_CHARS, False)['A']] == 255
    assert LP.class_table(DEFAULT_CHARS, True)[LX.code_table(DEFAULT_CHARS, True)['A']] == 2 + CHARACTER.index('a')
    t = LP.class_table('zyx-90', True)                                   # an alphabet in another order
    assert t[:6].tolist() == [37, 36, 35, 255, 11, 2] and (t[6:] == 255).all()
    assert LP.class_table('ab', True, characters='ba')[:2].tolist() == [3, 2]


# ---------------------------------------------------------------------------------------------
# the search: numpy specification against the pure-Python definition
# ---------------------------------------------------------------------------------------------
def test_word_score_definition():
    c = np.arange(26 * 38, dtype=np.int64).reshape(26, 38).tolist()
    t = LP.class_table(MGP_CHARS, True)
    assert LP.word_score_py(c, [], t) == c[0][1]                          # the empty word: [s] at position 0
    assert LP.word_score_py(c, [0], t) == c[0][2] + c[1][1]
    assert LP.word_score_py(c, [10, 11], t) == c[0][12] + c[1][13] + c[2][1]
    assert LP.word_score_py(c, [0] * 25, t) == sum(c[i][2] for i in range(25)) + c[25][1]
    assert LP.word_score_py(c, [0] * 26, t) is None                       # skipped, not truncated
    assert LP.word_score_py(c, [0, 255, 1], t) is None and LP.word_score_py(c, [254], t) is None and LP.word_score_py(c, [36], t) is None


@pytest.mark.parametrize('L', [1, 2, 40, 300])
def test_score_cpu_equals_the_definition(L):
    alphabet = MGP_CHARS + '-_'
    words = K.post_lexicon(L - 1, seed=L, alphabet=alphabet) if L > 1 else ['one']
    assert len(words) == L
    if L >= 40:
        assert {0, 1, 25, 26, 255} <= {len(w) for w in words} and len(set(words)) < L and any('-' in w or '_' in w for w in words)
    pool, offsets, table = K.encode(words, alphabet)
    N = 24
    costs = K.random_costs(N, seed=L)
    rng = np.random.RandomState(L)
    for ranges in (None, random_ranges(rng, N, L), image_ranges(N, 3, L)[0] if L >= 40 else [(0, L)] * N,
                   [(-5, L + 9), (L, 0), (3, 3), (L - 1, L)] * (N // 4)):
        want = LP.score_py(costs, pool, offsets, table, ranges)
        got = LP.score_cpu(costs, pool, offsets, table, ranges)
        assert got.dtype == np.uint64 and got.shape == (N, 2)
        assert (got == want).all()
    whole = LP.score_cpu(costs, pool, offsets, table)
    if L == 1:
        assert (whole[:, 1] == NONE).all() and (whole[:, 0] != NONE).all()        # no runner-up
    clamped = LP.score_cpu(costs, pool, offsets, table, [(-5, L + 9)] * N)
    assert (clamped == whole).all()
    inverted = LP.score_cpu(costs, pool, offsets, table, [(L, 0)] * N)
    assert (inverted == NONE).all()


def test_duplicates_ties_and_runner_up():
    words = ['clean', 'ocean', 'clean', 'c1ean', 'clean']
    pool, offsets, table = K.encode(words)
    x = np.zeros((1, 27, 38), dtype=np.float32)
    for i, ch in enumerate('c1ean'):
        x[0, 1 + i, 2 + MGP_CHARS.index(ch)] = 9.0
    x[0, 2, 2 + MGP_CHARS.index('l')] = 7.0                              # the posterior at position 2 says which the model meant
    x[0, 6:, 1] = 9.0
    costs = LP.costs_cpu(x)
    idx, score = LP.unpack_post(LP.score_cpu(costs, pool, offsets, table, [(0, 3)]))
    assert idx.tolist() == [[0, 2]] and score[0, 0] == score[0, 1]        # best = the lower index, runner-up = the other, equal score
    idx, score = LP.unpack_post(LP.score_cpu(costs, pool, offsets, table, [(0, 2)]))
    assert idx.tolist() == [[0, 1]] and score[0, 0] < score[0, 1]         # 'clean' before 'ocean'
    assert LX.nearest_cpu(['c1ean'], words[:2], alphabet=MGP_CHARS)[1].tolist() == [1]
    idx, score = LP.unpack_post(LP.score_cpu(costs, pool, offsets, table))
    assert idx.tolist() == [[3, 0]] and LP.greedy_cpu(costs)[0].tolist() == [int(score[0, 0]), 5]
    assert (LP.score_cpu(costs, pool, offsets, table) == LP.score_py(costs, pool, offsets, table)).all()


def test_unscorable_ranges_and_capped_costs():
    alphabet = MGP_CHARS + '-'
    words = ['a-b', '--', 'x' * 26, '-', 'fine', 'y' * 255]
    pool, offsets, table = K.encode(words, alphabet)
    costs = K.random_costs(3, seed=1)
    got = LP.score_cpu(costs, pool, offsets, table, [(0, 4), (0, 5), (5, 6)])
    assert (got[0] == NONE).all() and (got[2] == NONE).all()             # all-unscorable ranges
    assert int(got[1, 0]) & 0xffffffff == 4 and got[1, 1] == NONE
    assert (got == LP.score_py(costs, pool, offsets, table, [(0, 4), (0, 5), (5, 6)])).all()
    words = K.post_lexicon(60, seed=2)
    pool, offsets, table = K.encode(words)
    cap = np.full((2, 26, 38), LP.COST_CAP, dtype=np.int32)
    got = LP.score_cpu(cap, pool, offsets, table)
    assert (got == LP.score_py(cap, pool, offsets, table)).all()
    idx, score = LP.unpack_post(got)
    assert idx[0, 0] == 0 and score[0, 0] == LP.COST_CAP                 # the empty word: one term
    assert 26 * LP.COST_CAP == max(LP.word_score_py(cap[0].tolist(), [0] * 25, table), 0)


def test_damaged_offsets_have_a_defined_answer():
    words = K.post_lexicon(80, seed=4)
    pool, offsets, table = K.encode(words)
    costs = K.random_costs(4, seed=4)
    bad = offsets.copy()
    bad[10:30] = bad[10:30][::-1]
    bad[40] = -9
    bad[60:] += 100000
    for pb in (None, 0, 17):
        got = LP.score_cpu(costs, pool, bad, table, pool_bytes=pb)
        assert (got == LP.score_py(costs, pool, bad, table, pool_bytes=pb)).all()
    empty = LP.score_cpu(costs, pool, offsets, table, pool_bytes=0)
    assert [int(v) for v in empty[:, 0]] == [int(costs[q, 0, 1]) << 32 for q in range(4)]


# ---------------------------------------------------------------------------------------------
# the greedy path
# ---------------------------------------------------------------------------------------------
def test_greedy_cpu():
    c = np.full((5, 26, 38), 5000, dtype=np.int32)
    c[:, :, 7] = 10                                                      # a character wins everywhere ...
    c[0, 0, 1] = 3                                                       # ... but [s] at position 0
    c[1, 25, 1] = 4                                                      # [s] at position 25
    c[3, 4, 1] = 10                                                      # a tie between [s] and a character: [s] wins, the lower class
    c[4, 4, 0] = 10                                                      # a tie between [GO] and a character: [GO] wins and is no [s]
    c[4, 6, 1] = 0
    g = LP.greedy_cpu(c)
    assert g.dtype == np.int32 and g.tolist() == [[3, 0], [25 * 10 + 4, 25], [26 * 10, 26], [4 * 10 + 10, 4], [6 * 10 + 0, 6]]
    assert 'negative' in LP.__doc__ and 'negative' in LP.result_keys.__doc__


def test_greedy_cost_against_the_reference_confidence():
    """planted logits whose [GO] class can never win: decode_ids' conf[0] (fp32 max-softmax probabilities, cumprod to the first
    [s]) and greedy_cost agree within half a unit of rounding per term plus one unit for the fp32 product"""
    from advancedliteratemachinery_amd.model.mgp_str import decode_ids
    rng = np.random.RandomState(7)
    B = 64
    x = (rng.randn(B, 27, 38) * 3).astype(np.float32)
    x[:, :, 0] = -40.0
    x[:, :, 1] -= 25.0
    ends = rng.randint(0, 26, B)
    ends[:3] = (0, 25, 12)
    for b in range(B):
        x[b, 1 + ends[b], 1] = 15.0
    t = torch.from_numpy(x)
    prob, ids = torch.softmax(t, dim=2).max(dim=2)
    ids3 = [ids[:, 1:].int(), torch.zeros(B, 26, dtype=torch.int32), torch.zeros(B, 26, dtype=torch.int32)]
    probs3 = [prob[:, 1:], torch.zeros(B, 26), torch.zeros(B, 26)]
    res = decode_ids(ids3, probs3)
    g = LP.greedy_cpu(LP.costs_cpu(x))
    for b in range(B):
        cost, n = g[b].tolist()
        assert n == ends[b] and len(res[b]['char_text']) == n
        assert abs(cost + 1024 * math.log(res[b]['conf'][0])) <= 0.5 * (n + 1) + 1, (b, cost, res[b]['conf'][0])


def test_peaked_logits_choose_the_greedy_string():
    """the greedy string is in the lexicon and every position's margin exceeds the quantisation: the posterior choice is that string
    with gap 0, and nearest_cpu returns the same index with distance 0"""
    rng = np.random.RandomState(9)
    words = sorted({random_word(rng, 1, 25, MGP_CHARS) for _ in range(200)} | {'a' * 25})
    picks = [int(i) for i in rng.randint(0, len(words), 30)] + [words.index('a' * 25)]
    x = rng.randn(len(picks), 27, 38).astype(np.float32)
    for q, i in enumerate(picks):
        for k, ch in enumerate(words[i]):
            x[q, 1 + k, 2 + MGP_CHARS.index(ch)] += 14.0
        x[q, 1 + len(words[i]):, 1] += 14.0
    pool, offsets, table = K.encode(words)
    costs = LP.costs_cpu(x)
    idx, score = LP.unpack_post(LP.score_cpu(costs, pool, offsets, table))
    g = LP.greedy_cpu(costs)
    assert idx[:, 0].tolist() == picks and (score[:, 0] == g[:, 0]).all() and g[:, 1].tolist() == [len(words[i]) for i in picks]
    reads = [''.join(MGP_CHARS[c - 2] for c in costs[q, :g[q, 1]].argmin(axis=1)) for q in range(len(picks))]
    ni, nd = LX.nearest_cpu(reads, words, alphabet=MGP_CHARS)
    assert ni.tolist() == picks and (nd == 0).all()
    d = LP.describe(LP.score_cpu(costs, pool, offsets, table), g, words)
    keys = LP.result_keys(d[0], 'lex')
    assert keys['lex'] == words[picks[0]] and keys['lex_gap'] == 0.0 and keys['lex_index'] == picks[0] and keys['lex_logp'] <= 0.0


def test_the_gap_may_be_negative():
    c = np.full((1, 26, 38), 4000, dtype=np.int32)
    c[0, :6, 5] = 700                                                    # six mediocre characters, then [s] ...
    c[0, 6, 1] = 0
    c[0, 1, 1] = 800                                                     # ... and a fair [s] at position 1
    pool, offsets, table = K.encode(['3', '333333'])
    idx, score = LP.unpack_post(LP.score_cpu(c, pool, offsets, table))
    g = LP.greedy_cpu(c)
    assert g.tolist() == [[4200, 6]] and idx.tolist() == [[0, 1]] and score.tolist() == [[1500, 4200]]
    keys = LP.result_keys(LP.describe(LP.score_cpu(c, pool, offsets, table), g, ['3', '333333'])[0], 'mgp_lex', base=0)
    assert keys['mgp_lex'] == '3' and keys['mgp_lex_gap'] == (1500 - 4200) / 1024.0 and keys['mgp_lex_second'] == (1, -4200 / 1024.0)


# ---------------------------------------------------------------------------------------------
# acceptance
# ---------------------------------------------------------------------------------------------
def test_accept_post_boundaries():
    a = LP.accept_post
    assert a(0, None) and a(10 ** 6, 5) and not a(None, None) and not a(-1, None)
    limit = int(math.floor(-math.log(0.5) * 1024))                       # 709
    assert limit == 709
    assert a(709, None, min_prob=0.5) and not a(710, None, min_prob=0.5) and a(0, None, min_prob=1.0) and not a(1, None, min_prob=1.0)
    need = int(math.ceil(0.25 * 1024))                                   # 256
    assert a(100, 356, min_margin=0.25) and not a(100, 355, min_margin=0.25)
    assert a(100, None, min_margin=0.25) and a(100, -1, min_margin=0.25) and need == 256   # no runner-up: the margin does not apply
    assert not a(100, 100, min_margin=0.001) and a(100, 100, min_margin=0.0)
    assert not a(710, 5000, min_prob=0.5, min_margin=0.25) and a(709, 965, min_prob=0.5, min_margin=0.25)
    for bad in (dict(min_prob=0.0), dict(min_prob=1.5), dict(min_prob=-1), dict(min_margin=-0.1), dict(min_margin=float('nan'))):
        with pytest.raises(ValueError):
            LP.check_post_args(bad.get('min_prob'), bad.get('min_margin'))
    LP.check_post_args(None, None)
    LP.check_post_args(1.0, 0.0)


# ---------------------------------------------------------------------------------------------
# the entry points against the header
# ---------------------------------------------------------------------------------------------
def test_header_and_sigs():
    from advancedliteratemachinery_amd import _lib, build, ops
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24
    names = {'omp_logprob_costs': ['logits', 'n', 'costs', 'greedy', 's'],
             'omp_lexicon_posterior': ['costs', 'n', 'q_lo', 'q_hi', 'pool', 'pool_bytes', 'offsets', 'L', 'class_table', 'range_hint', 'best', 'work', 's']}
    for fn, want_names in names.items():
        m = re.search(r'int %s\((.*?)\);' % fn, text, re.S)
        params = [' '.join(p.split()) for p in m.group(1).split(',')]
        assert [p.split()[-1].lstrip('*') for p in params] == want_names
        want = []
        for p in params:
            if '*' in p or p.startswith('omp_stream_t'):
                want.append(ctypes.c_void_p)
            elif p.startswith('int64_t'):
                want.append(ctypes.c_int64)
            else:
                assert p.startswith('int '), p
                want.append(ctypes.c_int)
        res, args = _lib._SIGS[fn]
        assert res is ctypes.c_int and args == want
    comment = text[:text.index('int omp_logprob_costs(')].rsplit('/* ----', 1)[1]
    assert 'test_final.py:172-181' in comment and '[n][27][38]' in comment and '[n][26][38]' in comment
    comment = text[text.index('int omp_logprob_costs('):text.index('int omp_lexicon_posterior(')]
    assert 'uint64 [n][2]' in comment and '2 * (n + %d)' % ops.LEXICON_POST_WORK_SLICES in comment and 'OMP_ERR_INVALID' in comment
    assert ops.LEXICON_POST_WORK_SLICES == LP.WORK_SLICES
    assert 'lexicon_post.hip' in build.SOURCES and 'lexicon_post.hip' not in build.AUDITED
    assert callable(ops.logprob_costs) and callable(ops.lexicon_posterior)
    src = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'lexicon_post.hip')).read()
    assert 'LXP_SLICES = %d' % LP.WORK_SLICES in src and 'atomic' not in src.split('#include')[1]


def test_there_is_no_cpu_posterior_matcher():
    m = StubMatcher('cpu', ['word'], MGP_CHARS)
    m.chunk = 10
    with pytest.raises(RuntimeError, match='MI355X'):
        LP.PosteriorMatcher(m)
    with pytest.raises(RuntimeError):
        LP.posterior_of(m)


# ---------------------------------------------------------------------------------------------
# the engine's lexicon_mode=
# ---------------------------------------------------------------------------------------------
def test_entry_points_take_the_new_arguments():
    from advancedliteratemachinery_amd.engine import two_stage
    from advancedliteratemachinery_amd.model.mgp_str import MGPSTR
    sig = inspect.signature(two_stage.spot_and_recognize).parameters
    assert sig['lexicon_mode'].default == 'edit' and sig['lexicon_min_prob'].default is None and sig['lexicon_min_margin'].default is None
    assert inspect.signature(two_stage.recognize_crops).parameters['keep_logits'].default is False
    assert inspect.signature(MGPSTR.greedy).parameters['char_logits'].default is False
    sig = inspect.signature(MGPSTR.recognize).parameters
    for name in ('lexicon', 'lexicon_ranges', 'lexicon_min_prob', 'lexicon_min_margin'):
        assert sig[name].default is None
    assert list(sig)[:4] == ['self', 'input', 'bpe_vocab', 'wp_vocab']


class StubPosterior(object):
    """PosteriorMatcher without a device: costs_cpu / score_cpu / greedy_cpu behind the same interface, and a log of its calls"""
    calls = []

    def __init__(self, matcher, characters=None):
        self.matcher, self.words = matcher, matcher.words
        self.table_host = LP.class_table(matcher.alphabet, matcher.fold_case, characters)

    def __call__(self, logits, ranges=None, min_prob=None, min_margin=None):
        StubPosterior.calls.append(dict(post=self, n=int(logits.shape[0]), ranges=ranges, min_prob=min_prob, min_margin=min_margin))
        costs = LP.costs_cpu(logits.numpy())
        pool, offsets = LX.encode_words(self.words, self.matcher.alphabet, self.matcher.fold_case)
        return LP.describe(LP.score_cpu(costs, pool, offsets, self.table_host, ranges), LP.greedy_cpu(costs), self.words, min_prob, min_margin)


READS = ['hell0', 'w0rld', 'par1s', 'hello', 'zzz']
ALT = {'0': 'o', '1': 'i'}


def _planted(reads):
    """logits peaked on each read (+8), with the look-alike letter of a digit close behind (+6)"""
    x = np.zeros((len(reads), 27, 38), dtype=np.float32)
    for q, w in enumerate(reads):
        for k, ch in enumerate(w):
            x[q, 1 + k, 2 + MGP_CHARS.index(ch)] = 8.0
            if ch in ALT:
                x[q, 1 + k, 2 + MGP_CHARS.index(ALT[ch])] = 6.0
        x[q, 1 + len(w):, 1] = 8.0
    return torch.from_numpy(x)


@pytest.fixture
def two_stage(engine, monkeypatch):  # noqa: F811
    from advancedliteratemachinery_amd.engine import two_stage as TS
    StubPosterior.calls = []
    monkeypatch.setattr(LP, 'PosteriorMatcher', StubPosterior)
    seen = []

    def fake_recognize(mgp_model, imgs, boxes, resizer=None, chunk=512, polys=None, **kw):
        seen.append(kw)
        res = [dict(char_text=t, conf=[1.0, 0.0, 0.0], choice=0, char_ids=[], bpe_ids=[], wp_ids=[]) for t in READS[:len(boxes)]]
        return (res, resizer, _planted(READS[:len(boxes)])) if kw.get('keep_logits') else (res, resizer)

    monkeypatch.setattr(TS, 'recognize_crops', fake_recognize)
    TS.seen = seen
    return TS


class FakePre(object):
    def __call__(self, imgs):
        return torch.zeros(len(imgs), 3, 8, 8), None


IMAGES = [torch.zeros(8, 8, 3, dtype=torch.uint8)] * 3
BASE_KEYS = {'image_id', 'pts', 'score', 'polys', 'rec', 'box', 'mgp_text', 'mgp_conf', 'mgp_choice', 'mgp_ids'}
POST_KEYS = {'mgp_lex', 'mgp_lex_index', 'mgp_lex_logp', 'mgp_lex_second', 'mgp_lex_gap'}


def test_defaults_leave_the_key_sets_unchanged(two_stage):
    args = make_args()
    got, _, _ = two_stage.spot_and_recognize(_FakeModel(), None, IMAGES, args, preprocessor=FakePre())
    assert not StubMatcher.calls and not StubPosterior.calls and two_stage.seen == [{}]       # recognize_crops is called as before
    assert all(set(r) == BASE_KEYS for recs in got for r in recs)
    got, _, _ = two_stage.spot_and_recognize(_FakeModel(), None, IMAGES, args, preprocessor=FakePre(), lexicon=['hello', 'world', 'paris'], lexicon_max_dist=1)
    assert len(StubMatcher.calls) == 2 and not StubPosterior.calls and two_stage.seen[1] == {}
    assert all(set(r) == BASE_KEYS | {'lex', 'lex_index', 'lex_dist', 'mgp_lex', 'mgp_lex_index', 'mgp_lex_dist'} for recs in got for r in recs)


def test_posterior_makes_one_call_for_all_words(two_stage):
    from advancedliteratemachinery_amd.model.mgp_str import CHARACTER
    args = make_args()
    words = ['hello', 'world', 'paris']
    got, _, _ = two_stage.spot_and_recognize(_FakeModel(), None, IMAGES, args, preprocessor=FakePre(), lexicon=(w for w in words), lexicon_max_dist=1,
                                             lexicon_mode='posterior', lexicon_min_prob=1e-4, lexicon_min_margin=1.0)
    assert two_stage.seen == [{'keep_logits': True}]
    assert len(StubPosterior.calls) == 1 and len(StubMatcher.calls) == 1          # one posterior call for all words; `rec` keeps its edit-distance call
    call = StubPosterior.calls[0]
    assert call['n'] == 5 and call['ranges'] is None and call['min_prob'] == 1e-4 and call['min_margin'] == 1.0
    assert call['post'].matcher.alphabet == CHARACTER and StubMatcher.calls[0]['matcher'].alphabet == args.chars
    flat = [r for recs in got for r in recs]
    assert all(set(r) == BASE_KEYS | {'lex', 'lex_index', 'lex_dist'} | POST_KEYS for r in flat)       # no mgp_lex_dist
    assert [r['mgp_lex'] for r in flat] == ['hello', 'world', 'paris', 'hello', None]
    assert [r['mgp_lex_index'] for r in flat] == [0, 1, 2, 0, flat[4]['mgp_lex_index']] and flat[4]['mgp_lex_logp'] < math.log(1e-4)
    assert [r['lex'] for r in flat] == ['hello', 'world', 'paris', 'hello', None] and [r['lex_dist'] for r in flat] == [0, 1, 1, 0, 8]
    assert [r['mgp_text'] for r in flat] == READS
    for r in flat[:4]:
        assert r['mgp_lex_logp'] <= 0 and r['mgp_lex_second'][0] != r['mgp_lex_index'] and r['mgp_lex_second'][1] < r['mgp_lex_logp'] - 1.0
    assert flat[3]['mgp_lex_gap'] == 0.0 and abs(flat[0]['mgp_lex_gap'] - 2.0) < 0.01   # the 'o' lies 2 nats behind the '0'


def test_posterior_with_per_image_lists_and_a_prebuilt_matcher(two_stage):
    args = make_args()
    lists = [['help', 'hello', 'world'], ['unused'], ['pairs', 'paris', 'hello', 'hello']]
    got, _, _ = two_stage.spot_and_recognize(_FakeModel(), None, IMAGES, args, preprocessor=FakePre(), lexicon=lists, lexicon_mode='posterior')
    assert len(StubPosterior.calls) == 1
    assert StubPosterior.calls[0]['ranges'] == [(0, 3), (0, 3), (4, 8), (4, 8), (4, 8)]
    flat = [r for recs in got for r in recs]
    assert [r['mgp_lex'] for r in flat[:4]] == ['hello', 'world', 'paris', 'hello']
    assert [r['mgp_lex_index'] for r in flat[:4]] == [1, 2, 1, 2]                  # the index in the image's OWN list
    assert flat[3]['mgp_lex_second'] == (3, flat[3]['mgp_lex_logp'])                # the duplicate spelling is the runner-up, at its own-list index
    m = StubMatcher('anywhere', ['world', 'hello'], MGP_CHARS)
    two_stage.spot_and_recognize(_FakeModel(), None, IMAGES, args, preprocessor=FakePre(), lexicon=m, lexicon_mode='posterior')
    two_stage.spot_and_recognize(_FakeModel(), None, IMAGES, args, preprocessor=FakePre(), lexicon=m, lexicon_mode='posterior')
    assert len(StubPosterior.calls) == 3 and StubPosterior.calls[1]['post'] is StubPosterior.calls[2]['post'] is m._posterior   # built once, cached on it
    with pytest.raises(ValueError):
        two_stage.spot_and_recognize(_FakeModel(), None, IMAGES, args, preprocessor=FakePre(), lexicon=[['a'], ['b']], lexicon_mode='posterior')


def test_every_refusal_is_raised_ahead_of_any_work(two_stage):
    args = make_args()
    run = lambda **kw: two_stage.spot_and_recognize(_FakeModel(), None, IMAGES, args, preprocessor=None, **kw)   # noqa: E731  (no preprocessor: any work would fail differently)
    for kw, match in ((dict(lexicon=['a'], lexicon_mode='nearest'), 'lexicon_mode'), (dict(lexicon_mode=None), 'lexicon_mode'),
                      (dict(lexicon=['a'], lexicon_min_prob=0.5), 'posterior'), (dict(lexicon=['a'], lexicon_mode='edit', lexicon_min_margin=0.5), 'posterior'),
                      (dict(lexicon_min_margin=0.5), 'posterior'), (dict(lexicon_mode='posterior'), 'lexicon='),
                      (dict(lexicon=['a'], lexicon_mode='posterior', lexicon_min_prob=0.0), 'lexicon_min_prob'),
                      (dict(lexicon=['a'], lexicon_mode='posterior', lexicon_min_margin=-1.0), 'lexicon_min_margin')):
        with pytest.raises(ValueError, match=match):
            run(**kw)
    vie = make_args()
    vie.infer_vie = True
    for kw in (dict(lexicon=['a'], lexicon_mode='posterior'), dict(lexicon_mode='posterior')):
        with pytest.raises(ValueError, match='infer_vie'):
            two_stage.spot_and_recognize(_FakeModel(), None, [], vie, **kw)
    assert not StubMatcher.calls and not StubPosterior.calls and not two_stage.seen
