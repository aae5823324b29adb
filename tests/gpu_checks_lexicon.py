"""Lexicon correction: the case builders shared by the CPU tests (tests/test_lexicon_host.py) and
the GPU checks of omp_lexicon_nearest / LexiconMatcher / the engine's `lexicon=` against utils/lexicon.py: nearest_cpu.
Everything is integer on both sides, so every comparison is equality.  Same record format as tests/gpu_checks.py; the GPU
modules are imported inside the checks so that the builders stay usable without a device.

The length grid (length_grid_cases: 12 query lengths x 23 word lengths x 6 variants = 1656 pairs, a pool of 144 000 bytes) is
held to the DEFINITION, edit_distance_cpu: 3.74 M table cells in plain Python, measured at 0.7 s on the CPU host (1.2 s with
the 828 pairs of unknown_self_cases), so the inner loop stayed as it is; nearest_encoded_cpu on the 1656 single-word ranges takes
2 s there, on the grid's 182 distinct queries against the whole grid 1 s.  Grid, definition and the other operands are built
once per process and shared by the CPU tests and the GPU checks."""
import numpy as np

from advancedliteratemachinery_amd.utils import lexicon as LX
from advancedliteratemachinery_amd.utils.parser import DEFAULT_CHARS

MGP_CHARS = '0123456789abcdefghijklmnopqrstuvwxyz'


# ---------------------------------------------------------------------------------------------
# case builders (numpy only)
# ---------------------------------------------------------------------------------------------
def random_word(rng, lo, hi, chars=DEFAULT_CHARS):
    return ''.join(chars[i] for i in rng.randint(0, len(chars), int(rng.randint(lo, hi + 1))))


def edit(rng, word, n, chars=DEFAULT_CHARS):
    """`word` under n random edits (insert / delete / substitute)"""
    w = list(word)
    for _ in range(n):
        op = int(rng.randint(0, 3))
        if op == 0 or not w:
            w.insert(int(rng.randint(0, len(w) + 1)), chars[int(rng.randint(0, len(chars)))])
        elif op == 1:
            del w[int(rng.randint(0, len(w)))]
        else:
            w[int(rng.randint(0, len(w)))] = chars[int(rng.randint(0, len(chars)))]
    return ''.join(w)


def synthetic_lexicon(n=20000, seed=0, max_len=40, chars=DEFAULT_CHARS):
    """n words of length 1..max_len: random ones, every 7th a copy of an earlier word (duplicates: ties must go to the
    lowest index), every 5th an earlier word under one edit (near-duplicates), every 11th drawn from two letters only
    (periodic words: long runs of equal characters in the recurrence)"""
    rng = np.random.RandomState(seed)
    words = []
    for i in range(n):
        if i >= 10 and i % 7 == 3:
            w = words[int(rng.randint(0, i))]
        elif i >= 10 and i % 5 == 2:
            w = edit(rng, words[int(rng.randint(0, i))], 1, chars)[:max_len] or chars[0]
        elif i % 11 == 5:
            w = random_word(rng, 1, max_len, chars[33:35])
        else:
            w = random_word(rng, 1, max_len, chars)
        words.append(w)
    return words


def synthetic_queries(words, n=1024, seed=1, chars=DEFAULT_CHARS):
    """lexicon words under 0..4 random edits, random strings, the empty string, length-64 strings, strings of one
    repeated character, and strings with characters outside the alphabet"""
    rng = np.random.RandomState(seed)
    out = ['', '', chars[40] * 64, random_word(rng, 64, 64, chars), chars[33] * 1, chars[34] * 31, chars[35] * 32, chars[36] * 33,
           chars[37] * 63, 'été', 'naïve café', '中' * 5]
    while len(out) < n:
        k = len(out) % 8
        if k < 5:
            out.append(edit(rng, words[int(rng.randint(0, len(words)))], k, chars)[:64])
        elif k == 5:
            out.append(random_word(rng, 0, 64, chars))
        elif k == 6:
            out.append(random_word(rng, 1, 30, chars[33:35]))
        else:
            out.append(chars[int(rng.randint(0, len(chars)))] * int(rng.randint(1, 65)))
    return out


def random_ranges(rng, n, L):
    """n ranges over [0, L]: empty ones, single words, the whole lexicon, the rest random"""
    out = []
    for i in range(n):
        k = i % 8
        if k == 0:
            lo = int(rng.randint(0, L + 1))
            out.append((lo, lo))
        elif k == 1:
            lo = int(rng.randint(0, L))
            out.append((lo, lo + 1))
        elif k == 2:
            out.append((0, L))
        else:
            lo = int(rng.randint(0, L))
            out.append((lo, int(rng.randint(lo, min(L, lo + (300 if k < 6 else L)) + 1))))
    return out


def image_ranges(n_queries, n_images, L):
    """n_images adjacent ranges of unequal length covering [0, L), query i belongs to image i % n_images"""
    cuts = np.unique(np.concatenate([[0, L], np.random.RandomState(5).randint(1, L, n_images - 1)]))
    while cuts.size < n_images + 1:                                   # a repeated cut: split the longest range
        gaps = np.diff(cuts)
        k = int(gaps.argmax())
        cuts = np.insert(cuts, k + 1, cuts[k] + gaps[k] // 2)
    per = [(int(cuts[i]), int(cuts[i + 1])) for i in range(n_images)]
    return [per[i % n_images] for i in range(n_queries)], per


# the length grid: every (query length, word length) pair under every variant, one lexicon word per pair
GRID_M = (0, 1, 2, 7, 8, 9, 31, 32, 33, 62, 63, 64)
GRID_NW = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 247, 248, 249, 254, 255)
GRID_VARIANTS = ('one repeated code', 'two symbols', 'whole alphabet', 'near match', 'no common symbol', 'unknowns')
N_CODES = len(LX.code_table(DEFAULT_CHARS))            # the codes an encoded string of DEFAULT_CHARS can hold: 0 .. N_CODES - 1


def definition(q, w):
    """edit_distance_cpu (the definition, not the Myers specification) on a query's and a word's codes.  An unknown (254 or
    255, on either side) becomes a negative number of its own per side and position, so it equals nothing."""
    a = [c if c < LX.UNKNOWN_QUERY else -1 - i for i, c in enumerate(np.asarray(q).tolist())]
    b = [c if c < LX.UNKNOWN_QUERY else -1000 - j for j, c in enumerate(np.asarray(w).tolist())]
    return LX.edit_distance_cpu(a, b)


def _pack_pairs(pairs, m, n, variant, closed):
    N = len(pairs)
    q_codes = np.zeros((N, LX.QUERY_MAX), dtype=np.uint8)
    for i, (q, _) in enumerate(pairs):
        q_codes[i, :len(q)] = q
    offsets = np.zeros(N + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(w) for _, w in pairs])
    pool = np.concatenate([np.asarray(w, dtype=np.uint8) for _, w in pairs])
    return dict(q_codes=q_codes, q_len=np.asarray(m, dtype=np.int32), pool=pool, offsets=offsets, m=np.asarray(m), n=np.asarray(n),
                variant=np.asarray(variant), closed=np.asarray(closed, dtype=np.int64))


_CACHE = {}


def length_grid_cases():
    """-> dict(q_codes uint8 [1656, 64], q_len, pool, offsets, m, n, variant, closed): pair i = ((im * 23) + in) * 6 + variant is
    query i against lexicon word i, the words back to back.  `closed` holds the distance in closed form, -1 where there is none.
    The queries of variants 0 to 4 depend on (variant, m) only, so the grid holds about 200 distinct queries, which keeps the
    whole-lexicon oracle of check_length_grid at a few seconds; every word is its pair's own.  The variants:
      0  one repeated code on both sides (the longest carry chains): |m - n|
      1  random codes over two symbols
      2  random codes over the whole of DEFAULT_CHARS
      3  the word is the query tiled or cut to n codes (random when m == 0), then two substitutions at random positions below n
      4  no common symbol: max(m, n)
      5  unknowns.  Even m + n: the query all 254, the word all 255: max(m, n).  Odd m + n: the query is the word's head (and
         random codes beyond the word when m > n), except that position min(m, n) - 1, where it exists, holds 254 in the query
         and 255 in the word -- bit m - 1 of the column, the one the score follows, when m <= n."""
    if 'grid' in _CACHE:
        return _CACHE['grid']
    rng = np.random.RandomState(15)
    half = N_CODES // 2
    shared = {}
    for m in GRID_M:
        shared[m] = [np.full(m, 7), rng.randint(33, 35, m), rng.randint(0, N_CODES, m), rng.randint(0, N_CODES, m), rng.randint(0, half, m)]
    pairs, ms, ns, vs, closed = [], [], [], [], []
    for m in GRID_M:
        for n in GRID_NW:
            for v in range(6):
                c = -1
                if v < 5:
                    q = shared[m][v]
                if v == 0:
                    w, c = np.full(n, 7), abs(m - n)
                elif v == 1:
                    w = rng.randint(33, 35, n)
                elif v == 2:
                    w = rng.randint(0, N_CODES, n)
                elif v == 3:
                    w = np.resize(q, n).copy() if m else rng.randint(0, N_CODES, n)
                    for _ in range(2 if n else 0):
                        w[int(rng.randint(0, n))] = int(rng.randint(0, N_CODES))
                elif v == 4:
                    w, c = rng.randint(half, N_CODES, n), max(m, n)
                elif (m + n) % 2 == 0:
                    q, w, c = np.full(m, LX.UNKNOWN_QUERY), np.full(n, LX.UNKNOWN_WORD), max(m, n)
                else:
                    w = rng.randint(0, N_CODES, n)
                    q = np.concatenate([w[:m], rng.randint(0, N_CODES, max(m - n, 0))])
                    p = min(m, n) - 1
                    if p >= 0:
                        q[p], w[p] = LX.UNKNOWN_QUERY, LX.UNKNOWN_WORD
                assert len(q) == m and len(w) == n
                pairs.append((q, w))
                ms.append(m)
                ns.append(n)
                vs.append(v)
                closed.append(c)
    _CACHE['grid'] = _pack_pairs(pairs, ms, ns, vs, closed)
    return _CACHE['grid']


def unknown_self_cases():
    """the grid's lengths once more with whole queries and words of ONE unknown code: 254 against 254, 255 against 255 and 255
    against 254 (the grid's variant 5 holds 254 against 255).  None matches, itself included: max(m, n) for all 828 pairs."""
    if 'unknown' not in _CACHE:
        rows = [(m, n, qc, wc) for m in GRID_M for n in GRID_NW for qc, wc in ((254, 254), (255, 255), (255, 254))]
        _CACHE['unknown'] = _pack_pairs([(np.full(m, qc), np.full(n, wc)) for m, n, qc, wc in rows], [r[0] for r in rows], [r[1] for r in rows],
                                        [5] * len(rows), [max(r[0], r[1]) for r in rows])
    return _CACHE['unknown']


def pair_definition(g, key):
    """the definition on every pair of a case dict, int64 [N]; computed once per process (`key` names the dict)"""
    if key not in _CACHE:
        off = g['offsets']
        _CACHE[key] = np.asarray([definition(g['q_codes'][i, :g['q_len'][i]], g['pool'][off[i]:off[i + 1]]) for i in range(len(g['q_len']))],
                                 dtype=np.int64)
    return _CACHE[key]


def length_grid_expected():
    return pair_definition(length_grid_cases(), 'grid definition')


def materialise(pool, offsets, pool_bytes):
    """-> (pool', offsets'): the clean table omp_lexicon_nearest is documented to see in a damaged one.  Word w runs from
    s = clamp(offsets[w], 0, pool_bytes) to e = min(max(offsets[w + 1], s), pool_bytes, s + 255); the words are copied out back
    to back, so that the package's specification applies unchanged."""
    pool = np.asarray(pool, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.int64)
    pool_bytes = int(pool_bytes)
    assert 0 <= pool_bytes <= pool.size
    words = []
    for w in range(off.size - 1):
        s = min(max(int(off[w]), 0), pool_bytes)
        e = min(max(int(off[w + 1]), s), pool_bytes, s + LX.WORD_MAX)
        words.append(pool[s:e])
    out = np.zeros(len(words) + 1, dtype=np.int32)
    out[1:] = np.cumsum([w.size for w in words])
    return (np.concatenate(words) if words else np.zeros(0, dtype=np.uint8)), out


# ---------------------------------------------------------------------------------------------
# GPU checks
# ---------------------------------------------------------------------------------------------
def _same(name, got, want, note=''):
    from tests.gpu_checks import rec
    gi, gd = np.asarray(got[0]), np.asarray(got[1])
    wi, wd = np.asarray(want[0]), np.asarray(want[1])
    bad = int((gi != wi).sum() + (gd != wd).sum()) if gi.shape == wi.shape else gi.size + wi.size
    first = ''
    if bad:
        k = int(np.nonzero((gi != wi) | (gd != wd))[0][0]) if gi.shape == wi.shape else -1
        first = ' first at %d: got (%s, %s) want (%s, %s)' % (k, gi[k], gd[k], wi[k], wd[k]) if k >= 0 else ' shapes differ'
    return rec(name, bad, 0, '%d queries%s %s' % (gi.size, first, note))


def check_kernel_against_nearest_cpu(n_words=20000, n_queries=1024):
    """LexiconMatcher.nearest == nearest_cpu (idx and dist of every query) over the whole lexicon, random ranges
    (empty and single-word ones among them) and 64 per-image ranges"""
    import time
    from tests.gpu_checks import DEV, rec
    words = synthetic_lexicon(n_words)
    queries = synthetic_queries(words, n_queries)
    L = len(words)
    m = LX.LexiconMatcher(DEV, words, DEFAULT_CHARS)
    pool, offsets = LX.encode_words(words, DEFAULT_CHARS)
    codes, q_len = LX.encode_queries(queries, DEFAULT_CHARS)
    out = [rec('lexicon: duplicates in the synthetic lexicon', 0 if len(set(words)) < L else 1, 0, '%d distinct of %d' % (len(set(words)), L)),
           rec('lexicon: query lengths 0 and 64 present', 0 if {0, 64} <= set(q_len.tolist()) else 1, 0)]
    cases = (('whole lexicon', None), ('random ranges', random_ranges(np.random.RandomState(2), len(queries), L)),
             ('64 per-image ranges', image_ranges(len(queries), 64, L)[0]))
    for name, ranges in cases:
        t0 = time.time()
        want = LX.nearest_encoded_cpu(codes, q_len, pool, offsets, ranges)
        t1 = time.time()
        gi, gd, _ = m.nearest(queries, ranges)
        out.append(_same('lexicon[%s] == nearest_cpu' % name, (gi, gd), want, '(oracle %.1f s)' % (t1 - t0)))
        if ranges is not None:
            empty = [i for i, (lo, hi) in enumerate(ranges) if lo >= hi]
            ok = all(gi[i] == -1 and gd[i] == -1 for i in empty)
            out.append(rec('lexicon[%s]: empty ranges give (-1, -1)' % name, 0 if ok else 1, 0, '%d empty' % len(empty)))
    return out


def check_edges():
    """a lexicon of one word; L and N off every tile; several query chunks (chunk forced to 100); two consecutive calls
    with different ranges on one matcher; a call on a side stream; the acceptance rule of __call__"""
    import torch
    from tests.gpu_checks import DEV, rec
    out = []
    one = LX.LexiconMatcher(DEV, ['Hello'], DEFAULT_CHARS)
    qs = ['hello', '', 'help', 'x' * 64, 'HELLO!']
    out.append(_same('lexicon: one word', one.nearest(qs)[:2], LX.nearest_cpu(qs, ['Hello'], alphabet=DEFAULT_CHARS)))
    words = synthetic_lexicon(1237, seed=3)
    queries = synthetic_queries(words, 333, seed=4)
    pool, offsets = LX.encode_words(words, DEFAULT_CHARS)
    codes, q_len = LX.encode_queries(queries, DEFAULT_CHARS)
    want = LX.nearest_encoded_cpu(codes, q_len, pool, offsets)
    m = LX.LexiconMatcher(DEV, words, DEFAULT_CHARS)
    got = m.nearest(queries)
    out.append(_same('lexicon: L = 1237, N = 333', got[:2], want, '%d chunk' % m.last_chunks))
    m100 = LX.LexiconMatcher(DEV, words, DEFAULT_CHARS, chunk=100)
    got100 = m100.nearest(queries)
    out.append(_same('lexicon: query chunks of 100', got100[:2], want))
    out.append(rec('lexicon: 333 queries in 4 chunks of 100', abs(m100.last_chunks - 4), 0))
    rng = np.random.RandomState(6)
    for k in range(2):
        ranges = random_ranges(rng, len(queries), len(words))
        out.append(_same('lexicon: consecutive call %d with its own ranges' % k, m.nearest(queries, ranges)[:2],
                         LX.nearest_encoded_cpu(codes, q_len, pool, offsets, ranges)))
    out.append(_same('lexicon: and the whole lexicon again', m.nearest(queries)[:2], want))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got_side = m.nearest(queries)
    side.synchronize()
    out.append(_same('lexicon: on a side stream', got_side[:2], want))
    res = m(queries, max_dist=1, max_ratio=0.25)
    bad = 0
    for (word, idx, dist), i, d, n in zip(res, want[0].tolist(), want[1].tolist(), q_len.tolist()):
        keep = d <= 1 and d <= int(np.floor(0.25 * n))
        bad += int(idx != i or dist != d or word != (words[i] if keep else None))
    out.append(rec('lexicon: __call__ words, indices, distances and acceptance', bad, 0,
                   '%d of %d accepted' % (sum(1 for r in res if r[0] is not None), len(res))))
    return out


def check_hostile_descriptors():
    """q_len of -1 and 200 are refused (all ones), hi > L and lo < 0 are clamped, an inverted range is empty, placed
    through ops directly.  The buffers are sized so that even an unclamped read would stay inside allocated memory:
    q_codes holds four spare rows, the pool is followed by spare zeros and the offsets table lies inside a larger one."""
    import torch
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV, rec
    words = synthetic_lexicon(300, seed=7)
    L = len(words)
    pool, offsets = LX.encode_words(words, DEFAULT_CHARS)
    queries = ['hostile', 'descriptor', 'lexicon', 'word', 'range', 'clamp', 'refuse', 'reader']
    codes, q_len = LX.encode_queries(queries, DEFAULT_CHARS)
    N = len(queries)
    wide = np.zeros((N + 4, 64), dtype=np.uint8)                       # room for a 200-character read of the last query
    wide[:N] = codes
    q_len = q_len.copy()
    q_len[0], q_len[1] = -1, 200
    lo = np.asarray([0, 0, -50, 10, 250, 200, L, 0], dtype=np.int32)
    hi = np.asarray([L, L, 40, L + 100000, L + 150000, 100, L + 7, L], dtype=np.int32)
    pool_d = torch.from_numpy(np.concatenate([pool, np.zeros(4096, dtype=np.uint8)])).to(DEV)
    # the table sits inside a larger allocation: 64 entries before it (lo = -50) and 200 000 after it (hi = L + 150 000)
    off_pad = np.concatenate([np.zeros(64, dtype=np.int32), offsets, np.full(200000, offsets[-1], dtype=np.int32)])
    off_d = torch.from_numpy(off_pad).to(DEV)[64:]
    best = ops.lexicon_nearest(torch.from_numpy(wide).to(DEV), torch.from_numpy(q_len).to(DEV), torch.from_numpy(lo).to(DEV),
                               torch.from_numpy(hi).to(DEV), pool_d, int(pool.size), off_d, L, range_hint=L)
    gi, gd = LX.unpack_best(best.cpu().numpy())
    ok_len = q_len.copy()
    ok_len[:2] = 0
    want = LX.nearest_encoded_cpu(codes, ok_len, pool, offsets, np.stack([np.clip(lo, 0, L), np.clip(hi.astype(np.int64), 0, L)], 1))
    wi, wd = want[0].copy(), want[1].copy()
    wi[:2], wd[:2] = -1, -1                                            # refused
    out = [_same('lexicon: hostile descriptors give the documented outputs', (gi, gd), (wi, wd)),
           rec('lexicon: q_len -1 and 200 refused', 0 if (gi[:2] == -1).all() and (gd[:2] == -1).all() else 1, 0),
           rec('lexicon: inverted and past-the-end ranges are empty', 0 if gi[5] == -1 and gi[6] == -1 else 1, 0),
           rec('lexicon: clamped ranges still answer', 0 if (gi[[2, 3, 4, 7]] >= 0).all() else 1, 0)]
    # the host checks of the entry point
    for name, kw in (('N = 0', dict(q_len=torch.zeros(0, dtype=torch.int32, device=DEV))), ('L = 0', dict(L=0))):
        args = dict(q_codes=torch.from_numpy(wide).to(DEV), q_len=torch.from_numpy(ok_len).to(DEV), q_lo=None, q_hi=None, pool=pool_d,
                    pool_bytes=int(pool.size), offsets=off_d, L=L)
        args.update(kw)
        try:
            ops.lexicon_nearest(**args)
            refused = False
        except RuntimeError:
            refused = True
        out.append(rec('lexicon: %s is an argument error' % name, 0 if refused else 1, 0))
    return out


CANARY = 0x5a5a5a5a5a5a5a5a


def _dev(a):
    import torch
    from tests.gpu_checks import DEV
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _keys(q_codes, q_len, lo, hi, pool_d, pool_bytes, off_d, L, hint=0, best=None):
    """one omp_lexicon_nearest through ops on host queries and device tables -> the keys, uint64 [N]"""
    from advancedliteratemachinery_amd import ops
    best = ops.lexicon_nearest(_dev(q_codes), _dev(np.asarray(q_len, dtype=np.int32)), _dev(None if lo is None else np.asarray(lo, dtype=np.int32)),
                               _dev(None if hi is None else np.asarray(hi, dtype=np.int32)), pool_d, int(pool_bytes), off_d, int(L), best=best,
                               range_hint=int(hint))
    return best.cpu().numpy().view(np.uint64)[:len(q_len)].copy()


def _first_bad(got, want):
    k = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return '' if not k.size else 'first at %d: got %s want %s' % (k[0], got[k[0]], want[k[0]])


def check_length_grid():
    """length_grid_cases() on the device.  One launch of 1656 queries, query i against word i alone (range (i, i + 1),
    range_hint 1): every distance equals the DEFINITION and every index is i; the same launch under range_hint 0, L and
    2^31 - 1 (0 and L cut every single-word range into several slices, all but one of them empty) gives the same keys; the
    828 pairs of unknown_self_cases() the same way; and the grid's distinct queries against the whole lexicon equal
    nearest_encoded_cpu, with a word longer than 64 and the empty word among the answers."""
    import time
    from tests.gpu_checks import rec
    out = []
    for name, g, key in (('grid', length_grid_cases(), 'grid definition'), ('unknowns against themselves', unknown_self_cases(), 'unknown definition')):
        want = pair_definition(g, key)
        N = L = len(g['q_len'])
        pool_d = _dev(np.concatenate([g['pool'], np.zeros(64, dtype=np.uint8)]))
        off_d = _dev(g['offsets'])
        one = np.arange(N)
        base = _keys(g['q_codes'], g['q_len'], one, one + 1, pool_d, g['pool'].size, off_d, L, hint=1)
        gi, gd = LX.unpack_best(base)
        bad = np.nonzero(gd != want)[0]
        note = '' if not bad.size else 'first at %d (m %d, n %d, %s): got %d want %d' % (
            bad[0], g['m'][bad[0]], g['n'][bad[0]], GRID_VARIANTS[g['variant'][bad[0]]], gd[bad[0]], want[bad[0]])
        out.append(rec('lexicon %s: dist == the definition for every pair' % name, bad.size, 0, '%d pairs %s' % (N, note)))
        out.append(rec('lexicon %s: idx == i for every pair' % name, int((gi != one).sum()), 0, _first_bad(gi, one)))
        for hint in (0, L, 2 ** 31 - 1):
            again = _keys(g['q_codes'], g['q_len'], one, one + 1, pool_d, g['pool'].size, off_d, L, hint=hint)
            out.append(rec('lexicon %s: range_hint %d gives the keys of range_hint 1' % (name, hint), int((again != base).sum()), 0, _first_bad(again, base)))
    g = length_grid_cases()
    u = np.sort(np.unique(np.concatenate([g['q_len'][:, None].astype(np.uint8), g['q_codes']], 1), axis=0, return_index=True)[1])
    t0 = time.time()
    want = LX.nearest_encoded_cpu(g['q_codes'][u], g['q_len'][u], g['pool'], g['offsets'])
    t1 = time.time()
    L = len(g['q_len'])
    got = LX.unpack_best(_keys(g['q_codes'][u], g['q_len'][u], None, None, _dev(np.concatenate([g['pool'], np.zeros(64, dtype=np.uint8)])),
                               g['pool'].size, _dev(g['offsets']), L))
    out.append(_same('lexicon grid: %d distinct queries against the whole lexicon == nearest_cpu' % u.size, got, want, '(oracle %.1f s)' % (t1 - t0)))
    n_ans = np.diff(g['offsets'])[want[0]]
    out.append(rec('lexicon grid: a word longer than 64 and the empty word are among the answers', 0 if (n_ans > 64).any() and (n_ans == 0).any() else 1, 0,
                   '%d answers longer than 64, %d empty' % ((n_ans > 64).sum(), (n_ans == 0).sum())))
    return out


def check_slices():
    """2 queries against 2049 words of 6 to 12 characters: 9 slices of 228 words.  Equal spellings on both sides of a slice
    boundary (227 and 228) and at both ends of the lexicon (0 and 2048) answer with the lower index; a unique nearest word at
    the last index of the last slice is found; a tie between index 2048 and index 5 goes to 5; the same with ranges that re-cut
    the slices from another origin.  Everything also equals nearest_encoded_cpu."""
    import torch
    from tests.gpu_checks import DEV, rec
    out = []
    N, L = 2, 2049
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    chunks = min(-(-16 * cus // N), -(-L // 256))
    out.append(rec('lexicon slices: 2 queries x 2049 words are cut into 9 slices of 228', 0 if (chunks, -(-L // chunks)) == (9, 228) else 1, 0,
                   '%d compute units' % cus))
    rng = np.random.RandomState(21)
    words = [random_word(rng, 6, 12) for _ in range(L)]
    A, B, C = 'Boundary', 'BothEnds', 'LastIndex'
    C1, C5 = 'LastIndeX', 'LostIndeX'                  # C1 = C under one substitution, C5 = C1 under another one: two from C

    def run(name, words, queries, ranges=None, hint=0, expect=None):
        pool, offsets = LX.encode_words(words, DEFAULT_CHARS, fold_case=False)
        codes, q_len = LX.encode_queries(queries, DEFAULT_CHARS, fold_case=False)
        lo, hi = (None, None) if ranges is None else (np.asarray(ranges)[:, 0], np.asarray(ranges)[:, 1])
        want = LX.nearest_encoded_cpu(codes, q_len, pool, offsets, ranges)
        got = LX.unpack_best(_keys(codes, q_len, lo, hi, _dev(np.concatenate([pool, np.zeros(64, dtype=np.uint8)])), pool.size, _dev(offsets), L, hint))
        out.append(_same('lexicon slices[%s] == nearest_cpu' % name, got, want))
        ok = got[0].tolist() == expect[0] and got[1].tolist() == expect[1]
        out.append(rec('lexicon slices[%s]: idx %s dist %s' % (name, expect[0], expect[1]), 0 if ok else 1, 0, 'got %s %s' % (got[0].tolist(), got[1].tolist())))

    w1 = list(words)
    w1[227] = w1[228] = A
    w1[0] = w1[2048] = B
    run('equal spellings across a boundary and at both ends', w1, [A, B], expect=([227, 0], [0, 0]))
    w2 = list(words)
    w2[2048], w2[5] = C, C5
    run('nearest word at the last index; a tie of 2048 and 5', w2, [C, C1], expect=([2048, 5], [0, 1]))
    ranges = [(228, 2049), (1, 2048)]
    run('ranges (228, 2049) and (1, 2048), their true hint', w2, [C, C1], ranges, hint=2047, expect=([2048, 5], [0, 1]))
    run('ranges (228, 2049) and (1, 2048), hint 0', w2, [C, C1], ranges, hint=0, expect=([2048, 5], [0, 1]))
    return out


def pool_tail_case():
    """-> (words, queries) as code lists: 40 words of 1 to 15 codes below 30; the last three hold 15, 14 and 15 codes from
    three alphabets of their own (40..44, 45..49, 50..54), so a query that spells one of them in full is nearer to any
    non-empty head of it than to every other word.  Queries: the last three words, three earlier words, the empty query and
    20 x code 50 (the code the spare bytes behind the pool hold)."""
    rng = np.random.RandomState(31)
    words = [rng.randint(0, 30, int(rng.randint(1, 16))).tolist() for _ in range(37)]
    words += [rng.randint(40, 45, 15).tolist(), rng.randint(45, 50, 14).tolist(), rng.randint(50, 55, 15).tolist()]
    return words, [words[39], words[38], words[37], words[3], words[17], words[36], [], [50] * 20]


def _pack_codes(words, queries):
    offsets = np.zeros(len(words) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(w) for w in words])
    pool = np.asarray([c for w in words for c in w], dtype=np.uint8)
    codes = np.zeros((len(queries), LX.QUERY_MAX), dtype=np.uint8)
    for i, q in enumerate(queries):
        codes[i, :len(q)] = q
    return pool, offsets, codes, np.asarray([len(q) for q in queries], dtype=np.int32)


def check_pool_tail():
    """pool_tail_case() with pool_bytes = P - 16 .. P, the device pool followed by 64 spare bytes of code 50, which the
    queries hold: a byte read or used at or beyond pool_bytes (the rest of the true pool, or the spare bytes) changes a
    distance.  Every answer equals nearest_encoded_cpu on materialise(pool, offsets, pool_bytes); the queries that spell
    the last words are answered by the cut word itself at every residue of pool_bytes % 8, so the byte-wise branch of
    lex_load8 decides a reported distance at each."""
    from tests.gpu_checks import rec
    out = []
    words, queries = pool_tail_case()
    pool, offsets, codes, q_len = _pack_codes(words, queries)
    P, L = int(pool.size), len(words)
    pool_d = _dev(np.concatenate([pool, np.full(64, 50, dtype=np.uint8)]))
    off_d = _dev(offsets)
    bad, note, cut_answers = 0, '', set()
    for pb in range(P - 16, P + 1):
        want = LX.nearest_encoded_cpu(codes, q_len, *materialise(pool, offsets, pb))
        got = LX.unpack_best(_keys(codes, q_len, None, None, pool_d, pb, off_d, L))
        miss = (got[0] != want[0]) | (got[1] != want[1])
        if miss.any() and not note:
            k = int(np.nonzero(miss)[0][0])
            note = 'first at pool_bytes P - %d, query %d: got (%d, %d) want (%d, %d)' % (P - pb, k, got[0][k], got[1][k], want[0][k], want[1][k])
        bad += int(miss.sum())
        if pb < P and want[0][0] == L - 1 and 0 < want[1][0] < 15:       # the last word, cut but not empty, answers its own spelling
            cut_answers.add(pb % 8)
    out.append(rec('lexicon pool tail: pool_bytes P - 16 .. P == nearest_cpu on the materialised table', bad, 0, '17 x %d queries %s' % (len(queries), note)))
    out.append(rec('lexicon pool tail: the cut last word is the answer at every residue of pool_bytes % 8', 8 - len(cut_answers), 0))
    return out


def damaged_table_cases():
    """-> (pool, offsets, L, codes, q_len, cases): 300 synthetic words with a hand-built word of 300 codes at index 100 (legal
    for the kernel, which cuts it at 255; encode_words refuses it), 8 queries of which query 0 spells that word's first 64
    codes, and the cases as (name, offsets, pool_bytes, ranges)."""
    words = synthetic_lexicon(300, seed=7)
    pool0, off0 = LX.encode_words(words, DEFAULT_CHARS)
    rows = [pool0[off0[i]:off0[i + 1]].tolist() for i in range(len(words))]
    rows[100] = [(3 * i + i // 7) % N_CODES for i in range(300)]
    queries = [rows[100][:64]] + [LX.encode_queries([q], DEFAULT_CHARS)[0][0, :len(q)].tolist() for q in
                                  ('hostile', 'descriptor', 'lexicon', 'word', 'range', 'clamp', 'reader')]
    pool, offsets, codes, q_len = _pack_codes(rows, queries)
    L, P, N = len(rows), int(pool.size), len(queries)
    falling = offsets.copy()
    falling[40:80] = falling[40:80][::-1]
    falling[120] = -77
    past = offsets.copy()
    past[150:] += 50000                                                # beyond pool_bytes, inside the spare bytes
    huge = offsets.copy()
    huge[200] = 2 ** 31 - 1
    long_ranges = [(100, 101)] + [(0, L)] * (N - 1)
    cases = [('a reversed stretch and a negative offset', falling, P, None), ('offsets past pool_bytes', past, P, None),
             ('an offset of 2^31 - 1', huge, P, None), ('pool_bytes 0', offsets, 0, [(3 * q, L - q) for q in range(N)]),
             ('pool_bytes P / 2 + 3', offsets, P // 2 + 3, None), ('a word of 300 characters', offsets, P, long_ranges)]
    return pool, offsets, L, codes, q_len, cases


def check_damaged_tables():
    """damaged_table_cases() straight through ops: each case is answered, not refused, equals nearest_encoded_cpu on the
    materialised table, and leaves the canary words round `best` (a view [8 : 8 + N] of a buffer of 0x5a5a...) intact.
    Argument errors (null pointers, q_hi without q_lo, n = -1, L = -5, pool_bytes = -1, at the _lib level because ops would
    refuse some of them first) are a RuntimeError with the whole buffer untouched.
    Nothing here reads outside an allocation even if the kernel failed to clamp, sized as in
    gpu_checks_lexicon_post.check_hostile_descriptors: the offsets table lies inside a larger one (64 entries before, 4096
    after), the pool is preceded by 4 KiB (the offset -77) and followed by 64 KiB of a live symbol (offsets + 50 000, and any
    word read past a lowered pool_bytes).  The 2^31 - 1 case alone gets a pool allocation of 2 GiB + 68 KiB (uninitialised
    beyond the 64 KiB), because no smaller one holds that offset."""
    import torch
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    out = []
    pool, offsets, L, codes, q_len, cases = damaged_table_cases()
    N, P, LEAD = len(q_len), int(pool.size), 4096
    live = int(codes[1, 0])                                            # the 'H' of 'hostile'
    host_pool = np.concatenate([np.full(LEAD, live, dtype=np.uint8), pool, np.full(1 << 16, live, dtype=np.uint8)])
    pool_d = _dev(host_pool)[LEAD:]
    codes_d, len_d = _dev(codes), _dev(q_len)

    def table(off):
        return _dev(np.concatenate([np.zeros(64, dtype=np.int32), off, np.full(4096, off[-1], dtype=np.int32)]))[64:]

    big = None
    for name, off, pb, ranges in cases:
        p_d = pool_d
        if int(off.max()) > P + 50000:
            big = torch.empty(LEAD + 2 ** 31 + 4096 + (1 << 16), dtype=torch.uint8, device=DEV)
            big[:host_pool.size] = _dev(host_pool)
            p_d = big[LEAD:]
        buf = torch.full((N + 16,), CANARY, dtype=torch.int64, device=DEV)
        lo, hi = (None, None) if ranges is None else (np.asarray(ranges)[:, 0], np.asarray(ranges)[:, 1])
        try:
            got = LX.unpack_best(_keys(codes, q_len, lo, hi, p_d, pb, table(off), L, hint=0, best=buf[8:8 + N]))
            refused = False
        except RuntimeError:
            refused = True
        out.append(rec('lexicon damaged[%s]: answered' % name, 1 if refused else 0, 0))
        if refused:
            continue
        want = LX.nearest_encoded_cpu(codes, q_len, *materialise(pool, off, pb), ranges=ranges)
        out.append(_same('lexicon damaged[%s] == nearest_cpu on the materialised table' % name, got, want))
        b = buf.cpu().numpy()
        out.append(rec('lexicon damaged[%s]: canaries round best intact' % name, 0 if (b[:8] == CANARY).all() and (b[8 + N:] == CANARY).all() else 1, 0))
        if pb == 0:
            ok = got[0].tolist() == [r[0] for r in ranges] and got[1].tolist() == q_len.tolist()
            out.append(rec('lexicon damaged[pool_bytes 0]: every word is empty: the lowest index of the range at distance q_len', 0 if ok else 1, 0))
        if ranges is not None and ranges[0] == (100, 101):
            out.append(rec('lexicon damaged[a word of 300 characters]: cut at 255: (100, 255 - 64)', 0 if (got[0][0], got[1][0]) == (100, 191) else 1, 0,
                           'got (%d, %d)' % (got[0][0], got[1][0])))
        p_d = big = None
    off_d = table(offsets)
    zeros = torch.zeros(N, dtype=torch.int32, device=DEV)
    for name, kw in (('q_codes null', dict(q_codes=None)), ('q_len null', dict(q_len=None)), ('pool null', dict(pool=None)),
                     ('offsets null', dict(offsets=None)), ('best null', dict(best=None)), ('q_hi without q_lo', dict(q_hi=zeros)),
                     ('q_lo without q_hi', dict(q_lo=zeros)), ('n = -1', dict(n=-1)), ('n = 0', dict(n=0)), ('L = -5', dict(L=-5)), ('L = 0', dict(L=0)),
                     ('pool_bytes = -1', dict(pool_bytes=-1))):
        buf = torch.full((N + 16,), CANARY, dtype=torch.int64, device=DEV)
        a = dict(q_codes=codes_d, q_len=len_d, q_lo=None, q_hi=None, n=N, pool=pool_d, pool_bytes=P, offsets=off_d, L=L, best=buf[8:8 + N])
        a.update(kw)
        try:
            rc = _lib.lib().omp_lexicon_nearest(ops.ptr(a['q_codes']), ops.ptr(a['q_len']), ops.ptr(a['q_lo']), ops.ptr(a['q_hi']), a['n'], ops.ptr(a['pool']),
                                                a['pool_bytes'], ops.ptr(a['offsets']), a['L'], 0, ops.ptr(a['best']), ops.stream())
            _lib.check(rc, 'omp_lexicon_nearest')
            refused = False
        except RuntimeError:
            refused = True
        torch.cuda.synchronize()
        untouched = bool((buf.cpu().numpy() == CANARY).all())
        out.append(rec('lexicon damaged[%s]: an argument error, best untouched' % name, 0 if refused and untouched else 1, 0))
    return out


def check_fill_edges():
    """N = 1, 255, 256, 257, 513 (lexicon_fill_kernel off its 256 tile) into a `best` that holds canary words, not ones: with an
    empty range for every query every key is NONE_KEY (every search workgroup returns before its barrier); with a range for the
    odd queries only, those are answered as nearest_encoded_cpu answers them and the even ones are NONE_KEY.  The words
    round `best` stay."""
    import torch
    from tests.gpu_checks import DEV, rec
    out = []
    words = synthetic_lexicon(300, seed=11, max_len=12)
    queries = synthetic_queries(words, 513, seed=12)
    pool, offsets = LX.encode_words(words, DEFAULT_CHARS)
    codes, q_len = LX.encode_queries(queries, DEFAULT_CHARS)
    L = len(words)
    odd = [(0, L) if i % 2 else (L // 2, L // 2) for i in range(513)]
    want = LX.nearest_encoded_cpu(codes, q_len, pool, offsets, odd)
    pool_d, off_d = _dev(np.concatenate([pool, np.zeros(64, dtype=np.uint8)])), _dev(offsets)
    for N in (1, 255, 256, 257, 513):
        for name, ranges in (('empty ranges', [(7, 7)] * N), ('odd queries only', odd[:N])):
            buf = torch.full((N + 16,), CANARY, dtype=torch.int64, device=DEV)
            r = np.asarray(ranges)
            got = _keys(codes[:N], q_len[:N], r[:, 0], r[:, 1], pool_d, pool.size, off_d, L, hint=L, best=buf[8:8 + N])
            b = buf.cpu().numpy()
            intact = (b[:8] == CANARY).all() and (b[8 + N:] == CANARY).all()
            if name == 'empty ranges':
                out.append(rec('lexicon fill[N = %d]: every key is NONE_KEY' % N, int((got != np.uint64(LX.NONE_KEY)).sum()), 0))
            else:
                out.append(_same('lexicon fill[N = %d]: odd queries answered, even ones none' % N, LX.unpack_best(got), (want[0][:N], want[1][:N])))
                out.append(rec('lexicon fill[N = %d]: even keys are NONE_KEY' % N, int((got[0::2] != np.uint64(LX.NONE_KEY)).sum()), 0))
            out.append(rec('lexicon fill[N = %d, %s]: canaries round best intact' % (N, name), 0 if intact else 1, 0))
    return out


def _strip(records, keys):
    return [[{k: v for k, v in r.items() if k not in keys} for r in recs] for recs in records]


def _lex_bad(records, source, prefix, lists, alphabet, max_dist=None, max_ratio=None):
    """mismatches between the records' lexicon keys and nearest_cpu applied to their own source strings (per image)"""
    bad = n = 0
    for b, recs in enumerate(records):
        words = lists[b]
        if not recs:
            continue
        idx, dist = LX.nearest_cpu([r[source] for r in recs], words, alphabet=alphabet)
        q_len = LX.encode_queries([r[source] for r in recs], alphabet)[1]
        for r, i, d, m in zip(recs, idx.tolist(), dist.tolist(), q_len.tolist()):
            n += 1
            want = words[i] if LX.accept(d, m, max_dist, max_ratio) else None
            bad += int(r.get(prefix + '_index') != i or r.get(prefix + '_dist') != d or r.get(prefix, 0) != want)
    return bad, n


def check_end_to_end():
    """predict_images(lexicon=...) and spot_and_recognize(crop='polygon', lexicon=...) on the synthetic models of
    check_two_stage_polygon: records minus the new keys equal those of the call without `lexicon`, the new keys equal
    nearest_cpu on the records' own strings -- for a shared list, per-image lists and a prebuilt matcher"""
    import torch
    from advancedliteratemachinery_amd.engine.inference import predict_images
    from advancedliteratemachinery_amd.engine.two_stage import spot_and_recognize
    from advancedliteratemachinery_amd.utils import synthetic as weights
    from advancedliteratemachinery_amd.utils.parser import make_args
    from oracle import mgp_str_ref as R
    from tests.gpu_checks import DEV, build_model, rec
    from tests.gpu_checks_mgp import build
    depths = (2, 2, 2, 2)
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, pt_seq_length=6, test_min_size=64, test_max_size=112)
    sd = weights.make_state_dict(args, seed=5, depths=depths)
    omni = build_model(args, sd, depths, torch.float32)
    c = R.cfg(depth=2)
    mgp = build(c, R.make_state_dict(c, seed=17), torch.float32)
    rng = np.random.RandomState(3)
    images = [torch.from_numpy(rng.randint(0, 256, (90, 140, 3), dtype=np.uint8)), torch.from_numpy(rng.randint(0, 256, (70, 100, 3), dtype=np.uint8))]
    shared = synthetic_lexicon(400, seed=8, max_len=12) + synthetic_lexicon(200, seed=9, max_len=8, chars=MGP_CHARS)
    lists = [shared[:250], shared[250:]]
    LEX, MGP = ('lex', 'lex_index', 'lex_dist'), ('mgp_lex', 'mgp_lex_index', 'mgp_lex_dist')
    out = []
    base, _ = predict_images(omni, images, args)
    n_words = sum(len(r) for r in base)
    out.append(rec('lexicon e2e: words spotted', 0 if n_words > 0 else 1, 0, '%d words' % n_words))
    out.append(rec('lexicon e2e: no lexicon, no new keys', sum(int(k in r) for recs in base for r in recs for k in LEX), 0))
    for name, lexicon, per in (('shared list', shared, [shared, shared]), ('per-image lists', lists, lists),
                               ('prebuilt matcher', LX.LexiconMatcher(DEV, shared, args.chars), [shared, shared])):
        got, _ = predict_images(omni, images, args, lexicon=lexicon, lexicon_max_ratio=0.5)
        out.append(rec('lexicon e2e[%s]: records minus the new keys unchanged' % name, 0 if _strip(got, LEX) == base else 1, 0))
        bad, n = _lex_bad(got, 'rec', 'lex', per, args.chars, max_ratio=0.5)
        out.append(rec('lexicon e2e[%s]: lex keys == nearest_cpu on rec' % name, bad + int(n != n_words), 0, '%d words' % n))
    base2, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon')
    for name, lexicon, per in (('shared list', shared, [shared, shared]), ('per-image lists', lists, lists)):
        got, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon', lexicon=lexicon, lexicon_max_dist=3)
        out.append(rec('lexicon two-stage[%s]: records minus the new keys unchanged' % name, 0 if _strip(got, LEX + MGP) == base2 else 1, 0))
        bad, n = _lex_bad(got, 'rec', 'lex', per, args.chars, max_dist=3)
        out.append(rec('lexicon two-stage[%s]: lex keys == nearest_cpu on rec' % name, bad + int(n != n_words), 0, '%d words' % n))
        bad, n = _lex_bad(got, 'mgp_text', 'mgp_lex', per, MGP_CHARS, max_dist=3)
        out.append(rec('lexicon two-stage[%s]: mgp_lex keys == nearest_cpu on mgp_text' % name, bad + int(n != n_words), 0, '%d words' % n))
    return out


def check_timing():
    """tools/lexicon_bench.py: 512 queries against 90 000 words, the median of 30 device calls after 5 at or below
    nearest_cpu's time for the same 512 queries (timed on 32 of them and scaled linearly)"""
    import os
    import sys
    from tests.gpu_checks import rec
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import lexicon_bench
    r = lexicon_bench.measure(queries=512, words=90000, calls=30, warmup=5, cpu_queries=32)
    note = 'device p10 / median / p90 %.3f / %.3f / %.3f ms; nearest_cpu %.1f ms for %d queries -> %.1f ms for %d; %.3g pairs/s' % (
        r['device_ms']['p10'], r['device_ms']['median'], r['device_ms']['p90'], r['cpu_ms_measured'], r['cpu_queries'], r['cpu_ms_scaled'],
        r['queries'], r['pairs_per_s'])
    print(note)
    return [rec('lexicon: 512 x 90 000, device median <= nearest_cpu (32 queries, scaled)', r['device_ms']['median'], r['cpu_ms_scaled'], note),
            rec('lexicon: the bench outputs equal nearest_cpu on the timed subset', 0 if r['outputs_equal'] else 1, 0),
            rec('lexicon: one query chunk, two launches', abs(r['chunks'] - 1), 0)]
