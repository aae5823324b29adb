"""Lexicon correction: the case builders shared by the CPU tests (tests/test_lexicon_host.py) and
the GPU checks of omp_lexicon_nearest / LexiconMatcher / the engine's `lexicon=` against utils/lexicon.py: nearest_cpu.
Everything is integer on both sides, so every comparison is equality.  Same record format as tests/gpu_checks.py; the GPU
modules are imported inside the checks so that the builders stay usable without a device."""
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
