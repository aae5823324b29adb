"""Posterior lexicon decoding: the case builders shared by the CPU tests (tests/test_lexicon_post_host.py)
and the GPU checks of omp_logprob_costs / omp_lexicon_posterior / PosteriorMatcher / the engine's lexicon_mode='posterior' against
utils/lexicon_post.py.  Costs are held to costs_cpu within one unit (fp32 against float64 at a rounding boundary); everything after
the costs is integer on both sides, so every other comparison is equality.  Same record format as tests/gpu_checks.py; the GPU
modules are imported inside the checks so that the builders stay usable without a device."""
import numpy as np

from advancedliteratemachinery_amd.utils import lexicon as LX
from advancedliteratemachinery_amd.utils import lexicon_post as LP
from tests.gpu_checks_lexicon import MGP_CHARS, image_ranges, random_ranges, random_word

WORD_LENGTHS = (0, 1, 7, 8, 9, 25, 26, 255)


# ---------------------------------------------------------------------------------------------
# case builders (numpy only)
# ---------------------------------------------------------------------------------------------
def worked_logits():
    """[2, 27, 38]: row 0 all equal (cost 3725 everywhere), row 1 class p % 38 at +20 over zeros at position p"""
    x = np.zeros((2, 27, 38), dtype=np.float32)
    x[0] = 1.5
    for p in range(27):
        x[1, p, p % 38] = 20.0
    return x


def random_logits(n, scale, seed):
    """random normal times `scale`, with planted rows: every 5th query's position 3 all equal, every 7th query's position 9 a tie
    between [s] and a character at the top"""
    rng = np.random.RandomState(seed)
    x = (rng.randn(n, 27, 38) * scale).astype(np.float32)
    x[::5, 3, :] = np.float32(0.25)
    x[::7, 9, :] = np.float32(-3.0)
    x[::7, 9, 1] = np.float32(4.0)
    x[::7, 9, 20] = np.float32(4.0)
    return x


def random_costs(n, seed, peak=None):
    """int32 [n, 26, 38] costs as costs_cpu makes them from random logits (scale 4: a few classes per position are cheap)"""
    rng = np.random.RandomState(seed)
    x = (rng.randn(n, 27, 38) * (4.0 if peak is None else peak)).astype(np.float32)
    return LP.costs_cpu(x)


def post_lexicon(n, seed=0, chars=MGP_CHARS, alphabet=MGP_CHARS, tail_odd=True):
    """n words: the lengths of WORD_LENGTHS first (26 and 255 are too long to score), then random lengths 0..12; every 7th a copy of
    an earlier word (duplicates), every 9th with one character outside MGP-STR's set when the alphabet has one.  tail_odd: the last
    word is grown until the pool's size is no multiple of 8, so that it ends exactly at an odd pool_bytes."""
    rng = np.random.RandomState(seed)
    extra = [c for c in alphabet if c.lower() not in MGP_CHARS]
    words = []
    for i in range(n):
        if i < len(WORD_LENGTHS):
            w = random_word(rng, WORD_LENGTHS[i], WORD_LENGTHS[i], chars)
        elif i % 7 == 3:
            w = words[int(rng.randint(0, i))]
        else:
            w = random_word(rng, 0, 12, chars)
            if extra and i % 9 == 4 and w:
                k = int(rng.randint(0, len(w)))
                w = w[:k] + extra[int(rng.randint(0, len(extra)))] + w[k + 1:]
        words.append(w)
    if tail_odd:
        last = random_word(rng, 3, 3, chars)
        while (sum(len(w) for w in words) + len(last)) % 8 == 0:
            last += chars[0]
        words.append(last)
    return words


def encode(words, alphabet=MGP_CHARS, fold_case=True):
    pool, offsets = LX.encode_words(words, alphabet, fold_case)
    return pool, offsets, LP.class_table(alphabet, fold_case)


# ---------------------------------------------------------------------------------------------
# GPU checks
# ---------------------------------------------------------------------------------------------
def _keys_same(name, got, want, note=''):
    from tests.gpu_checks import rec
    g = np.asarray(got).view(np.uint64).reshape(-1, 2)
    w = np.asarray(want).view(np.uint64).reshape(-1, 2)
    if g.shape != w.shape:
        return rec(name, g.size + w.size, 0, 'shapes differ')
    bad = int((g != w).sum())
    first = ''
    if bad:
        k = int(np.nonzero((g != w).any(axis=1))[0][0])
        first = ' first at %d: got %s want %s' % (k, [hex(int(v)) for v in g[k]], [hex(int(v)) for v in w[k]])
    return rec(name, bad, 0, '%d queries%s %s' % (g.shape[0], first, note))


def check_costs():
    """omp_logprob_costs against costs_cpu: N in (1, 2, 63, 65, 513), random normal logits times 1, 8 and 50 with planted equal rows
    and ties, the worked rows in front; every cost within one unit, the worked rows exact, a -1e4 .. 1e4 row at COST_CAP and 0, and
    greedy == greedy_cpu of the device's own costs"""
    import torch
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV, rec
    out = []
    for N in (1, 2, 63, 65, 513):
        for scale in (1.0, 8.0, 50.0):
            x = random_logits(N, scale, seed=N)
            if N >= 2:
                x[:2] = worked_logits()
            if N >= 63:
                x[2, 5] = np.linspace(-1e4, 1e4, 38).astype(np.float32)
            costs, greedy = ops.logprob_costs(torch.from_numpy(x).to(DEV))
            got, g = costs.cpu().numpy(), greedy.cpu().numpy()
            want = LP.costs_cpu(x)
            diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
            name = 'logprob_costs[N=%d, x%g]' % (N, scale)
            out.append(rec(name + ': |cost - costs_cpu| <= 1 unit', int(diff.max()), 1, '%d of %d differ' % (int((diff > 0).sum()), diff.size)))
            out.append(rec(name + ': costs inside [0, COST_CAP]', 0 if got.min() >= 0 and got.max() <= LP.COST_CAP else 1, 0))
            out.append(rec(name + ': greedy == greedy_cpu(device costs)', int((g != LP.greedy_cpu(got)).sum()), 0))
            if N >= 2:
                out.append(rec(name + ': worked rows exact', int((got[:2] != want[:2]).sum()) + int((got[0] != 3725).sum())
                               + int(sum(got[1, p, (p + 1) % 38] != 0 for p in range(26))) + int((got[1] == 20480).sum() != 26 * 37), 0))
            if N >= 63:
                out.append(rec(name + ': a -1e4 .. 1e4 row reaches COST_CAP and 0', 0 if got[2, 4, 0] == LP.COST_CAP and got[2, 4, 37] == 0 else 1, 0))
    return out


def _device_lexicon(words, alphabet=MGP_CHARS):
    import torch
    from tests.gpu_checks import DEV
    pool, offsets, table = encode(words, alphabet)
    pool_d = torch.from_numpy(np.concatenate([pool, np.zeros(8, dtype=np.uint8)])).to(DEV)
    return pool, offsets, table, pool_d, torch.from_numpy(offsets).to(DEV), torch.from_numpy(table).to(DEV)


def _run(costs, ranges, pool_d, pool_bytes, off_d, L, table_d, hint=None):
    import torch
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV
    c = torch.from_numpy(np.ascontiguousarray(costs, dtype=np.int32)).to(DEV)
    lo = hi = None
    if ranges is not None:
        r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
        lo = torch.from_numpy(np.clip(r[:, 0], -2 ** 31, 2 ** 31 - 1).astype(np.int32)).to(DEV)
        hi = torch.from_numpy(np.clip(r[:, 1], -2 ** 31, 2 ** 31 - 1).astype(np.int32)).to(DEV)
        if hint is None:
            hint = max(int(np.clip(r[:, 1] - r[:, 0], 0, L).max()), 0)
    return ops.lexicon_posterior(c, lo, hi, pool_d, pool_bytes, off_d, L, table_d, range_hint=hint or 0).cpu().numpy()


def check_search():
    """omp_lexicon_posterior against score_cpu on every key of both columns, fed the same int32 costs: N in (1, 2, 63, 65), L in
    (1, 2, 255, 256, 257, 1025, 20000), words of length 0, 1, 7, 8, 9, 25, 26, 255 among them, the last word ending exactly at a
    pool_bytes that is no multiple of 8; whole, per-image, single-word, empty and inverted ranges; range_hint 0 and the largest"""
    from tests.gpu_checks import rec
    out = []
    for L in (1, 2, 255, 256, 257, 1025, 20000):
        words = post_lexicon(L - 1, seed=L, alphabet=MGP_CHARS + '-') if L > 1 else ['word7']
        pool, offsets, table, pool_d, off_d, table_d = _device_lexicon(words, MGP_CHARS + '-')
        if L > 1:
            out.append(rec('posterior[L=%d]: pool_bytes %d is no multiple of 8' % (L, pool.size), 0 if pool.size % 8 else 1, 0))
        lex = LP._Classes(pool, offsets, table)
        for N in (1, 2, 63, 65):
            if L == 20000 and N == 2:
                continue
            costs = random_costs(N, seed=N + L)
            cases = [('whole', None, None)]
            if N > 2:
                rr = random_ranges(np.random.RandomState(N), N, L)
                rr[3] = (min(5, L), 2)                                   # inverted
                cases += [('random ranges, hint = largest', rr, None), ('random ranges, hint 0', rr, 0)]
                if L >= 64:
                    cases.append(('7 per-image ranges', image_ranges(N, 7, L)[0], None))
            for name, ranges, hint in cases:
                want = LP.score_cpu(costs, pool, offsets, table, ranges)
                got = _run(costs, ranges, pool_d, int(pool.size), off_d, L, table_d, hint)
                out.append(_keys_same('posterior[L=%d, N=%d, %s] == score_cpu' % (L, N, name), got, want,
                                      '(%d words scorable)' % int(lex.ok.sum())))
            if N == 1 and L == 1:
                want = LP.score_cpu(costs, pool, offsets, table)
                out.append(rec('posterior[L=1]: no runner-up', 0 if int(want[0, 1]) == LX.NONE_KEY and int(want[0, 0]) != LX.NONE_KEY else 1, 0))
    return out


def check_search_edges():
    """duplicates across a slice boundary (one query against 2 049 words is cut into 9 slices of 228: the same spelling planted at
    indices 227 and 228, and at 0 and 2 048), an all-unscorable lexicon, costs all at COST_CAP, a single-word range, an empty range"""
    from tests.gpu_checks import rec
    out = []
    rng = np.random.RandomState(11)
    words = [random_word(rng, 6, 12, MGP_CHARS) for _ in range(2049)]
    words[227] = words[228] = 'slice'
    words[0] = words[2048] = 'edges'
    pool, offsets, table, pool_d, off_d, table_d = _device_lexicon(words)
    costs = np.full((2, 26, 38), 9000, dtype=np.int32)
    for i, ch in enumerate('slice'):
        costs[0, i, 2 + MGP_CHARS.index(ch)] = 3
    for i, ch in enumerate('edges'):
        costs[1, i, 2 + MGP_CHARS.index(ch)] = 3
    costs[:, 5, 1] = 1
    got = _run(costs, None, pool_d, int(pool.size), off_d, len(words), table_d)
    want = LP.score_cpu(costs, pool, offsets, table)
    out.append(_keys_same('posterior: duplicates across slice boundaries == score_cpu', got, want))
    idx, score = LP.unpack_post(got)
    ok = idx.tolist() == [[227, 228], [0, 2048]] and score.tolist() == [[16, 16], [16, 16]]
    out.append(rec('posterior: best = the lower index, runner-up = the other, equal score', 0 if ok else 1, 0, '%s %s' % (idx.tolist(), score.tolist())))
    cap = np.full((3, 26, 38), LP.COST_CAP, dtype=np.int32)
    got = _run(cap, None, pool_d, int(pool.size), off_d, len(words), table_d)
    out.append(_keys_same('posterior: every cost at COST_CAP == score_cpu', got, LP.score_cpu(cap, pool, offsets, table)))
    ranges = [(5, 6), (9, 9)]
    got = _run(costs, ranges, pool_d, int(pool.size), off_d, len(words), table_d)
    out.append(_keys_same('posterior: a single-word and an empty range == score_cpu', got, LP.score_cpu(costs, pool, offsets, table, ranges)))
    ok = int(got.view(np.uint64)[0, 1]) == LX.NONE_KEY and (got.view(np.uint64)[1] == np.uint64(LX.NONE_KEY)).all()
    out.append(rec('posterior: no runner-up in a single-word range, no key in an empty one', 0 if ok else 1, 0))
    bad_words = ['a-b', '--', 'x' * 26, '-']
    p2, o2, t2, p2d, o2d, t2d = _device_lexicon(bad_words, MGP_CHARS + '-')
    got = _run(costs, None, p2d, int(p2.size), o2d, len(bad_words), t2d)
    ok = (got.view(np.uint64) == np.uint64(LX.NONE_KEY)).all() and (LP.score_cpu(costs, p2, o2, t2) == np.uint64(LX.NONE_KEY)).all()
    out.append(rec('posterior: an all-unscorable lexicon leaves both keys NONE_KEY', 0 if ok else 1, 0))
    return out


def check_hostile_descriptors():
    """falling and overlong offsets, pool_bytes 0, ranges outside [0, L], null pointers and negative counts straight through ops: an
    error code, or the specification's answer under its clamping rules; the canary words round best and work stay intact.  The
    buffers are sized so that even an unclamped read would stay inside allocated memory."""
    import torch
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV, rec
    out = []
    words = post_lexicon(300, seed=7)
    L = len(words)
    pool, offsets, table = encode(words)
    N = 8
    costs = random_costs(N, seed=3)
    costs_d = torch.from_numpy(costs).to(DEV)
    table_d = torch.from_numpy(table).to(DEV)
    pool_d = torch.from_numpy(np.concatenate([pool, np.full(1 << 16, 5, dtype=np.uint8)])).to(DEV)
    CANARY = 0x5a5a5a5a5a5a5a5a
    nw = 2 * (N + ops.LEXICON_POST_WORK_SLICES)

    def run(off, lo=None, hi=None, pool_bytes=int(pool.size), hint=0, **kw):
        off_pad = np.concatenate([np.zeros(64, dtype=np.int32), off, np.full(4096, off[-1], dtype=np.int32)])
        off_d = torch.from_numpy(off_pad).to(DEV)[64:]
        best_buf = torch.full((2 * N + 16,), CANARY, dtype=torch.int64, device=DEV)
        work_buf = torch.full((nw + 16,), CANARY, dtype=torch.int64, device=DEV)
        args = dict(costs=costs_d, q_lo=None if lo is None else torch.from_numpy(np.asarray(lo, dtype=np.int32)).to(DEV),
                    q_hi=None if hi is None else torch.from_numpy(np.asarray(hi, dtype=np.int32)).to(DEV), pool=pool_d, pool_bytes=pool_bytes,
                    offsets=off_d, L=L, class_table=table_d, range_hint=hint, best=best_buf[8:8 + 2 * N].view(N, 2), work=work_buf[8:8 + nw])
        args.update(kw)
        try:
            ops.lexicon_posterior(**args)
            refused = False
        except RuntimeError:
            refused = True
        torch.cuda.synchronize()
        b, w = best_buf.cpu().numpy(), work_buf.cpu().numpy()
        intact = bool((b[:8] == CANARY).all() and (b[8 + 2 * N:] == CANARY).all() and (w[:8] == CANARY).all() and (w[8 + nw:] == CANARY).all())
        untouched = bool((b == CANARY).all() and (w == CANARY).all())
        return refused, b[8:8 + 2 * N].reshape(N, 2), intact, untouched

    def answered(name, off, lo=None, hi=None, pool_bytes=int(pool.size), hint=0):
        refused, got, intact, _ = run(off, lo, hi, pool_bytes, hint)
        ranges = None if lo is None else np.stack([np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)], 1)
        want = LP.score_cpu(costs, pool, off, table, ranges, pool_bytes=pool_bytes)
        out.append(rec('posterior hostile[%s]: answered' % name, 1 if refused else 0, 0))
        out.append(_keys_same('posterior hostile[%s] == score_cpu under the clamping rules' % name, got, want))
        out.append(rec('posterior hostile[%s]: canaries round best and work intact' % name, 0 if intact else 1, 0))
        return got

    falling = offsets.copy()
    falling[40:80] = falling[40:80][::-1]
    falling[100] = -77
    answered('falling offsets', falling)
    overlong = offsets.copy()
    overlong[150:] += 50000                                            # beyond pool_bytes, inside the allocation
    overlong[200] = 2 ** 31 - 1
    answered('overlong offsets', overlong)
    got = answered('pool_bytes 0', offsets, pool_bytes=0)
    ok = all(int(got.view(np.uint64)[q, 0]) == (int(costs[q, 0, 1]) << 32) and int(got.view(np.uint64)[q, 1]) == ((int(costs[q, 0, 1]) << 32) | 1) for q in range(N))
    out.append(rec('posterior hostile[pool_bytes 0]: every word is the empty word', 0 if ok else 1, 0))
    lo = [0, -50, 10, 250, 200, L, 0, -2 ** 31]
    hi = [L, 40, L + 100000, 2 ** 31 - 1, 100, L + 7, 0, 2 ** 31 - 1]
    got = answered('ranges outside [0, L], inverted, empty', offsets, lo, hi, hint=L)
    none = got.view(np.uint64) == np.uint64(LX.NONE_KEY)
    out.append(rec('posterior hostile: inverted, past-the-end and empty ranges leave NONE_KEY', 0 if none[[4, 5, 6]].all() and not none[[0, 1, 2, 3, 7], 0].any() else 1, 0))
    for name, kw in (('costs null', dict(costs=None, n=N)), ('pool null', dict(pool=None)), ('offsets null', dict(offsets=None)),
                     ('class_table null', dict(class_table=None)), ('q_hi without q_lo', dict(q_hi=torch.zeros(N, dtype=torch.int32, device=DEV))),
                     ('n = -1', dict(n=-1)), ('n = 0', dict(n=0)), ('L = -5', dict(L=-5)), ('L = 0', dict(L=0)), ('pool_bytes = -1', dict(pool_bytes=-1)),
                     ('range_hint = -1', dict(range_hint=-1))):
        refused, _, _, untouched = run(offsets, **kw)
        out.append(rec('posterior hostile[%s]: an argument error, nothing written' % name, 0 if refused and untouched else 1, 0))
    x = torch.zeros(2, 27, 38, device=DEV)
    for name, call in (('logits null', lambda: ops.logprob_costs(None, costs=torch.empty(2, 26, 38, dtype=torch.int32, device=DEV),
                                                                 greedy=torch.empty(2, 2, dtype=torch.int32, device=DEV), n=2)),
                       ('n = -3', lambda: ops.logprob_costs(x, n=-3)), ('n = 0', lambda: ops.logprob_costs(x, n=0))):
        try:
            call()
            refused = False
        except RuntimeError:
            refused = True
        out.append(rec('logprob_costs hostile[%s]: an argument error' % name, 0 if refused else 1, 0))
    return out


def check_matcher():
    """PosteriorMatcher: one chunk and chunks of 100, per-image ranges, a side stream, the acceptance rule; a CPU device is refused"""
    import torch
    from tests.gpu_checks import DEV, rec
    out = []
    words = post_lexicon(1237, seed=3)
    pool, offsets, table = encode(words)
    x = random_logits(333, 6.0, seed=4)
    xd = torch.from_numpy(x).to(DEV)
    m = LX.LexiconMatcher(DEV, words, MGP_CHARS)
    post = LP.PosteriorMatcher(m)
    post.keep_costs = True
    best, greedy = post.score(xd)
    costs = post.last_costs[0].cpu().numpy()
    diff = np.abs(costs.astype(np.int64) - LP.costs_cpu(x))
    out.append(rec('PosteriorMatcher: device costs within one unit of costs_cpu', int(diff.max()), 1))
    want = LP.score_cpu(costs, pool, offsets, table)
    out.append(_keys_same('PosteriorMatcher: L = 1238, N = 333 == score_cpu(device costs)', best, want, '%d chunk' % post.last_chunks))
    out.append(rec('PosteriorMatcher: greedy == greedy_cpu(device costs)', int((greedy != LP.greedy_cpu(costs)).sum()), 0))
    m100 = LX.LexiconMatcher(DEV, words, MGP_CHARS, chunk=100)
    p100 = LP.PosteriorMatcher(m100)
    ranges = image_ranges(333, 5, len(words))[0]
    b100, g100 = p100.score(xd, ranges)
    out.append(_keys_same('PosteriorMatcher: chunks of 100 with per-image ranges', b100, LP.score_cpu(costs, pool, offsets, table, ranges)))
    out.append(rec('PosteriorMatcher: 333 queries in 4 chunks of 100', abs(p100.last_chunks - 4) + int((g100 != greedy).sum()), 0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b_side, _ = post.score(xd)
    side.synchronize()
    out.append(_keys_same('PosteriorMatcher: on a side stream', b_side, want))
    res = post(xd, min_prob=1e-3, min_margin=0.5)
    idx, score = LP.unpack_post(want)
    bad = 0
    for d, (i, j), (s, t) in zip(res, idx.tolist(), score.tolist()):
        keep = i >= 0 and LP.accept_post(s, t if j >= 0 else None, 1e-3, 0.5)
        bad += int(d['index'] != i or d['word'] != (words[i] if keep else None) or d['second'] != ((j, t) if j >= 0 else None))
    out.append(rec('PosteriorMatcher: __call__ words, indices, runner-ups and acceptance', bad, 0,
                   '%d of %d accepted' % (sum(1 for d in res if d['word'] is not None), len(res))))
    return out


def _post_bad(records, prefix, costs, lists, alphabet, min_prob=None, min_margin=None):
    """mismatches between the records' posterior keys and score_cpu / greedy_cpu / accept_post on the device's costs (record order)"""
    bad = k = 0
    for b, recs in enumerate(records):
        words = lists[b]
        pool, offsets, table = encode(words, alphabet)
        for r in recs:
            c = costs[k:k + 1]
            k += 1
            idx, score = LP.unpack_post(LP.score_cpu(c, pool, offsets, table))
            gc, _ = LP.greedy_cpu(c)[0].tolist()
            (i, j), (s, t) = idx[0].tolist(), score[0].tolist()
            if i < 0:
                want = {prefix: None, prefix + '_index': -1, prefix + '_logp': None, prefix + '_second': None, prefix + '_gap': None}
            else:
                ok = LP.accept_post(s, t if j >= 0 else None, min_prob, min_margin)
                want = {prefix: words[i] if ok else None, prefix + '_index': i, prefix + '_logp': -s / 1024.0,
                        prefix + '_second': (j, -t / 1024.0) if j >= 0 else None, prefix + '_gap': (s - gc) / 1024.0}
            bad += int(any(r.get(key, 'missing') != v for key, v in want.items()) or (prefix + '_dist') in r)
    return bad, k


def check_end_to_end(dtype_name='fp32'):
    """MGPSTR.recognize(lexicon=...) and spot_and_recognize(crop='polygon', lexicon=..., lexicon_mode='posterior') on the synthetic
    models of gpu_checks_lexicon.check_end_to_end: records minus the new keys equal those of the call without them, the new keys equal
    score_cpu / greedy_cpu / accept_post on the costs the device produced for those crops, `lex*` equals the 'edit' call's"""
    import torch
    from advancedliteratemachinery_amd.engine.two_stage import spot_and_recognize
    from advancedliteratemachinery_amd.utils import synthetic as weights
    from advancedliteratemachinery_amd.utils.parser import make_args
    from oracle import mgp_str_ref as R
    from tests.gpu_checks import DEV, ENGINES, build_model, rec
    from tests.gpu_checks_lexicon import _strip, synthetic_lexicon
    from tests.gpu_checks_mgp import build
    dtype = ENGINES[dtype_name]
    depths = (2, 2, 2, 2)
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, pt_seq_length=6, test_min_size=64, test_max_size=112)
    sd = weights.make_state_dict(args, seed=5, depths=depths)
    omni = build_model(args, sd, depths, dtype)
    c = R.cfg(depth=2)
    mgp = build(c, R.make_state_dict(c, seed=17), dtype)
    rng = np.random.RandomState(3)
    images = [torch.from_numpy(rng.randint(0, 256, (90, 140, 3), dtype=np.uint8)), torch.from_numpy(rng.randint(0, 256, (70, 100, 3), dtype=np.uint8))]
    shared = synthetic_lexicon(400, seed=8, max_len=12) + synthetic_lexicon(200, seed=9, max_len=8, chars=MGP_CHARS)
    lists = [shared[:250], shared[250:]]
    LEX = ('lex', 'lex_index', 'lex_dist')
    POST = ('mgp_lex', 'mgp_lex_index', 'mgp_lex_logp', 'mgp_lex_second', 'mgp_lex_gap')
    out = []
    tag = 'posterior e2e[%s]' % dtype_name

    # MGPSTR.recognize
    batch = torch.from_numpy(rng.rand(5, 3, 32, 128).astype(np.float32)).to(DEV)
    plain = mgp.recognize(batch)
    matcher = LX.LexiconMatcher(DEV, shared, MGP_CHARS)
    post = LP.posterior_of(matcher)
    post.keep_costs = True
    got = mgp.recognize(batch, lexicon=matcher, lexicon_min_prob=1e-30, lexicon_min_margin=0.01)
    costs = post.last_costs[0].cpu().numpy()
    keys = ('lex', 'lex_index', 'lex_logp', 'lex_second', 'lex_gap')
    out.append(rec(tag + ': recognize minus the new keys unchanged', 0 if [{k: v for k, v in r.items() if k not in keys} for r in got] == plain else 1, 0))
    bad, n = _post_bad([got], 'lex', costs, [shared], MGP_CHARS, 1e-30, 0.01)
    out.append(rec(tag + ': recognize lex keys == score_cpu / greedy_cpu / accept_post on the device costs', bad + int(n != 5), 0))
    again = mgp.recognize(batch)
    out.append(rec(tag + ': the default recognize call is unchanged', 0 if again == plain else 1, 0))
    res, logits = mgp.recognize(batch, char_logits=True)
    diff = np.abs(LP.costs_cpu(logits.cpu().numpy()).astype(np.int64) - costs)
    out.append(rec(tag + ': the device costs are those of the returned character logits', int(diff.max()) + (0 if res == plain else 2), 1))

    # spot_and_recognize
    base, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon')
    n_words = sum(len(r) for r in base)
    out.append(rec(tag + ': words spotted', 0 if n_words > 0 else 1, 0, '%d words' % n_words))
    for name, make, per in (('shared list', lambda: LX.LexiconMatcher(DEV, shared, MGP_CHARS), [shared, shared]),
                            ('per-image lists', lambda: LX.LexiconMatcher.from_lists(DEV, lists, MGP_CHARS), lists)):
        m = make()
        edit, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon', lexicon=m, lexicon_max_dist=3)
        p = LP.posterior_of(m)
        p.keep_costs = True
        got, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon', lexicon=m, lexicon_max_dist=3, lexicon_mode='posterior',
                                       lexicon_min_margin=0.25)
        out.append(rec('%s[%s]: one posterior call, one chunk' % (tag, name), abs(p.last_chunks - 1), 0))
        costs = p.last_costs[0].cpu().numpy()
        out.append(rec('%s[%s]: records minus the new keys unchanged' % (tag, name), 0 if _strip(got, LEX + POST) == base else 1, 0))
        out.append(rec('%s[%s]: lex keys equal the edit call\'s' % (tag, name),
                       0 if _strip(got, POST) == _strip(edit, ('mgp_lex', 'mgp_lex_index', 'mgp_lex_dist')) else 1, 0))
        bad, n = _post_bad(got, 'mgp_lex', costs, per, MGP_CHARS, None, 0.25)
        out.append(rec('%s[%s]: mgp_lex keys == score_cpu / greedy_cpu / accept_post on the device costs' % (tag, name), bad + int(n != n_words), 0,
                       '%d words, %d accepted' % (n, sum(1 for recs in got for r in recs if r['mgp_lex'] is not None))))
    again, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon')
    out.append(rec(tag + ': the default call is unchanged', 0 if again == base else 1, 0))
    raw, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon', lexicon=lists, lexicon_mode='posterior')
    out.append(rec(tag + ': raw per-image lists give the keys too', 0 if all(set(POST) <= set(r) and 'mgp_lex_dist' not in r and 'lex_dist' in r
                                                                        for recs in raw for r in recs) else 1, 0))
    return out


def check_timing():
    """tools/lexicon_post_bench.py: 512 queries against 90 000 words, the median of 30 device calls after 5 at or below score_cpu's
    time for the same 512 queries (timed on 32 of them and scaled linearly), with no margin"""
    import os
    import sys
    from tests.gpu_checks import rec
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import lexicon_post_bench
    r = lexicon_post_bench.measure(queries=512, words=90000, calls=30, warmup=5, cpu_queries=32)
    note = 'device p10 / median / p90 %.3f / %.3f / %.3f ms; entry point %.3f ms; score_cpu %.1f ms for %d queries -> %.1f ms for %d; omp_lexicon_nearest %.3f ms' % (
        r['device_ms']['p10'], r['device_ms']['median'], r['device_ms']['p90'], r['entry_ms']['median'], r['cpu_ms_measured'], r['cpu_queries'],
        r['cpu_ms_scaled'], r['queries'], r['nearest_entry_ms']['median'])
    print(note)
    return [rec('posterior: 512 x 90 000, device median <= score_cpu (32 queries, scaled)', r['device_ms']['median'], r['cpu_ms_scaled'], note),
            rec('posterior: the bench outputs equal score_cpu on the timed subset', 0 if r['outputs_equal'] else 1, 0),
            rec('posterior: one query chunk', abs(r['chunks'] - 1), 0)]
