"""GPU checks of page expressions: omp_page_regex_search against search_cpu (utils/page_regex.py) on every integer
at the edges of chunks, rounds and byte tables, with carries that cross lanes and rounds, hits whose decision needs the next owner's first
column, starts in other chunks and rounds, at the page length limit, the order of the hits, what the entry point refuses, find_regex on
the device against the host searcher on the records of a real engine call, and the structural time gate.  Every check returns records
{name, err, tol, ok, note} like tests/gpu_checks.py."""
import copy
import re
import statistics
import time

import numpy as np
import torch

from advancedliteratemachinery_amd.utils import page_regex as PR

C = PR.CHUNK
R = PR.ROUND
POS = (1, 8, 9, 16, 17, 63, 64)                                             # the byte-table edges
SHORT = (0, 1, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1)
LONG = (R - 1, R, R + 1)
GARBAGE = 0x5a5a5a5a


def random_mask(rng, P, sigma, density):
    """uint64 [sigma + 1]: every position's class holds each code with probability `density` and at least one code"""
    member = rng.rand(sigma, P) < density
    member[rng.randint(0, sigma, P), np.arange(P)] = True
    mask = np.zeros(sigma + 1, dtype=np.uint64)
    for i in range(P):
        mask[:sigma] |= member[:, i].astype(np.uint64) << np.uint64(i)
    return mask


def automaton(mask, first, last, follow):
    """the words of one expression; pred is follow transposed"""
    rows = [int(f) for f in follow] + [0] * (PR.POS_MAX - len(follow))
    return dict(mask=mask, first=int(first), last=int(last), follow=rows, pred=PR._transpose(rows), P=len(follow))


def random_automaton(rng, P, mask):
    """any (first, last, follow) below P is an input of the definition: position i goes on to i + 1 (so that states cross every byte of
    the word), to itself (a loop, so that carries live long) and to a random position, each with its own probability"""
    bit = lambda: 1 << int(rng.randint(0, P))                                # noqa: E731
    follow = []
    for i in range(P):
        f = (1 << ((i + 1) % P)) if rng.rand() < 0.8 else 0
        f |= (1 << i) if rng.rand() < 0.25 else 0
        f |= bit() if rng.rand() < 0.4 else 0
        follow.append(f)
    return automaton(mask, bit() | (bit() if rng.rand() < 0.5 else 0), bit() | bit() | (1 << (P - 1)), follow)


def literal(codes, width):
    """the automaton of a literal: position i holds code codes[i] alone and goes on to i + 1"""
    P = len(codes)
    mask = np.zeros(width, dtype=np.uint64)
    for i, c in enumerate(np.asarray(codes).tolist()):
        mask[c] |= np.uint64(1) << np.uint64(i)
    return automaton(mask, 1, 1 << (P - 1), [(1 << (i + 1)) if i + 1 < P else 0 for i in range(P)])


def _variants():
    """(name, sigma, make_mask(rng, P), make_text(rng, n))"""
    def rand(sigma, density):
        return lambda rng, P: random_mask(rng, P, sigma, density)

    def text(sigma):
        return lambda rng, n: rng.randint(0, sigma, n).astype(np.uint8)
    every = lambda rng, P: np.asarray([(1 << P) - 1, 0], dtype=np.uint64)                                      # noqa: E731
    half = lambda rng, P: np.asarray([(1 << P) - 1, sum(1 << i for i in range(0, P, 2)), 0], dtype=np.uint64)   # noqa: E731
    return [('one code in every class, sigma=1', 1, every, text(1)),
            ('random sigma=2', 2, rand(2, 0.6), text(2)),
            ('random sigma=26', 26, rand(26, 0.3), text(26)),
            ('random sigma=254', 254, rand(254, 0.15), text(254)),
            ('a text of codes at or above sigma', 26, rand(26, 0.5), lambda rng, n: rng.randint(26, 256, n).astype(np.uint8)),
            ('a code in every class, a code in every other', 2, half, text(2))]


def edge_cases(seed=0):
    """-> [(variant, sigma, [(automaton, t), ...])]: per variant and P one random automaton against a text of every short length and of one
    of the lengths around a round of the wave, rotating, so that every variant holds every length"""
    rng = np.random.RandomState(seed)
    cases = []
    for v, (name, sigma, make_mask, make_text) in enumerate(_variants()):
        jobs = []
        for i, P in enumerate(POS):
            a = random_automaton(rng, P, make_mask(rng, P))
            for n in SHORT + (LONG[(i + v) % 3],):
                jobs.append((a, make_text(rng, n)))
        cases.append((name, sigma, jobs))
    return cases


def pack(specs, sigma):
    """[(automaton, t)] -> [pool, page_off, page_len, masks [Q, sigma + 1], first, last, follow, pred, pat_len, jobs]: texts and automata
    that are the same object get one page and one expression.  A mask table narrower than sigma + 1 is padded with zeros: its codes at
    or above its own sigma are in no class either way."""
    chunks, total = [], 0
    pages, exprs, jobs = {}, {}, []
    po, pl, masks, autos = [], [], [], []
    for a, t in specs:
        if id(t) not in pages:
            pages[id(t)] = len(pages)
            po.append(total)
            pl.append(len(t))
            chunks.append(np.asarray(t, dtype=np.uint8))
            total += len(t)
        if id(a) not in exprs:
            exprs[id(a)] = len(exprs)
            row = np.zeros(sigma + 1, dtype=np.uint64)
            keep = min(len(a['mask']) - 1, sigma)
            row[:keep] = a['mask'][:keep]
            masks.append(row)
            autos.append(a)
        jobs.append((pages[id(t)], exprs[id(a)]))
    i32 = lambda v: np.asarray(v, dtype=np.int32)                            # noqa: E731
    u64 = lambda v: np.asarray(v, dtype=np.uint64)                           # noqa: E731
    return [np.concatenate(chunks + [np.zeros(0, np.uint8)]), i32(po), i32(pl), np.stack(masks), u64([a['first'] for a in autos]), u64([a['last'] for a in autos]),
            u64([a['follow'] for a in autos]).reshape(-1, 64), u64([a['pred'] for a in autos]).reshape(-1, 64), i32([a['P'] for a in autos]), i32(jobs).reshape(-1, 2)]


def from_strings(texts, exprs, jobs):
    """page strings, expression strings and (page, expression) pairs -> the list pack() gives"""
    enc = PR.encode_regex(texts, exprs)
    return list(enc[:9]) + [np.asarray(jobs, dtype=np.int32).reshape(-1, 2)]


_EDGE = {}


def edge_reference():
    """the cases, all of them packed into one call, and search_cpu on it at max_hits 64 and 1: computed once and shared by the checks.
    search_cpu judges every job by itself, so a variant's own answer is its slice of the mixed call's."""
    if not _EDGE:
        cases = edge_cases()
        specs = [j for _, _, jobs in cases for j in jobs]
        _EDGE.update(cases=cases, specs=specs, packed=pack(specs, PR.SIGMA_MAX))
        _EDGE['want'] = {H: PR.search_cpu(*_EDGE['packed'], H) for H in (64, 1)}
    return _EDGE


def _bad(got, want):
    bad = 0
    for key in ('best', 'n_hits', 'hits'):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        bad += int((g != w).sum()) if g.shape == w.shape else 1 << 20
    return bad


def _slice(res, lo, hi):
    return {k: v[lo:hi] for k, v in res.items()}


def _device(packed):
    from tests.gpu_checks import DEV
    pool, po, pl, masks, first, last, follow, pred, P, jobs = packed
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)          # noqa: E731
    i64 = lambda x: t(np.ascontiguousarray(x).reshape(-1).view(np.int64))    # noqa: E731
    return dict(pool=t(np.concatenate([pool, np.zeros(1, np.uint8)])), po=t(po), pl=t(pl), masks=i64(masks), first=i64(first), last=i64(last), follow=i64(follow),
                pred=i64(pred), P=t(P), jobs=t(jobs.reshape(-1)))


def run_raw(packed, H, tabs=None):
    """ops.page_regex_search on output buffers prefilled with garbage -> the dict of search_cpu"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV
    d = _device(packed) if tabs is None else tabs
    J, sigma = packed[9].shape[0], packed[3].shape[1] - 1
    outs = [torch.full((n,), GARBAGE, dtype=torch.int32, device=DEV) for n in (2 * J, J, 3 * H * J)]
    best, n_hits, hits = ops.page_regex_search(d['pool'], packed[0].size, d['po'], d['pl'], d['masks'], d['first'], d['last'], d['follow'], d['pred'], d['P'], d['jobs'],
                                               sigma, H, best=outs[0], n_hits=outs[1], hits=outs[2])
    return dict(best=best.cpu().numpy(), n_hits=n_hits.cpu().numpy(), hits=hits.cpu().numpy())


def check_edges():
    from tests.gpu_checks import DEV, rec
    E = edge_reference()
    want = E['want'][64]
    out, lo = [], 0
    for name, sigma, jobs in E['cases']:
        hi = lo + len(jobs)
        w = _slice(want, lo, hi)
        got = run_raw(pack(jobs, sigma), 64)
        out.append(rec('page regex[%s] alone, sigma=%d: %d jobs == search_cpu' % (name, sigma, len(jobs)), _bad(got, w), 0,
                       'n_hits %d .. %d, %d jobs with an end' % (int(w['n_hits'].min()), int(w['n_hits'].max()), int((w['best'][:, 1] > 0).sum()))))
        lo = hi
    packed = E['packed']
    for H in (64, 1):
        w = E['want'][H]
        got = run_raw(packed, H)
        out.append(rec('page regex: all variants in one call of %d jobs, max_hits %d == search_cpu' % (len(E['specs']), H), _bad(got, w), 0,
                       '%d jobs with more hits than are kept' % int((w['n_hits'] > H).sum())))
        out.append(rec('page regex: max_hits %d is exceeded by some job' % H, 0 if (w['n_hits'] > H).any() else 1, 0, 'most %d' % int(w['n_hits'].max())))
    sc = PR.RegexSearcher(DEV)
    got = sc.run(*packed, 64)
    out.append(rec('page regex: the mixed call through RegexSearcher == search_cpu', _bad(got, want) + abs(sc.chunks - 1), 0, '%d hits' % int(want['n_hits'].sum())))
    # the cases cover what they claim to cover
    seen = {(a['P'], len(t)) for a, t in E['specs']}
    miss = sum((P, n) not in seen for P in POS for n in SHORT) + sum(not any((P, n) in seen for P in POS) for n in LONG) + sum(not any((P, n) in seen for n in LONG) for P in POS)
    for name, _, jobs in E['cases']:
        miss += len({len(t) for _, t in jobs} & set(LONG)) != 3
    out.append(rec('page regex: the cases hold every short length per P, and every variant every length around a round', miss, 0, '%d (P, n)' % len(seen)))
    some = sum(int((_slice(want, i * len(E['cases'][0][2]), (i + 1) * len(E['cases'][0][2]))['n_hits'] > 0).sum()) > 0 for i in range(len(E['cases'])))
    out.append(rec('page regex: every variant but the text above sigma has hits', abs(some - (len(E['cases']) - 1)), 0, '%d variants' % some))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# carries, hit decisions across owners, starts: real expressions on planted texts
# ---------------------------------------------------------------------------------------------------------------------------------
def _planted(n, plants, pad='x'):
    """a text of n pad characters with strings planted at 1-based columns: [(first column, string)]"""
    t = [pad] * n
    for col, s in plants:
        assert 1 <= col and col - 1 + len(s) <= n
        t[col - 1:col - 1 + len(s)] = list(s)
    return ''.join(t)


def _run(lo, hi):
    """a run of digits over the columns lo .. hi"""
    return (lo, '7' * (hi - lo + 1))


def carry_cases():
    """-> (texts, expressions, [(what, page, expression, the hits it must have or None)])"""
    texts, exprs, jobs = [], [], []

    def add(what, text, src, hits=None):
        if text not in texts:
            texts.append(text)
        if src not in exprs:
            exprs.append(src)
        jobs.append((what, texts.index(text), exprs.index(src), hits))
    word = 'abcabd'
    # -- carry --
    add('a bounded expression across a 128-column edge', _planted(300, [(C - 2, word)]), word, [(C + 3, 0, C - 3)])
    add('a bounded expression across the 8192 edge', _planted(R + 300, [(R - 2, word)]), word, [(R + 3, 0, R - 3)])
    add('a digit run of 300 characters: three lanes', _planted(700, [_run(100, 399)]), r'\d+', [(399, 0, 99)])
    add('a digit run of 9000 characters: across a round', _planted(9500, [_run(100, 9099)]), r'\d+', [(9099, 0, 99)])
    for n in (C + 1, R + 1, 20000):
        add('a.*b with a at column 1 and b at column %d: the never-dying carry' % n, 'a' + 'x' * (n - 2) + 'b', r'a.*b', [(n, 0, 0)])
    add('a carried state that is a subset of the speculative one', 'ab' * 600, r'(a|b)+', [(1200, 0, 0)])
    add('a loop inside a bounded tail, planted in every lane of a round', _planted(R, [(1 + C * l + (l % 7), 'ab' * (20 + 9 * (l % 13)) + 'c') for l in range(0, 64, 2)]), r'(ab)+c')
    # -- hit decisions across owners --
    add('a run of ends across column 128 / 129', _planted(400, [_run(120, 135)]), r'\d+', [(135, 0, 119)])
    add('a run of ends that stops exactly at 128', _planted(400, [_run(120, C)]), r'\d+', [(C, 0, 119)])
    add('a single end at 128 and one at 129', _planted(400, [_run(C, C), _run(C + 2, C + 2)]), r'\d+', [(C, 0, C - 1), (C + 2, 0, C + 1)])
    add('a run of ends across 8192 / 8193', _planted(R + 200, [_run(R - 5, R + 5)]), r'\d+', [(R + 5, 0, R - 6)])
    add('a run that stops exactly at 8192, a non-end after it: the pending end is a hit', _planted(R + 200, [_run(R - 5, R), _run(R + 2, R + 3)]), r'\d+',
        [(R, 0, R - 6), (R + 3, 0, R + 1)])
    add('a pending end at 8192 followed by an end', _planted(R + 200, [_run(R, R + 1)]), r'\d+', [(R + 1, 0, R - 1)])
    add('a run that stops exactly at n = 8192', _planted(R, [_run(R - 5, R)]), r'\d+', [(R, 0, R - 6)])
    add('a run that stops exactly at n = 16384: the last column of the second round', _planted(2 * R, [_run(R, R), _run(2 * R - 3, 2 * R)]), r'\d+',
        [(R, 0, R - 1), (2 * R, 0, 2 * R - 4)])
    add('a run that reaches n', _planted(333, [_run(300, 333)]), r'\d+', [(333, 0, 299)])
    add('a run of ends across column 64 / 65: the two words of a lane', _planted(300, [_run(60, 70)]), r'\d+', [(70, 0, 59)])
    add('single ends at 1, 64, 66, 126, 128 and 130', _planted(300, [_run(c, c) for c in (1, 64, 66, 126, 128, 130)]), r'\d', [(c, 0, c - 1) for c in (1, 64, 66, 126, 128, 130)])
    # -- starts --
    add('a start in the same chunk', _planted(400, [(150, 'a77b')]), r'a\d+b', [(153, 0, 149)])
    add('a start in the previous chunk', _planted(400, [(100, 'a' + '7' * 60 + 'b')]), r'a\d+b', [(161, 0, 99)])
    add('a start in the previous round', _planted(R + 400, [(R - 100, 'a' + '7' * 200 + 'b')]), r'a\d+b', [(R + 101, 0, R - 101)])
    add('a start at 0', _planted(400, [(1, 'a' + '7' * 140 + 'b')]), r'a\d+b', [(142, 0, 0)])
    amb = _planted(300, [(C - 6, 'xab abcd ac'), (200, 'abc xbc')])
    add('the longest of several starts: (a|ab)(c|bcd)?', amb, r'(a|ab)(c|bcd)?', [(C - 4, 0, C - 6), (C + 1, 0, C - 3), (C + 4, 0, C + 2), (202, 0, 199)])
    add('the longest of several starts: (b|ab)c', amb, r'(b|ab)c', [(C, 0, C - 3), (202, 0, 199), (206, 0, 204)])
    add('an amount with thousands groups across an edge', _planted(400, [(C - 8, ' 1,234,567.89 ')]), r'\d{1,3}(,\d{3})*\.\d{2}', [(C + 4, 0, C - 8)])
    return texts, exprs, jobs


def check_carry():
    from tests.gpu_checks import rec
    texts, exprs, jobs = carry_cases()
    packed = from_strings(texts, exprs, [(p, q) for _, p, q, _ in jobs])
    out = []
    for H in (64, 1):
        want = PR.search_cpu(*packed, H)
        got = run_raw(packed, H)
        for j, (what, _, _, hits) in enumerate(jobs):
            w = _slice(want, j, j + 1)
            out.append(rec('page regex[%s], max_hits %d == search_cpu' % (what, H), _bad(_slice(got, j, j + 1), w), 0,
                           'n_hits %d, first hits %s' % (int(w['n_hits'][0]), w['hits'][0][:3].tolist())))
            if H == 64 and hits is not None:                                # the case is what it says it is: the definition finds the planted hits
                rows = [tuple(r) for r in w['hits'][0].tolist() if r[0] >= 0]
                out.append(rec('page regex[%s]: the definition has exactly the planted hits' % what, 0 if rows == hits and int(w['n_hits'][0]) == len(hits) else 1, 0,
                               '%s, planted %s' % (rows[:6], hits)))
    return out


def check_limit():
    """one page of 65 535 characters (all 8 rounds): a 64-position literal planted at the start, in the middle and as the last 64
    characters; a loop over the whole page; an expression that occurs nowhere"""
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(4)
    n = PR.LEN_MAX
    t = rng.randint(0, 26, n).astype(np.uint8)
    exact = rng.randint(0, 26, 64).astype(np.uint8)
    places = (0, 30000, n - 64)
    for at in places:
        t[at:at + 64] = exact
    every = np.zeros(28, dtype=np.uint64)
    every[:26] = 1
    nowhere = np.zeros(28, dtype=np.uint64)
    nowhere[26] = np.uint64((1 << 64) - 1)                                   # code 26 in every class; t holds no 26
    packed = pack([(literal(exact, 28), t), (automaton(every, 1, 1, [1]), t), (automaton(nowhere, 1, 1 << 63, [(1 << (i + 1)) % (1 << 64) for i in range(64)]), t)], 27)
    want = PR.search_cpu(*packed, 16)
    got = PR.RegexSearcher(DEV).run(*packed, 16)
    out = [rec('page regex[65535]: == search_cpu', _bad(got, want), 0, 'n_hits %s best %s' % (want['n_hits'].tolist(), want['best'].tolist()))]
    out.append(rec('page regex[65535]: the planted literals are the hits', 0 if want['hits'][0][:3].tolist() == [[at + 64, 0, at] for at in places] and want['n_hits'][0] == 3 else 1, 0))
    out.append(rec('page regex[65535]: a loop over the whole page is one hit from 0 to n', 0 if want['hits'][1][0].tolist() == [n, 0, 0] and want['n_hits'][1] == 1 else 1, 0))
    out.append(rec('page regex[65535]: an expression that occurs nowhere has no hit and (1, 0) as its best', 0 if want['n_hits'][2] == 0 and want['best'][2].tolist() == [1, 0] else 1, 0))
    return out


def check_ordering():
    """64 jobs on one page of 20 000 characters of 4 codes, random automata of 6 positions: hits in many chunks and rounds"""
    from tests.gpu_checks import rec
    rng = np.random.RandomState(6)
    t = rng.randint(0, 4, 20000).astype(np.uint8)
    specs = []
    while len(specs) < 64:
        a = random_automaton(rng, 6, random_mask(rng, 6, 4, 0.0))
        a = automaton(a['mask'], a['first'], 1 << 5, a['follow'][:6])
        if 4 <= len(PR.ends_cpu(PR.Tables(a['mask'], a['first'], a['last'], a['follow'], a['pred'], 6), t[:3000])) <= 12:    # few enough that the kept hits reach far
            specs.append((a, t))
    packed = pack(specs, 4)
    want = PR.search_cpu(*packed, 64)
    got = run_raw(packed, 64)
    again = run_raw(packed, 64)
    ends = got['hits'][:, :, 0]
    kept = np.minimum(got['n_hits'], 64)
    rising = all((np.diff(ends[j, :kept[j]]) > 0).all() for j in range(64))
    spread = min(len(set((ends[j, :kept[j]] // C).tolist())) for j in range(64))
    rounds = max(len(set((ends[j, :kept[j]] // R).tolist())) for j in range(64))
    return [rec('page regex ordering: 64 jobs on one page == search_cpu', _bad(got, want), 0, 'n_hits %d .. %d' % (int(want['n_hits'].min()), int(want['n_hits'].max()))),
            rec('page regex ordering: every hits list ascends', 0 if rising else 1, 0),
            rec('page regex ordering: the kept hits of every job fall in at least 4 chunks, and those of some job in all three rounds', 0 if spread >= 4 and rounds == 3 else 1, 0,
                'least %d chunks, most %d rounds' % (spread, rounds)),
            rec('page regex ordering: the same call again gives identical bytes', 0 if all(got[k].tobytes() == again[k].tobytes() for k in got) else 1, 0)]


def check_refusals():
    """what the entry point refuses comes back as an error code and a message before any launch, and what only the device tables show
    as n_hits = -1; nothing aborts.  Every refused job is in bounds: the kernel rejects it by its own checks."""
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(9)
    t1, t2 = rng.randint(0, 5, 300).astype(np.uint8), rng.randint(0, 5, 40).astype(np.uint8)
    a1, a2 = random_automaton(rng, 4, random_mask(rng, 4, 5, 0.4)), random_automaton(rng, 12, random_mask(rng, 12, 5, 0.4))
    packed = pack([(a1, t1), (a2, t1), (a1, t2), (a2, t2), (a1, t1)], 5)
    pool, po, pl, masks, first, last, follow, pred, P, jobs = packed
    H, J = 4, jobs.shape[0]
    want = PR.search_cpu(*packed, H)
    d = _device(packed)
    out = [rec('page regex: the refusal case itself == search_cpu', _bad(run_raw(packed, H, d), want), 0, str(want['n_hits'].tolist()))]
    res = [torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (2 * J, J, 3 * H * J)]
    args = [ops.ptr(d['pool']), pool.size, ops.ptr(d['po']), ops.ptr(d['pl']), len(pl), ops.ptr(d['masks']), ops.ptr(d['first']), ops.ptr(d['last']), ops.ptr(d['follow']),
            ops.ptr(d['pred']), ops.ptr(d['P']), len(P), ops.ptr(d['jobs']), J, 5, H, ops.ptr(res[0]), ops.ptr(res[1]), ops.ptr(res[2]), ops.stream()]
    for i, what in ((0, 'pool'), (2, 'page_off'), (3, 'page_len'), (5, 'masks'), (6, 'first'), (7, 'last'), (8, 'follow'), (9, 'pred'), (10, 'pat_len'), (12, 'jobs'),
                    (16, 'best'), (17, 'n_hits'), (18, 'hits')):
        a = list(args)
        a[i] = None
        rc = _lib.lib().omp_page_regex_search(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page regex refuses a null %s with an error code' % what, 0 if rc == -22 and 'null pointer' in msg else 1, 0, msg))
    for what, i, v in (('J = 0', 13, 0), ('J = -1', 13, -1), ('J above 2^20', 13, (1 << 20) + 1), ('max_hits 0', 15, 0), ('max_hits 65', 15, 65), ('sigma 255', 14, 255),
                       ('sigma -1', 14, -1), ('no pages', 4, 0), ('no expressions', 11, 0), ('a negative pool', 1, -1),
                       ('masks off their alignment', 5, d['masks'].data_ptr() + 4), ('first off its alignment', 6, d['first'].data_ptr() + 4),
                       ('last off its alignment', 7, d['last'].data_ptr() + 4), ('follow off its alignment', 8, d['follow'].data_ptr() + 4),
                       ('pred off its alignment', 9, d['pred'].data_ptr() + 4)):
        a = list(args)
        a[i] = v
        rc = _lib.lib().omp_page_regex_search(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page regex refuses %s with an error code' % what, 0 if rc == -22 and 'omp_page_regex_search' in msg else 1, 0, msg))
    try:
        ops.page_regex_search(d['pool'], pool.size, d['po'], d['pl'], d['masks'], d['first'], d['last'], d['follow'], d['pred'], d['P'], d['jobs'], 5, 65)
        bad = 1
    except RuntimeError as e:
        bad = 0 if 'omp_page_regex_search' in str(e) and '(-22)' in str(e) and 'max_hits' in str(e) else 1
    out.append(rec('the wrapper raises on max_hits 65', bad, 0))
    torch.cuda.synchronize()
    out.append(rec('page regex: nothing was written by the refused calls', sum(int((r != -7).sum().item()) for r in res), 0))
    # what only the device tables show: the job is refused on the device, its neighbours are answered.  Expressions: 0 = a1 (P 4), 1 = a2
    # (P 12); pages: 0 = t1, 1 = t2; jobs (0, 0) (0, 1) (1, 0) (1, 1) (0, 0)
    top = -(1 << 63)
    for what, key, idx, v, hit in (('P = 0', 'P', 0, 0, (0, 2, 4)), ('P = 65', 'P', 1, 65, (1, 3)), ('P below the bits of the words', 'P', 1, 11, (1, 3)),
                                   ('a first bit at P', 'first', 0, a1['first'] | 1 << 4, (0, 2, 4)), ('a first bit at 63 under P = 12', 'first', 1, top, (1, 3)),
                                   ('a last bit at P', 'last', 1, a2['last'] | 1 << 12, (1, 3)), ('first == 0', 'first', 0, 0, (0, 2, 4)), ('last == 0', 'last', 1, 0, (1, 3)),
                                   ('a follow bit at P', 'follow', 2, a1['follow'][2] | 1 << 4, (0, 2, 4)), ('a follow row at P', 'follow', 4, 1, (0, 2, 4)),
                                   ('a follow row at 63 under P = 12', 'follow', 64 + 63, 1, (1, 3)), ('a pred bit at 63 under P = 12', 'pred', 64 + 3, top, (1, 3)),
                                   ('a pred row at P', 'pred', 64 + 12, 2, (1, 3)),
                                   ('a page of 65536 characters', 'pl', 1, PR.LEN_MAX + 1, (2, 3)), ('a negative page length', 'pl', 0, -1, (0, 1, 4)),
                                   ('a negative offset', 'po', 1, -1, (2, 3)), ('a page range past pool_bytes', 'po', 0, pool.size - 299, (0, 1, 4)),
                                   ('a page that is not there', 'jobs', 0, 2, (0,)), ('a negative page', 'jobs', 8, -1, (4,)),
                                   ('an expression that is not there', 'jobs', 3, 2, (1,)), ('a negative expression', 'jobs', 5, -1, (2,))):
        tabs = dict(d, **{key: d[key].clone()})
        tabs[key][idx] = v
        got = run_raw(packed, H, tabs)
        w = {n: a.copy() for n, a in want.items()}
        for j in hit:
            w['best'][j] = -1
            w['n_hits'][j] = -1
            w['hits'][j] = -1
        out.append(rec('page regex refuses %s on the device: n_hits -1, the other jobs answered' % what, _bad(got, w), 0, str(got['n_hits'].tolist())))
    # the device stage
    try:
        PR.RegexSearcher('cpu')
        bad = 1
    except RuntimeError:
        bad = 0
    out.append(rec('RegexSearcher refuses a device that is not cuda', bad, 0))
    sc = PR.RegexSearcher(DEV)
    ok = dict(zip('pool page_off page_len masks first last follow pred pat_len jobs'.split(), packed), max_hits=4)
    for what, kw in (('a page above the limit', dict(page_len=[PR.LEN_MAX + 1, 40])), ('a range outside the pool', dict(page_off=[0, 301])),
                     ('P = 0', dict(pat_len=[0, 12])), ('max_hits 65', dict(max_hits=65)), ('a first bit at P', dict(first=[16, a2['first']])),
                     ('last == 0', dict(last=[0, a2['last']])), ('a mask table of 256 words', dict(masks=np.zeros((2, 256), np.uint64)))):
        try:
            sc.run(**dict(ok, **kw))
            bad = 1
        except ValueError:
            bad = 0
        out.append(rec('the regex searcher refuses %s on the host' % what, bad, 0))
    empty = sc.run(**dict(ok, jobs=np.zeros((0, 2), np.int32)))
    out.append(rec('the regex searcher on no jobs: empty outputs', 0 if empty['best'].shape == (0, 2) and empty['n_hits'].shape == (0,) and empty['hits'].shape == (0, 4, 3) else 1, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
class _Counting(object):
    def __init__(self, inner):
        self.inner, self.calls = inner, 0

    def run(self, *a, **kw):
        self.calls += 1
        return self.inner.run(*a, **kw)


def engine_expressions(recs):
    """expressions from the call's own records: an alternation of two of its words, and a `+` loop over a class -> [(name, expression)]"""
    from advancedliteratemachinery_amd.utils.page_search import page_index
    text, start, ln = page_index(recs, normalise=None)
    texts = [text[s:s + n] for s, n in zip(start.tolist(), ln.tolist())]
    fit = sorted({w for w in texts if 2 <= len(w) <= 30 and w == ' '.join(w.split())}, key=lambda w: (text.count(w), -len(w), w))
    out = []
    if len(fit) >= 2:
        out.append(('either', '(%s|%s)' % (re.escape(fit[0]), re.escape(fit[1]))))
    out.append(('run', r'[^ ]+'))
    return out


def check_engine_search(dtype_name):
    """the image, weights and call of the page-pattern engine check (windows = [default, 2 x 2 grid], suppress=0.5, reading_order=True,
    blocks=True); find_regex on the device == find_regex with HostRegexSearcher on every field"""
    from advancedliteratemachinery_amd.engine import inference as inf
    from advancedliteratemachinery_amd.engine.search import find_regex
    from advancedliteratemachinery_amd.utils import windows as WN
    from advancedliteratemachinery_amd.utils.nested_tensor import NestedTensor
    from tests.gpu_checks import DEV, ENGINES, build_model, golden, rec
    from tests.gpu_checks_windows import fixture_case
    gold = golden('spot_windows')
    args, sd, img, mask, _ = fixture_case(gold, 'eos')
    model = build_model(args, sd, gold['case']['depths'], ENGINES[dtype_name])
    nt = NestedTensor(img.to(DEV), mask.to(DEV))
    wins = [WN.default_window(args)] + WN.grid_windows(2, 2, args.num_bins)
    records = inf.predict(model, nt, args, windows=wins, suppress=0.5, reading_order=True, blocks=True)
    tag = 'page regex engine[%s]' % dtype_name
    per_image = [engine_expressions(recs) for recs in records]
    note = '%s records; expressions %s' % ([len(r) for r in records], per_image)
    out = [rec(tag + ' the records give an alternation of two words and a loop per image', 0 if all(len(ps) == 2 for ps in per_image) else 1, 0, note)]
    dev = _Counting(PR.RegexSearcher(DEV))
    got = find_regex(copy.deepcopy(records), per_image, max_hits=64, searcher=dev)
    want = find_regex(copy.deepcopy(records), per_image, max_hits=64, searcher=PR.HostRegexSearcher())
    out.append(rec(tag + ' find_regex on the device == find_regex with HostRegexSearcher on every field', 0 if got == want else 1, 0, note))
    out.append(rec(tag + ' the whole call issues one RegexSearcher.run', abs(dev.calls - 1) + abs(dev.inner.chunks - 1), 0))
    missing = 0
    for res, recs in zip(want, records):
        either, run = res
        missing += either['n_hits'] < 2 or len(either['hits']) < 2                  # both words stand on the page
        missing += run['n_hits'] < 1 or any(' ' in h['text'] for h in run['hits'])  # a run never crosses a separator
    out.append(rec(tag + ' both words of the alternation are found, and no run of the loop crosses a separator', missing, 0, note))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the structural time gate
# ---------------------------------------------------------------------------------------------------------------------------------
def timing_case(n_pages=16, n_chars=2000, n_expr=32, seed=21):
    """pages of words, numbers and dates, and a mix of the bench families: (a) flat shapes, (b) alternations of literals, (c) loops over
    planted digit runs longer than a chunk -> (page strings, expression strings)"""
    rng = np.random.RandomState(seed)
    words = ['invoice', 'rechnung', 'total', 'EUR', 'USD', 'CHF', 'Jan', 'Feb', 'Mar', 'no', 'nr', 'date', 'amount', 'id', 'page', 'sum']
    pages = []
    for _ in range(n_pages):
        parts, size = [], 0
        while size <= n_chars:                                               # the join holds size - 1 characters
            kind = rng.randint(0, 10)
            if kind < 5:
                w = words[rng.randint(0, len(words))]
            elif kind < 7:
                w = '%02d.%02d.%04d' % (rng.randint(1, 29), rng.randint(1, 13), rng.randint(1990, 2030))
            elif kind < 9:
                w = '{:,}.{:02d}'.format(int(rng.randint(0, 10 ** 7)), rng.randint(0, 100))
            else:
                w = ''.join(str(d) for d in rng.randint(0, 10, int(rng.randint(100, 400))))      # a digit run across lanes
            parts.append(w)
            size += len(w) + 1
        pages.append(' '.join(parts)[:n_chars])
    flat = [r'\d{2}[./-]\d{2}[./-]\d{4}', r'[A-Z]{3} ?\d{1,3}', r'\d{1,3},\d{3}', r'\.\d{2} ', r'[a-z]{2,6} \d{2}', r'id ?\d{4}', r'no? ?\d', r'[A-Z][a-z]{2} \d{1,2}']
    alts = ['(%s)' % '|'.join(words[i:i + 3 + i % 3]) for i in range(0, 12)]
    loops = [r'\d+', r'[a-z]+ \d+', r'\d{1,3}(,\d{3})*\.\d{2}', r'(EUR|USD|CHF) ?\d+', r'[A-Z]{2}\d+', r'(\d+\.)+\d+', r'(no|nr) ?\d+', r'\d+ [A-Z]+', r'([a-z]+ )+\d', r'\d{5,}',
             r'(\d\d)+ ', r'[a-z]+']
    exprs = (flat + alts + loops)[:n_expr]
    return pages, exprs


def check_timing():
    """16 pages of 2000 characters x 32 expressions, a mix of the bench families (a) to (c): the median of 3 whole RegexSearcher.run calls
    (upload, launch, download) at or below ONE search_cpu call on the same inputs.  No margin: it catches a launch or a synchronisation per
    job, not a tuning."""
    from tests.gpu_checks import DEV, rec
    pages, exprs = timing_case()
    packed = from_strings(pages, exprs, [(p, q) for q in range(len(exprs)) for p in range(len(pages))])
    sc = PR.RegexSearcher(DEV)
    got = sc.run(*packed, 16)                                                # warm: library load, allocator
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = sc.run(*packed, 16)
        ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    want = PR.search_cpu(*packed, 16)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    note = 'device run %s ms (median %.3f), search_cpu %.1f ms, %d pages of %d x %d expressions, %d hits' % (
        [round(v, 3) for v in ms], statistics.median(ms), cpu_ms, len(pages), len(pages[0]), len(exprs), int(want['n_hits'].sum()))
    print(note)
    return [rec('page regex: 16 pages of 2000 x 32 expressions, median of 3 device runs <= one search_cpu call', statistics.median(ms), cpu_ms, note),
            rec('page regex: the timed outputs are equal', _bad(got, want), 0),
            rec('page regex: the timed case holds 16 pages of 2000 characters, 32 expressions and hits', 0 if len(pages) == 16 and all(len(p) == 2000 for p in pages) and
                len(exprs) == 32 and int((want['n_hits'] > 0).sum()) > 100 else 1, 0)]
