"""GPU checks of page expressions with errors: omp_page_regex_fuzzy_search against fuzzy_search_cpu
(utils/page_regex.py) on every integer, into buffers prefilled with garbage: random automata at the byte-table edges crossed with every
tolerance on texts around the chunk and round edges, planted carries of rows above 0 across lanes and rounds, valley and plateau
decisions across the two words of a lane, across lanes and across rounds, the pending last column of a round, starts in other chunks and
rounds, the page length limit at k = 4, k = 0 against omp_page_regex_search, the order of the hits, the refusals, find_regex(max_dist=1)
on the device against the host searcher on the records of a real engine call, and the structural time gate.  Every check returns records
{name, err, tol, ok, note} like tests/gpu_checks.py."""
import copy
import re
import statistics
import time

import numpy as np
import torch

from advancedliteratemachinery_amd.utils import page_regex as PR
from tests.gpu_checks_page_regex import GARBAGE, LONG, POS, SHORT, _bad, _Counting, _device, _planted, _slice, automaton, random_mask, timing_case

C = PR.CHUNK
R = PR.ROUND
KS = tuple(range(PR.K_MAX + 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# random automata with a tolerance, and texts that hold noisy words of their languages
# ---------------------------------------------------------------------------------------------------------------------------------
def chain_automaton(rng, P, mask, k):
    """position i goes on to i + 1 (the shortest word stays long, so that k is allowed), to itself and backwards at random; the tolerance
    is k bounded by min_len - 1"""
    follow = []
    for i in range(P):
        f = (1 << (i + 1)) if i + 1 < P else 0
        f |= (1 << i) if rng.rand() < 0.2 else 0
        f |= (1 << int(rng.randint(0, i + 1))) if rng.rand() < 0.3 else 0
        follow.append(f)
    last = (1 << (P - 1)) | ((1 << int(rng.randint(P // 2, P))) if rng.rand() < 0.5 else 0)
    a = automaton(mask, 1, last, follow)
    a['k'] = min(k, PR.min_len(a['first'], a['last'], a['follow']) - 1)
    return a


def noisy_word(rng, a, sigma, errors):
    """codes of a word of the language (a random walk from first to last), with `errors` random substitutions, deletions or insertions"""
    member = [[c for c in range(min(sigma, len(a['mask']) - 1)) if (int(a['mask'][c]) >> p) & 1] for p in range(a['P'])]
    bits = lambda w: [i for i in range(64) if (w >> i) & 1]                  # noqa: E731
    p = int(rng.choice(bits(a['first'])))
    word = []
    while len(word) < 150:
        word.append(int(rng.choice(member[p])))
        nxt = bits(a['follow'][p])
        if ((a['last'] >> p) & 1 and (not nxt or rng.rand() < 0.5)) or not nxt:
            break
        p = max(nxt) if len(word) > 100 else int(rng.choice(nxt))
    for _ in range(errors):
        at = int(rng.randint(0, len(word) + 1))
        kind = rng.randint(0, 3)
        if kind == 0 and at < len(word):
            word[at] = int(rng.randint(0, sigma))
        elif kind == 1 and at < len(word) and len(word) > 1:
            del word[at]
        else:
            word.insert(at, int(rng.randint(0, sigma)))
    return word


def noisy_text(rng, a, sigma, n, filler):
    """n codes of filler with noisy words of a's language planted about every 300 columns, the first across column 128 when it fits"""
    t = filler(rng, n)
    at = max(0, min(n, C) - 3)
    while at < n:
        w = noisy_word(rng, a, sigma, int(rng.randint(0, a['k'] + 2)))[:n - at]
        t[at:at + len(w)] = w
        at += len(w) + int(rng.randint(20, 600))
    return t


def _variants():
    """(name, sigma, make_mask(rng, P), filler(rng, n))"""
    every = lambda rng, P: np.asarray([(1 << P) - 1, 0], dtype=np.uint64)                                      # noqa: E731
    return [('one code in every class, sigma=1', 1, every, lambda rng, n: np.zeros(n, np.uint8)),
            ('random sigma=254', 254, lambda rng, P: random_mask(rng, P, 254, 0.05), lambda rng, n: rng.randint(0, 254, n).astype(np.uint8)),
            ('random sigma=26 in a text that also holds codes at or above sigma', 26, lambda rng, P: random_mask(rng, P, 26, 0.2),
             lambda rng, n: rng.randint(0, 40, n).astype(np.uint8))]


def edge_cases(seed=0):
    """-> [(variant, sigma, [(automaton with k, t), ...])]: per variant every P crossed with every k (bounded by min_len - 1), each against
    one short length and, rotating over (P, k), every short length and every length around a round of the wave"""
    rng = np.random.RandomState(seed)
    cases = []
    for v, (name, sigma, make_mask, filler) in enumerate(_variants()):
        jobs = []
        for i, P in enumerate(POS):
            for k in KS:
                a = chain_automaton(rng, P, make_mask(rng, P), k)
                lengths = [SHORT[(i + k + v + s) % len(SHORT)] for s in (0, 3)]
                if k == (i + v) % len(KS):
                    lengths.append(LONG[(i + v) % 3])
                for n in lengths:
                    jobs.append((a, noisy_text(rng, a, sigma, n, filler)))
        cases.append((name, sigma, jobs))
    return cases


def pack(specs, sigma):
    """[(automaton with k, t)] -> ([pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs], k int32 [Q]): texts and
    automata that are the same object get one page and one expression"""
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
    packed = [np.concatenate(chunks + [np.zeros(0, np.uint8)]), i32(po), i32(pl), np.stack(masks), u64([a['first'] for a in autos]), u64([a['last'] for a in autos]),
              u64([a['follow'] for a in autos]).reshape(-1, 64), u64([a['pred'] for a in autos]).reshape(-1, 64), i32([a['P'] for a in autos]), i32(jobs).reshape(-1, 2)]
    return packed, i32([a['k'] for a in autos])


def from_strings(texts, exprs, jobs, max_dist):
    """page strings, expression strings, (page, expression) pairs and max_dist -> (the list pack() gives, k)"""
    parsed = [PR.parse_regex(e) for e in exprs]
    enc = PR.encode_regex(texts, parsed)
    k = np.asarray([PR.regex_tolerance(r.min_len, max_dist, None) for r in parsed], dtype=np.int32)
    return list(enc[:9]) + [np.asarray(jobs, dtype=np.int32).reshape(-1, 2)], k


def run_raw(packed, k, H, tabs=None):
    """ops.page_regex_fuzzy_search on output buffers prefilled with garbage -> the dict of fuzzy_search_cpu"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV
    d = _device(packed) if tabs is None else tabs
    dk = d['k'] if 'k' in d else torch.from_numpy(np.ascontiguousarray(k, dtype=np.int32)).to(DEV)
    J, sigma = packed[9].shape[0], packed[3].shape[1] - 1
    outs = [torch.full((n,), GARBAGE, dtype=torch.int32, device=DEV) for n in (2 * J, J, 3 * H * J)]
    best, n_hits, hits = ops.page_regex_fuzzy_search(d['pool'], packed[0].size, d['po'], d['pl'], d['masks'], d['first'], d['last'], d['follow'], d['pred'], d['P'], dk,
                                                     d['jobs'], sigma, H, best=outs[0], n_hits=outs[1], hits=outs[2])
    return dict(best=best.cpu().numpy(), n_hits=n_hits.cpu().numpy(), hits=hits.cpu().numpy())


_EDGE = {}


def edge_reference():
    """the cases, all of them packed into one call, and fuzzy_search_cpu on it at max_hits 64 (max_hits 1 is its first row): computed once
    and shared by the checks.  fuzzy_search_cpu judges every job by itself, so a variant's own answer is its slice of the mixed call's."""
    if not _EDGE:
        cases = edge_cases()
        specs = [j for _, _, jobs in cases for j in jobs]
        packed, k = pack(specs, PR.SIGMA_MAX)
        want = PR.fuzzy_search_cpu(*packed, k, 64)
        _EDGE.update(cases=cases, specs=specs, packed=packed, k=k, want={64: want, 1: dict(want, hits=want['hits'][:, :1].copy())})
    return _EDGE


def check_edges():
    from tests.gpu_checks import DEV, rec
    E = edge_reference()
    want = E['want'][64]
    out, lo = [], 0
    for name, sigma, jobs in E['cases']:
        hi = lo + len(jobs)
        w = _slice(want, lo, hi)
        packed, k = pack(jobs, sigma)
        got = run_raw(packed, k, 64)
        out.append(rec('page regex fuzzy[%s] alone, sigma=%d: %d jobs == fuzzy_search_cpu' % (name, sigma, len(jobs)), _bad(got, w), 0,
                       'n_hits %d .. %d, %d hits with errors, distances %s' % (int(w['n_hits'].min()), int(w['n_hits'].max()), int((w['hits'][:, :, 1] > 0).sum()),
                                                                             sorted(set(w['hits'][:, :, 1].ravel().tolist()) - {-1}))))
        lo = hi
    for H in (64, 1):
        w = E['want'][H]
        got = run_raw(E['packed'], E['k'], H)
        out.append(rec('page regex fuzzy: all variants in one call of %d jobs with k %s, max_hits %d == fuzzy_search_cpu' % (len(E['specs']), sorted(set(E['k'].tolist())), H),
                       _bad(got, w), 0, '%d jobs with more hits than are kept' % int((w['n_hits'] > H).sum())))
    sc = PR.FuzzyRegexSearcher(DEV)
    got = sc.run(*E['packed'], E['k'], 64)
    out.append(rec('page regex fuzzy: the mixed call through FuzzyRegexSearcher == fuzzy_search_cpu', _bad(got, want) + abs(sc.chunks - 1), 0, '%d hits' % int(want['n_hits'].sum())))
    # the cases cover what they claim to cover
    seen = {(a['P'], a['k'], len(t)) for a, t in E['specs']}
    miss = sum(not any((P, min(k, P - 1), n) in seen for n in SHORT + LONG) for P in POS for k in KS)
    miss += sum(not any(s[2] == n for s in seen) for n in SHORT + LONG) + sum(not any(s[0] == P and s[2] in LONG for s in seen) for P in POS)
    out.append(rec('page regex fuzzy: the cases hold every P with every k up to min(4, P - 1), every length, and a length around a round per P', miss, 0, '%d (P, k, n)' % len(seen)))
    dists = set(want['hits'][:, :, 1].ravel().tolist())
    out.append(rec('page regex fuzzy: the hits of the cases hold every distance 0 .. 4', 0 if dists >= set(KS) else 1, 0, str(sorted(dists))))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# planted cases: real expressions
# ---------------------------------------------------------------------------------------------------------------------------------
def carry_cases():
    """-> (texts, expressions, [(what, page, expression, the hits it must have or None)], max_dist)"""
    texts, exprs, jobs = [], [], []

    def add(what, text, src, hits=None):
        if text not in texts:
            texts.append(text)
        if src not in exprs:
            exprs.append(src)
        jobs.append((what, texts.index(text), exprs.index(src), hits))
    word = 'abcdefgh'
    # -- carries of the rows above 0 --
    for edge, n in ((C, 300), (R, R + 300)):
        for err, side in ((edge - 1, 'before'), (edge + 2, 'after')):        # the word stands on the columns edge - 3 .. edge + 4
            bad = list(word)
            bad[err - (edge - 3)] = 'X'
            add('a misread bounded expression across column %d, the error %s the edge' % (edge, side), _planted(n, [(edge - 3, ''.join(bad))]), word, [(edge + 4, 1, edge - 4)])
    for run in (300, 9000):
        body = '7' * (run // 2) + 'X' + '7' * (run - run // 2 - 1)
        add('a digit run of %d characters with one letter inside, between a and b' % run, _planted(run + 500, [(100, 'a' + body + 'b')]), r'a\d+b', [(101 + run, 1, 99)])
        add('a digit run of %d characters with one letter inside' % run, _planted(run + 500, [(100, body)]), r'\d{2,}')
    for n in (C + 1, R + 1):
        add('a.*b with a substituted a at column 1 and b at column %d' % n, 'X' + 'x' * (n - 2) + 'b', r'a.*b', [(n, 1, 0)])
    # -- valleys (v = 1, 0, 1 around an exact word) and plateaus (v = 1, 1, 2 around a word whose last character is misread) --
    lit = 'abcdef'
    for shift in (-1, 0, 1, 2):
        ends = [e + shift for e in (64, C, R)]                              # bits 63 / 64 of a lane's words, lanes, rounds
        n = R + 300
        add('valleys: exact words that end at %s' % ends, _planted(n, [(e - 5, lit) for e in ends]), lit, [(e, 0, e - 6) for e in ends])
        add('plateaus: words with a misread last character that end at %s' % ends, _planted(n, [(e - 5, 'abcdeX') for e in ends]), lit, [(e, 1, e - 6) for e in ends])
    add('a pending end of distance 1 at 8192 followed by distance 0', _planted(R + 100, [(R - 4, lit)]), lit, [(R + 1, 0, R - 5)])
    add('a pending end of distance 1 at 8192 followed by an equal one', _planted(R + 100, [(R - 4, 'abcdeX')]), lit, [(R + 1, 1, R - 5)])
    add('a pending end of distance 1 at 8192 followed by a greater one', _planted(R + 100, [(R - 5, 'abcdeX')]), lit, [(R, 1, R - 6)])
    add('a plateau that ends at n = 8192', _planted(R, [(R - 5, 'abcdeX')]), lit, [(R, 1, R - 6)])
    add('a valley whose lowest column is the last of two rounds', _planted(2 * R, [(2 * R - 5, lit)]), lit, [(2 * R, 0, 2 * R - 6)])
    # -- starts --
    add('a start in the same chunk', _planted(400, [(150, 'a7X7b')]), r'a\d+b', [(154, 1, 149)])
    add('a start in the previous chunk', _planted(400, [(100, 'a' + '7' * 30 + 'X' + '7' * 30 + 'b')]), r'a\d+b', [(162, 1, 99)])
    add('a start in the previous round', _planted(R + 400, [(R - 100, 'a' + '7' * 100 + 'X' + '7' * 100 + 'b')]), r'a\d+b', [(R + 102, 1, R - 101)])
    add('a start at 0', _planted(400, [(1, 'a' + '7' * 70 + 'X' + '7' * 70 + 'b')]), r'a\d+b', [(143, 1, 0)])
    add('a start that a walk which goes on injecting last would put too early: abc in abcbc', 'abcbc', 'abc', [(3, 0, 0), (5, 1, 2)])
    add('a deleted first character: the character before it, substituted, is the least start', _planted(300, [(C - 2, 'bcdefgh')]), word, [(C + 4, 1, C - 4)])
    add('an amount with a misread digit across an edge', _planted(400, [(C - 8, ' 1,2O4,567.89 ')]), r'\d,\d{3},\d{3}\.\d{2}', [(C + 4, 1, C - 8)])
    add('EUP 120 and 12 Jau 2024', 'total EUP 120 on 12 Jau 2024', r'(EUR|USD|CHF) ?\d+', [(13, 1, 6)])
    add('EUP 120 and 12 Jau 2024', 'total EUP 120 on 12 Jau 2024', r'\d{1,2} (Jan|Feb|Mar) \d{4}', [(28, 1, 17)])
    return texts, exprs, jobs, 1


def check_carry():
    from tests.gpu_checks import rec
    texts, exprs, jobs, max_dist = carry_cases()
    packed, k = from_strings(texts, exprs, [(p, q) for _, p, q, _ in jobs], max_dist)
    want = PR.fuzzy_search_cpu(*packed, k, 64)
    out = []
    for H in (64, 1):
        got = run_raw(packed, k, H)
        for j, (what, _, q, hits) in enumerate(jobs):
            w = _slice(want, j, j + 1)
            w = dict(w, hits=w['hits'][:, :H])
            out.append(rec('page regex fuzzy[%s], k %d, max_hits %d == fuzzy_search_cpu' % (what, k[q], H), _bad(_slice(got, j, j + 1), w), 0,
                           'n_hits %d, first hits %s' % (int(w['n_hits'][0]), w['hits'][0][:3].tolist())))
            if H == 64 and hits is not None:                                # the case is what it says it is: the definition holds the planted hits
                rows = [tuple(r) for r in w['hits'][0].tolist() if r[0] >= 0]
                out.append(rec('page regex fuzzy[%s]: the definition holds the planted hits' % what, sum(h not in rows for h in hits), 0, '%s, planted %s' % (rows[:6], hits)))
    out.append(rec('page regex fuzzy: every planted expression got k = 1', 0 if (k == 1).all() else 1, 0, str(k.tolist())))
    return out


def check_limit():
    """one page of 65 535 characters (all 8 rounds) and a 64-position literal at k = 4, planted with 0 .. 4 errors at the start, in the
    middle, across the second round's edge and as the last characters"""
    from tests.gpu_checks import DEV, rec
    from tests.gpu_checks_page_regex import literal
    rng = np.random.RandomState(4)
    n = PR.LEN_MAX
    t = rng.randint(0, 26, n).astype(np.uint8)
    exact = rng.randint(0, 26, 64).astype(np.uint8)
    sub = exact.copy()
    sub[[5, 40]] = 26                                                        # two substitutions
    short = np.delete(exact, [0, 20, 63])                                    # three deletions, the first and the last position among them
    longer = np.insert(exact, [10, 30, 31, 50], 26)                          # four insertions
    t[0:62] = sub[2:]                                                        # the start of the page cuts two more positions off: distance 4
    t[30000:30064] = sub
    t[2 * R - 30:2 * R - 30 + 61] = short                                    # a substituted neighbour costs what a deleted end costs: the hit is one wider either way
    t[n - 68:] = longer
    a = dict(literal(exact, 28), k=4)
    packed, k = pack([(a, t)], 27)
    want = PR.fuzzy_search_cpu(*packed, k, 16)
    got = PR.FuzzyRegexSearcher(DEV).run(*packed, k, 16)
    rows = [tuple(r) for r in want['hits'][0].tolist() if r[0] >= 0]
    return [rec('page regex fuzzy[65535, P = 64, k = 4]: == fuzzy_search_cpu', _bad(got, want), 0, 'n_hits %s best %s hits %s' % (want['n_hits'].tolist(), want['best'].tolist(), rows)),
            rec('page regex fuzzy[65535]: the planted words are the hits, with their distances and starts',
                0 if rows == [(62, 4, 0), (2 * R + 32, 3, 2 * R - 31), (30064, 2, 30000), (n, 4, n - 68)] else 1, 0, str(rows))]


def exact_cases():
    """k = 0 on planted texts: -> (texts, expressions, [(what, page, expression, the hits it must have)])"""
    lit = 'abcdef'
    texts = [_planted(R + 100, [(R - 5, lit)]), _planted(R + 100, [(R - 3, '7' * 7)]), _planted(R, [(R - 5, lit)])]
    return texts, [lit, r'\d+'], [('a pending end at column 8192 that is a hit', 0, 0, [(R, 0, R - 6)]),
                                  ('a pending end at column 8192 inside a run of ends', 1, 1, [(R + 3, 0, R - 4)]),
                                  ('an end at n = 8192, which is not pending', 2, 0, [(R, 0, R - 6)]),
                                  ('a page without an end', 0, 1, [])]


def check_exact():
    """k = 0: omp_page_regex_search launches the instance of the kernel that holds one row only, omp_page_regex_fuzzy_search at k = 0 the one
    that dispatches over k; both against each other and against search_cpu on every integer.  The edge jobs hold every P of POS (so
    every NB) and texts of 0, 1, 127 .. 129, 255 .. 257 and 8191 .. 8193 characters (check_edges asserts that); the planted jobs hold a
    pending end at column 8192 that is a hit, one that is none, an end at n = 8192, and one refused job."""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import rec

    def both(packed):
        d = _device(packed)
        J, sigma = packed[9].shape[0], packed[3].shape[1] - 1
        best, n_hits, hits = ops.page_regex_search(d['pool'], packed[0].size, d['po'], d['pl'], d['masks'], d['first'], d['last'], d['follow'], d['pred'], d['P'], d['jobs'], sigma, 64)
        return dict(best=best.cpu().numpy(), n_hits=n_hits.cpu().numpy(), hits=hits.cpu().numpy()), run_raw(packed, np.zeros(packed[8].size, np.int32), 64, d)
    E = edge_reference()
    packed = E['packed']
    if 'exact' not in E:
        E['exact'] = PR.search_cpu(*packed, 64)
    exact, got = both(packed)
    J = packed[9].shape[0]
    out = [rec('page regex fuzzy at k = 0 == omp_page_regex_search on the %d edge jobs: best, n_hits, ends and starts' % J, _bad(got, exact), 0,
               '%d hits' % int(exact['n_hits'].sum())),
           rec('page regex at one row == search_cpu on the %d edge jobs' % J, _bad(exact, E['exact']), 0),
           rec('page regex fuzzy at k = 0: the jobs hold hits', 0 if int((exact['n_hits'] > 0).sum()) > 20 else 1, 0)]
    texts, exprs, jobs = exact_cases()
    planted, _ = from_strings(texts, exprs, [(p, q) for _, p, q, _ in jobs], 0)
    want = PR.search_cpu(*planted, 64)
    for j, (what, _, _, hits) in enumerate(jobs):
        rows = [tuple(r) for r in want['hits'][j].tolist() if r[0] >= 0]
        out.append(rec('page regex at k = 0[%s]: the definition holds the planted hits' % what, 0 if rows == hits else 1, 0, '%s, planted %s' % (rows[:4], hits)))
    refused = list(planted)
    refused[9] = np.concatenate([planted[9], np.asarray([[len(texts), 0]], np.int32)])       # a page that is not there
    want = {key: np.concatenate([v, np.full((1,) + v.shape[1:], -1, v.dtype)]) for key, v in want.items()}
    exact, got = both(refused)
    out.append(rec('page regex at one row == search_cpu on the planted jobs, the refused job -1', _bad(exact, want), 0, str(exact['n_hits'].tolist())))
    out.append(rec('page regex fuzzy at k = 0 == omp_page_regex_search on the planted jobs and the refused one', _bad(got, exact), 0, str(got['n_hits'].tolist())))
    return out


def check_ordering():
    """32 jobs on one page of 20 000 characters of 4 codes, a random literal of 8 positions each at k = 1: hits in many chunks and rounds"""
    from tests.gpu_checks import rec
    from tests.gpu_checks_page_regex import literal
    rng = np.random.RandomState(6)
    t = rng.randint(0, 4, 20000).astype(np.uint8)
    specs = [(dict(literal(rng.randint(0, 4, 8), 5), k=1), t) for _ in range(32)]
    packed, k = pack(specs, 4)
    want = PR.fuzzy_search_cpu(*packed, k, 64)
    got, again = run_raw(packed, k, 64), run_raw(packed, k, 64)
    one = run_raw(packed, k, 1)
    ends = got['hits'][:, :, 0]
    kept = np.minimum(got['n_hits'], 64)
    rising = all((np.diff(ends[j, :kept[j]]) > 0).all() for j in range(32))
    rounds = max(len(set((want['hits'][j, :min(int(want['n_hits'][j]), 64), 0] // R).tolist())) for j in range(32))
    return [rec('page regex fuzzy ordering: 32 jobs on one page == fuzzy_search_cpu', _bad(got, want), 0, 'n_hits %d .. %d' % (int(want['n_hits'].min()), int(want['n_hits'].max()))),
            rec('page regex fuzzy ordering: max_hits 1 keeps the first hit and counts them all', _bad(one, dict(want, hits=want['hits'][:, :1])), 0),
            rec('page regex fuzzy ordering: every hits list ascends', 0 if rising else 1, 0),
            rec('page regex fuzzy ordering: the kept hits of some job fall in all three rounds, and every job has hits', 0 if rounds == 3 and (want['n_hits'] > 0).all() else 1, 0,
                'most %d rounds' % rounds),
            rec('page regex fuzzy ordering: the same call again gives identical bytes', 0 if all(got[key].tobytes() == again[key].tobytes() for key in got) else 1, 0)]


def check_refusals():
    """what the entry point refuses comes back as an error code and a message before any launch, and what only the device tables show
    as n_hits = -1; nothing aborts.  Every refused job is in bounds: the kernel rejects it by its own checks."""
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(9)
    t1, t2 = rng.randint(0, 5, 300).astype(np.uint8), rng.randint(0, 5, 40).astype(np.uint8)
    a1, a2 = chain_automaton(rng, 4, random_mask(rng, 4, 5, 0.4), 1), chain_automaton(rng, 12, random_mask(rng, 12, 5, 0.4), 2)
    packed, k = pack([(a1, t1), (a2, t1), (a1, t2), (a2, t2), (a1, t1)], 5)
    pool, po, pl, masks, first, last, follow, pred, P, jobs = packed
    H, J = 4, jobs.shape[0]
    want = PR.fuzzy_search_cpu(*packed, k, H)
    d = dict(_device(packed), k=torch.from_numpy(k).to(DEV))
    out = [rec('page regex fuzzy: the refusal case itself == fuzzy_search_cpu', _bad(run_raw(packed, k, H, d), want), 0, str(want['n_hits'].tolist()))]
    res = [torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (2 * J, J, 3 * H * J)]
    args = [ops.ptr(d['pool']), pool.size, ops.ptr(d['po']), ops.ptr(d['pl']), len(pl), ops.ptr(d['masks']), ops.ptr(d['first']), ops.ptr(d['last']), ops.ptr(d['follow']),
            ops.ptr(d['pred']), ops.ptr(d['P']), ops.ptr(d['k']), len(P), ops.ptr(d['jobs']), J, 5, H, ops.ptr(res[0]), ops.ptr(res[1]), ops.ptr(res[2]), ops.stream()]
    for i, what in ((0, 'pool'), (2, 'page_off'), (3, 'page_len'), (5, 'masks'), (6, 'first'), (7, 'last'), (8, 'follow'), (9, 'pred'), (10, 'pat_len'), (11, 'k'), (13, 'jobs'),
                    (17, 'best'), (18, 'n_hits'), (19, 'hits')):
        a = list(args)
        a[i] = None
        rc = _lib.lib().omp_page_regex_fuzzy_search(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page regex fuzzy refuses a null %s with an error code' % what, 0 if rc == -22 and 'null pointer' in msg else 1, 0, msg))
    for what, i, v in (('J = 0', 14, 0), ('J = -1', 14, -1), ('J above 2^20', 14, (1 << 20) + 1), ('max_hits 0', 16, 0), ('max_hits 65', 16, 65), ('sigma 255', 15, 255),
                       ('sigma -1', 15, -1), ('no pages', 4, 0), ('no expressions', 12, 0), ('a negative pool', 1, -1),
                       ('masks off their alignment', 5, d['masks'].data_ptr() + 4), ('first off its alignment', 6, d['first'].data_ptr() + 4),
                       ('last off its alignment', 7, d['last'].data_ptr() + 4), ('follow off its alignment', 8, d['follow'].data_ptr() + 4),
                       ('pred off its alignment', 9, d['pred'].data_ptr() + 4)):
        a = list(args)
        a[i] = v
        rc = _lib.lib().omp_page_regex_fuzzy_search(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page regex fuzzy refuses %s with an error code' % what, 0 if rc == -22 and 'omp_page_regex_fuzzy_search' in msg else 1, 0, msg))
    try:
        ops.page_regex_fuzzy_search(d['pool'], pool.size, d['po'], d['pl'], d['masks'], d['first'], d['last'], d['follow'], d['pred'], d['P'], d['k'], d['jobs'], 5, 65)
        bad = 1
    except RuntimeError as e:
        bad = 0 if 'omp_page_regex_fuzzy_search' in str(e) and '(-22)' in str(e) and 'max_hits' in str(e) else 1
    out.append(rec('the fuzzy wrapper raises on max_hits 65', bad, 0))
    torch.cuda.synchronize()
    out.append(rec('page regex fuzzy: nothing was written by the refused calls', sum(int((r != -7).sum().item()) for r in res), 0))
    # what only the device tables show.  Expressions: 0 = a1 (P 4), 1 = a2 (P 12); pages: 0 = t1, 1 = t2; jobs (0, 0) (0, 1) (1, 0) (1, 1) (0, 0)
    top = -(1 << 63)
    for what, key, idx, v, hit in (('k = -1', 'k', 0, -1, (0, 2, 4)), ('k = 5', 'k', 1, 5, (1, 3)), ('P = 0', 'P', 0, 0, (0, 2, 4)), ('P = 65', 'P', 1, 65, (1, 3)),
                                   ('a first bit at P', 'first', 0, a1['first'] | 1 << 4, (0, 2, 4)), ('a last bit at 63 under P = 12', 'last', 1, top, (1, 3)),
                                   ('first == 0', 'first', 0, 0, (0, 2, 4)), ('last == 0', 'last', 1, 0, (1, 3)),
                                   ('a follow row at P', 'follow', 4, 1, (0, 2, 4)), ('a pred bit at 63 under P = 12', 'pred', 64 + 3, top, (1, 3)),
                                   ('a page of 65536 characters', 'pl', 1, PR.LEN_MAX + 1, (2, 3)), ('a negative page length', 'pl', 0, -1, (0, 1, 4)),
                                   ('a negative offset', 'po', 1, -1, (2, 3)), ('a page range past pool_bytes', 'po', 0, pool.size - 299, (0, 1, 4)),
                                   ('a page that is not there', 'jobs', 0, 2, (0,)), ('a negative expression', 'jobs', 5, -1, (2,))):
        tabs = dict(d, **{key: d[key].clone()})
        tabs[key][idx] = v
        got = run_raw(packed, k, H, tabs)
        w = {n: a.copy() for n, a in want.items()}
        for j in hit:
            w['best'][j] = -1
            w['n_hits'][j] = -1
            w['hits'][j] = -1
        out.append(rec('page regex fuzzy refuses %s on the device: n_hits -1, the other jobs answered' % what, _bad(got, w), 0, str(got['n_hits'].tolist())))
    # the device stage
    try:
        PR.FuzzyRegexSearcher('cpu')
        bad = 1
    except RuntimeError:
        bad = 0
    out.append(rec('FuzzyRegexSearcher refuses a device that is not cuda', bad, 0))
    sc = PR.FuzzyRegexSearcher(DEV)
    ok = dict(zip('pool page_off page_len masks first last follow pred pat_len jobs'.split(), packed), k=k, max_hits=4)
    for what, kw in (('k = 5', dict(k=[5, 2])), ('k = -1', dict(k=[1, -1])), ('k = min_len', dict(k=[PR.min_len(a1['first'], a1['last'], a1['follow']), 2])),
                     ('a page above the limit', dict(page_len=[PR.LEN_MAX + 1, 40])), ('max_hits 65', dict(max_hits=65)), ('last == 0', dict(last=[0, a2['last']]))):
        try:
            sc.run(**dict(ok, **kw))
            bad = 1
        except ValueError:
            bad = 0
        out.append(rec('the fuzzy regex searcher refuses %s on the host' % what, bad, 0))
    empty = sc.run(**dict(ok, jobs=np.zeros((0, 2), np.int32)))
    out.append(rec('the fuzzy regex searcher on no jobs: empty outputs', 0 if empty['best'].shape == (0, 2) and empty['n_hits'].shape == (0,) and empty['hits'].shape == (0, 4, 3) else 1, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
def misread_expressions(recs):
    """expressions from the call's own words with one character changed to one the page does not hold, so that the exact search misses them
    and one error finds them: an alternation of two such words, and the rarest one alone -> [(name, expression)]"""
    from advancedliteratemachinery_amd.utils.page_search import page_index
    text, start, ln = page_index(recs, normalise=None)
    texts = [text[s:s + n] for s, n in zip(start.tolist(), ln.tolist())]
    fit = sorted({w for w in texts if 2 <= len(w) <= 30 and w == ' '.join(w.split())}, key=lambda w: (text.count(w), -len(w), w))
    absent = next(ch for ch in '#@~^`' + ''.join(chr(c) for c in range(0x100, 0x200)) if ch not in text)
    bad = [re.escape(w[:len(w) // 2] + absent + w[len(w) // 2 + 1:]) for w in fit[:2]]
    out = []
    if len(bad) >= 2:
        out.append(('either', '(%s|%s)' % tuple(bad)))
    if bad:
        out.append(('one', bad[0]))
    return out


def check_engine_search(dtype_name):
    """the image, weights and call of tests.gpu_checks_page_regex.check_engine_search; find_regex(max_dist=1) on the device == find_regex
    with HostFuzzyRegexSearcher on every field"""
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
    tag = 'page regex fuzzy engine[%s]' % dtype_name
    per_image = [misread_expressions(recs) for recs in records]
    note = '%s records; expressions %s' % ([len(r) for r in records], per_image)
    out = [rec(tag + ' the records give an alternation of two misread words and one misread word per image', 0 if all(len(ps) == 2 for ps in per_image) else 1, 0, note)]
    dev = _Counting(PR.FuzzyRegexSearcher(DEV))
    got = find_regex(copy.deepcopy(records), per_image, max_hits=64, max_dist=1, searcher=dev)
    want = find_regex(copy.deepcopy(records), per_image, max_hits=64, max_dist=1, searcher=PR.HostFuzzyRegexSearcher())
    exact = find_regex(copy.deepcopy(records), per_image, max_hits=64, searcher=PR.HostRegexSearcher())
    out.append(rec(tag + ' find_regex(max_dist=1) on the device == find_regex with HostFuzzyRegexSearcher on every field', 0 if got == want else 1, 0, note))
    out.append(rec(tag + ' the whole call issues one FuzzyRegexSearcher.run', abs(dev.calls - 1) + abs(dev.inner.chunks - 1), 0))
    missing = 0
    for res, ex in zip(want, exact):
        missing += sum(d['n_hits'] != 0 or d['best'] is not None for d in ex)                       # the exact search misses every misread word
        missing += sum(d['best'] != 1 or d['k'] != 1 or not d['hits'] or any(h['dist'] != 1 for h in d['hits']) for d in res)
        missing += len(res[0]['hits']) < 2 if len(res) == 2 else 1                                # both words of the alternation are found
    out.append(rec(tag + ' the exact search misses the misread words, and one error finds them all at distance 1', missing, 0, note))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the structural time gate
# ---------------------------------------------------------------------------------------------------------------------------------
def check_timing():
    """4 pages of 2000 characters x 32 expressions (tests.gpu_checks_page_regex.timing_case: the mix of the bench families) at max_dist = 1:
    the median of 3 whole FuzzyRegexSearcher.run calls (upload, launch, download) at or below ONE fuzzy_search_cpu call on the same inputs.
    No margin: it catches a launch or a synchronisation per job, not a tuning."""
    from tests.gpu_checks import DEV, rec
    pages, exprs = timing_case(n_pages=4)
    packed, k = from_strings(pages, exprs, [(p, q) for q in range(len(exprs)) for p in range(len(pages))], 1)
    sc = PR.FuzzyRegexSearcher(DEV)
    got = sc.run(*packed, k, 16)                                             # warm: library load, allocator
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = sc.run(*packed, k, 16)
        ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    want = PR.fuzzy_search_cpu(*packed, k, 16)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    note = 'device run %s ms (median %.3f), fuzzy_search_cpu %.1f ms, %d pages of %d x %d expressions with k %s, %d hits' % (
        [round(v, 3) for v in ms], statistics.median(ms), cpu_ms, len(pages), len(pages[0]), len(exprs), sorted(set(k.tolist())), int(want['n_hits'].sum()))
    print(note)
    return [rec('page regex fuzzy: 4 pages of 2000 x 32 expressions, median of 3 device runs <= one fuzzy_search_cpu call', statistics.median(ms), cpu_ms, note),
            rec('page regex fuzzy: the timed outputs are equal', _bad(got, want), 0),
            rec('page regex fuzzy: the timed case holds 4 pages of 2000 characters, 32 expressions, k = 0 and k = 1 and hits', 0 if len(pages) == 4 and
                all(len(p) == 2000 for p in pages) and len(exprs) == 32 and set(k.tolist()) == {0, 1} and int((want['n_hits'] > 0).sum()) > 30 else 1, 0)]
