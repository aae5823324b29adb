"""GPU checks of page patterns: omp_page_pattern_search against search_cpu (utils/page_pattern.py) on every
integer at the edges of chunks, warm-up, pattern length and optional runs, at the page length limit, the chunked device stage, the order
of the hits, what the entry point refuses, find_pattern on the device against the host searcher on the records of a real engine call,
and the structural time gate.  Every check returns records {name, err, tol, ok, note} like tests/gpu_checks.py."""
import copy
import re
import statistics
import time

import numpy as np
import torch

from advancedliteratemachinery_amd.utils import page_pattern as PP

C = PP.CHUNK
POS = (1, 2, 31, 32, 33, 63, 64)
GARBAGE = 0x5a5a5a5a


def lengths(P, k):
    return sorted({0, 1, P + k - 1, P + k, P + k + 1, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 5 * C + 3})


def opt_shapes(P):
    """name -> the opt word of a pattern of P positions; at least one position stays mandatory"""
    run = lambda lo, hi: sum(1 << i for i in range(max(lo, 0), min(hi, P)))  # noqa: E731
    out = [('no optional position', 0)]
    if P >= 2:
        out.append(('a leading optional run', run(0, max(1, P // 4))))
        out.append(('a trailing optional run', run(P - max(1, P // 4), P)))
        out.append(('all but one position optional', run(0, P) & ~(1 << (P // 2))))
    if P >= 33:
        out.append(('an optional run across bit 31 / 32', run(29, 35 if P > 35 else P - 1)))
    return out


def kmax(P, opt):
    return min(P - bin(opt).count('1') - 1, PP.K_MAX)


def tolerances(P, opt):
    top = kmax(P, opt)
    return (0, top, top // 2)


def random_mask(rng, P, sigma, density):
    """uint64 [sigma + 1]: every position's class holds each code with probability `density` and at least one code"""
    member = rng.rand(sigma, P) < density
    member[rng.randint(0, sigma, P), np.arange(P)] = True
    mask = np.zeros(sigma + 1, dtype=np.uint64)
    for i in range(P):
        mask[:sigma] |= member[:, i].astype(np.uint64) << np.uint64(i)
    return mask


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


def _planted(rng, P):
    """a pattern of P two-code classes over 26 codes, an instance of it planted in 5C + 3 random characters so that a hit ends at C - 1,
    C, C + 1 and n, across 2C, and inside the first P + k columns: exact under k = 0 and the largest k, and with one substitution, one
    lost character and one extra character (code 26, in no class) under the largest k -> [(mask, opt, P, t, k)]"""
    n = 5 * C + 3
    member = np.zeros((27, P), dtype=bool)
    first = rng.randint(0, 26, P)
    member[first, np.arange(P)] = True
    member[(first + 1 + rng.randint(0, 25, P)) % 26, np.arange(P)] = True
    mask = np.zeros(28, dtype=np.uint64)
    for i in range(P):
        mask[:27] |= member[:, i].astype(np.uint64) << np.uint64(i)
    top = kmax(P, 0)
    jobs = []
    for end in (C - 1, C, C + 1, n, 2 * C + (P + 1) // 2, P + top // 2 + 1):
        inst = np.asarray([rng.choice(np.flatnonzero(member[:26, i])) for i in range(P)], dtype=np.uint8)
        t = rng.randint(0, 26, n).astype(np.uint8)
        t[end - P:end] = inst
        jobs += [(mask, 0, P, t, 0), (mask, 0, P, t, top)]
        if top >= 1:
            sub = t.copy()
            sub[end - P + P // 2] = 26
            lost = np.concatenate([rng.randint(0, 26, 1).astype(np.uint8), t[:end - P + P // 2], t[end - P + P // 2 + 1:]])
            extra = np.concatenate([t[1:end - P + P // 2], np.asarray([26], np.uint8), t[end - P + P // 2:]])
            jobs += [(mask, 0, P, sub, top), (mask, 0, P, lost, top), (mask, 0, P, extra, top)]
    return jobs


def edge_cases(seed=0):
    """-> [(variant, sigma, [(mask, opt, P, t, k), ...])]: per variant and P one pattern per tolerance against a text of every length of
    lengths(P, k), the optional runs rotating; then every optional run per P against every length at sigma 3; then the planted cases"""
    rng = np.random.RandomState(seed)
    cases = []
    for name, sigma, make_mask, make_text in _variants():
        jobs = []
        for P in POS:
            shapes = opt_shapes(P)
            for s, (_, opt) in enumerate(shapes[:3]):
                mask = make_mask(rng, P)
                for i, k in enumerate(tolerances(P, opt)):
                    for n in lengths(P, k)[(s + i) % 2::2] if s else lengths(P, k):
                        jobs.append((mask, opt, P, make_text(rng, n), k))
        cases.append((name, sigma, jobs))
    jobs = []
    for P in POS:
        for _, opt in opt_shapes(P):
            mask = random_mask(rng, P, 3, 0.5)
            for i, n in enumerate(lengths(P, kmax(P, opt))):
                jobs.append((mask, opt, P, rng.randint(0, 3, n).astype(np.uint8), tolerances(P, opt)[i % 3]))
    cases.append(('every optional run, sigma=3', 3, jobs))
    cases.append(('planted', 27, [j for P in POS for j in _planted(rng, P)]))
    return cases


def pack(specs, sigma):
    """[(mask, opt, P, t, k)] -> (pool, page_off, page_len, masks [Q, sigma + 1], opt, pat_len, jobs, k): texts that are the same object
    get one pool range and one page; a mask under another opt, P or k is another pattern.  A mask table narrower than sigma + 1 is padded
    with zeros: its codes at or above its own sigma are in no class either way."""
    chunks, total = [], 0
    pages, pats, jobs = {}, {}, []
    po, pl, masks, opts, Ps, ks = [], [], [], [], [], []
    for mask, opt, P, t, k in specs:
        if id(t) not in pages:
            pages[id(t)] = len(pages)
            po.append(total)
            pl.append(len(t))
            chunks.append(np.asarray(t, dtype=np.uint8))
            total += len(t)
        key = (id(mask), opt, P, k)
        if key not in pats:
            pats[key] = len(pats)
            row = np.zeros(sigma + 1, dtype=np.uint64)
            row[:min(len(mask) - 1, sigma)] = mask[:min(len(mask) - 1, sigma)]
            masks.append(row)
            opts.append(opt)
            Ps.append(P)
            ks.append(k)
        jobs.append((pages[id(t)], pats[key]))
    i32 = lambda v: np.asarray(v, dtype=np.int32)                            # noqa: E731
    return [np.concatenate(chunks + [np.zeros(0, np.uint8)]), i32(po), i32(pl), np.stack(masks), np.asarray(opts, dtype=np.uint64), i32(Ps),
            i32(jobs).reshape(-1, 2), i32(ks)]


_EDGE = {}


def edge_reference():
    """the cases, all of them packed into one call, and search_cpu on it at max_hits 64 and 1: computed once and shared by the checks.
    search_cpu judges every job by itself, so a variant's own answer is its slice of the mixed call's."""
    if not _EDGE:
        cases = edge_cases()
        specs = [j for _, _, jobs in cases for j in jobs]
        _EDGE.update(cases=cases, specs=specs, packed=pack(specs, PP.SIGMA_MAX))
        _EDGE['want'] = {H: PP.search_cpu(*_EDGE['packed'], H) for H in (64, 1)}
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
    pool, po, pl, masks, opt, P, jobs, k = packed
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)          # noqa: E731
    return dict(pool=t(pool), po=t(po), pl=t(pl), masks=t(masks.reshape(-1).view(np.int64)), opt=t(opt.view(np.int64)), P=t(P), jobs=t(jobs.reshape(-1)), k=t(k))


def run_raw(packed, H, tabs=None):
    """ops.page_pattern_search on output buffers prefilled with garbage -> the dict of search_cpu"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV
    d = _device(packed) if tabs is None else tabs
    J, sigma = packed[6].shape[0], packed[3].shape[1] - 1
    scratch = torch.full((ops.page_pattern_scratch_bytes(J, H),), 0x5a, dtype=torch.uint8, device=DEV)
    outs = [torch.full((n,), GARBAGE, dtype=torch.int32, device=DEV) for n in (2 * J, J, 3 * H * J)]
    best, n_hits, hits = ops.page_pattern_search(d['pool'], packed[0].size, d['po'], d['pl'], d['masks'], d['opt'], d['P'], d['k'], d['jobs'], sigma, H, scratch,
                                                 best=outs[0], n_hits=outs[1], hits=outs[2])
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
        out.append(rec('page pattern[%s] alone, sigma=%d: %d jobs == search_cpu' % (name, sigma, len(jobs)), _bad(got, w), 0,
                       'n_hits %d .. %d, best %d .. %d' % (int(w['n_hits'].min()), int(w['n_hits'].max()), int(w['best'][:, 0].min()), int(w['best'][:, 0].max()))))
        lo = hi
    packed = E['packed']
    for H in (64, 1):
        w = E['want'][H]
        got = run_raw(packed, H)
        out.append(rec('page pattern: all variants in one call of %d jobs, max_hits %d == search_cpu' % (len(E['specs']), H), _bad(got, w), 0,
                       '%d jobs with more hits than are kept' % int((w['n_hits'] > H).sum())))
        out.append(rec('page pattern: max_hits %d is exceeded by some job' % H, 0 if (w['n_hits'] > H).any() else 1, 0, 'most %d' % int(w['n_hits'].max())))
    sc = PP.PatternSearcher(DEV)
    got = sc.run(*packed, 64)
    out.append(rec('page pattern: the mixed call through PatternSearcher == search_cpu', _bad(got, want) + abs(sc.chunks - 1), 0, '%d hits' % int(want['n_hits'].sum())))
    # the cases cover what they claim to cover
    seen = {(P, k, len(t)) for _, _, P, t, k in E['specs']}
    miss = sum((P, k, n) not in seen for P in POS for k in tolerances(P, 0) for n in lengths(P, k))
    shapes = {(P, opt) for _, opt, P, _, _ in E['specs']}
    miss += sum((P, opt) not in shapes for P in POS for _, opt in opt_shapes(P))
    out.append(rec('page pattern: the cases hold every length, tolerance and optional run per P', miss, 0, '%d (P, k, n), %d (P, opt)' % (len(seen), len(shapes))))
    dists = np.bincount(want['hits'][:, :, 1][want['hits'][:, :, 1] >= 0], minlength=PP.K_MAX + 1)
    out.append(rec('page pattern: the kept hits hold every distance 0 .. %d' % PP.K_MAX, int((dists[:PP.K_MAX + 1] == 0).sum()), 0, str(dists.tolist())))
    # the planted hits are where they were put: per P six ends, per end the exact text under k = 0 and the largest k, then three worn texts
    at = len(E['specs']) - len(E['cases'][-1][2])
    missing = 0
    for P in POS:
        for _ in range(6):
            for kind in range(5 if kmax(P, 0) else 2):
                rows = [r for r in want['hits'][at].tolist() if r[0] >= 0]
                if P >= 31:                                                 # a short pattern also occurs by chance
                    missing += int(len(rows) != 1 or rows[0][1] != (0 if kind < 2 else 1) or (kind < 2 and rows[0][0] - rows[0][2] != P))
                at += 1
    out.append(rec('page pattern: a planted text (P >= 31) has exactly its planted hit, at distance 0 exact and 1 with one error', missing, 0))
    return out


def check_limit():
    """one page of 65 535 characters; a 64-position pattern planted at the start, in the middle and as the last 64 characters, exact and
    with 3 substitutions; a pattern that occurs nowhere"""
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(4)
    n = PP.LEN_MAX
    t = rng.randint(0, 26, n).astype(np.uint8)

    def literal(codes):
        mask = np.zeros(28, dtype=np.uint64)
        for i, c in enumerate(codes.tolist()):
            mask[c] |= np.uint64(1) << np.uint64(i)
        return mask
    exact, edited = rng.randint(0, 26, 64).astype(np.uint8), rng.randint(0, 26, 64).astype(np.uint8)
    places = (0, 30000, n - 64)
    for at in places:
        t[at:at + 64] = exact
    worn = t.copy()
    for at in places:
        worn[at:at + 64] = edited
        worn[at + np.asarray([5, 31, 60])] = 26
    m_exact, m_edited = literal(exact), literal(edited)
    nowhere = np.zeros(28, dtype=np.uint64)
    nowhere[26] = np.uint64((1 << 64) - 1)                                   # code 26 in every class; t holds no 26
    k = PP.tolerance(64, max_ratio=0.2)
    packed = pack([(m_exact, 0, 64, t, k), (m_edited, 0, 64, worn, k), (nowhere, 0, 64, t, k), (m_exact, 0, 64, worn, k)], 27)
    want = PP.search_cpu(*packed, 16)
    got = PP.PatternSearcher(DEV).run(*packed, 16)
    ends = [at + 64 for at in places]
    out = [rec('page pattern[65535]: == search_cpu', _bad(got, want), 0, 'k %d n_hits %s best %s' % (k, want['n_hits'].tolist(), want['best'].tolist()))]
    out.append(rec('page pattern[65535]: the exact plants are hits of distance 0', 0 if want['hits'][0][:3].tolist() == [[e, 0, e - 64] for e in ends] else 1, 0))
    out.append(rec('page pattern[65535]: the worn plants are hits of distance 3', 0 if want['hits'][1][:3].tolist() == [[e, 3, e - 64] for e in ends] else 1, 0))
    out.append(rec('page pattern[65535]: a pattern that occurs nowhere has no hit and (k + 1, 0) as its best',
                   0 if k == 8 and want['n_hits'][2] == 0 and want['best'][2].tolist() == [k + 1, 0] else 1, 0))
    return out


def check_chunked():
    """the mixed call with the scratch cap lowered so that it runs in at least 3 chunks == the unchunked definition"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV, rec
    E = edge_reference()
    want = E['want'][1]
    J = len(E['specs'])
    out = []
    for per in (J // 3, 7, J):
        sc = PP.PatternSearcher(DEV, scratch_cap=ops.page_pattern_scratch_bytes(per, 1))
        got = sc.run(*E['packed'], 1)
        out.append(rec('chunked pattern searcher, %d jobs a chunk == search_cpu' % per, _bad(got, want), 0, '%d chunks' % sc.chunks))
        out.append(rec('chunked pattern searcher, %d jobs a chunk: %s' % (per, 'one chunk' if per == J else 'at least 3 chunks'),
                       0 if (sc.chunks == 1 if per == J else sc.chunks >= 3) else 1, 0, '%d chunks' % sc.chunks))
        out.append(rec('chunked pattern searcher, %d jobs a chunk: the scratch holds one chunk' % per,
                       0 if sc.scratch.numel() == ops.page_pattern_scratch_bytes(min(per, J), 1) else 1, 0))
    return out


def check_ordering():
    """64 jobs on one page of 20 000 characters of 4 codes, patterns of 6 one-code positions, the fourth optional, under k = 1: hits in
    many chunks and rounds"""
    from tests.gpu_checks import rec
    rng = np.random.RandomState(6)
    t = rng.randint(0, 4, 20000).astype(np.uint8)
    packed = pack([(random_mask(rng, 6, 4, 0.0), 1 << 3, 6, t, 1) for _ in range(64)], 4)
    want = PP.search_cpu(*packed, 64)
    got = run_raw(packed, 64)
    again = run_raw(packed, 64)
    ends = got['hits'][:, :, 0]
    kept = np.minimum(got['n_hits'], 64)
    rising = all((np.diff(ends[j, :kept[j]]) > 0).all() for j in range(64))
    spread = min(len(set((ends[j, :kept[j]] // C).tolist())) for j in range(64))
    return [rec('page pattern ordering: 64 jobs on one page == search_cpu', _bad(got, want), 0, 'n_hits %d .. %d' % (int(want['n_hits'].min()), int(want['n_hits'].max()))),
            rec('page pattern ordering: every hits list ascends', 0 if rising else 1, 0),
            rec('page pattern ordering: the kept hits of every job fall in at least 8 chunks', 0 if spread >= 8 else 1, 0, 'least %d' % spread),
            rec('page pattern ordering: the same call again gives identical bytes', 0 if all(got[k].tobytes() == again[k].tobytes() for k in got) else 1, 0)]


def check_refusals():
    """what the entry point refuses comes back as an error code and a message before any launch, and what only the device tables show
    as n_hits = -1; nothing aborts"""
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(9)
    t1, t2 = rng.randint(0, 5, 300).astype(np.uint8), rng.randint(0, 5, 40).astype(np.uint8)
    m1, m2 = random_mask(rng, 4, 5, 0.4), random_mask(rng, 12, 5, 0.4)
    packed = pack([(m1, 0, 4, t1, 1), (m2, 1 << 5, 12, t1, 2), (m1, 0, 4, t2, 1), (m2, 1 << 5, 12, t2, 2), (m1, 0, 4, t1, 0)], 5)
    pool, po, pl, masks, opt, P, jobs, k = packed
    H, J = 4, jobs.shape[0]
    want = PP.search_cpu(*packed, H)
    d = _device(packed)
    out = [rec('page pattern: the refusal case itself == search_cpu', _bad(run_raw(packed, H, d), want), 0, str(want['n_hits'].tolist()))]
    scratch = torch.empty(ops.page_pattern_scratch_bytes(J, H), dtype=torch.uint8, device=DEV)
    res = [torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (2 * J, J, 3 * H * J)]
    args = [ops.ptr(d['pool']), pool.size, ops.ptr(d['po']), ops.ptr(d['pl']), len(pl), ops.ptr(d['masks']), ops.ptr(d['opt']), ops.ptr(d['P']), ops.ptr(d['k']), len(P),
            ops.ptr(d['jobs']), J, 5, H, ops.ptr(scratch), scratch.numel(), ops.ptr(res[0]), ops.ptr(res[1]), ops.ptr(res[2]), ops.stream()]
    for i, what in ((0, 'pool'), (2, 'page_off'), (3, 'page_len'), (5, 'masks'), (6, 'opt'), (7, 'pat_len'), (8, 'k'), (10, 'jobs'), (14, 'scratch'), (16, 'best'),
                    (17, 'n_hits'), (18, 'hits')):
        a = list(args)
        a[i] = None
        rc = _lib.lib().omp_page_pattern_search(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page pattern refuses a null %s with an error code' % what, 0 if rc == -22 and 'null pointer' in msg else 1, 0, msg))
    for what, i, v in (('J = 0', 11, 0), ('J = -1', 11, -1), ('J above 2^20', 11, (1 << 20) + 1), ('max_hits 0', 13, 0), ('max_hits 65', 13, 65), ('sigma 255', 12, 255),
                       ('sigma -1', 12, -1), ('no pages', 4, 0), ('no patterns', 9, 0), ('a negative pool', 1, -1), ('too little scratch', 15, scratch.numel() - 1),
                       ('no scratch', 15, 0), ('masks off their alignment', 5, d['masks'].data_ptr() + 4), ('opt off its alignment', 6, d['opt'].data_ptr() + 4),
                       ('scratch off its alignment', 14, scratch.data_ptr() + 4)):
        a = list(args)
        a[i] = v
        rc = _lib.lib().omp_page_pattern_search(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page pattern refuses %s with an error code' % what, 0 if rc == -22 and 'omp_page_pattern_search' in msg else 1, 0, msg))
    try:
        ops.page_pattern_search(d['pool'], pool.size, d['po'], d['pl'], d['masks'], d['opt'], d['P'], d['k'], d['jobs'], 5, H, scratch[:scratch.numel() - 8])
        bad = 1
    except RuntimeError as e:
        bad = 0 if 'omp_page_pattern_search' in str(e) and '(-22)' in str(e) and 'scratch' in str(e) else 1
    out.append(rec('the wrapper raises on too little scratch', bad, 0))
    torch.cuda.synchronize()
    out.append(rec('page pattern: nothing was written by the refused calls', sum(int((r != -7).sum().item()) for r in res), 0))
    # what only the device tables show: the job is refused on the device, its neighbours are answered.  Patterns: 0 = (m1, k 1),
    # 1 = (m2, k 2; Mand 11), 2 = (m1, k 0); pages: 0 = t1, 1 = t2
    for what, key, idx, v, hit in (('P = 0', 'P', 0, 0, (0, 2)), ('P = 65', 'P', 1, 65, (1, 3)), ('k = Mand', 'k', 0, 4, (0, 2)), ('k = -1', 'k', 1, -1, (1, 3)),
                                   ('k = 9 under Mand = 11', 'k', 1, 9, (1, 3)), ('an opt bit at P', 'opt', 2, 1 << 4, (4,)),
                                   ('an opt bit at 63 under P = 12', 'opt', 1, -(1 << 63), (1, 3)), ('no mandatory position', 'opt', 0, 15, (0, 2)),
                                   ('a page of 65536 characters', 'pl', 1, PP.LEN_MAX + 1, (2, 3)), ('a negative page length', 'pl', 0, -1, (0, 1, 4)),
                                   ('a negative offset', 'po', 1, -1, (2, 3)), ('a page range past pool_bytes', 'po', 0, pool.size - 299, (0, 1, 4)),
                                   ('a page that is not there', 'jobs', 0, 2, (0,)), ('a negative page', 'jobs', 8, -1, (4,)),
                                   ('a pattern that is not there', 'jobs', 3, 3, (1,)), ('a negative pattern', 'jobs', 5, -1, (2,))):
        tabs = dict(d, **{key: d[key].clone()})
        tabs[key][idx] = v
        got = run_raw(packed, H, tabs)
        w = {n: a.copy() for n, a in want.items()}
        for j in hit:
            w['best'][j] = -1
            w['n_hits'][j] = -1
            w['hits'][j] = -1
        out.append(rec('page pattern refuses %s on the device: n_hits -1, the other jobs answered' % what, _bad(got, w), 0, str(got['n_hits'].tolist())))
    # the device stage
    try:
        PP.PatternSearcher('cpu')
        bad = 1
    except RuntimeError:
        bad = 0
    out.append(rec('PatternSearcher refuses a device that is not cuda', bad, 0))
    sc = PP.PatternSearcher(DEV)
    ok = dict(pool=np.asarray([0, 1, 2], np.uint8), page_off=[0], page_len=[3], masks=np.asarray([[1, 2, 3, 0]], np.uint64), opt=[0], pat_len=[2], jobs=[[0, 0]], k=[1],
              max_hits=4)
    for what, kw in (('a page above the limit', dict(page_len=[PP.LEN_MAX + 1])), ('a range outside the pool', dict(page_off=[1])), ('k = Mand', dict(k=[2])),
                     ('P = 0', dict(pat_len=[0])), ('max_hits 65', dict(max_hits=65)), ('an opt bit at P', dict(opt=[4])), ('no mandatory position', dict(opt=[3])),
                     ('a mask table of 256 words', dict(masks=np.zeros((1, 256), np.uint64)))):
        try:
            sc.run(**dict(ok, **kw))
            bad = 1
        except ValueError:
            bad = 0
        out.append(rec('the pattern searcher refuses %s on the host' % what, bad, 0))
    empty = sc.run(**dict(ok, jobs=np.zeros((0, 2), np.int32)))
    out.append(rec('the pattern searcher on no jobs: empty outputs', 0 if empty['best'].shape == (0, 2) and empty['n_hits'].shape == (0,) and empty['hits'].shape == (0, 4, 3) else 1, 0))
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


def engine_patterns(recs):
    """patterns from the call's own records: a word as a literal, a word with a class for one of its characters, and a two-word shape
    with an optional separator -> [(name, pattern, (first, last))] -- whichever of the three the records allow"""
    from advancedliteratemachinery_amd.utils.page_search import page_index
    text, start, ln = page_index(recs, normalise=None)
    texts = [text[s:s + n] for s, n in zip(start.tolist(), ln.tolist())]
    fit = lambda s: 2 <= len(s) <= 30 and s == ' '.join(s.split())           # noqa: E731
    singles = sorted((i for i, w in enumerate(texts) if fit(w)), key=lambda i: (text.count(texts[i]), -len(texts[i]), i))
    out = []
    if singles:
        i = singles[0]
        out.append(('literal', re.escape(texts[i]), (i, i)))
    if len(singles) > 1:
        i = singles[1]
        w, at = texts[i], len(texts[i]) // 2
        cls = r'\d' if w[at].isdigit() else r'\w' if re.fullmatch(r'\w', w[at]) else r'\W'
        out.append(('class', re.escape(w[:at]) + cls + re.escape(w[at + 1:]), (i, i)))
    pairs = sorted((i for i in range(len(texts) - 1) if fit(texts[i]) and fit(texts[i + 1])), key=lambda i: (text.count(texts[i] + ' ' + texts[i + 1]), i))
    if pairs:
        i = pairs[0]
        out.append(('pair', re.escape(texts[i]) + ' ?' + re.escape(texts[i + 1]), (i, i + 1)))
    return out


def check_engine_search(dtype_name):
    """the image, weights and call of the page-search engine check (windows = [default, 2 x 2 grid], suppress=0.5, reading_order=True,
    blocks=True); find_pattern on the device == find_pattern with HostPatternSearcher on every field"""
    from advancedliteratemachinery_amd.engine import inference as inf
    from advancedliteratemachinery_amd.engine.search import find_pattern
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
    tag = 'page pattern engine[%s]' % dtype_name
    own = [engine_patterns(recs) for recs in records]
    per_image = [[(name, src) for name, src, _ in ps] for ps in own]
    note = '%s records; patterns %s' % ([len(r) for r in records], per_image)
    out = [rec(tag + ' the records give a literal, a word with a class and a two-word shape per image', 0 if all(len(ps) == 3 for ps in own) else 1, 0, note)]
    dev = _Counting(PP.PatternSearcher(DEV))
    got = find_pattern(copy.deepcopy(records), per_image, max_hits=64, max_dist=2, max_ratio=0.34, searcher=dev)
    want = find_pattern(copy.deepcopy(records), per_image, max_hits=64, max_dist=2, max_ratio=0.34, searcher=PP.HostPatternSearcher())
    out.append(rec(tag + ' find_pattern on the device == find_pattern with HostPatternSearcher on every field', 0 if got == want else 1, 0, note))
    out.append(rec(tag + ' the whole call issues one PatternSearcher.run', abs(dev.calls - 1) + abs(dev.inner.chunks - 1), 0))
    missing = 0
    for res, ps in zip(got, own):
        for d, (name, src, (first, last)) in zip(res, ps):
            missing += not any(h['dist'] == 0 and h['words'][0] <= first and last <= h['words'][1] for h in d['hits'])
    out.append(rec(tag + ' every pattern has a hit of distance 0 at its own words', missing, 0, note))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the structural time gate
# ---------------------------------------------------------------------------------------------------------------------------------
def check_timing():
    """16 pages of 2000 characters x 32 patterns of 12 positions: the median of 3 whole PatternSearcher.run calls (upload, launch,
    download) at or below ONE search_cpu call on the same inputs.  No margin: it catches a launch or a synchronisation per job, not a tuning."""
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(21)
    pages = [rng.randint(0, 60, 2000).astype(np.uint8) for _ in range(16)]
    specs = []
    for i in range(32):                                                      # cut from the pages, so that there are hits to report
        at = int(rng.randint(0, 2000 - 12))
        mask = random_mask(rng, 12, 60, 0.03)
        for j, c in enumerate(pages[i % 16][at:at + 12].tolist()):
            mask[c] |= np.uint64(1) << np.uint64(j)
        specs += [(mask, 1 << 6, 12, t, 2) for t in pages]
    packed = pack(specs, 60)
    sc = PP.PatternSearcher(DEV)
    got = sc.run(*packed, 16)                                                # warm: library load, allocator, scratch
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = sc.run(*packed, 16)
        ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    want = PP.search_cpu(*packed, 16)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    note = 'device run %s ms (median %.3f), search_cpu %.1f ms, 16 pages of 2000 x 32 patterns of 12, %d hits' % (
        [round(v, 3) for v in ms], statistics.median(ms), cpu_ms, int(want['n_hits'].sum()))
    print(note)
    return [rec('page pattern: 16 pages of 2000 x 32 patterns of 12, median of 3 device runs <= one search_cpu call', statistics.median(ms), cpu_ms, note),
            rec('page pattern: the timed outputs are equal', _bad(got, want), 0)]
