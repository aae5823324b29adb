"""GPU checks of page search: omp_page_search against search_cpu (utils/page_search.py) on every integer at the
edges of chunks, warm-up and query length, at the page length limit, the chunked device stage, the order of the hits, what the entry
point refuses, find_text on the device against the host searcher on the records of a real engine call, and the structural time gate.
Every check returns records {name, err, tol, ok, note} like tests/gpu_checks.py."""
import copy
import statistics
import time

import numpy as np
import torch

from advancedliteratemachinery_amd.utils import page_search as PS

C = PS.CHUNK
M = (1, 2, 31, 32, 33, 63, 64)
GARBAGE = 0x5a5a5a5a


def lengths(m):
    return sorted({0, 1, m - 1, m, m + 1, 2 * m - 1, 2 * m, 2 * m + 1, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 5 * C + 3})


def _variants():
    """name -> (sigma, make(rng, m, n) -> (q, t))"""
    def rand(sigma):
        return lambda rng, m, n: (rng.randint(0, sigma, m).astype(np.uint8), rng.randint(0, sigma, n).astype(np.uint8))
    out = [('all equal, sigma=1', 1, lambda rng, m, n: (np.zeros(m, np.uint8), np.zeros(n, np.uint8)))]
    out += [('random sigma=%d' % s, s, rand(s)) for s in (2, 26, 254)]
    out.append(('no common character', 4, lambda rng, m, n: (rng.randint(0, 2, m).astype(np.uint8), rng.randint(2, 4, n).astype(np.uint8))))
    out.append(('text all 255', 26, lambda rng, m, n: (rng.randint(0, 26, m).astype(np.uint8), np.full(n, PS.NONE, np.uint8))))
    return out


def _planted(rng, m):
    """the query of m characters planted in 5C + 3 random characters of 26 so that a hit ends at C - 1, C and C + 1 (the last column of
    a chunk, the first of the next, the look-ahead across the boundary), at n, across the boundary 2C, and inside the first 2m columns;
    every place exact under k = 0 and k = m - 1, and with one substitution under k = m - 1 -> [(q, t, k)]"""
    n = 5 * C + 3
    q = rng.randint(0, 26, m).astype(np.uint8)
    jobs = []
    for end in (C - 1, C, C + 1, n, 2 * C + (m + 1) // 2, m + m // 2):
        t = rng.randint(0, 26, n).astype(np.uint8)
        t[end - m:end] = q
        jobs += [(q, t, 0), (q, t, m - 1)]
        if m > 1:
            e = t.copy()
            e[end - m + m // 2] = 26                                         # a character the query does not hold
            jobs.append((q, e, m - 1))
    return jobs


def edge_cases(seed=0):
    """-> [(variant, sigma, [(q, t, k), ...])]: per variant and m ONE query against a text of every length of lengths(m), k rotating
    through 0, m - 1 and m // 4; then the planted cases per m"""
    rng = np.random.RandomState(seed)
    cases = []
    for name, sigma, make in _variants():
        jobs = []
        for m in M:
            q = make(rng, m, 0)[0]
            for i, n in enumerate(lengths(m)):
                jobs.append((q, make(rng, m, n)[1], (0, m - 1, m // 4)[i % 3]))
        cases.append((name, sigma, jobs))
    cases.append(('planted', 27, [j for m in M for j in _planted(rng, m)]))
    return cases


def pack(specs):
    """[(q, t, k)] -> (pool, page_off, page_len, query_off, query_len, jobs, k): arrays that are the same object get one pool range and
    one page; a query under another k is another query on the same range"""
    chunks, where, total = [], {}, 0
    pages, queries, jobs = {}, {}, []
    tabs = [[], [], [], [], []]

    def place(s):
        nonlocal total
        if id(s) not in where:
            where[id(s)] = total
            chunks.append(np.asarray(s, dtype=np.uint8))
            total += len(s)
        return where[id(s)]
    for q, t, k in specs:
        if id(t) not in pages:
            pages[id(t)] = len(pages)
            tabs[0].append(place(t))
            tabs[1].append(len(t))
        if (id(q), k) not in queries:
            queries[(id(q), k)] = len(queries)
            tabs[2].append(place(q))
            tabs[3].append(len(q))
            tabs[4].append(k)
        jobs.append((pages[id(t)], queries[(id(q), k)]))
    i32 = lambda v: np.asarray(v, dtype=np.int32)                            # noqa: E731
    return [np.concatenate(chunks + [np.zeros(0, np.uint8)]), i32(tabs[0]), i32(tabs[1]), i32(tabs[2]), i32(tabs[3]), i32(jobs).reshape(-1, 2), i32(tabs[4])]


_EDGE = {}


def edge_reference():
    """the cases, all of them packed into one call, and search_cpu on it at max_hits 64 and 1: computed once and shared by the checks.
    search_cpu judges every job by itself, so a variant's own answer is its slice of the mixed call's."""
    if not _EDGE:
        cases = edge_cases()
        specs = [j for _, _, jobs in cases for j in jobs]
        _EDGE.update(cases=cases, specs=specs, packed=pack(specs))
        _EDGE['want'] = {H: PS.search_cpu(*_EDGE['packed'], H) for H in (64, 1)}
    return _EDGE


def _bad(got, want):
    bad = 0
    for key in ('best', 'n_hits', 'hits'):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        bad += int((g != w).sum()) if g.shape == w.shape else 1 << 20
    return bad


def _slice(res, lo, hi):
    return {k: v[lo:hi] for k, v in res.items()}


def run_raw(packed, sigma, H):
    """ops.page_search on output buffers prefilled with garbage -> the dict of search_cpu"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in packed]
    J = packed[5].shape[0]
    scratch = torch.full((ops.page_search_scratch_bytes(J, H),), 0x5a, dtype=torch.uint8, device=DEV)
    outs = [torch.full((n,), GARBAGE, dtype=torch.int32, device=DEV) for n in (2 * J, J, 3 * H * J)]
    best, n_hits, hits = ops.page_search(d[0], packed[0].size, d[1], d[2], d[3], d[4], d[6], d[5].reshape(-1), sigma, H, scratch, best=outs[0], n_hits=outs[1],
                                         hits=outs[2])
    return dict(best=best.cpu().numpy(), n_hits=n_hits.cpu().numpy(), hits=hits.cpu().numpy())


def check_edges():
    from tests.gpu_checks import DEV, rec
    E = edge_reference()
    want = E['want'][64]
    out, lo = [], 0
    for name, sigma, jobs in E['cases']:
        hi = lo + len(jobs)
        w = _slice(want, lo, hi)
        got = run_raw(pack(jobs), sigma, 64)
        out.append(rec('page search[%s] alone, sigma=%d: %d jobs == search_cpu' % (name, sigma, len(jobs)), _bad(got, w), 0,
                       'n_hits %d .. %d, best %d .. %d' % (int(w['n_hits'].min()), int(w['n_hits'].max()), int(w['best'][:, 0].min()), int(w['best'][:, 0].max()))))
        lo = hi
    packed = E['packed']
    for H in (64, 1):
        w = E['want'][H]
        got = run_raw(packed, PS.SIGMA_MAX, H)
        out.append(rec('page search: all variants in one call of %d jobs, max_hits %d == search_cpu' % (len(E['specs']), H), _bad(got, w), 0,
                       '%d jobs with more hits than are kept' % int((w['n_hits'] > H).sum())))
        out.append(rec('page search: max_hits %d is exceeded by some job' % H, 0 if (w['n_hits'] > H).any() else 1, 0, 'most %d' % int(w['n_hits'].max())))
    sc = PS.PageSearcher(DEV)
    got = sc.run(*packed, 64)
    out.append(rec('page search: the mixed call through PageSearcher == search_cpu', _bad(got, want) + abs(sc.chunks - 1), 0, '%d hits' % int(want['n_hits'].sum())))
    shared = len(packed[3]) - len(set(packed[3].tolist()))
    lens = set(packed[2].tolist())
    out.append(rec('page search: the mixed call shares ranges and covers every length', 0 if shared > 50 and all(set(lengths(m)) <= lens for m in M) else 1, 0,
                   '%d shared query ranges' % shared))
    # the planted hits are where they were put
    lo = len(E['specs']) - len(E['cases'][-1][2])
    missing = 0
    for i, (q, t, k) in enumerate(E['cases'][-1][2]):
        ends = want['hits'][lo + i][:, 0].tolist()
        at = [e for e in (C - 1, C, C + 1, len(t), 2 * C + (len(q) + 1) // 2, len(q) + len(q) // 2) if (t[e - len(q):e] == q).all()]
        missing += int(k == 0 and len(q) >= 31 and sorted(at) != [e for e in ends if e >= 0])   # a short query also occurs by chance
    out.append(rec('page search: under k = 0 the hits of a planted text (m >= 31) are exactly the planted ends', missing, 0))
    return out


def check_limit():
    """one page of 65 535 characters; a 64-character query planted at the start, in the middle and as the last 64 characters, exact and
    with 3 substitutions; a query that occurs nowhere"""
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(4)
    n = PS.LEN_MAX
    t = rng.randint(0, 26, n).astype(np.uint8)
    exact, edited = rng.randint(0, 26, 64).astype(np.uint8), rng.randint(0, 26, 64).astype(np.uint8)
    places = (0, 30000, n - 64)
    for at in places:
        t[at:at + 64] = exact
    worn = t.copy()
    for at in places:
        worn[at:at + 64] = edited
        worn[at + np.asarray([5, 31, 60])] = 26
    nowhere = np.full(64, 26, np.uint8)
    k = PS.tolerance(64)
    packed = pack([(exact, t, k), (edited, worn, k), (nowhere, t, k), (exact, worn, k)])
    want = PS.search_cpu(*packed, 16)
    got = PS.PageSearcher(DEV).run(*packed, 16)
    ends = [at + 64 for at in places]
    out = [rec('page search[65535]: == search_cpu', _bad(got, want), 0, 'n_hits %s best %s' % (want['n_hits'].tolist(), want['best'].tolist()))]
    out.append(rec('page search[65535]: the exact plants are hits of distance 0', 0 if want['hits'][0][:3].tolist() == [[e, 0, e - 64] for e in ends] else 1, 0))
    out.append(rec('page search[65535]: the worn plants are hits of distance 3', 0 if want['hits'][1][:3].tolist() == [[e, 3, e - 64] for e in ends] else 1, 0))
    out.append(rec('page search[65535]: a query that occurs nowhere has no hit and the empty match as its best',
                   0 if want['n_hits'][2] == 0 and want['best'][2].tolist() == [64, 0] else 1, 0))
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
        sc = PS.PageSearcher(DEV, scratch_cap=ops.page_search_scratch_bytes(per, 1))
        got = sc.run(*E['packed'], 1)
        out.append(rec('chunked searcher, %d jobs a chunk == search_cpu' % per, _bad(got, want), 0, '%d chunks' % sc.chunks))
        out.append(rec('chunked searcher, %d jobs a chunk: %s' % (per, 'one chunk' if per == J else 'at least 3 chunks'),
                       0 if (sc.chunks == 1 if per == J else sc.chunks >= 3) else 1, 0, '%d chunks' % sc.chunks))
        out.append(rec('chunked searcher, %d jobs a chunk: the scratch holds one chunk' % per,
                       0 if sc.scratch.numel() == ops.page_search_scratch_bytes(min(per, J), 1) else 1, 0))
    return out


def check_ordering():
    """64 jobs on one page of 20 000 characters of 4 letters, queries of 6 characters under k = 1: hits in many chunks and rounds"""
    from tests.gpu_checks import rec
    rng = np.random.RandomState(6)
    t = rng.randint(0, 4, 20000).astype(np.uint8)
    packed = pack([(rng.randint(0, 4, 6).astype(np.uint8), t, 1) for _ in range(64)])
    want = PS.search_cpu(*packed, 64)
    got = run_raw(packed, 4, 64)
    again = run_raw(packed, 4, 64)
    ends = got['hits'][:, :, 0]
    kept = np.minimum(got['n_hits'], 64)
    rising = all((np.diff(ends[j, :kept[j]]) > 0).all() for j in range(64))
    spread = min(len(set((ends[j, :kept[j]] // C).tolist())) for j in range(64))
    return [rec('page search ordering: 64 jobs on one page == search_cpu', _bad(got, want), 0, 'n_hits %d .. %d' % (int(want['n_hits'].min()), int(want['n_hits'].max()))),
            rec('page search ordering: every hits list ascends', 0 if rising else 1, 0),
            rec('page search ordering: the kept hits of every job fall in at least 8 chunks', 0 if spread >= 8 else 1, 0, 'least %d' % spread),
            rec('page search ordering: the same call again gives identical bytes', 0 if all(got[k].tobytes() == again[k].tobytes() for k in got) else 1, 0)]


def check_refusals():
    """what the entry point refuses comes back as an error code and a message before any launch, and what only the device tables show
    as n_hits = -1; nothing aborts"""
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(9)
    t1, t2 = rng.randint(0, 5, 300).astype(np.uint8), rng.randint(0, 5, 40).astype(np.uint8)
    q1, q2 = rng.randint(0, 5, 4).astype(np.uint8), rng.randint(0, 5, 9).astype(np.uint8)
    packed = pack([(q1, t1, 1), (q2, t1, 2), (q1, t2, 1), (q2, t2, 2), (q1, t1, 0)])
    pool, po, pl, qo, ql, jobs, k = packed
    H, J = 4, jobs.shape[0]
    want = PS.search_cpu(*packed, H)
    out = [rec('page search: the refusal case itself == search_cpu', _bad(run_raw(packed, 5, H), want), 0)]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)        # noqa: E731
    d = dict(pool=t(pool), po=t(po), pl=t(pl), qo=t(qo), ql=t(ql), jobs=t(jobs.reshape(-1)), k=t(k))
    scratch = torch.empty(ops.page_search_scratch_bytes(J, H), dtype=torch.uint8, device=DEV)
    res = [torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (2 * J, J, 3 * H * J)]
    args = [ops.ptr(d['pool']), pool.size, ops.ptr(d['po']), ops.ptr(d['pl']), len(pl), ops.ptr(d['qo']), ops.ptr(d['ql']), ops.ptr(d['k']), len(ql),
            ops.ptr(d['jobs']), J, 5, H, ops.ptr(scratch), scratch.numel(), ops.ptr(res[0]), ops.ptr(res[1]), ops.ptr(res[2]), ops.stream()]
    for i, what in ((0, 'pool'), (2, 'page_off'), (3, 'page_len'), (5, 'query_off'), (6, 'query_len'), (7, 'k'), (9, 'jobs'), (13, 'scratch'), (15, 'best'),
                    (16, 'n_hits'), (17, 'hits')):
        a = list(args)
        a[i] = None
        rc = _lib.lib().omp_page_search(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page search refuses a null %s with an error code' % what, 0 if rc == -22 and 'null pointer' in msg else 1, 0, msg))
    for what, i, v in (('J = 0', 10, 0), ('J = -1', 10, -1), ('J above 2^20', 10, (1 << 20) + 1), ('max_hits 0', 12, 0), ('max_hits 65', 12, 65), ('sigma 255', 11, 255),
                       ('sigma -1', 11, -1), ('no pages', 4, 0), ('no queries', 8, 0), ('too little scratch', 14, scratch.numel() - 1), ('no scratch', 14, 0)):
        a = list(args)
        a[i] = v
        rc = _lib.lib().omp_page_search(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page search refuses %s with an error code' % what, 0 if rc == -22 and 'omp_page_search' in msg else 1, 0, msg))
    try:
        ops.page_search(d['pool'], pool.size, d['po'], d['pl'], d['qo'], d['ql'], d['k'], d['jobs'], 5, H, scratch[:scratch.numel() - 8])
        bad = 1
    except RuntimeError as e:
        bad = 0 if 'omp_page_search' in str(e) and '(-22)' in str(e) and 'scratch' in str(e) else 1
    out.append(rec('the wrapper raises on too little scratch', bad, 0))
    torch.cuda.synchronize()
    out.append(rec('page search: nothing was written by the refused calls', sum(int((r != -7).sum().item()) for r in res), 0))
    # what only the device tables show: the job is refused on the device, its neighbours are answered
    for what, key, idx, v, hit in (('m = 0', 'ql', 0, 0, (0, 2)), ('m = 65', 'ql', 1, 65, (1, 3)), ('k = m', 'k', 0, 4, (0, 2)), ('k = -1', 'k', 1, -1, (1, 3)),
                                   ('a page of 65536 characters', 'pl', 1, PS.LEN_MAX + 1, (2, 3)), ('a negative page length', 'pl', 0, -1, (0, 1, 4)),
                                   ('a negative offset', 'qo', 2, -1, (4,)), ('a page range past pool_bytes', 'po', 0, pool.size - 299, (0, 1, 4)),
                                   ('a query range past pool_bytes', 'qo', 1, pool.size - 8, (1, 3)), ('a page that is not there', 'jobs', 0, 2, (0,)),
                                   ('a query that is not there', 'jobs', 3, -1, (1,))):
        tabs = {n: d[n].clone() for n in ('po', 'pl', 'qo', 'ql', 'k', 'jobs')}
        tabs[key][idx] = v
        outs = [torch.full((n,), GARBAGE, dtype=torch.int32, device=DEV) for n in (2 * J, J, 3 * H * J)]
        best, n_hits, hits = ops.page_search(d['pool'], pool.size, tabs['po'], tabs['pl'], tabs['qo'], tabs['ql'], tabs['k'], tabs['jobs'], 5, H, scratch,
                                             best=outs[0], n_hits=outs[1], hits=outs[2])
        got = dict(best=best.cpu().numpy(), n_hits=n_hits.cpu().numpy(), hits=hits.cpu().numpy())
        w = {n: a.copy() for n, a in want.items()}
        for j in hit:
            w['best'][j] = -1
            w['n_hits'][j] = -1
            w['hits'][j] = -1
        out.append(rec('page search refuses %s on the device: n_hits -1, the other jobs answered' % what, _bad(got, w), 0, str(got['n_hits'].tolist())))
    # the device stage
    try:
        PS.PageSearcher('cpu')
        bad = 1
    except RuntimeError:
        bad = 0
    out.append(rec('PageSearcher refuses a device that is not cuda', bad, 0))
    sc = PS.PageSearcher(DEV)
    ok = dict(pool=np.asarray([0, 1, 2, 0, 1], np.uint8), page_off=[0], page_len=[3], query_off=[3], query_len=[2], jobs=[[0, 0]], k=[1], max_hits=4)
    for what, kw in (('a page above the limit', dict(page_len=[PS.LEN_MAX + 1])), ('a range outside the pool', dict(query_off=[4])), ('k = m', dict(k=[2])),
                     ('m = 0', dict(query_len=[0])), ('max_hits 65', dict(max_hits=65)), ('sigma 255', dict(sigma=255)), ('a code at or above sigma', dict(sigma=2))):
        try:
            sc.run(**dict(ok, **kw))
            bad = 1
        except ValueError:
            bad = 0
        out.append(rec('the searcher refuses %s on the host' % what, bad, 0))
    empty = sc.run(**dict(ok, jobs=np.zeros((0, 2), np.int32)))
    out.append(rec('the searcher on no jobs: empty outputs', 0 if empty['best'].shape == (0, 2) and empty['n_hits'].shape == (0,) and empty['hits'].shape == (0, 4, 3) else 1, 0))
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


def engine_queries(recs):
    """queries from the call's own records: three single words, two two-word phrases, one phrase with a character substituted ->
    [(query, (first, last) or None for the edited one)]"""
    words = PS.page_index(recs)
    text = words[0]
    texts = [text[s:s + n] for s, n in zip(words[1].tolist(), words[2].tolist())]
    fit = lambda s: 1 <= len(s) <= PS.QUERY_MAX and s == ' '.join(s.split())   # noqa: E731
    singles = sorted((i for i, w in enumerate(texts) if fit(w)), key=lambda i: (text.count(texts[i]), -len(texts[i]), i))
    pairs = sorted((i for i in range(len(texts) - 1) if fit(texts[i] + ' ' + texts[i + 1])), key=lambda i: (text.count(texts[i] + ' ' + texts[i + 1]), i))
    out, seen = [], set()
    for i in singles:
        if texts[i] not in seen and len(out) < 3:
            seen.add(texts[i])
            out.append((texts[i], (i, i)))
    n_single = len(out)
    for i in pairs:
        s = texts[i] + ' ' + texts[i + 1]
        if s not in seen and len(out) < n_single + 2:
            seen.add(s)
            out.append((s, (i, i + 1)))
    edited = None
    for s, _ in out[n_single:] + out[:n_single]:
        if len(s) >= 5:
            at = len(s) // 2
            edited = s[:at] + ('#' if s[at] != '#' else '@') + s[at + 1:]
            break
    return out, n_single, edited


def check_engine_search(dtype_name):
    """the image, weights and call of the page-text engine check (windows = [default, 2 x 2 grid], suppress=0.5, reading_order=True,
    blocks=True); find_text on the device == find_text with HostSearcher on every field"""
    from advancedliteratemachinery_amd.engine import inference as inf
    from advancedliteratemachinery_amd.engine.search import find_text
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
    tag = 'page search engine[%s]' % dtype_name
    per_image, own, shape = [], [], []
    for recs in records:
        qs, n_single, edited = engine_queries(recs)
        shape.append((n_single, len(qs) - n_single, edited is not None))
        own.append(qs)
        per_image.append([q for q, _ in qs] + ([edited] if edited is not None else []))
    note = '%s records; queries %s' % ([len(r) for r in records], per_image)
    out = [rec(tag + ' the records give three single words, two two-word phrases and one edited phrase per image',
               0 if all(s == (3, 2, True) for s in shape) else 1, 0, note)]
    dev = _Counting(PS.PageSearcher(DEV))
    got = find_text(copy.deepcopy(records), per_image, max_hits=64, max_dist=2, searcher=dev)
    want = find_text(copy.deepcopy(records), per_image, max_hits=64, max_dist=2, searcher=PS.HostSearcher())
    out.append(rec(tag + ' find_text on the device == find_text with HostSearcher on every field', 0 if got == want else 1, 0, note))
    out.append(rec(tag + ' the whole call issues one PageSearcher.run', abs(dev.calls - 1) + abs(dev.inner.chunks - 1), 0))
    missing = 0
    for res, qs in zip(got, own):
        for d, (q, (first, last)) in zip(res, qs):
            missing += not any(h['dist'] == 0 and h['words'][0] <= first and last <= h['words'][1] and q in h['text'] for h in d['hits'])
    out.append(rec(tag + ' every unedited query has a hit of distance 0 at its own words', missing, 0, note))
    worn = [res[len(qs)] for res, qs in zip(got, own) if len(res) > len(qs)]
    out.append(rec(tag + ' the edited phrase is found at distance 1', 0 if worn and all(d['best'] == 1 and any(h['dist'] == 1 for h in d['hits']) for d in worn) else 1, 0,
                   str([(d['query'], d['best'], d['n_hits']) for d in worn])))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the structural time gate
# ---------------------------------------------------------------------------------------------------------------------------------
def check_timing():
    """16 pages of 2000 characters x 32 queries of 12 characters: the median of 3 whole PageSearcher.run calls (upload, launch, download)
    at or below ONE search_cpu call on the same inputs.  No margin: it catches a launch or a synchronisation per job, not a tuning."""
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(21)
    pages = [rng.randint(0, 60, 2000).astype(np.uint8) for _ in range(16)]
    queries = []
    for i in range(32):                                                      # cut from the pages, so that there are hits to report
        at = int(rng.randint(0, 2000 - 12))
        queries.append(pages[i % 16][at:at + 12].copy())
    packed = pack([(q, t, 2) for t in pages for q in queries])
    sc = PS.PageSearcher(DEV)
    got = sc.run(*packed, 16, sigma=60)                                      # warm: library load, allocator, scratch
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = sc.run(*packed, 16, sigma=60)
        ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    want = PS.search_cpu(*packed, 16)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    note = 'device run %s ms (median %.3f), search_cpu %.1f ms, 16 pages of 2000 x 32 queries of 12, %d hits' % (
        [round(v, 3) for v in ms], statistics.median(ms), cpu_ms, int(want['n_hits'].sum()))
    print(note)
    return [rec('page search: 16 pages of 2000 x 32 queries of 12, median of 3 device runs <= one search_cpu call', statistics.median(ms), cpu_ms, note),
            rec('page search: the timed outputs are equal', _bad(got, want), 0)]
