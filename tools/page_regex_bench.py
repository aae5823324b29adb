"""Page expressions: ONE RegexSearcher.run (utils/page_regex.py -- the packed upload, omp_page_regex_search, the download) over jobs =
pages x expressions, per family of expressions, against the numpy definition search_cpu on a subsample of the same jobs, and for the flat
family against omp_page_pattern_search at k = 0 on the same jobs.

  python tools/page_regex_bench.py [--pages 500] [--chars 5000] [--expressions 200] [--long_pages 16] [--long_chars 40000]
                                   [--long_expressions 1000] [--alphabet 60] [--max_hits 16] [--cpu_jobs 100] [--long_cpu_jobs 20]
                                   [--repeats 5] [--warmup 1] [--k 0,1,2,4] [--out profiles/page_regex_bench.json]

Seeded pages as tools/page_pattern_bench.py makes them: `chars` (+- 10 %) characters drawn from `alphabet` codes, a blank every 3 to 9
characters; the codes 0 .. 9 are the digits, and every page gets runs of 150 to 400 digits planted at four places (longer than a lane's
128 columns).  The families, timed separately on both page sets:
  flat        the shapes of tools/page_pattern_bench.py (8 to 24 positions cut from a page, every third a class of 10 codes, two optional
              positions in the middle), as position automata; the same jobs also go through omp_page_pattern_search at k = 0
  alternation (w1|w2|...): 3 to 5 literals of 4 to 10 characters cut from the pages
  loop        \\d+, `blank \\d+` and \\d{m,} with m = 2 .. 20: the carry crosses chunk boundaries inside the planted runs
  never-dying ONE expression a.*b (a and b two codes of the alphabet): the carry never dies, the split degenerates to the serial run
Per leg the tool times whole run calls (host clock; the call ends with the download), the kernel alone between device events on tables
that are already on the device, and search_cpu on the first `cpu_jobs` jobs of a fixed random permutation; that host time is SCALED to
the leg by the ratio of text columns and is stated as such.  One JSON document; every leg is also printed as it ends.
--k 0,1,2,4 adds, per leg and per value, the search WITH ERRORS: every expression gets min(k, min_len - 1), and the
tool times one FuzzyRegexSearcher.run, omp_page_regex_fuzzy_search alone (stated as a ratio to omp_page_regex_search on the same jobs),
for the flat family omp_page_pattern_search at the same tolerances, and checks fuzzy_search_cpu on a few jobs of the permutation."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from page_pattern_bench import events, make_pages, make_shapes, spread, tables  # noqa: E402

DIGITS = 10


def plant_runs(rng, texts):
    for t in texts:
        for _ in range(4):
            m = int(rng.randint(150, 401))
            at = int(rng.randint(0, max(t.size - m, 1)))
            t[at:at + m] = rng.randint(0, DIGITS, min(m, t.size - at))
    return texts


def _words(first, last, follow):
    rows = [int(f) for f in follow] + [0] * (64 - len(follow))
    pred = [0] * 64
    for i, f in enumerate(rows):
        for j in range(64):
            if (f >> j) & 1:
                pred[j] |= 1 << i
    return int(first), int(last), rows, pred, len(follow)


def flat_words(opt, P):
    """the position automaton of a flat pattern whose optional positions are the bits of opt"""
    def reach(i):                                                             # the positions that can come next when position i is next in line
        out = 0
        while i < P:
            out |= 1 << i
            if not (opt >> i) & 1:
                break
            i += 1
        return out
    last = 0
    for i in range(P - 1, -1, -1):
        last |= 1 << i
        if not (opt >> i) & 1:
            break
    return _words(reach(0), last, [reach(i + 1) for i in range(P)])


def pack_words(masks, words):
    u64 = lambda v: np.asarray(v, dtype=np.uint64)                           # noqa: E731
    return (masks, u64([w[0] for w in words]), u64([w[1] for w in words]), u64([w[2] for w in words]).reshape(-1, 64), u64([w[3] for w in words]).reshape(-1, 64),
            np.asarray([w[4] for w in words], dtype=np.int32))


def make_flat(rng, texts, count, alphabet):
    masks, opt, P, k = make_shapes(rng, texts, count, alphabet, 0)
    return pack_words(masks, [flat_words(int(o), int(p)) for o, p in zip(opt.tolist(), P.tolist())]), (masks, opt, P, k)


def make_alternations(rng, texts, count, alphabet):
    masks, words = np.zeros((count, alphabet + 1), dtype=np.uint64), []
    for q in range(count):
        first, last, follow = 0, 0, []
        for _ in range(int(rng.randint(3, 6))):
            t = texts[int(rng.randint(0, len(texts)))]
            m = int(rng.randint(4, 11))
            at = int(rng.randint(0, t.size - m))
            base = len(follow)
            first |= 1 << base
            last |= 1 << (base + m - 1)
            for i, c in enumerate(t[at:at + m].tolist()):
                masks[q, c] |= np.uint64(1) << np.uint64(base + i)
                follow.append((1 << (base + i + 1)) if i + 1 < m else 0)
        words.append(_words(first, last, follow))
    return pack_words(masks, words)


def make_loops(rng, count, alphabet):
    masks, words = np.zeros((count, alphabet + 1), dtype=np.uint64), []
    for q in range(count):
        kind = q % 3
        if kind == 0:                                                        # \d+
            P, lead = 1, 0
        elif kind == 1:                                                      # blank \d+
            P, lead = 2, 1
            masks[q, alphabet - 1] |= np.uint64(1)
        else:                                                                # \d{m,}
            P, lead = 2 + q % 19, 0
        for i in range(lead, P):
            masks[q, :DIGITS] |= np.uint64(1) << np.uint64(i)
        follow = [(1 << (i + 1)) if i + 1 < P else 0 for i in range(P)]
        follow[P - 1] |= 1 << (P - 1)
        words.append(_words(1, 1 << (P - 1), follow))
    return pack_words(masks, words)


def make_never_dying(alphabet):
    masks = np.zeros((1, alphabet + 1), dtype=np.uint64)
    masks[0, 11] |= np.uint64(1)                                             # a
    masks[0, :alphabet] |= np.uint64(2)                                      # .
    masks[0, 12] |= np.uint64(4)                                             # b
    return pack_words(masks, [_words(1, 4, [0b110, 0b110, 0])])


def time_fuzzy(K, d, e, host, J, sigma, max_hits, exact_ms, pick, repeats, warmup):
    """the leg's jobs with errors: every expression at min(K, min_len - 1).  d: the device tables of the exact leg; e: those of the flat
    family's patterns or None; host: the numpy inputs"""
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.utils import page_pattern as PP
    from advancedliteratemachinery_amd.utils import page_regex as PR
    pool, po, pl, masks, first, last, follow, pred, P, jobs = host
    tol = np.asarray([min(K, PR.min_len(f, l, fo.tolist()) - 1) for f, l, fo in zip(first.tolist(), last.tolist(), follow)], dtype=np.int32)
    sc = PR.FuzzyRegexSearcher('cuda')
    run_ms, got = [], None
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        got = sc.run(pool, po, pl, masks, first, last, follow, pred, P, jobs, tol, max_hits)
        if i >= warmup:
            run_ms.append((time.perf_counter() - t0) * 1e3)
    dk = torch.from_numpy(tol).to('cuda')
    outs = [torch.empty(n, dtype=torch.int32, device='cuda') for n in (2 * J, J, 3 * max_hits * J)]

    def launch():
        ops.page_regex_fuzzy_search(d[0], pool.size, d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], dk, d[9], sigma, max_hits, best=outs[0], n_hits=outs[1],
                                    hits=outs[2])
    ms = events(launch, repeats, warmup)
    t0 = time.perf_counter()
    want = PR.fuzzy_search_cpu(pool, po, pl, masks, first, last, follow, pred, P, jobs[pick], tol, max_hits)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    doc = dict(k=K, tolerances={str(v): int((tol == v).sum()) for v in sorted(set(tol.tolist()))}, hits=int(got['n_hits'].sum()),
               hits_with_errors=int((got['hits'][:, :, 1] > 0).sum()), run=spread(run_ms), kernel=dict(spread(ms), launches=1),
               fuzzy_over_exact_kernel=round(statistics.median(ms) / exact_ms, 2),
               host=dict(jobs=int(pick.size), ms=round(cpu_ms, 1)),
               answers_equal_on_the_subsample=all(bool((got[key][pick] == want[key]).all()) for key in ('best', 'n_hits', 'hits')))
    if e is not None:                                                       # the flat family through omp_page_pattern_search at the same tolerances
        parts = PP.chunk_jobs(J, max_hits)
        scratch = torch.empty(ops.page_pattern_scratch_bytes(max(hi - lo for lo, hi in parts), max_hits), dtype=torch.uint8, device='cuda')
        outs2 = [torch.empty(n, dtype=torch.int32, device='cuda') for n in (2 * J, J, 3 * max_hits * J)]

        def launch2():
            for lo, hi in parts:
                ops.page_pattern_search(d[0], pool.size, d[1], d[2], e[0], e[1], e[2], dk, d[9][2 * lo:2 * hi], sigma, max_hits, scratch,
                                        best=outs2[0][2 * lo:2 * hi], n_hits=outs2[1][lo:hi], hits=outs2[2][3 * max_hits * lo:3 * max_hits * hi])
        ms2 = events(launch2, repeats, warmup)
        doc['page_pattern_same_k'] = dict(spread(ms2), launches=len(parts), fuzzy_regex_over_pattern=round(statistics.median(ms) / statistics.median(ms2), 2),
                                          n_hits_equal=bool((outs[1] == outs2[1]).all().item()), hits_equal=bool((outs[2] == outs2[2]).all().item()),
                                          best_equal=bool((outs[0] == outs2[0]).all().item()))
    return doc


def time_leg(name, texts, auto, max_hits, cpu_jobs, repeats, warmup, flat=None, ks=()):
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.utils import page_pattern as PP
    from advancedliteratemachinery_amd.utils import page_regex as PR
    masks, first, last, follow, pred, P = auto
    pool, po, pl, jobs = tables(texts, P.size)
    J, sigma = jobs.shape[0], masks.shape[1] - 1
    columns = int(pl[jobs[:, 0]].astype(np.int64).sum())
    sc = PR.RegexSearcher('cuda')
    run_ms, got = [], None
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        got = sc.run(pool, po, pl, masks, first, last, follow, pred, P, jobs, max_hits)   # ends with the download: synchronous
        if i >= warmup:
            run_ms.append((time.perf_counter() - t0) * 1e3)
    # the kernel alone, between device events, on tables that are already on the device
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to('cuda')      # noqa: E731
    i64 = lambda v: up(np.ascontiguousarray(v).reshape(-1).view(np.int64))   # noqa: E731
    d = [up(pool), up(po), up(pl), i64(masks), i64(first), i64(last), i64(follow), i64(pred), up(P), up(jobs.reshape(-1))]
    outs = [torch.empty(n, dtype=torch.int32, device='cuda') for n in (2 * J, J, 3 * max_hits * J)]

    def launch():
        ops.page_regex_search(d[0], pool.size, d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], sigma, max_hits, best=outs[0], n_hits=outs[1], hits=outs[2])
    ms = events(launch, repeats, warmup)
    same = bool((outs[1].cpu().numpy() == got['n_hits']).all() and (outs[2].cpu().numpy().reshape(J, max_hits, 3) == got['hits']).all())
    # the definition on a subsample, scaled by text columns
    pick = np.sort(np.random.RandomState(1).permutation(J)[:min(cpu_jobs, J)])
    t0 = time.perf_counter()
    want = PR.search_cpu(pool, po, pl, masks, first, last, follow, pred, P, jobs[pick], max_hits)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    sub_columns = int(pl[jobs[pick, 0]].astype(np.int64).sum())
    scaled = cpu_ms * columns / sub_columns
    equal = all(bool((got[key][pick] == want[key]).all()) for key in ('best', 'n_hits', 'hits'))
    doc = dict(leg=name, jobs=int(J), pages=int(pl.size), expressions=int(P.size), pool_bytes=int(pool.size), sigma=int(sigma), max_hits=max_hits, text_columns=columns,
               mean_page=round(float(pl.mean()), 1), mean_P=round(float(P.mean()), 1), hits=int(got['n_hits'].sum()), jobs_with_hits=int((got['n_hits'] > 0).sum()),
               run=spread(run_ms), kernel=dict(spread(ms), launches=1, g_columns_per_s=round(columns / statistics.median(ms) / 1e6, 2), equal_to_the_run=same),
               host=dict(jobs=int(pick.size), ms=round(cpu_ms, 1), columns=sub_columns, scaled_ms=round(scaled, 1),
                         scaling='search_cpu on %d jobs of a fixed permutation, multiplied by (columns of the leg) / (columns of those jobs) = %.1f'
                         % (pick.size, columns / sub_columns)),
               answers_equal_on_the_subsample=equal, speedup_scaled=round(scaled / statistics.median(run_ms), 1))
    if flat is not None:
        # the same jobs through omp_page_pattern_search at k = 0
        fmasks, opt, fP, k = flat
        e = [i64(fmasks), up(opt.view(np.int64)), up(fP), up(k)]
        parts = PP.chunk_jobs(J, max_hits)
        scratch = torch.empty(ops.page_pattern_scratch_bytes(max(hi - lo for lo, hi in parts), max_hits), dtype=torch.uint8, device='cuda')
        outs2 = [torch.empty(n, dtype=torch.int32, device='cuda') for n in (2 * J, J, 3 * max_hits * J)]

        def launch2():
            for lo, hi in parts:
                ops.page_pattern_search(d[0], pool.size, d[1], d[2], e[0], e[1], e[2], e[3], d[9][2 * lo:2 * hi], sigma, max_hits, scratch,
                                        best=outs2[0][2 * lo:2 * hi], n_hits=outs2[1][lo:hi], hits=outs2[2][3 * max_hits * lo:3 * max_hits * hi])
        ms2 = events(launch2, repeats, warmup)
        doc['page_pattern_k0'] = dict(spread(ms2), launches=len(parts), regex_over_pattern=round(statistics.median(ms) / statistics.median(ms2), 2),
                                      n_hits_equal=bool((outs[1] == outs2[1]).all().item()), hits_equal=bool((outs[2] == outs2[2]).all().item()),
                                      best_equal=bool((outs[0] == outs2[0]).all().item()))
    if ks:
        e = None if flat is None else [i64(flat[0]), up(flat[1].view(np.int64)), up(flat[2])]
        doc['with_errors'] = [time_fuzzy(K, d, e, (pool, po, pl, masks, first, last, follow, pred, P, jobs), J, sigma, max_hits, statistics.median(ms), pick[:4], repeats,
                                         warmup) for K in ks]
    print(json.dumps(doc), flush=True)
    return doc


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pages', type=int, default=500)
    p.add_argument('--chars', type=int, default=5000)
    p.add_argument('--expressions', type=int, default=200)
    p.add_argument('--long_pages', type=int, default=16)
    p.add_argument('--long_chars', type=int, default=40000)
    p.add_argument('--long_expressions', type=int, default=1000)
    p.add_argument('--alphabet', type=int, default=60)
    p.add_argument('--max_hits', type=int, default=16)
    p.add_argument('--cpu_jobs', type=int, default=100)
    p.add_argument('--long_cpu_jobs', type=int, default=20)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--k', default='', help='comma-separated tolerances, e.g. 0,1,2,4: adds the search with errors to every leg')
    p.add_argument('--out', default=os.path.join('profiles', 'page_regex_bench.json'))
    a = p.parse_args()
    ks = tuple(int(v) for v in a.k.split(',') if v.strip() != '')
    if any(not 0 <= v <= 4 for v in ks):
        raise SystemExit('--k takes tolerances 0 .. 4, got %r' % (a.k,))
    if not torch.cuda.is_available():
        raise SystemExit('page_regex_bench needs the GPU: a timing taken anywhere else says nothing')
    rng = np.random.RandomState(0)
    sets = (('%d pages of about %d' % (a.pages, a.chars), plant_runs(rng, make_pages(rng, a.pages, a.chars, a.alphabet)), a.expressions, a.cpu_jobs),
            ('%d pages of about %d' % (a.long_pages, a.long_chars), plant_runs(rng, make_pages(rng, a.long_pages, a.long_chars, a.alphabet)), a.long_expressions,
             a.long_cpu_jobs))
    legs = []
    for what, texts, count, cpu_jobs in sets:
        auto, flat = make_flat(np.random.RandomState(1), texts, count, a.alphabet)
        legs.append(time_leg('%s x %d flat shapes' % (what, count), texts, auto, a.max_hits, cpu_jobs, a.repeats, a.warmup, flat=flat, ks=ks))
        legs.append(time_leg('%s x %d alternations of literals' % (what, count), texts, make_alternations(np.random.RandomState(2), texts, count, a.alphabet), a.max_hits,
                             cpu_jobs, a.repeats, a.warmup, ks=ks))
        legs.append(time_leg('%s x %d loops over planted digit runs' % (what, count), texts, make_loops(np.random.RandomState(3), count, a.alphabet), a.max_hits, cpu_jobs,
                             a.repeats, a.warmup, ks=ks))
        legs.append(time_leg('%s x 1 never-dying a.*b' % what, texts, make_never_dying(a.alphabet), a.max_hits, min(cpu_jobs, 4), a.repeats, a.warmup, ks=ks))
    doc = dict(device=torch.cuda.get_device_name(0), k=list(ks), alphabet=a.alphabet, repeats=a.repeats, warmup=a.warmup, legs=legs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
