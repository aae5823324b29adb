"""Page patterns: ONE PatternSearcher.run (utils/page_pattern.py -- the packed upload, omp_page_pattern_search, the download) over jobs =
pages x patterns, against the numpy definition search_cpu on a subsample of the same jobs, and against omp_page_search on the same jobs
where every pattern is a literal.

  python tools/page_pattern_bench.py [--pages 500] [--chars 5000] [--patterns 200] [--long_pages 16] [--long_chars 40000]
                                     [--long_patterns 1000] [--alphabet 60] [--max_hits 16] [--cpu_jobs 200] [--long_cpu_jobs 40]
                                     [--repeats 5] [--warmup 1] [--out profiles/page_pattern_bench.json]

Seeded pages as tools/page_search_bench.py makes them: `chars` (+- 10 %) characters drawn from `alphabet` codes, a blank every 3 to 9
characters.  A shape is 8 to 24 positions cut from a random page at a random place: every position's class holds the page's character
there, a third of the positions hold 9 more codes (a `\\d`), and two positions in the middle are optional.  The legs `shapes k=0`, `k=2`
and `k=8` give every shape that tolerance (capped at Mand - 1); every shape is searched on every page.  The leg `literals` runs
tools/page_search_bench.py's phrases (4 to 24 characters, half with one character replaced, k = page_search.tolerance(m) capped at 8)
through BOTH kernels: a literal is a pattern of one-code classes with no optional position, and n_hits and every (end, dist) must agree.
Per leg the tool times whole run calls (host clock; the call ends with the download), the kernel alone between device events on tables
that are already on the device, and search_cpu on the first `cpu_jobs` jobs of a fixed random permutation; that host time is SCALED to
the leg by the ratio of table cells (sum of P x n) and is stated as such.  One JSON document; every leg is also printed as it ends."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_pages(rng, pages, chars, alphabet):
    texts = []
    for _ in range(pages):
        n = int(chars * (0.9 + 0.2 * rng.rand()))
        t = rng.randint(0, alphabet - 1, n).astype(np.uint8)
        at = np.cumsum(rng.randint(4, 11, n // 4))
        t[at[at < n]] = alphabet - 1
        texts.append(t)
    return texts


def tables(texts, jobs_of):
    page_len = np.asarray([t.size for t in texts], dtype=np.int32)
    off = (np.cumsum(page_len.astype(np.int64)) - page_len).astype(np.int32)
    jobs = np.stack(np.meshgrid(np.arange(len(texts)), np.arange(jobs_of), indexing='ij'), -1).reshape(-1, 2).astype(np.int32)
    return np.concatenate(texts), off, page_len, jobs


def make_shapes(rng, texts, patterns, alphabet, k):
    """-> (masks [Q, alphabet + 1], opt, pat_len, k)"""
    masks = np.zeros((patterns, alphabet + 1), dtype=np.uint64)
    opt, P, ks = [], [], []
    for q in range(patterns):
        t = texts[int(rng.randint(0, len(texts)))]
        m = int(rng.randint(8, 25))
        at = int(rng.randint(0, t.size - m))
        for i, c in enumerate(t[at:at + m].tolist()):
            masks[q, c] |= np.uint64(1) << np.uint64(i)
            if i % 3 == 0:
                masks[q, rng.permutation(alphabet - 1)[:9]] |= np.uint64(1) << np.uint64(i)
        opt.append((1 << (m // 2)) | (1 << (m // 2 + 1)))
        P.append(m)
        ks.append(min(k, m - 2 - 1, 8))
    return masks, np.asarray(opt, dtype=np.uint64), np.asarray(P, dtype=np.int32), np.asarray(ks, dtype=np.int32)


def make_literals(rng, texts, patterns, alphabet):
    """tools/page_search_bench.py's phrases -> (the phrases, masks, opt, pat_len, k)"""
    from advancedliteratemachinery_amd.utils import page_search as PS
    qs, masks = [], np.zeros((patterns, alphabet + 1), dtype=np.uint64)
    for i in range(patterns):
        t = texts[int(rng.randint(0, len(texts)))]
        m = int(rng.randint(4, 25))
        at = int(rng.randint(0, t.size - m))
        q = t[at:at + m].copy()
        if i % 2:
            q[int(rng.randint(0, m))] = rng.randint(0, alphabet - 1)
        for j, c in enumerate(q.tolist()):
            masks[i, c] |= np.uint64(1) << np.uint64(j)
        qs.append(q)
    P = np.asarray([q.size for q in qs], dtype=np.int32)
    k = np.asarray([min(PS.tolerance(int(m)), 8) for m in P], dtype=np.int32)
    return qs, masks, np.zeros(patterns, dtype=np.uint64), P, k


def spread(ms):
    v = sorted(ms)
    return dict(ms=[round(t, 3) for t in ms], ms_median=round(statistics.median(v), 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3))


def events(fn, repeats, warmup):
    ms = []
    for i in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def time_leg(name, texts, pats, max_hits, cpu_jobs, repeats, warmup, literals=None):
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.utils import page_pattern as PP
    from advancedliteratemachinery_amd.utils import page_search as PS
    masks, opt, P, k = pats
    pool, po, pl, jobs = tables(texts, P.size)
    J, sigma = jobs.shape[0], masks.shape[1] - 1
    cells = int((pl[jobs[:, 0]].astype(np.int64) * P[jobs[:, 1]].astype(np.int64)).sum())
    columns = int(pl[jobs[:, 0]].astype(np.int64).sum())
    sc = PP.PatternSearcher('cuda')
    run_ms, got = [], None
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        got = sc.run(pool, po, pl, masks, opt, P, jobs, k, max_hits)         # ends with the download: synchronous
        if i >= warmup:
            run_ms.append((time.perf_counter() - t0) * 1e3)
    # the kernel alone, between device events, on tables that are already on the device; chunked as the run chunks
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to('cuda')      # noqa: E731
    d = [up(v) for v in (pool, po, pl, masks.reshape(-1).view(np.int64), opt.view(np.int64), P, k, jobs.reshape(-1))]
    parts = PP.chunk_jobs(J, max_hits)
    scratch = torch.empty(ops.page_pattern_scratch_bytes(max(hi - lo for lo, hi in parts), max_hits), dtype=torch.uint8, device='cuda')
    outs = [torch.empty(n, dtype=torch.int32, device='cuda') for n in (2 * J, J, 3 * max_hits * J)]

    def launch():
        for lo, hi in parts:
            ops.page_pattern_search(d[0], pool.size, d[1], d[2], d[3], d[4], d[5], d[6], d[7][2 * lo:2 * hi], sigma, max_hits, scratch,
                                    best=outs[0][2 * lo:2 * hi], n_hits=outs[1][lo:hi], hits=outs[2][3 * max_hits * lo:3 * max_hits * hi])
    ms = events(launch, repeats, warmup)
    same = bool((outs[1].cpu().numpy() == got['n_hits']).all() and (outs[2].cpu().numpy().reshape(J, max_hits, 3) == got['hits']).all())
    # the definition on a subsample, scaled by table cells
    pick = np.sort(np.random.RandomState(1).permutation(J)[:min(cpu_jobs, J)])
    t0 = time.perf_counter()
    want = PP.search_cpu(pool, po, pl, masks, opt, P, jobs[pick], k, max_hits)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    sub_cells = int((pl[jobs[pick, 0]].astype(np.int64) * P[jobs[pick, 1]].astype(np.int64)).sum())
    scaled = cpu_ms * cells / sub_cells
    equal = all(bool((got[key][pick] == want[key]).all()) for key in ('best', 'n_hits', 'hits'))
    doc = dict(leg=name, jobs=int(J), pages=int(pl.size), patterns=int(P.size), pool_bytes=int(pool.size), sigma=int(sigma), max_hits=max_hits, cells=cells,
               text_columns=columns, mean_page=round(float(pl.mean()), 1), mean_P=round(float(P.mean()), 1), mean_k=round(float(k.mean()), 2), chunks=sc.chunks,
               hits=int(got['n_hits'].sum()), jobs_with_hits=int((got['n_hits'] > 0).sum()), run=spread(run_ms),
               kernel=dict(spread(ms), launches=len(parts), g_columns_per_s=round(columns / statistics.median(ms) / 1e6, 2),
                           ns_per_column_per_row=round(statistics.median(ms) * 1e6 / float((pl[jobs[:, 0]].astype(np.int64) * (k[jobs[:, 1]] + 1)).sum()), 5),
                           equal_to_the_run=same),
               host=dict(jobs=int(pick.size), ms=round(cpu_ms, 1), cells=sub_cells, scaled_ms=round(scaled, 1),
                         scaling='search_cpu on %d jobs of a fixed permutation, multiplied by (cells of the leg) / (cells of those jobs) = %.1f'
                         % (pick.size, cells / sub_cells)),
               answers_equal_on_the_subsample=equal, speedup_scaled=round(scaled / statistics.median(run_ms), 1))
    if literals is not None:
        # the same jobs through omp_page_search: the phrases go behind the pages in one pool
        lens = np.asarray([q.size for q in literals], dtype=np.int64)
        qo = (pool.size + np.cumsum(lens) - lens).astype(np.int32)
        pool2 = np.concatenate([pool] + literals)
        e = [up(v) for v in (pool2, qo, lens.astype(np.int32))]
        parts2 = PS.chunk_jobs(J, max_hits)
        scratch2 = torch.empty(ops.page_search_scratch_bytes(max(hi - lo for lo, hi in parts2), max_hits), dtype=torch.uint8, device='cuda')
        outs2 = [torch.empty(n, dtype=torch.int32, device='cuda') for n in (2 * J, J, 3 * max_hits * J)]

        def launch2():
            for lo, hi in parts2:
                ops.page_search(e[0], pool2.size, d[1], d[2], e[1], e[2], d[6], d[7][2 * lo:2 * hi], sigma, max_hits, scratch2, best=outs2[0][2 * lo:2 * hi],
                                n_hits=outs2[1][lo:hi], hits=outs2[2][3 * max_hits * lo:3 * max_hits * hi])
        ms2 = events(launch2, repeats, warmup)
        h1, h2 = outs[2].cpu().numpy().reshape(J, max_hits, 3), outs2[2].cpu().numpy().reshape(J, max_hits, 3)
        doc['page_search'] = dict(spread(ms2), launches=len(parts2), pattern_over_search=round(statistics.median(ms) / statistics.median(ms2), 2),
                                  n_hits_equal=bool((outs[1] == outs2[1]).all().item()), ends_and_dists_equal=bool((h1[:, :, :2] == h2[:, :, :2]).all()),
                                  starts_at_or_before=bool((h1[:, :, 2] <= h2[:, :, 2]).all()))
    print(json.dumps(doc), flush=True)
    return doc


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pages', type=int, default=500)
    p.add_argument('--chars', type=int, default=5000)
    p.add_argument('--patterns', type=int, default=200)
    p.add_argument('--long_pages', type=int, default=16)
    p.add_argument('--long_chars', type=int, default=40000)
    p.add_argument('--long_patterns', type=int, default=1000)
    p.add_argument('--alphabet', type=int, default=60)
    p.add_argument('--max_hits', type=int, default=16)
    p.add_argument('--cpu_jobs', type=int, default=200)
    p.add_argument('--long_cpu_jobs', type=int, default=40)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--out', default=os.path.join('profiles', 'page_pattern_bench.json'))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('page_pattern_bench needs the GPU: a timing taken anywhere else says nothing')
    rng = np.random.RandomState(0)
    texts = make_pages(rng, a.pages, a.chars, a.alphabet)
    long_texts = make_pages(rng, a.long_pages, a.long_chars, a.alphabet)
    legs = []
    for k in (0, 2, 8):
        legs.append(time_leg('shapes k=%d' % k, texts, make_shapes(np.random.RandomState(1), texts, a.patterns, a.alphabet, k), a.max_hits, a.cpu_jobs, a.repeats,
                             a.warmup))
    legs.append(time_leg('long pages, shapes k=2', long_texts, make_shapes(rng, long_texts, a.long_patterns, a.alphabet, 2), a.max_hits, a.long_cpu_jobs, a.repeats,
                         a.warmup))
    lit = make_literals(rng, texts, a.patterns, a.alphabet)
    legs.append(time_leg('literals', texts, lit[1:], a.max_hits, a.cpu_jobs, a.repeats, a.warmup, literals=lit[0]))
    doc = dict(device=torch.cuda.get_device_name(0), alphabet=a.alphabet, repeats=a.repeats, warmup=a.warmup, legs=legs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
