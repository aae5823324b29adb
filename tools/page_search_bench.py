"""Page search: ONE PageSearcher.run (utils/page_search.py -- the packed upload, omp_page_search, the download) over jobs = pages x
queries, against the numpy definition search_cpu on a subsample of the same jobs.

  python tools/page_search_bench.py [--pages 500] [--chars 5000] [--queries 200] [--long_pages 16] [--long_chars 40000]
                                    [--long_queries 1000] [--alphabet 60] [--max_hits 16] [--cpu_jobs 200] [--long_cpu_jobs 40]
                                    [--repeats 5] [--warmup 1] [--out profiles/page_search_bench.json]

Seeded pages: `chars` (+- 10 %) characters drawn from `alphabet` letters, a blank every 3 to 9 characters.  A query is 4 to 24
characters cut from a random page at a random place, half of them with one character replaced (a misread label); its tolerance is
tolerance(m) = the default of find_text.  Every query is searched on every page.
Per leg the tool times whole run calls (host clock; the call ends with the download), the kernel alone between device events on tables
that are already on the device, and search_cpu on the first `cpu_jobs` jobs of a fixed random permutation; that host time is SCALED
to the leg by the ratio of table cells (sum of m x n), which is what the definition's work grows with, and is stated as such.  The
answers of the subsample are compared.  One JSON document; every leg is also printed as it ends."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_leg(rng, pages, chars, queries, alphabet):
    """-> (pool, page_off, page_len, query_off, query_len, jobs, k, sigma): code alphabet - 1 is the blank"""
    from advancedliteratemachinery_amd.utils import page_search as PS
    texts = []
    for _ in range(pages):
        n = int(chars * (0.9 + 0.2 * rng.rand()))
        t = rng.randint(0, alphabet - 1, n).astype(np.uint8)
        at = np.cumsum(rng.randint(4, 11, n // 4))
        t[at[at < n]] = alphabet - 1
        texts.append(t)
    qs = []
    for i in range(queries):
        t = texts[int(rng.randint(0, pages))]
        m = int(rng.randint(4, 25))
        at = int(rng.randint(0, t.size - m))
        q = t[at:at + m].copy()
        if i % 2:
            q[int(rng.randint(0, m))] = rng.randint(0, alphabet - 1)
        qs.append(q)
    page_len = np.asarray([t.size for t in texts], dtype=np.int32)
    query_len = np.asarray([q.size for q in qs], dtype=np.int32)
    lens = np.concatenate([page_len, query_len]).astype(np.int64)
    off = (np.cumsum(lens) - lens).astype(np.int32)
    jobs = np.stack(np.meshgrid(np.arange(pages), np.arange(queries), indexing='ij'), -1).reshape(-1, 2).astype(np.int32)
    k = np.asarray([PS.tolerance(int(m)) for m in query_len], dtype=np.int32)
    return np.concatenate(texts + qs), off[:pages], page_len, off[pages:], query_len, jobs, k, alphabet


def spread(ms):
    v = sorted(ms)
    return dict(ms=[round(t, 3) for t in ms], ms_median=round(statistics.median(v), 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3))


def time_leg(name, leg, max_hits, cpu_jobs, repeats, warmup):
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.utils import page_search as PS
    pool, po, pl, qo, ql, jobs, k, sigma = leg
    J = jobs.shape[0]
    cells = int((pl[jobs[:, 0]].astype(np.int64) * ql[jobs[:, 1]].astype(np.int64)).sum())
    columns = int(pl[jobs[:, 0]].astype(np.int64).sum())
    sc = PS.PageSearcher('cuda')
    run_ms, got = [], None
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        got = sc.run(pool, po, pl, qo, ql, jobs, k, max_hits, sigma=sigma)   # ends with the download: synchronous
        if i >= warmup:
            run_ms.append((time.perf_counter() - t0) * 1e3)
    # the kernel alone, between device events, on tables that are already on the device; chunked as the run chunks
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to('cuda')      # noqa: E731
    d = [up(v) for v in (pool, po, pl, qo, ql, jobs.reshape(-1), k)]
    parts = PS.chunk_jobs(J, max_hits)
    scratch = torch.empty(ops.page_search_scratch_bytes(max(hi - lo for lo, hi in parts), max_hits), dtype=torch.uint8, device='cuda')
    outs = [torch.empty(n, dtype=torch.int32, device='cuda') for n in (2 * J, J, 3 * max_hits * J)]
    ms = []
    for i in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for lo, hi in parts:
            ops.page_search(d[0], pool.size, d[1], d[2], d[3], d[4], d[6], d[5][2 * lo:2 * hi], sigma, max_hits, scratch, best=outs[0][2 * lo:2 * hi],
                            n_hits=outs[1][lo:hi], hits=outs[2][3 * max_hits * lo:3 * max_hits * hi])
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    same = bool((outs[1].cpu().numpy() == got['n_hits']).all() and (outs[2].cpu().numpy().reshape(J, max_hits, 3) == got['hits']).all())
    # the definition on a subsample, scaled by table cells
    pick = np.sort(np.random.RandomState(1).permutation(J)[:min(cpu_jobs, J)])
    t0 = time.perf_counter()
    want = PS.search_cpu(pool, po, pl, qo, ql, jobs[pick], k, max_hits)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    sub_cells = int((pl[jobs[pick, 0]].astype(np.int64) * ql[jobs[pick, 1]].astype(np.int64)).sum())
    scaled = cpu_ms * cells / sub_cells
    equal = all(bool((got[key][pick] == want[key]).all()) for key in ('best', 'n_hits', 'hits'))
    doc = dict(leg=name, jobs=int(J), pages=int(pl.size), queries=int(ql.size), pool_bytes=int(pool.size), sigma=int(sigma), max_hits=max_hits, cells=cells,
               text_columns=columns, mean_page=round(float(pl.mean()), 1), mean_query=round(float(ql.mean()), 1), chunks=sc.chunks,
               hits=int(got['n_hits'].sum()), jobs_with_hits=int((got['n_hits'] > 0).sum()), run=spread(run_ms),
               kernel=dict(spread(ms), launches=len(parts), g_columns_per_s=round(columns / statistics.median(ms) / 1e6, 2), equal_to_the_run=same),
               host=dict(jobs=int(pick.size), ms=round(cpu_ms, 1), cells=sub_cells, scaled_ms=round(scaled, 1),
                         scaling='search_cpu on %d jobs of a fixed permutation, multiplied by (cells of the leg) / (cells of those jobs) = %.1f'
                         % (pick.size, cells / sub_cells)),
               answers_equal_on_the_subsample=equal, speedup_scaled=round(scaled / statistics.median(run_ms), 1))
    print(json.dumps(doc), flush=True)
    return doc


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pages', type=int, default=500)
    p.add_argument('--chars', type=int, default=5000)
    p.add_argument('--queries', type=int, default=200)
    p.add_argument('--long_pages', type=int, default=16)
    p.add_argument('--long_chars', type=int, default=40000)
    p.add_argument('--long_queries', type=int, default=1000)
    p.add_argument('--alphabet', type=int, default=60)
    p.add_argument('--max_hits', type=int, default=16)
    p.add_argument('--cpu_jobs', type=int, default=200)
    p.add_argument('--long_cpu_jobs', type=int, default=40)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--out', default=os.path.join('profiles', 'page_search_bench.json'))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('page_search_bench needs the GPU: a timing taken anywhere else says nothing')
    rng = np.random.RandomState(0)
    legs = [time_leg('pages', make_leg(rng, a.pages, a.chars, a.queries, a.alphabet), a.max_hits, a.cpu_jobs, a.repeats, a.warmup),
            time_leg('long pages', make_leg(rng, a.long_pages, a.long_chars, a.long_queries, a.alphabet), a.max_hits, a.long_cpu_jobs, a.repeats, a.warmup)]
    doc = dict(device=torch.cuda.get_device_name(0), alphabet=a.alphabet, repeats=a.repeats, warmup=a.warmup, legs=legs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
