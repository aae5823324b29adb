"""Page text alignment: ONE PageAligner.run (utils/page_align.py -- the packed upload, omp_page_align per chunk, the download) over the
pairs of the page-text bench, against omp_page_edit_distance on the same pairs (what recording and walking cost on top of the
distance) and against the numpy definition pairs_align_cpu on a subsample.

  python tools/page_align_bench.py [--pages 500] [--chars 5000] [--long_pages 16] [--long_chars 40000] [--alphabet 80] [--cpu_pairs 2]
                                   [--long_cpu_chars 8000] [--repeats 5] [--warmup 1] [--out profiles/page_align_bench.json]

The pairs are tools/page_text_bench.py's (make_leg with one setting: a page against itself cut into 12 pieces, two neighbours swapped,
5 % character errors).  Per leg the tool times whole run calls (host clock; the call ends with the download), the launches of all
chunks alone between device events on tables that are already on the device, omp_page_edit_distance alone on the same pairs, and
pairs_align_cpu on the first `cpu_pairs` pairs; that host time is SCALED to the leg by the ratio of table cells (sum of la x lb).  The
definition keeps the whole table, so on the long leg it runs on the first pair CUT to `long_cpu_chars` characters a side and is scaled
from there; the leg says so.  Counts and maps of the (uncut) subsample are compared.  One JSON document; every leg is also printed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def spread(ms):
    v = sorted(ms)
    return dict(ms=[round(t, 3) for t in ms], ms_median=round(statistics.median(v), 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3))


def time_leg(name, packed, sigma, cpu_pairs, cpu_chars, repeats, warmup):
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.utils import page_align as PA
    pool, a_off, a_len, b_off, b_len = packed
    P = a_len.size
    cells = int((a_len.astype(np.int64) * b_len.astype(np.int64)).sum())
    al = PA.PageAligner('cuda')
    run_ms, got = [], None
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        got = al.run(pool, a_off, a_len, b_off, b_len, sigma)                # ends with the download: synchronous
        if k >= warmup:
            run_ms.append((time.perf_counter() - t0) * 1e3)
    parts = PA.chunk_pairs(a_len, b_len, al.scratch_cap)
    need = np.asarray([ops.page_align_scratch_bytes(la, lb) for la, lb in zip(a_len.tolist(), b_len.tolist())], dtype=np.int64)
    # the launches alone, between device events, on tables that are already on the device
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to('cuda')      # noqa: E731
    map_off = PA.dense_map_off(a_len, b_len)
    scratch_off = np.concatenate([np.cumsum(need[lo:hi]) - need[lo:hi] for lo, hi in parts])
    d = [up(v) for v in (pool, a_off, a_len, b_off, b_len, map_off, scratch_off)]
    maps = torch.empty(int(got['maps'].size) + 1, dtype=torch.int32, device='cuda')
    counts = torch.empty(4 * P, dtype=torch.int32, device='cuda')
    ms = []
    for k in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for lo, hi in parts:
            ops.page_align(d[0], pool.size, d[1][lo:hi], d[2][lo:hi], d[3][lo:hi], d[4][lo:hi], d[5][lo:hi], d[6][lo:hi], sigma, al.scratch, maps,
                           counts=counts[4 * lo:4 * hi])
        e1.record()
        e1.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    same = bool((counts.cpu().numpy().reshape(P, 4) == got['counts']).all() and (maps[:-1].cpu().numpy() == got['maps']).all())
    kernel = dict(spread(ms), launches=len(parts), g_cells_per_s=round(cells / statistics.median(ms) / 1e6, 2), equal_to_the_run=same)
    # the distance alone on the same pairs
    pt_scratch = torch.empty(ops.page_scratch_bytes(P), dtype=torch.uint8, device='cuda')
    dist = torch.empty(P, dtype=torch.int32, device='cuda')
    dms = []
    for k in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.page_edit_distance(d[0], pool.size, d[1], d[2], d[3], d[4], sigma, pt_scratch, dist=dist)
        e1.record()
        e1.synchronize()
        if k >= warmup:
            dms.append(e0.elapsed_time(e1))
    distance = dict(spread(dms), equal_to_the_counts=bool((dist.cpu().numpy() == got['counts'][:, 1:].sum(1)).all()))
    # the definition on a subsample, scaled by table cells
    n = min(cpu_pairs, P)
    cut = cpu_chars is not None and int(max(a_len[:n].max(), b_len[:n].max())) > cpu_chars
    sa_len = np.minimum(a_len[:n], cpu_chars) if cut else a_len[:n]
    sb_len = np.minimum(b_len[:n], cpu_chars) if cut else b_len[:n]
    t0 = time.perf_counter()
    want_counts, want_maps = PA.pairs_align_cpu(pool, a_off[:n], sa_len, b_off[:n], sb_len, PA.dense_map_off(sa_len, sb_len))
    cpu_ms = (time.perf_counter() - t0) * 1e3
    sub_cells = int((sa_len.astype(np.int64) * sb_len.astype(np.int64)).sum())
    scaled = cpu_ms * cells / sub_cells
    equal = None if cut else bool((got['counts'][:n] == want_counts).all() and (got['maps'][:want_maps.size] == want_maps).all())
    doc = dict(leg=name, pairs=int(P), pool_bytes=int(pool.size), sigma=int(sigma), cells=cells, mean_la=round(float(a_len.mean()), 1),
               mean_lb=round(float(b_len.mean()), 1), chunks=al.chunks, scratch_cap=al.scratch_cap, scratch_bytes_all_pairs=int(need.sum()),
               scratch_bytes_largest_pair=int(need.max()), pairs_per_chunk=[hi - lo for lo, hi in parts][:8], map_entries=int(got['maps'].size),
               counts_sum=got['counts'].sum(0).tolist(), run=spread(run_ms), kernel=kernel, distance_kernel=distance,
               kernel_over_distance=round(statistics.median(ms) / statistics.median(dms), 2),
               host=dict(pairs=int(n), cut_to=int(cpu_chars) if cut else None, ms=round(cpu_ms, 1), cells=sub_cells, scaled_ms=round(scaled, 1),
                         scaling='pairs_align_cpu on the first %d pairs%s, multiplied by (cells of the leg) / (cells of those pairs) = %.1f'
                                 % (n, ' cut to %d characters a side' % cpu_chars if cut else '', cells / sub_cells)),
               answers_equal_on_the_subsample=equal, speedup_scaled=round(scaled / statistics.median(run_ms), 1))
    print(json.dumps(doc), flush=True)
    return doc


def main():
    from page_text_bench import make_leg
    p = argparse.ArgumentParser()
    p.add_argument('--pages', type=int, default=500)
    p.add_argument('--chars', type=int, default=5000)
    p.add_argument('--long_pages', type=int, default=16)
    p.add_argument('--long_chars', type=int, default=40000)
    p.add_argument('--alphabet', type=int, default=80)
    p.add_argument('--cpu_pairs', type=int, default=2)
    p.add_argument('--long_cpu_chars', type=int, default=8000)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--out', default=os.path.join('profiles', 'page_align_bench.json'))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('page_align_bench needs the GPU: a timing taken anywhere else says nothing')
    rng = np.random.RandomState(0)
    legs = []
    if a.pages > 0:
        legs.append(time_leg('pages', make_leg(rng, a.pages, 1, a.chars, a.alphabet), a.alphabet, a.cpu_pairs, None, a.repeats, a.warmup))
    if a.long_pages > 0:
        legs.append(time_leg('long pages', make_leg(rng, a.long_pages, 1, a.long_chars, a.alphabet), a.alphabet, 1, a.long_cpu_chars, a.repeats, a.warmup))
    doc = dict(device=torch.cuda.get_device_name(0), alphabet=a.alphabet, repeats=a.repeats, warmup=a.warmup, legs=legs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
