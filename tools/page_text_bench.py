"""Page text scoring: ONE PageTextScorer.run (utils/page_text.py -- the packed upload, omp_page_edit_distance, the download) over
pairs = pages x settings, against the numpy definition pairs_cpu on a subsample of the same pairs.

  python tools/page_text_bench.py [--pages 500] [--settings 8] [--chars 5000] [--long_pages 16] [--long_chars 40000] [--alphabet 80]
                                  [--cpu_pairs 4] [--long_cpu_pairs 1] [--repeats 5] [--warmup 1] [--out profiles/page_text_bench.json]

Seeded pages: a ground-truth page is `chars` (+- 10 %) characters drawn from `alphabet` letters; its prediction under a setting is the
page cut into 12 pieces that are permuted (the reading-order error a setting makes), with substitutions, insertions and deletions at
5 % (the recogniser's errors).  A page's ground truth is stored once and shared by its settings, as sweep_reading packs it.
Per leg the tool times whole run calls (host clock; the call ends with the download), the kernel alone between device events, and
pairs_cpu on the first `cpu_pairs` pairs; that host time is SCALED to the leg by the ratio of table cells (sum of la x lb), which is what
the definition's work grows with.  The distances of the subsample are compared.  A third leg repeats the first with the kernel told a
larger alphabet than the pages hold (sigma 128 and 254: the same work with (sigma + 1) x 512 bytes of LDS per wave), which shows what
the LDS footprint of one wave per workgroup costs in occupancy; a fourth repeats it on pages of 26 letters (13.8 KB of LDS per wave).
One JSON document; every leg is also printed as it ends."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_leg(rng, pages, settings, chars, alphabet, rate=0.05, pieces=12):
    """-> (pool, a_off, a_len, b_off, b_len): pair (page g, setting k) at index k * pages + g, ground truth shared"""
    chunks, total = [], 0
    a_off, a_len, b_off, b_len = [], [], [], []
    truth = []
    for _ in range(pages):
        n = int(chars * (0.9 + 0.2 * rng.rand()))
        t = rng.randint(0, alphabet, n).astype(np.uint8)
        truth.append((total, t))
        chunks.append(t)
        total += n
    for _ in range(settings):
        for off, t in truth:
            cuts = np.sort(rng.choice(np.arange(1, t.size), pieces - 1, replace=False))
            parts = np.split(t, cuts)
            order = np.arange(pieces)
            swap = rng.randint(0, pieces - 1)
            order[[swap, swap + 1]] = order[[swap + 1, swap]]           # two neighbouring pieces change places
            p = np.concatenate([parts[k] for k in order])
            u = rng.rand(p.size)
            keep = u >= rate / 3
            p = np.where((u >= rate / 3) & (u < 2 * rate / 3), rng.randint(0, alphabet, p.size), p)[keep].astype(np.uint8)
            ins = np.flatnonzero(rng.rand(p.size) < rate / 3)
            p = np.insert(p, ins, rng.randint(0, alphabet, ins.size).astype(np.uint8))
            a_off.append(total)
            a_len.append(p.size)
            b_off.append(off)
            b_len.append(t.size)
            chunks.append(p)
            total += p.size
    i32 = lambda v: np.asarray(v, dtype=np.int32)                            # noqa: E731
    return np.concatenate(chunks), i32(a_off), i32(a_len), i32(b_off), i32(b_len)


def spread(ms):
    v = sorted(ms)
    return dict(ms=[round(t, 3) for t in ms], ms_median=round(statistics.median(v), 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3))


def time_leg(name, packed, sigma, cpu_pairs, repeats, warmup, told_sigmas=()):
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.utils import page_text as PT
    pool, a_off, a_len, b_off, b_len = packed
    P = a_len.size
    cells = int((a_len.astype(np.int64) * b_len.astype(np.int64)).sum())
    sc = PT.PageTextScorer('cuda')
    run_ms, got = [], None
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        got = sc.run(pool, a_off, a_len, b_off, b_len, sigma)                # ends with the download: synchronous
        if k >= warmup:
            run_ms.append((time.perf_counter() - t0) * 1e3)
    # the kernel alone, between device events, on tables that are already on the device
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to('cuda')      # noqa: E731
    d = [up(v) for v in (pool, a_off, a_len, b_off, b_len)]
    scratch = torch.empty(ops.page_scratch_bytes(P), dtype=torch.uint8, device='cuda')
    dist = torch.empty(P, dtype=torch.int32, device='cuda')
    kernel = {}
    for s in (sigma,) + tuple(s for s in told_sigmas if s > sigma):
        ms = []
        for k in range(warmup + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.page_edit_distance(d[0], pool.size, d[1], d[2], d[3], d[4], s, scratch, dist=dist)
            e1.record()
            e1.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
        same = bool((dist.cpu().numpy() == got).all())
        kernel[str(s)] = dict(spread(ms), lds_bytes_per_wave=(s + 1) * 512, waves_per_cu_by_lds=min(32, (160 * 1024) // ((s + 1) * 512)),
                              g_cells_per_s=round(cells / statistics.median(ms) / 1e6, 2), equal_to_the_run=same)
    # the definition on a subsample, scaled by table cells
    n = min(cpu_pairs, P)
    t0 = time.perf_counter()
    want = PT.pairs_cpu(pool, a_off[:n], a_len[:n], b_off[:n], b_len[:n])
    cpu_ms = (time.perf_counter() - t0) * 1e3
    sub_cells = int((a_len[:n].astype(np.int64) * b_len[:n].astype(np.int64)).sum())
    scaled = cpu_ms * cells / sub_cells
    doc = dict(leg=name, pairs=int(P), pool_bytes=int(pool.size), sigma=int(sigma), cells=cells, mean_la=round(float(a_len.mean()), 1),
               mean_lb=round(float(b_len.mean()), 1), chunks=sc.chunks, mean_distance=round(float(got.mean()), 1), run=spread(run_ms), kernel=kernel,
               run_g_cells_per_s=round(cells / statistics.median(run_ms) / 1e6, 2),
               host=dict(pairs=int(n), ms=round(cpu_ms, 1), cells=sub_cells, scaled_ms=round(scaled, 1),
                         scaling='pairs_cpu on the first %d pairs, multiplied by (cells of the leg) / (cells of those pairs) = %.1f' % (n, cells / sub_cells)),
               answers_equal_on_the_subsample=bool((got[:n] == want).all()),
               speedup_scaled=round(scaled / statistics.median(run_ms), 1))
    print(json.dumps(doc), flush=True)
    return doc


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pages', type=int, default=500)
    p.add_argument('--settings', type=int, default=8)
    p.add_argument('--chars', type=int, default=5000)
    p.add_argument('--long_pages', type=int, default=16)
    p.add_argument('--long_chars', type=int, default=40000)
    p.add_argument('--alphabet', type=int, default=80)
    p.add_argument('--cpu_pairs', type=int, default=4)
    p.add_argument('--long_cpu_pairs', type=int, default=1)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--out', default=os.path.join('profiles', 'page_text_bench.json'))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('page_text_bench needs the GPU: a timing taken anywhere else says nothing')
    rng = np.random.RandomState(0)
    legs = [time_leg('pages', make_leg(rng, a.pages, a.settings, a.chars, a.alphabet), a.alphabet, a.cpu_pairs, a.repeats, a.warmup, told_sigmas=(128, 254)),
            time_leg('long pages', make_leg(rng, a.long_pages, a.settings, a.long_chars, a.alphabet), a.alphabet, a.long_cpu_pairs, a.repeats, a.warmup),
            time_leg('pages, 26 letters', make_leg(rng, a.pages, a.settings, a.chars, 26), 26, a.cpu_pairs, a.repeats, a.warmup)]
    doc = dict(device=torch.cuda.get_device_name(0), alphabet=a.alphabet, settings=a.settings, repeats=a.repeats, warmup=a.warmup, legs=legs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
