"""Overlap suppression: ONE device call (utils/overlap.py: OverlapSuppressor -- host packing, the upload, omp_polygon_overlap,
omp_polygon_keep, the download) against the numpy specification suppress_cpu on the host, for the same polygons.

  python tools/overlap_bench.py [--images 160] [--words 64,512] [--grid 1000] [--t 500] [--measure iou] [--repeats 5] [--warmup 1]
                                [--host-images 8] [--out profiles/overlap_bench.json]

Seeded word-like polygons: every image holds --words rotated rectangles resampled to 16 points, a third of them near-duplicates of
another word of the image (what overlapping windows return).  The two sides alternate inside every repeat; per side the tool reports
the median wall-clock ms and the min .. max spread, and `faster` only when the device's SLOWEST repeat beats the host's FASTEST.  The
host specification is a brute force; on more than --host-images images it is timed on the first --host-images and scaled by the image
count (images are independent groups, its cost is a sum over them), which the document says in `host_scaled_from`.  The answers of
the two sides are compared on the images both ran.  One JSON document, also printed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def page(rng, words, grid):
    """one image's polygons: words on text lines, a third of them jittered copies of an earlier word"""
    out = np.zeros((words, 32), dtype=np.int32)
    for i in range(words):
        if i and rng.rand() < 1.0 / 3.0:
            out[i] = out[rng.randint(i)] + rng.randint(-2, 3, 32)
            continue
        w, h = rng.randint(grid // 30, grid // 8), rng.randint(grid // 80, grid // 30)
        x, y = rng.randint(w, grid - w), rng.randint(h, grid - h)
        th = rng.uniform(-0.15, 0.15)
        u = np.linspace(-w / 2.0, w / 2.0, 8)
        px, py = np.concatenate([u, u[::-1]]), np.concatenate([np.full(8, -h / 2.0), np.full(8, h / 2.0)])
        out[i, 0::2] = np.round(x + px * np.cos(th) - py * np.sin(th))
        out[i, 1::2] = np.round(y + px * np.sin(th) + py * np.cos(th))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--images', type=int, default=160)
    p.add_argument('--words', default='64,512')
    p.add_argument('--grid', type=int, default=1000)
    p.add_argument('--t', type=int, default=500)
    p.add_argument('--measure', default='iou')
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--host-images', type=int, default=8)
    p.add_argument('--out', default=os.path.join('profiles', 'overlap_bench.json'))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('overlap_bench needs the GPU: a timing taken anywhere else says nothing')
    from advancedliteratemachinery_amd.utils import overlap as OV
    sup = OV.OverlapSuppressor('cuda', a.grid)
    doc = dict(images=a.images, grid=a.grid, t=a.t, measure=a.measure, repeats=a.repeats, warmup=a.warmup, results=[])
    for words in (int(v) for v in a.words.split(',')):
        rng = np.random.RandomState(words)
        polys = np.concatenate([page(rng, words, a.grid) for _ in range(a.images)])
        gs = np.arange(a.images + 1, dtype=np.int32) * words
        hb = min(a.images, a.host_images)
        d_polys = torch.from_numpy(polys).to('cuda')          # the raw ids are on the device already (r[0][1] of the engine's result)

        def device():
            t0 = time.perf_counter()
            owner, _ = sup(d_polys, gs, None, a.t, a.measure)   # ends with the download: synchronous
            return (time.perf_counter() - t0) * 1e3, owner

        def host():
            t0 = time.perf_counter()
            owner, _ = OV.suppress_cpu(polys[:hb * words], gs[:hb + 1], np.arange(hb * words), a.t, a.measure, a.grid)
            return (time.perf_counter() - t0) * 1e3 * a.images / hb, owner

        ms = dict(device=[], host=[])
        for _ in range(a.warmup):
            device(), host()
        for _ in range(a.repeats):
            for name, fn in (('device', device), ('host', host)):   # alternating: both sides see the same state of a shared machine
                t, owner = fn()
                ms[name].append(t)
                ms[name + '_owner'] = owner
        same = bool((ms['device_owner'][:hb * words] == ms['host_owner']).all())
        res = dict(words_per_image=words, polygons=int(polys.shape[0]), kept=int((ms['device_owner'] == np.arange(len(polys))).sum()),
                   answers_equal_on_host_images=same, host_scaled_from=hb)
        for name in ('device', 'host'):
            v = sorted(ms[name])
            res[name] = dict(ms=[round(t, 3) for t in ms[name]], ms_median=round(statistics.median(v), 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3))
        res['speedup_median'] = round(res['host']['ms_median'] / res['device']['ms_median'], 1)
        res['faster'] = bool(res['device']['ms_max'] < res['host']['ms_min'])   # beyond the spread of both
        doc['results'].append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
