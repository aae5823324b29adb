"""Reading order: ONE device call (utils/reading.py: ReadingOrder -- host packing, the upload, omp_reading_links, omp_reading_lines,
the download) against the numpy specification lines_cpu on the host, for the same synthetic pages.

  python tools/reading_bench.py [--pages 160x500,1x8192] [--grid 4096] [--repeats 5] [--warmup 1] [--host-images 4]
                                [--out profiles/reading_bench.json]

Seeded pages: every image holds rows of word polygons (8 points along the top, 8 back along the bottom), slightly rotated, shuffled.
The two sides alternate inside every repeat; per side the tool reports the median wall-clock ms and the min .. max spread, and
`faster` only when the device's SLOWEST repeat beats the host's FASTEST.  On more than --host-images images the host specification
is timed on the first --host-images and scaled by the image count (images are independent groups, its cost is a sum over them),
which the document says in `host_scaled_from`.  The answers of the two sides are compared on the images both ran.  No ratio is a
gate.  One JSON document, also printed.
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
    """one image's polygons: rows of words, rotated by up to 2 degrees, in random order"""
    cols = max(1, int(np.ceil(np.sqrt(words / 2.0))))
    rows = (words + cols - 1) // cols
    pitch_x, pitch_y = 0.9 * grid / cols, 0.9 * grid / rows
    w, h = max(2.0, 0.78 * pitch_x), max(2.0, 0.55 * pitch_y)
    u = np.linspace(0.0, w, 8)
    one = np.concatenate([np.stack([u, np.zeros(8)], 1), np.stack([u[::-1], np.full(8, h)], 1)])
    org = np.stack([(0.05 * grid + c * pitch_x, 0.05 * grid + r * pitch_y) for r in range(rows) for c in range(cols)])
    pts = (one[None] + org[:, None] + rng.uniform(-0.05 * h, 0.05 * h, (rows * cols, 1, 2))) - grid / 2.0
    t = np.deg2rad(rng.uniform(-2, 2))
    pts = np.stack([pts[..., 0] * np.cos(t) - pts[..., 1] * np.sin(t), pts[..., 0] * np.sin(t) + pts[..., 1] * np.cos(t)], -1) + grid / 2.0
    return np.rint(pts[rng.permutation(rows * cols)[:words]]).astype(np.int32).reshape(words, 32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pages', default='160x500,1x8192')
    p.add_argument('--grid', type=int, default=4096)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--host-images', type=int, default=4)
    p.add_argument('--out', default=os.path.join('profiles', 'reading_bench.json'))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('reading_bench needs the GPU: a timing taken anywhere else says nothing')
    from advancedliteratemachinery_amd.utils import reading as RD
    reader = RD.ReadingOrder('cuda', a.grid)
    doc = dict(grid=a.grid, repeats=a.repeats, warmup=a.warmup, params=RD.DEFAULTS, results=[])
    for spec in a.pages.split(','):
        images, words = (int(v) for v in spec.split('x'))
        rng = np.random.RandomState(words)
        polys = np.concatenate([page(rng, words, a.grid) for _ in range(images)])
        gs = np.arange(images + 1, dtype=np.int32) * words
        aspect = np.tile(np.asarray([[256, 181]], np.int32), (images, 1))
        hb = min(images, a.host_images)
        d_polys = torch.from_numpy(polys).to('cuda')          # the raw ids are on the device already (r[0][1] of the engine's result)

        def device():
            t0 = time.perf_counter()
            res = reader(d_polys, gs, aspect)                 # ends with the download: synchronous
            return (time.perf_counter() - t0) * 1e3, res

        def host():
            t0 = time.perf_counter()
            res = RD.lines_cpu(polys[:hb * words], gs[:hb + 1], aspect[:hb], grid=a.grid)
            return (time.perf_counter() - t0) * 1e3 * images / hb, res

        ms, last = dict(device=[], host=[]), {}
        for _ in range(a.warmup):
            device(), host()
        for _ in range(a.repeats):
            for name, fn in (('device', device), ('host', host)):   # alternating: both sides see the same state of a shared machine
                t, last[name] = fn()
                ms[name].append(t)
        same = all(bool((last['device'][k][:hb * words if k != 'n_lines' else hb] == last['host'][k]).all())
                   for k in ('succ', 'pred', 'line', 'line_pos', 'rank', 'n_lines'))
        res = dict(images=images, words_per_image=words, words=int(polys.shape[0]), lines=int(last['device']['n_lines'].sum()),
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
