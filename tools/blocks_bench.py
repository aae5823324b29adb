"""Blocks: ONE device call (utils/reading.py: ReadingOrder with blocks= -- host packing, the upload, omp_reading_links,
omp_reading_lines, omp_reading_blocks, the download) against the numpy specification lines_cpu + blocks_cpu on the host, for the same
synthetic pages.

  python tools/blocks_bench.py [--pages 160x64,160x512] [--grid 4096] [--repeats 5] [--warmup 1] [--host-images 4]
                               [--out profiles/blocks_bench.json]

Seeded pages: the images alternate between two and three columns of lines of word polygons under a headline that spans the columns,
slightly jittered, in random order.  The two sides alternate inside every repeat; per side the tool reports the median wall-clock ms
and the min .. max spread.  On more than --host-images images the host specification is timed on the first --host-images and scaled
by the image count (images are independent groups, its cost is a sum over them), which the document says in `host_scaled_from`.  The
answers of the two sides are compared on the images both ran.
The one gate is structural: the device's median for the whole call is at or below the host specification's.
It has no margin: it catches a launch or a synchronisation per level or per group, it does not rank tunings.  The exit status is 1
when it fails or when the answers differ.  One JSON document, also printed.
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


def page(rng, words, grid, cols):
    """one image's polygons: a headline over `cols` columns of lines of 4 words (the last line may be shorter), in random order"""
    per_line = 4
    body = words - 1
    lines = (body + per_line - 1) // per_line
    rows = (lines + cols - 1) // cols
    col_w = 0.9 * grid / cols
    h = max(2.0, min(0.55 * 0.8 * grid / max(rows, 1), 0.08 * col_w))         # a gutter of 0.2 col_w is 2.5 heights at least
    pitch_y = min(0.8 * grid / max(rows, 1), 1.8 * h)                        # rows 0.8 heights apart: no band inside a column
    w, gap = 0.8 * col_w / per_line * 0.9, 0.8 * col_w / per_line * 0.1
    u = lambda ww: np.linspace(0.0, ww, 8)                                    # noqa: E731

    def word(x, y, ww):
        return np.concatenate([np.stack([x + u(ww), np.full(8, y)], 1), np.stack([x + u(ww)[::-1], np.full(8, y + h)], 1)])

    y0 = 0.15 * grid
    pts = [word(0.05 * grid, y0 - 3 * h, 0.9 * grid - 0.2 * col_w)]           # two heights above the columns
    for k in range(body):
        l, q = divmod(k, per_line)
        c, r = divmod(l, rows)
        pts.append(word(0.05 * grid + c * col_w + q * (w + gap), y0 + r * pitch_y, w) + rng.uniform(-0.04 * h, 0.04 * h, (1, 2)))
    pts = np.stack(pts)
    return np.clip(np.rint(pts[rng.permutation(words)]), 0, grid - 1).astype(np.int32).reshape(words, 32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pages', default='160x64,160x512')
    p.add_argument('--grid', type=int, default=4096)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--host-images', type=int, default=4)
    p.add_argument('--out', default=os.path.join('profiles', 'blocks_bench.json'))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('blocks_bench needs the GPU: a timing taken anywhere else says nothing')
    from advancedliteratemachinery_amd.utils import reading as RD
    reader = RD.ReadingOrder('cuda', a.grid)
    cut = tuple(RD.BLOCK_DEFAULTS[k] for k in ('gap_x', 'gap_y', 'depth'))
    doc = dict(grid=a.grid, repeats=a.repeats, warmup=a.warmup, params=RD.DEFAULTS, block_params=RD.BLOCK_DEFAULTS, results=[])
    ok = True
    for spec in a.pages.split(','):
        images, words = (int(v) for v in spec.split('x'))
        rng = np.random.RandomState(words)
        polys = np.concatenate([page(rng, words, a.grid, 2 + b % 2) for b in range(images)])
        gs = np.arange(images + 1, dtype=np.int32) * words
        aspect = np.tile(np.asarray([[256, 181]], np.int32), (images, 1))
        hb = min(images, a.host_images)
        d_polys = torch.from_numpy(polys).to('cuda')          # the raw ids are on the device already (r[0][1] of the engine's result)

        def device():
            t0 = time.perf_counter()
            res = reader.run(d_polys, gs, aspect, blocks=cut)  # ends with the download: synchronous
            return (time.perf_counter() - t0) * 1e3, res

        def host():
            t0 = time.perf_counter()
            res = RD.lines_cpu(polys[:hb * words], gs[:hb + 1], aspect[:hb], grid=a.grid)
            res['blocks'] = RD.blocks_cpu(polys[:hb * words], gs[:hb + 1], aspect[:hb], res['line'], res['line_pos'], res['n_lines'], *cut, grid=a.grid)
            return (time.perf_counter() - t0) * 1e3 * images / hb, res

        ms, last = dict(device=[], host=[]), {}
        for _ in range(a.warmup):
            device(), host()
        for _ in range(a.repeats):
            for name, fn in (('device', device), ('host', host)):   # alternating: both sides see the same state of a shared machine
                t, last[name] = fn()
                ms[name].append(t)
        dv, hv = last['device']['blocks'], last['host']['blocks']
        same = all(bool((dv[k][:hb * words if k in ('block', 'line', 'rank') else hb] == hv[k]).all()) for k in ('block', 'line', 'rank', 'n_blocks', 'levels'))
        res = dict(images=images, words_per_image=words, words=int(polys.shape[0]), lines=int(last['device']['n_lines'].sum()),
                   blocks=int(dv['n_blocks'].sum()), blocks_per_image=sorted(set(dv['n_blocks'].tolist())), levels_max=int(dv['levels'].max()),
                   answers_equal_on_host_images=same, host_scaled_from=hb)
        for name in ('device', 'host'):
            v = sorted(ms[name])
            res[name] = dict(ms=[round(t, 3) for t in ms[name]], ms_median=round(statistics.median(v), 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3))
        res['speedup_median'] = round(res['host']['ms_median'] / res['device']['ms_median'], 1)
        res['device_at_or_below_host'] = bool(res['device']['ms_median'] <= res['host']['ms_median'])   # the structural gate
        ok = ok and same and res['device_at_or_below_host']
        doc['results'].append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
