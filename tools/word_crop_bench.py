#!/usr/bin/env python
"""Word crops for the recogniser: 512 polygons through PolygonCropper (omp_polygon_rectify + omp_resize_crops, two
launches per chunk) against the same 512 rectangles as boxes through CropResizer (one omp_resize_normalize_pad launch
per crop), timed back to back with device events around each whole call (host packing and uploads included: that is what
a caller waits for).  Prints one JSON line; exit status 1 when the polygon median is above the box path's p90.

    python tools/word_crop_bench.py [--crops 512] [--calls 30] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(ms):
    a = np.asarray(ms, dtype=np.float64)
    return dict(p10=float(np.percentile(a, 10)), median=float(np.median(a)), p90=float(np.percentile(a, 90)), calls=len(ms))


def word_rects(rng, H, W, n):
    """word-shaped integer rectangles: 16..400 wide, 8..96 high"""
    out = []
    for _ in range(n):
        w, h = int(rng.randint(16, 401)), int(rng.randint(8, 97))
        x0, y0 = int(rng.randint(0, W - w + 1)), int(rng.randint(0, H - h + 1))
        out.append((x0, y0, x0 + w, y0 + h))
    return out


def measure(crops=512, calls=30, warmup=5, device='cuda'):
    from advancedliteratemachinery_amd.utils.preprocess import CropResizer
    from advancedliteratemachinery_amd.utils.word_crops import PolygonCropper
    rng = np.random.RandomState(0)
    images = [torch.from_numpy(rng.randint(0, 256, (1080, 1920, 3), dtype=np.uint8)).to(device),
              torch.from_numpy(rng.randint(0, 256, (720, 1280, 3), dtype=np.uint8)).to(device)]
    boxes, polys = [], []
    for i in range(crops):
        bi = i % 2
        x0, y0, x1, y1 = word_rects(rng, int(images[bi].shape[0]), int(images[bi].shape[1]), 1)[0]
        xs = np.linspace(x0, x1, 8)
        boxes.append((bi, x0, y0, x1, y1))
        polys.append((bi, [(float(x), float(y0)) for x in xs] + [(float(x), float(y1)) for x in xs[::-1]]))
    box_path, poly_path = CropResizer(device), PolygonCropper(device)
    t = {'box': [], 'polygon': []}
    same = None
    for it in range(warmup + calls):
        for name, fn, arg in (('box', box_path, boxes), ('polygon', poly_path, polys)):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = fn(images, arg)
            e1.record()
            e1.synchronize()
            if it >= warmup:
                t[name].append(e0.elapsed_time(e1))
            if it == 0:
                same = y if same is None else bool(torch.equal(same, y))
    return dict(crops=crops, chunks=poly_path.last_chunks, outputs_equal=same, box_ms=_stats(t['box']), polygon_ms=_stats(t['polygon']),
                box_launches_per_call=crops, polygon_launches_per_call=2 * poly_path.last_chunks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--crops', type=int, default=512)
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.calls < 20:
        ap.error('--calls: at least 20 timed calls')
    r = measure(a.crops, a.calls, a.warmup)
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return 0 if r['outputs_equal'] and r['polygon_ms']['median'] <= r['box_ms']['p90'] else 1


if __name__ == '__main__':
    sys.exit(main())
