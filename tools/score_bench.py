"""Scoring: ONE SpottingScorer.run (utils/scoring.py -- host packing, the upload, omp_polygon_overlap with the dense intersections,
omp_spotting_match, the download) against the numpy specification match_pages_cpu on the host, for the same pages.

  python tools/score_bench.py [--images 500] [--gt 100] [--det 120] [--thresholds 21] [--grid 1000] [--repeats 5] [--warmup 1]
                              [--out profiles/score_bench.json]

Seeded pages of word-like rectangles (tests/scoring_cases.py draws them: detections are jittered copies and exact duplicates of
ground-truth words, words of their own and empty polygons).  match_pages_cpu is handed the intersections the device computed, so the
host side times the MATCHING alone while the device side times everything; the two sides alternate inside every repeat; per side the
tool prints the median wall-clock ms and the min .. max spread.  The answers are compared.  One JSON document, also printed.
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--images', type=int, default=500)
    p.add_argument('--gt', type=int, default=100)
    p.add_argument('--det', type=int, default=120)
    p.add_argument('--thresholds', type=int, default=21)
    p.add_argument('--grid', type=int, default=1000)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--out', default=os.path.join('profiles', 'score_bench.json'))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('score_bench needs the GPU: a timing taken anywhere else says nothing')
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.utils import overlap as OV
    from advancedliteratemachinery_amd.utils import scoring as SC
    from tests.scoring_cases import pages
    case = pages(0, ((a.gt, a.det),) * a.images, a.grid, a.thresholds)
    gs = case['group_start']
    tables = (gs, case['n_gt'], case['gt_dc'], case['text'], case['level'], a.thresholds, 500, 500, 0)
    sc = SC.SpottingScorer('cuda', a.grid)
    d_polys = torch.from_numpy(case['polys']).to('cuda')
    # the intersections for the host side, once and untimed (the device's own: tests/test_gpu_overlap.py holds them to pair_overlap_cpu)
    ms_, ist = OV.mask_layout(gs)
    up = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v)).to(dt).to('cuda')      # noqa: E731
    flat = ops.polygon_overlap(d_polys, up(gs, torch.int32), up(np.arange(len(case['polys'])), torch.int32), up(ms_, torch.int64), int(ms_[-1]), a.grid,
                               500, 0, inter_start=up(ist, torch.int64), inter_total=int(ist[-1]))['inter'].cpu().numpy()

    def device():
        t0 = time.perf_counter()
        r = sc.run(d_polys, *tables)                              # ends with the download: synchronous
        return (time.perf_counter() - t0) * 1e3, (r['counts'], r['det_gt'], r['gt_det'])

    def host():
        t0 = time.perf_counter()
        r = SC.match_pages_cpu(flat, ist, *tables)
        return (time.perf_counter() - t0) * 1e3, r

    ms, last = dict(device=[], host=[]), {}
    for _ in range(a.warmup):
        device(), host()
    for _ in range(a.repeats):
        for name, fn in (('device', device), ('host', host)):    # alternating: both sides see the same state of a shared machine
            t, last[name] = fn()
            ms[name].append(t)
    same = all(bool((x == y).all()) for x, y in zip(last['device'], last['host']))
    doc = dict(images=a.images, gt_per_image=a.gt, det_per_image=a.det, thresholds=a.thresholds, grid=a.grid, repeats=a.repeats, warmup=a.warmup,
               polygons=int(gs[-1]), inter_entries=int(ist[-1]), chunks=sc.chunks, matched_first_threshold=int(last['host'][0][:, 0, 2].sum()),
               answers_equal=same, host_times='match_pages_cpu on the device\'s intersections: matching only')
    for name in ('device', 'host'):
        v = sorted(ms[name])
        doc[name] = dict(ms=[round(t, 3) for t in ms[name]], ms_median=round(statistics.median(v), 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3))
    doc['speedup_median'] = round(doc['host']['ms_median'] / doc['device']['ms_median'], 1)
    doc['faster'] = bool(doc['device']['ms_max'] < doc['host']['ms_min'])   # beyond the spread of both
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
