"""Tiled pages: ONE tiled predict_images call (all tiles of all pages in one engine flow, one omp_tile_remap call) against what the
engine could already do -- a loop of predict_images calls, one per tile view -- pages/s timed with hipEvents.

  python tools/tiles_bench.py [--dtypes bf16,bf16x3] [--pages 2] [--size 3508x2480] [--tiles 3x4] [--overlap 0.125]
                              [--min-size 640] [--max-size 1024] [--pt-seq-length 64] [--repeats 5] [--warmup 1]
                              [--ways one_call,loop] [--out profiles/tiles_bench.json]

Seeded weights (bench.py's procedural checkpoint) and seeded uint8 pages; --size is HxW (the default is an A4 scan at 300 dpi).  EOS is
honoured; both ways run ragged=True, so both decode every tile exactly as if it had been submitted alone -- the same words for the
same number of steps (the tool checks that the two ways return the same number of words per page with tile_cut='keep').  The loop
reuses one preprocessor, so neither way rebuilds resize tables inside the timed region.  The two ways alternate inside every repeat;
per way the tool reports the median pages/s over the repeats and their spread (min .. max), and whether the one call beats the loop by
more than that spread: `faster` is true only when the one call's SLOWEST repeat beats the loop's FASTEST.  The stage's own cost is
reported separately (`stage_ms`: TileStage.run on the call's ids -- the upload, three launches, the download).  One JSON document,
also printed.
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


def build(dtype, a):
    from advancedliteratemachinery_amd.model import OmniParser
    from advancedliteratemachinery_amd.utils.parser import make_args
    from advancedliteratemachinery_amd.utils import synthetic as weights
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, test_min_size=a.min_size, test_max_size=a.max_size,
                     pt_seq_length=a.pt_seq_length)
    model = OmniParser(args, engine_dtype=dtype)
    model.load_state_dict(weights.make_state_dict(args, seed=0))
    return model.to('cuda'), args


def timed(st, fn):
    with torch.cuda.stream(st):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
    st.synchronize()
    return t0.elapsed_time(t1), out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--dtypes', default='bf16,bf16x3')
    p.add_argument('--pages', type=int, default=2)
    p.add_argument('--size', default='3508x2480')
    p.add_argument('--tiles', default='3x4', help='nx x ny')
    p.add_argument('--overlap', type=float, default=0.125)
    p.add_argument('--min-size', type=int, default=640)
    p.add_argument('--max-size', type=int, default=1024)
    p.add_argument('--pt-seq-length', type=int, default=64)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--ways', default='one_call,loop')
    p.add_argument('--out', default=os.path.join('profiles', 'tiles_bench.json'))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tiles_bench needs the GPU: a timing taken anywhere else says nothing')
    from advancedliteratemachinery_amd.engine.inference import predict_images
    from advancedliteratemachinery_amd.utils import tiles as TL
    from advancedliteratemachinery_amd.utils.preprocess import DevicePreprocessor
    H, W = (int(v) for v in a.size.split('x'))
    nx, ny = (int(v) for v in a.tiles.split('x'))
    ways = a.ways.split(',')
    st = torch.cuda.Stream()
    rng = np.random.RandomState(0)
    pages = [torch.from_numpy(rng.randint(0, 256, (H, W, 3), dtype=np.uint8)).to('cuda') for _ in range(a.pages)]
    rect = TL.plan_tiles(H, W, nx, ny, TL.overlap_permille(a.overlap)).tolist()
    doc = dict(pages=a.pages, size=a.size, tiles=a.tiles, tiles_per_page=nx * ny, overlap=a.overlap, test_min_size=a.min_size, test_max_size=a.max_size,
               pt_seq_length=a.pt_seq_length, repeats=a.repeats, warmup=a.warmup, results=[])
    for dtype in a.dtypes.split(','):
        model, args = build(dtype, a)
        pre = DevicePreprocessor(args.test_min_size, args.test_max_size, 'cuda')
        kw = dict(ragged=True, preprocessor=pre)

        def one_call():
            return predict_images(model, pages, args, tiles=(nx, ny), tile_overlap=a.overlap, tile_cut='keep', **kw)[0]

        def loop():
            out = []
            for page in pages:
                words = []
                for x0, y0, x1, y1 in rect:
                    words.extend(predict_images(model, [page[y0:y1, x0:x1]], args, **kw)[0][0])
                out.append(words)
            return out
        fns = dict(one_call=one_call, loop=loop)
        ms, words = {w: [] for w in ways}, {}
        for _ in range(a.warmup):
            for w in ways:
                timed(st, fns[w])
        for _ in range(a.repeats):
            for w in ways:   # alternating: both ways see the same state of a shared machine
                t, out = timed(st, fns[w])
                ms[w].append(t)
                words[w] = [len(r) for r in out]
        res = dict(dtype=dtype, tiles=nx * ny * a.pages, words_per_page=words)
        for w in ways:
            rate = sorted(a.pages * 1000.0 / t for t in ms[w])
            res[w] = dict(ms_per_call=[round(t, 2) for t in ms[w]], pages_per_s_median=round(statistics.median(rate), 3),
                          pages_per_s_min=round(rate[0], 3), pages_per_s_max=round(rate[-1], 3))
        if len(ways) == 2:
            one, lp = res['one_call'], res['loop']
            res['same_words'] = words['one_call'] == words['loop']
            res['speedup_median'] = round(one['pages_per_s_median'] / lp['pages_per_s_median'], 3)
            res['faster'] = bool(one['pages_per_s_min'] > lp['pages_per_s_max'])   # beyond the spread of both
        # the stage alone, on as many random words as the call decoded
        n = max(1, sum(words[ways[0]]))
        T = nx * ny * a.pages
        ids = torch.from_numpy(rng.randint(0, args.num_bins, (n, 34)).astype(np.int32)).to('cuda')
        row_start = np.linspace(0, n, T + 1).astype(np.int64)
        stage = TL.TileStage('cuda', args.num_bins)
        tabs = (np.asarray(rect * a.pages), np.repeat(np.arange(a.pages), nx * ny), np.asarray([[W, H]] * a.pages))
        stage_ms = []
        for _ in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stage.run(ids[:, :32].contiguous(), ids[:, 32:].contiguous(), row_start, tabs[0], tabs[1], tabs[2], TL.default_page_bins(args.num_bins, [(nx, ny)]))
            stage_ms.append((time.perf_counter() - t0) * 1e3)
        res['stage_ms'] = dict(words=n, median=round(statistics.median(stage_ms[a.warmup:]), 3), min=round(min(stage_ms[a.warmup:]), 3),
                               max=round(max(stage_ms[a.warmup:]), 3))
        doc['results'].append(res)
        print(json.dumps(res), flush=True)
        del model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
