"""Window prompts: W windows per image in ONE engine call against what the engine could already do -- one forward per window with that
window's prompt (each forward takes all images at once, the strongest form of that loop) -- img/s timed with hipEvents.

  python tools/window_bench.py [--dtypes bf16,bf16x3] [--images 16] [--size 1024x1024] [--grids 2x2,3x3] [--instances 16]
                               [--repeats 5] [--warmup 1] [--ways one_call,loop] [--point-only] [--out profiles/window_bench.json]

Seeded weights (bench.py's procedural checkpoint) and seeded images.  Decoding is forced to --instances instances per WINDOW (EOS
suppressed), so both ways decode the same rows for the same number of steps.  The two ways alternate inside every repeat; per way the
tool reports the median img/s over the repeats and their spread (min .. max), and per grid whether the one call beats the loop by more
than that spread: `faster` is true only when the one call's SLOWEST repeat beats the loop's FASTEST.  The phase split (encode, K/V
projection, point phase, polygon + recognition) comes from events recorded between the phases of the last repeat.
--point-only times the point phase alone on one precomputed K/V projection (Decoder.decode_points: B x W rows in one phase against W
phases of B rows); under `rocprofv3 --kernel-trace --stats -- python tools/window_bench.py --point-only --ways one_call ...` the
per-kernel statistics are then the point phase's kernels.  One JSON document, also printed.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(dtype):
    from advancedliteratemachinery_amd.model import OmniParser
    from advancedliteratemachinery_amd.utils.parser import make_args
    from advancedliteratemachinery_amd.utils import synthetic as weights
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    model = OmniParser(args, engine_dtype=dtype)
    model.load_state_dict(weights.make_state_dict(args, seed=0))
    return model.to('cuda'), args


def timed(st, fn):
    with torch.cuda.stream(st):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
    st.synchronize()
    return t0.elapsed_time(t1)


def phases(model, st, fn):
    """ms per phase of one call of fn, from the marks OmniParser.infer records (summed over the calls fn makes)"""
    model.phase_events = []
    with torch.cuda.stream(st):
        fn()
    st.synchronize()
    ev, model.phase_events = model.phase_events, None
    out = {}
    for (_, a), (name, b) in zip(ev[:-1], ev[1:]):
        if name != 'start':
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
    return {k: round(v, 2) for k, v in out.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--dtypes', default='bf16,bf16x3')
    p.add_argument('--images', type=int, default=16)
    p.add_argument('--size', default='1024x1024')
    p.add_argument('--grids', default='2x2,3x3')
    p.add_argument('--instances', type=int, default=16, help='forced instances per window')
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--ways', default='one_call,loop')
    p.add_argument('--point-only', action='store_true')
    p.add_argument('--out', default=os.path.join('profiles', 'window_bench.json'))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('window_bench needs the GPU: a timing taken anywhere else says nothing')
    from advancedliteratemachinery_amd.engine.inference import build_prompts
    from advancedliteratemachinery_amd.utils import windows as WN
    H, W_ = (int(v) for v in a.size.split('x'))
    ways = a.ways.split(',')
    st = torch.cuda.Stream()
    g = torch.Generator().manual_seed(0)
    imgs = torch.randn(a.images, 3, H, W_, generator=g).to('cuda')
    mask = torch.zeros(a.images, H, W_, dtype=torch.bool, device='cuda')
    doc = dict(images=a.images, size=a.size, instances_per_window=a.instances, repeats=a.repeats, warmup=a.warmup, point_only=a.point_only,
               results=[])
    for dtype in a.dtypes.split(','):
        model, args = build(dtype)
        seqs = build_prompts(args, 'cuda')
        enc, dec = model.engine()
        kv = None
        if a.point_only:
            with torch.cuda.stream(st):
                e = model._encode_chunked(enc, imgs, mask, no_padding=True)
                kv = dec.project_memory(e['memory'], e['mem_pos'], a.images, e['M'], None)
            st.synchronize()
        for grid in a.grids.split(','):
            nx, ny = (int(v) for v in grid.split('x'))
            wins = WN.grid_windows(nx, ny, args.num_bins)
            W = len(wins)
            per_window = []
            for w in wins:
                s = list(seqs)
                s[0] = WN.window_prompts(args, [w]).to('cuda')
                per_window.append(s)
            if a.point_only:
                rows = torch.cat([WN.window_prompts(args, wins)] * a.images, 0)
                fns = {'one_call': lambda: dec.decode_points(kv, rows, forced_instances=a.instances, rows_per_image=[W] * a.images),
                       'loop': lambda: [dec.decode_points(kv, [int(t) for t in s[0].reshape(-1).tolist()], forced_instances=a.instances)
                                        for s in per_window]}
            else:
                fns = {'one_call': lambda: model.infer(imgs, mask, seqs, forced_instances=a.instances, has_padding=False, windows=wins),
                       'loop': lambda: [model.infer(imgs, mask, s, forced_instances=a.instances, has_padding=False) for s in per_window]}
            ms = {w: [] for w in ways}
            for _ in range(a.warmup):
                for w in ways:
                    timed(st, fns[w])
            for _ in range(a.repeats):
                for w in ways:   # alternating: both ways see the same state of a shared machine
                    ms[w].append(timed(st, fns[w]))
            res = dict(dtype=dtype, grid=grid, windows=W, rows=a.images * W)
            for w in ways:
                rate = sorted(a.images * 1000.0 / t for t in ms[w])
                res[w] = dict(ms_per_call=[round(t, 2) for t in ms[w]], img_per_s_median=round(statistics.median(rate), 2),
                              img_per_s_min=round(rate[0], 2), img_per_s_max=round(rate[-1], 2))
                if not a.point_only:
                    res[w]['phase_ms'] = phases(model, st, fns[w])
            if len(ways) == 2:
                one, loop = res['one_call'], res['loop']
                res['speedup_median'] = round(one['img_per_s_median'] / loop['img_per_s_median'], 3)
                res['faster'] = bool(one['img_per_s_min'] > loop['img_per_s_max'])   # beyond the spread of both
            if a.point_only:
                _, ph = next(reversed(dec._phases.items()))
                res['last_phase'] = dec.phase_path(ph)
            doc['results'].append(res)
            print(json.dumps(res), flush=True)
        del model, enc, dec, kv
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
