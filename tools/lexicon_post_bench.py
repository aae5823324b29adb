#!/usr/bin/env python
"""Posterior lexicon decoding: N rows of character logits against a synthetic L-word lexicon through PosteriorMatcher (per call:
omp_logprob_costs, the search and merge launches of omp_lexicon_posterior, one download), timed with device events around each
whole call (that is what a caller waits for) and, apart, around omp_lexicon_posterior alone.  Two yardsticks:

    utils/lexicon_post.py: score_cpu on the first --cpu-queries rows of the device's own costs, scaled linearly to N
    omp_lexicon_nearest on the same rows' greedy strings against the same lexicon: "the same streaming problem"

The logits are peaked on a lexicon word under 0..2 substituted characters, as a reader's misreadings are.  Prints one JSON line;
exit status 1 when the device median is above the scaled host time or the outputs differ.

    python tools/lexicon_post_bench.py [--queries 512] [--words 90000] [--calls 30] [--warmup 5] [--cpu-queries 32] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CHARS = '0123456789abcdefghijklmnopqrstuvwxyz'


def _stats(ms):
    a = np.asarray(ms, dtype=np.float64)
    return dict(p10=float(np.percentile(a, 10)), median=float(np.median(a)), p90=float(np.percentile(a, 90)), calls=len(ms))


def synthetic(words, queries, seed=0):
    """-> (lexicon: word-like strings of length 2..16 over MGP-STR's 36 characters; logits fp32 [queries, 27, 38]: noise of
    unit scale with +6 on the characters of a lexicon word under 0..2 substitutions and on [s] behind it; the greedy strings)"""
    rng = np.random.RandomState(seed)
    lens = rng.randint(2, 17, words)
    flat = rng.randint(0, len(CHARS), int(lens.sum()))
    lex, p = [], 0
    for n in lens.tolist():
        lex.append(''.join(CHARS[i] for i in flat[p:p + n]))
        p += n
    x = rng.randn(queries, 27, 38).astype(np.float32)
    reads = []
    for i in range(queries):
        w = list(lex[int(rng.randint(0, words))])
        for _ in range(i % 3):
            w[int(rng.randint(0, len(w)))] = CHARS[int(rng.randint(0, len(CHARS)))]
        for k, ch in enumerate(w):
            x[i, 1 + k, 2 + CHARS.index(ch)] += 6.0
        x[i, 1 + len(w):, 1] += 6.0
        reads.append(''.join(w))
    return lex, x, reads


def _timed(fn, calls, warmup):
    ms = []
    for it in range(warmup + calls):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms, out


def measure(queries=512, words=90000, calls=30, warmup=5, cpu_queries=32, device='cuda'):
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.utils import lexicon as LX
    from advancedliteratemachinery_amd.utils import lexicon_post as LP
    lex, x, reads = synthetic(words, queries)
    m = LX.LexiconMatcher(device, lex, CHARS)
    post = LP.PosteriorMatcher(m)
    pool, offsets = LX.encode_words(lex, CHARS)
    xd = torch.from_numpy(x).to(device)
    whole, (best, greedy) = _timed(lambda: post.score(xd), calls, warmup)
    chunks = post.last_chunks
    # the entry point alone (search + merge launches), operands already on the device
    costs, _ = ops.logprob_costs(xd)
    out = torch.empty((queries, 2), dtype=torch.int64, device=device)
    work = torch.empty(2 * (queries + ops.LEXICON_POST_WORK_SLICES), dtype=torch.int64, device=device)
    entry, _ = _timed(lambda: ops.lexicon_posterior(costs, None, None, m.pool, m.pool_bytes, m.offsets, m.L, post.table, best=out, work=work),
                      calls, warmup)
    cost_ms, _ = _timed(lambda: ops.logprob_costs(xd), calls, warmup)
    # the yardstick on the device: omp_lexicon_nearest on the same rows' greedy strings
    codes, q_len = LX.encode_queries(reads, CHARS)
    d_codes, d_len = torch.from_numpy(codes).to(device), torch.from_numpy(q_len).to(device)
    nbest = torch.empty(queries, dtype=torch.int64, device=device)
    nearest, _ = _timed(lambda: ops.lexicon_nearest(d_codes, d_len, None, None, m.pool, m.pool_bytes, m.offsets, m.L, best=nbest), calls, warmup)
    nq = min(cpu_queries, queries)
    host_costs = costs.cpu().numpy()
    t0 = time.perf_counter()
    want = LP.score_cpu(host_costs[:nq], pool, offsets, post.table_host)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(best[:nq], want) and np.array_equal(out.cpu().numpy().view(np.uint64), best)
                and np.array_equal(greedy, LP.greedy_cpu(host_costs)))
    dev, ent = _stats(whole), _stats(entry)
    pairs = float(queries) * words
    return dict(queries=queries, words=words, lexicon_chars=int(pool.size), chunks=chunks, launches_per_call=3 * chunks, outputs_equal=same,
                device_ms=dev, entry_ms=ent, costs_ms=_stats(cost_ms), nearest_entry_ms=_stats(nearest), cpu_queries=nq, cpu_ms_measured=cpu_ms,
                cpu_ms_scaled=cpu_ms * queries / nq, cpu_scaling='score_cpu timed on the first %d queries, scaled linearly to %d' % (nq, queries),
                pairs_per_s=pairs / (dev['median'] * 1e-3), entry_pairs_per_s=pairs / (ent['median'] * 1e-3),
                entry_over_nearest=ent['median'] / float(np.median(nearest)),
                cpu_pairs_per_s=float(nq) * words / (cpu_ms * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--queries', type=int, default=512)
    ap.add_argument('--words', type=int, default=90000)
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cpu-queries', type=int, default=32)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    r = measure(a.queries, a.words, a.calls, a.warmup, a.cpu_queries)
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return 0 if r['outputs_equal'] and r['device_ms']['median'] <= r['cpu_ms_scaled'] else 1


if __name__ == '__main__':
    sys.exit(main())
