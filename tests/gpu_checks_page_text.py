"""GPU checks of page text scoring: omp_page_edit_distance against pairs_cpu (utils/page_text.py) on every
integer at the edges of blocks and stripes, closed forms at the length limit, the chunked device stage, what the entry point refuses,
score_page_text and sweep_reading on the device against the host scorer on the records of a real engine call, and the structural time
gate.  Every check returns records {name, err, tol, ok, note} like tests/gpu_checks.py."""
import copy
import statistics
import time

import numpy as np
import torch

from advancedliteratemachinery_amd.utils import page_text as PT

LA = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8193)
LB = (0, 1, 64, 65, 300, 4097)
LB_CAP = 4097                   # the largest table of the definition is 8193 x 4097


def _edited(rng, a, sigma, rate=0.05):
    """a with substitutions, insertions and deletions at `rate` each third"""
    out = []
    for v in a.tolist():
        u = rng.rand()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(int(rng.randint(0, sigma)))
            continue
        if u < rate:
            out.append(int(rng.randint(0, sigma)))
        out.append(v)
    return np.asarray(out, dtype=np.uint8)


def _variants():
    """name -> (sigma, make(rng, la, lb) -> (a, b)); lb is ignored by the variants that derive b from a"""
    def rand(sigma):
        return lambda rng, la, lb: (rng.randint(0, sigma, la).astype(np.uint8), rng.randint(0, sigma, lb).astype(np.uint8))
    out = [('all equal, sigma=1', 1, lambda rng, la, lb: (np.zeros(la, np.uint8), np.zeros(lb, np.uint8)))]   # the longest carry chains
    out += [('random sigma=%d' % s, s, rand(s)) for s in (2, 26, 254)]
    out.append(('no common character', 4, lambda rng, la, lb: (rng.randint(0, 2, la).astype(np.uint8), rng.randint(2, 4, lb).astype(np.uint8))))
    out.append(('b all 255', 26, lambda rng, la, lb: (rng.randint(0, 26, la).astype(np.uint8), np.full(lb, PT.NONE, np.uint8))))

    def edits(rng, la, lb):
        a = rng.randint(0, 26, la).astype(np.uint8)
        return a, _edited(rng, a, 26)[:LB_CAP]

    def halves(rng, la, lb):
        a = rng.randint(0, 26, la).astype(np.uint8)
        return a, np.concatenate([a[la // 2:], a[:la // 2]])[:LB_CAP]
    out.append(('5% edits', 26, edits))
    out.append(('halves swapped', 26, halves))
    return out


def edge_cases(seed=0):
    """-> [(variant, sigma, [(a, b), ...])]: per variant every la of LA with two lb of LB (rotated by variant, so that every (la, lb)
    class occurs across them), and each pair swapped"""
    rng = np.random.RandomState(seed)
    cases = []
    for v, (name, sigma, make) in enumerate(_variants()):
        pairs = []
        for i, la in enumerate(LA):
            for lb in (LB[(i + v) % len(LB)], LB[(i + v + 3) % len(LB)]):
                a, b = make(rng, la, lb)
                pairs += [(a, b), (b, a)]
        cases.append((name, sigma, pairs))
    return cases


def pack(pairs, share=True):
    """pairs of code arrays -> (pool, a_off, a_len, b_off, b_len); share: arrays that are the same object get one pool range"""
    chunks, where, total = [], {}, 0
    tabs = [[], [], [], []]
    for a, b in pairs:
        for k, s in enumerate((a, b)):
            key = id(s) if share else len(chunks)
            if key not in where:
                where[key] = total
                chunks.append(np.asarray(s, dtype=np.uint8))
                total += len(s)
            tabs[2 * k].append(where[key])
            tabs[2 * k + 1].append(len(s))
    return [np.concatenate(chunks + [np.zeros(0, np.uint8)])] + [np.asarray(t, dtype=np.int32) for t in tabs]


_EDGE = {}


def edge_reference():
    """the cases and pairs_cpu on each variant, computed once and shared by the checks"""
    if not _EDGE:
        cases = edge_cases()
        _EDGE['cases'] = cases
        _EDGE['want'] = [PT.pairs_cpu(*pack(pairs)) for _, _, pairs in cases]
    return _EDGE['cases'], _EDGE['want']


def _bad(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return int((got != want).sum()) if got.shape == want.shape else 1 << 20


def mixed_call():
    """all variants in ONE call: sigma 254, every b of a variant's pairs shared with its swapped partner's a -> (packed, want)"""
    cases, want = edge_reference()
    pairs = [p for _, _, ps in cases for p in ps]
    return pack(pairs), np.concatenate(want)


def check_edges():
    from tests.gpu_checks import DEV, rec
    cases, want = edge_reference()
    sc = PT.PageTextScorer(DEV)
    out = []
    for (name, sigma, pairs), w in zip(cases, want):
        got = sc.run(*pack(pairs), sigma)
        out.append(rec('page text[%s] alone, sigma=%d: %d pairs == pairs_cpu' % (name, sigma, len(pairs)), _bad(got, w), 0,
                       'distances %d .. %d' % (int(w.min()), int(w.max()))))
        if sigma < PT.SIGMA_MAX:                                             # the same codes under the largest table: 130 560 bytes of LDS
            got = sc.run(*pack(pairs[:8] + pairs[-8:]), PT.SIGMA_MAX)
            out.append(rec('page text[%s] sigma=%d: == pairs_cpu' % (name, PT.SIGMA_MAX), _bad(got, np.concatenate([w[:8], w[-8:]])), 0))
    packed, w = mixed_call()
    got = sc.run(*packed, PT.SIGMA_MAX)
    shared = len(packed[1]) + len(packed[3]) - len(set(packed[1].tolist()) | set(packed[3].tolist()))
    out.append(rec('page text: all variants in one call of %d pairs == pairs_cpu' % len(w), _bad(got, w), 0, '%d chunks, %d shared ranges' % (sc.chunks, shared)))
    out.append(rec('page text: the mixed call shares ranges and covers every length', 0 if shared > 100 and set(LA) | set(LB) <= set(packed[2].tolist()) else 1, 0))
    return out


def check_limit():
    """the length limit, where the definition is too slow: closed forms"""
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(4)
    n = PT.LEN_MAX
    a = rng.randint(0, 26, n).astype(np.uint8)
    sub = a.copy()
    at = rng.choice(n, 7, replace=False)
    sub[at] = 26                                                            # a code that occurs nowhere else
    short = rng.randint(0, 26, 64).astype(np.uint8)
    empty = np.zeros(0, np.uint8)
    pairs = [(a, a), (a, sub), (sub, a), (a, a[100:]), (a[100:], a), (a, empty), (empty, a), (a, short), (short, a)]
    want = [0, 7, 7, 100, 100, n, n, PT.distance_cpu(a, short), PT.distance_cpu(short, a)]
    names = ['itself', '7 substitutions', '7 substitutions, swapped', 'its tail from 100', 'its tail from 100, swapped', 'the empty string',
             'the empty string, swapped', '64 characters (the definition)', '64 characters, swapped (the definition)']
    got = PT.PageTextScorer(DEV).run(*pack(pairs), 27)
    return [rec('page text[65535] against %s: %d' % (nm, w), abs(int(g) - int(w)), 0, 'got %d' % int(g)) for nm, g, w in zip(names, got, want)]


def check_chunked():
    """the mixed call with the scratch cap lowered so that it runs in at least 3 chunks == the unchunked specification"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV, rec
    packed, want = mixed_call()
    P = len(want)
    out = []
    for per in (P // 3, 7, P):
        sc = PT.PageTextScorer(DEV, scratch_cap=per * ops.PAGE_TEXT_SLICE_BYTES)
        got = sc.run(*packed, PT.SIGMA_MAX)
        out.append(rec('chunked scorer, %d pairs a chunk == pairs_cpu' % per, _bad(got, want), 0, '%d chunks' % sc.chunks))
        out.append(rec('chunked scorer, %d pairs a chunk: %s' % (per, 'one chunk' if per == P else 'at least 3 chunks'),
                       0 if (sc.chunks == 1 if per == P else sc.chunks >= 3) else 1, 0, '%d chunks' % sc.chunks))
        out.append(rec('chunked scorer, %d pairs a chunk: the scratch holds one chunk' % per, 0 if sc.scratch.numel() == ops.page_scratch_bytes(min(per, P)) else 1, 0))
    return out


def check_refusals():
    """what the entry point refuses comes back as an error code and a message before any launch, and what only the device tables show
    as a distance of -1; nothing aborts"""
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(9)
    strings = [rng.randint(0, 5, n).astype(np.uint8) for n in (10, 70, 200, 5000, 33)]
    pairs = [(strings[0], strings[1]), (strings[2], strings[3]), (strings[3], strings[2]), (strings[4], strings[4]), (strings[1], strings[4])]
    pool, a_off, a_len, b_off, b_len = pack(pairs)
    want = PT.pairs_cpu(pool, a_off, a_len, b_off, b_len)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)        # noqa: E731
    d = dict(pool=t(pool), a_off=t(a_off), a_len=t(a_len), b_off=t(b_off), b_len=t(b_len))
    P = len(pairs)
    scratch = torch.empty(ops.page_scratch_bytes(P), dtype=torch.uint8, device=DEV)
    good = ops.page_edit_distance(d['pool'], pool.size, d['a_off'], d['a_len'], d['b_off'], d['b_len'], 5, scratch).cpu().numpy()
    out = [rec('page text: the refusal case itself == pairs_cpu', _bad(good, want), 0)]
    res = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    args = [ops.ptr(d['pool']), pool.size, ops.ptr(d['a_off']), ops.ptr(d['a_len']), ops.ptr(d['b_off']), ops.ptr(d['b_len']), P, 5, ops.ptr(scratch),
            scratch.numel(), ops.ptr(res), ops.stream()]
    for k, what in ((0, 'pool'), (2, 'a_off'), (3, 'a_len'), (4, 'b_off'), (5, 'b_len'), (8, 'scratch'), (10, 'dist')):
        a = list(args)
        a[k] = None
        rc = _lib.lib().omp_page_edit_distance(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page text refuses a null %s with an error code' % what, 0 if rc == -22 and 'null pointer' in msg else 1, 0, msg))
    for what, k, v in (('n_pairs 0', 6, 0), ('n_pairs -1', 6, -1), ('sigma 255', 7, 255), ('sigma -1', 7, -1), ('too little scratch', 9, scratch.numel() - 1),
                       ('no scratch', 9, 0)):
        a = list(args)
        a[k] = v
        rc = _lib.lib().omp_page_edit_distance(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page text refuses %s with an error code' % what, 0 if rc == -22 and 'omp_page_edit_distance' in msg else 1, 0, msg))
    try:
        ops.page_edit_distance(d['pool'], pool.size, d['a_off'], d['a_len'], d['b_off'], d['b_len'], 5, scratch[:ops.page_scratch_bytes(P) - 8])
        bad = 1
    except RuntimeError as e:
        bad = 0 if 'omp_page_edit_distance' in str(e) and '(-22)' in str(e) and 'scratch' in str(e) else 1
    out.append(rec('the wrapper raises on too little scratch', bad, 0))
    torch.cuda.synchronize()
    out.append(rec('page text: nothing was written by the refused calls', int((res != -7).sum().item()), 0))
    # what only the device tables show: the pair is refused on the device, its neighbours are scored
    for what, key, idx, v in (('a length of 65536', 'a_len', 1, PT.LEN_MAX + 1), ('a negative length', 'b_len', 2, -1), ('a negative offset', 'a_off', 3, -1),
                              ('a range past pool_bytes', 'b_off', 0, pool.size - int(b_len[0]) + 1), ('a length past pool_bytes', 'a_len', 4, pool.size)):
        tabs = {k: d[k].clone() for k in ('a_off', 'a_len', 'b_off', 'b_len')}
        tabs[key][idx] = v
        got = ops.page_edit_distance(d['pool'], pool.size, tabs['a_off'], tabs['a_len'], tabs['b_off'], tabs['b_len'], 5, scratch).cpu().numpy()
        w = want.copy()
        w[idx] = -1
        out.append(rec('page text refuses %s on the device: dist -1, the other pairs scored' % what, _bad(got, w), 0, str(got.tolist())))
    # the device stage
    sc = PT.PageTextScorer(DEV)
    for what, kw in (('a length above the limit', dict(a_len=[PT.LEN_MAX + 1])), ('a range outside the pool', dict(b_off=[1])), ('sigma 255', dict(sigma=255)),
                     ('a code at or above sigma', dict(sigma=2))):
        a = dict(pool=np.asarray([0, 1, 2], np.uint8), a_off=[0], a_len=[3], b_off=[0], b_len=[3], sigma=3)
        a.update(kw)
        try:
            sc.run(**a)
            bad = 1
        except ValueError:
            bad = 0
        out.append(rec('the scorer refuses %s on the host' % what, bad, 0))
    empty = sc.run(np.zeros(0, np.uint8), [], [], [], [], 0)
    out.append(rec('the scorer on no pairs: no distances', int(empty.size) + int(empty.dtype != np.int32), 0))
    zero = sc.run(np.zeros(0, np.uint8), [0, 0], [0, 0], [0, 0], [0, 0], 0)
    out.append(rec('the scorer on empty strings: zeros', _bad(zero, [0, 0]), 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
class _HostReader(object):
    def __init__(self, grid):
        self.grid = grid

    def __call__(self, polys, group_start, aspect, gap=2000, back=500, offset=500, blocks=None):
        from advancedliteratemachinery_amd.utils import reading as RD
        polys = torch.as_tensor(polys).cpu().numpy()
        res = RD.lines_cpu(polys, group_start, aspect, gap, back, offset, self.grid)
        if blocks is not None:
            res['blocks'] = RD.blocks_cpu(polys, group_start, aspect, res['line'], res['line_pos'], res['n_lines'], *blocks, grid=self.grid)
        return res


def check_engine_page_text(dtype_name):
    """spot_windows' image and weights, windows = [default, 2 x 2 grid], suppress=0.5; ground truth = the reading_order=True, blocks=True
    call's own page strings: score_page_text and sweep_reading on the device == the host scorer and the host reader"""
    from advancedliteratemachinery_amd.engine import evaluate as EV
    from advancedliteratemachinery_amd.engine import inference as inf
    from advancedliteratemachinery_amd.utils import windows as WN
    from advancedliteratemachinery_amd.utils.nested_tensor import NestedTensor
    from tests.gpu_checks import DEV, ENGINES, build_model, golden, rec
    from tests.gpu_checks_windows import fixture_case
    gold = golden('spot_windows')
    args, sd, img, mask, _ = fixture_case(gold, 'eos')
    model = build_model(args, sd, gold['case']['depths'], ENGINES[dtype_name])
    nt = NestedTensor(img.to(DEV), mask.to(DEV))
    wins = [WN.default_window(args)] + WN.grid_windows(2, 2, args.num_bins)
    sizes = [(int(img.shape[2]), int(img.shape[3]))] * int(img.shape[0])
    tag = 'page text engine[%s]' % dtype_name
    plain = inf.predict(model, nt, args, windows=wins, suppress=0.5)
    blocks = inf.predict(model, nt, args, windows=wins, suppress=0.5, reading_order=True, blocks=True)
    truth = [PT.page_string(recs, normalise=None) for recs in blocks]
    out = []
    host = PT.HostPageScorer()
    results = {}
    for name, recs in (('plain', plain), ('blocks=True', blocks)):
        got = EV.score_page_text(copy.deepcopy(recs), truth, device=DEV)
        want = EV.score_page_text(copy.deepcopy(recs), truth, scorer=host)
        results[name] = got
        note = '%d records, %s characters, distances %s' % (sum(len(r) for r in recs), got['len_gt'].tolist(), got['dist'].tolist())
        out.append(rec('%s %s: dist, len_pred, len_gt == the host scorer' % (tag, name),
                       _bad(got['dist'], want['dist']) + _bad(got['len_pred'], want['len_pred']) + _bad(got['len_gt'], want['len_gt']), 0, note))
        out.append(rec('%s %s: score, mean, micro' % (tag, name), 0 if (got['score'] == want['score']).all() and got['mean'] == want['mean'] and
                       got['micro'] == want['micro'] else 1, 0))
    b = results['blocks=True']
    out.append(rec(tag + ' the blocks=True records score 1.0 against their own page strings', 0 if (b['score'] == 1.0).all() and b['mean'] == 1.0 and
                   (b['dist'] == 0).all() else 1, 0, 'lengths %s' % b['len_gt'].tolist()))
    settings = [None, dict(), dict(blocks=True), dict(line_gap=0.5, blocks=True, block_gap_x=0.2)]
    scorer = PT.PageTextScorer(DEV)
    got = EV.sweep_reading(copy.deepcopy(plain), sizes, args.num_bins, truth, settings, scorer=scorer, device=DEV)
    want = EV.sweep_reading(copy.deepcopy(plain), sizes, args.num_bins, truth, settings, scorer=host, reader=_HostReader(args.num_bins))
    bad = sum(_bad(g['dist'], w['dist']) + _bad(g['len_pred'], w['len_pred']) + int(g['mean'] != w['mean']) for g, w in zip(got['settings'], want['settings']))
    out.append(rec(tag + ' sweep_reading over 4 settings == the host sweep', bad + int(got['best'] != want['best']), 0,
                   'means %s, best %d' % ([round(s['mean'], 4) for s in got['settings']], got['best'])))
    out.append(rec(tag + ' sweep_reading: the setting None is score_page_text on the records as given', _bad(got['settings'][0]['dist'], results['plain']['dist']), 0))
    out.append(rec(tag + ' sweep_reading runs one device call', abs(scorer.calls - 1) + abs(scorer.chunks - 1), 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the structural time gate
# ---------------------------------------------------------------------------------------------------------------------------------
def check_timing():
    """16 pairs of about 2000 x 2000 (b = a with 5 % edits): the median of 3 whole PageTextScorer.run calls (upload, launch, download) at
    or below ONE pairs_cpu call on the same inputs.  No margin: it catches a launch or a synchronisation per pair, not a tuning."""
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(21)
    pairs = []
    for _ in range(16):
        a = rng.randint(0, 60, 2000).astype(np.uint8)
        pairs.append((a, _edited(rng, a, 60)))
    packed = pack(pairs)
    sc = PT.PageTextScorer(DEV)
    got = sc.run(*packed, 60)                                               # warm: library load, allocator, scratch
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = sc.run(*packed, 60)
        ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    want = PT.pairs_cpu(*packed)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    note = 'device run %s ms (median %.3f), pairs_cpu %.1f ms, 16 pairs of 2000 x about 2000' % ([round(v, 3) for v in ms], statistics.median(ms), cpu_ms)
    print(note)
    return [rec('page text: 16 pairs of 2000 x 2000, median of 3 device runs <= one pairs_cpu call', statistics.median(ms), cpu_ms, note),
            rec('page text: the timed outputs are equal', _bad(got, want), 0)]
