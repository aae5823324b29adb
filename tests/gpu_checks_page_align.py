"""GPU checks of page text alignment: omp_page_align against pairs_align_cpu (utils/page_align.py) on every
integer of the counts and of both maps at the edges of blocks and stripes, through three stripes, at the length limit, the chunked device
stage, what is written outside the owned slices (nothing), what the entry point and the device refuse, and align_page_text on the device
against the host aligner on the records of a real engine call.  Every check returns records {name, err, tol, ok, note} like
tests/gpu_checks.py."""
import copy
import ctypes

import numpy as np
import torch

from advancedliteratemachinery_amd.utils import page_align as PA
from advancedliteratemachinery_amd.utils import page_text as PT
from tests.gpu_checks_page_text import _edited, pack

LA = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)
LB = (0, 1, 63, 64, 65, 300, 4097)
BIG = 4095                      # pairs with both sides at or above this run under '5% edits' and 'sigma 1' only: the definition's table
SENTINEL = -77


def _variants():
    """name -> (sigma, big pairs allowed, make(rng, la, lb) -> (a, b) or None)"""
    def rand(sigma):
        return lambda rng, la, lb: (rng.randint(0, sigma, la).astype(np.uint8), rng.randint(0, sigma, lb).astype(np.uint8))

    def equal(rng, la, lb):
        if lb != LB[0]:                                                     # one pair per la: b is a
            return None
        a = rng.randint(0, 26, la).astype(np.uint8)
        return a, a

    def edits(rng, la, lb):
        if lb != LB[0]:                                                     # one pair per la: b is a with edits
            return None
        a = rng.randint(0, 26, la).astype(np.uint8)
        return a, _edited(rng, a, 26)

    def halves(rng, la, lb):
        a = rng.randint(0, 26, la).astype(np.uint8)
        return a, np.concatenate([a[la // 2:], a[:la // 2]])[:lb]
    return [('equal strings', 26, False, equal),
            ('sigma 1, la != lb', 1, True, lambda rng, la, lb: None if la == lb else (np.zeros(la, np.uint8), np.zeros(lb, np.uint8))),   # every cell a tie
            ('random sigma=2', 2, False, rand(2)), ('random sigma=26', 26, False, rand(26)), ('random sigma=254', 254, False, rand(254)),
            ('no common character', 4, False, lambda rng, la, lb: (rng.randint(0, 2, la).astype(np.uint8), rng.randint(2, 4, lb).astype(np.uint8))),
            ('b all 255', 26, False, lambda rng, la, lb: (rng.randint(0, 26, la).astype(np.uint8), np.full(lb, PT.NONE, np.uint8))),
            ('5% edits', 26, True, edits), ('halves swapped', 26, False, halves)]


def edge_cases(seed=0):
    """-> [(variant, sigma, [(a, b), ...])]: every la of LA against every lb of LB, and each pair swapped"""
    rng = np.random.RandomState(seed)
    cases = []
    for name, sigma, big, make in _variants():
        pairs = []
        for la in LA:
            for lb in LB:
                made = make(rng, la, lb)
                if made is None or (not big and min(len(made[0]), len(made[1])) >= BIG):
                    continue
                a, b = made
                pairs += [(a, b), (b, a)]
        cases.append((name, sigma, pairs))
    return cases


def reference(pairs, share=True):
    """-> (packed, counts, maps): pairs_align_cpu with the maps laid out back to back, as the device stage lays them out"""
    packed = pack(pairs, share)
    counts, maps = PA.pairs_align_cpu(*packed, PA.dense_map_off(packed[2], packed[4]))
    return packed, counts, maps


_EDGE = {}


def edge_reference():
    """the cases and pairs_align_cpu on each variant, computed once and shared by the checks"""
    if not _EDGE:
        _EDGE['cases'] = edge_cases()
        _EDGE['want'] = [reference(pairs) for _, _, pairs in _EDGE['cases']]
    return _EDGE['cases'], _EDGE['want']


def _bad(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return int((got != want).sum()) if got.shape == want.shape else 1 << 20


def _bad_run(res, counts, maps):
    return _bad(res['counts'], counts) + _bad(res['maps'], maps)


def mixed_call():
    """all variants in ONE call: sigma 254, every b of a variant's pairs shared with its swapped partner's a -> (packed, counts, maps)"""
    if 'mixed' not in _EDGE:
        cases, want = edge_reference()
        pairs = [p for _, _, ps in cases for p in ps]
        packed = pack(pairs)
        counts = np.concatenate([w[1] for w in want])
        maps = np.concatenate([w[2] for w in want])                         # dense offsets: the variants' maps follow one another
        _EDGE['mixed'] = (packed, counts, maps)
    return _EDGE['mixed']


def check_edges():
    from tests.gpu_checks import DEV, rec
    cases, want = edge_reference()
    al = PA.PageAligner(DEV)
    out = []
    for (name, sigma, pairs), (packed, counts, maps) in zip(cases, want):
        res = al.run(*packed, sigma)
        d = counts[:, 1:].sum(1)
        out.append(rec('page align[%s] alone, sigma=%d: %d pairs, counts and maps == pairs_align_cpu' % (name, sigma, len(pairs)), _bad_run(res, counts, maps), 0,
                       '%d map entries, distances %d .. %d' % (maps.size, int(d.min()), int(d.max()))))
    packed, counts, maps = mixed_call()
    res = al.run(*packed, PT.SIGMA_MAX)
    shared = len(packed[1]) + len(packed[3]) - len(set(packed[1].tolist()) | set(packed[3].tolist()))
    out.append(rec('page align: all variants in one call of %d pairs == pairs_align_cpu' % len(counts), _bad_run(res, counts, maps), 0,
                   '%d chunks, %d shared ranges' % (al.chunks, shared)))
    lens = set(zip(packed[2].tolist(), packed[4].tolist()))
    every = all((la, lb) in lens and (lb, la) in lens for la in LA for lb in LB if la != lb and min(la, lb) < BIG)
    out.append(rec('page align: the mixed call shares ranges and covers every (la, lb)', 0 if shared > 100 and every else 1, 0))
    return out


def check_stripes():
    """8193 x 300 and 300 x 8193: three stripes, the carries through scratch together with the recording"""
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(5)
    a = rng.randint(0, 3, 8193).astype(np.uint8)
    b = _edited(rng, a[4000:4300], 3)[:300]
    z, y = np.zeros(8193, np.uint8), np.zeros(300, np.uint8)
    c = rng.randint(0, 26, 8193).astype(np.uint8)
    d = c[np.sort(rng.choice(8193, 300, replace=False))]                    # 300 characters spread over all three stripes
    pairs = [(a, b), (b, a), (z, y), (y, z), (c, d), (d, c)]
    packed, counts, maps = reference(pairs)
    res = PA.PageAligner(DEV).run(*packed, 26)
    return [rec('page align 8193 x 300 and 300 x 8193 (sigma 3 with edits, sigma 1, a spread subsequence) == pairs_align_cpu', _bad_run(res, counts, maps), 0,
                'counts %s' % counts.tolist())]


def check_limit():
    """65 535 x 64 and 64 x 65 535 against the definition (a table of 17 MB)"""
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(4)
    n = PT.LEN_MAX
    a = rng.randint(0, 26, n).astype(np.uint8)
    short = a[np.sort(rng.choice(n, 64, replace=False))].copy()
    short[::9] = 26                                                         # a code that occurs nowhere in a
    pairs = [(a, short), (short, a)]
    packed, counts, maps = reference(pairs)
    res = PA.PageAligner(DEV).run(*packed, 27)
    return [rec('page align 65535 x 64 and 64 x 65535 == pairs_align_cpu', _bad_run(res, counts, maps), 0, 'counts %s' % counts.tolist())]


def check_chunked():
    """the mixed call with the scratch cap lowered so that it runs in at least 4 chunks == the unchunked definition"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV, rec
    packed, counts, maps = mixed_call()
    need = [ops.page_align_scratch_bytes(la, lb) for la, lb in zip(packed[2].tolist(), packed[4].tolist())]
    out = []
    for cap in (max(max(need), sum(need) // 5), max(need)):
        al = PA.PageAligner(DEV, scratch_cap=cap)
        res = al.run(*packed, PT.SIGMA_MAX)
        out.append(rec('chunked aligner, scratch_cap %d == pairs_align_cpu' % cap, _bad_run(res, counts, maps), 0, '%d chunks' % al.chunks))
        out.append(rec('chunked aligner, scratch_cap %d: at least 4 chunks, the scratch within the cap' % cap,
                       0 if al.chunks >= 4 and al.chunks == len(PA.chunk_pairs(packed[2], packed[4], cap)) and al.scratch.numel() <= cap else 1, 0,
                       '%d chunks, %d bytes' % (al.chunks, al.scratch.numel())))
    try:
        PA.PageAligner(DEV, scratch_cap=max(need) - 1).run(*packed, PT.SIGMA_MAX)
        bad = 1
    except ValueError as e:
        bad = 0 if str(max(need)) in str(e) else 1
    out.append(rec('the aligner refuses a pair above scratch_cap and names the bytes it needs', bad, 0))
    return out


def _device_case(pairs, gap=64, tail=4096, sigma=5):
    """pairs on the device for a direct ops.page_align call: maps pre-filled with SENTINEL, `gap` sentinel entries before, between and
    after the pairs' slices; scratch with a sentinel tail of `tail` bytes behind the declared size"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV
    pool, a_off, a_len, b_off, b_len = pack(pairs)
    n = a_len.astype(np.int64) + b_len
    map_off = gap + np.cumsum(n + gap) - (n + gap)
    maps_len = int(map_off[-1] + n[-1] + gap)
    need = np.asarray([ops.page_align_scratch_bytes(la, lb) for la, lb in zip(a_len.tolist(), b_len.tolist())], dtype=np.int64)
    scratch_off = np.cumsum(need) - need
    declared = int(need.sum())
    counts, maps = PA.pairs_align_cpu(pool, a_off, a_len, b_off, b_len, map_off)
    want = np.full(maps_len, SENTINEL, np.int32)
    want[:maps.size] = np.where(maps == PA.GAP, SENTINEL, maps)            # the entries no pair owns keep the sentinel
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)        # noqa: E731
    return dict(pool=t(pool), pool_bytes=int(pool.size), a_off=t(a_off), a_len=t(a_len), b_off=t(b_off), b_len=t(b_len), map_off=t(map_off),
                scratch_off=t(scratch_off), sigma=sigma, declared=declared, tail=tail, maps_len=maps_len, want_counts=counts, want_maps=want,
                host=dict(a_len=a_len, b_len=b_len, map_off=map_off, n=n, need=need, scratch_off=scratch_off, pool_size=int(pool.size)))


def _launch(case, **over):
    """one direct call with fresh sentinel buffers -> (counts, maps, scratch tail) as numpy; over: tables or scalars to replace"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV
    c = dict(case, **over)
    scratch = torch.full((c['declared'] + c['tail'],), 0x5a, dtype=torch.uint8, device=DEV)
    maps = torch.full((c['maps_len'],), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((4 * int(c['a_len'].numel()),), SENTINEL, dtype=torch.int32, device=DEV)
    ops.page_align(c['pool'], c['pool_bytes'], c['a_off'], c['a_len'], c['b_off'], c['b_len'], c['map_off'], c['scratch_off'], c['sigma'],
                   scratch[:c['declared']], maps, c['maps_len'], counts=counts)
    return counts.cpu().numpy().reshape(-1, 4), maps.cpu().numpy(), scratch[c['declared']:].cpu().numpy()


def _guard_pairs():
    rng = np.random.RandomState(9)
    strings = [rng.randint(0, 5, n).astype(np.uint8) for n in (10, 70, 200, 4100, 33, 0)]
    return [(strings[0], strings[1]), (strings[2], strings[3]), (strings[3], strings[2]), (strings[4], strings[4]), (strings[1], strings[4]),
            (strings[5], strings[0]), (strings[1], strings[5])]


def _refused(case, p):
    """what a call must give when pair p is refused: its counts -1, its slice of maps untouched"""
    counts, maps = case['want_counts'].copy(), case['want_maps'].copy()
    counts[p] = -1
    at, n = int(case['host']['map_off'][p]), int(case['host']['n'][p])
    maps[at:at + n] = SENTINEL
    return counts, maps


def check_guards():
    """maps with 64 sentinel entries around every slice, a 4 KiB sentinel tail behind the declared scratch: only the owned slices change;
    a refused pair's slice keeps the sentinel, its counts are -1 and the other pairs of the call are right"""
    from tests.gpu_checks import rec
    case = _device_case(_guard_pairs())
    counts, maps, tail = _launch(case)
    out = [rec('page align guards: counts == pairs_align_cpu', _bad(counts, case['want_counts']), 0),
           rec('page align guards: the owned slices == pairs_align_cpu and every other entry of maps keeps the sentinel', _bad(maps, case['want_maps']), 0,
               '%d of %d entries owned' % (int((case['want_maps'] != SENTINEL).sum()), maps.size)),
           rec('page align guards: the 4 KiB behind the declared scratch are untouched', int((tail != 0x5a).sum()), 0)]
    # the largest pair refused (its scratch slice would end past scratch_bytes): nothing of it is written, the others are right
    p = 2
    so = case['scratch_off'].clone()
    so[p] = case['declared'] - int(case['host']['need'][p]) + 8
    counts, maps, tail = _launch(case, scratch_off=so)
    wc, wm = _refused(case, p)
    out.append(rec('page align guards, a refused pair: counts -1, its slice keeps the sentinel, the other pairs are right', _bad(counts, wc) + _bad(maps, wm), 0))
    out.append(rec('page align guards, a refused pair: the scratch tail is untouched', int((tail != 0x5a).sum()), 0))
    return out


def check_refusals():
    """what the entry point refuses comes back as an error code and a message before any launch; what only the device tables show gives
    counts of -1 for that pair alone; nothing aborts"""
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    case = _device_case(_guard_pairs())
    h = case['host']
    P = int(case['a_len'].numel())
    out = []
    scratch = torch.zeros(case['declared'] + 8, dtype=torch.uint8, device=DEV)
    maps = torch.full((case['maps_len'],), SENTINEL, dtype=torch.int32, device=DEV)
    res = torch.full((4 * P,), SENTINEL, dtype=torch.int32, device=DEV)
    args = [ops.ptr(case['pool']), case['pool_bytes'], ops.ptr(case['a_off']), ops.ptr(case['a_len']), ops.ptr(case['b_off']), ops.ptr(case['b_len']),
            ops.ptr(case['map_off']), ops.ptr(case['scratch_off']), P, case['sigma'], ops.ptr(scratch), case['declared'], ops.ptr(maps), case['maps_len'],
            ops.ptr(res), ops.stream()]
    for k, what in ((0, 'pool'), (2, 'a_off'), (3, 'a_len'), (4, 'b_off'), (5, 'b_len'), (6, 'map_off'), (7, 'scratch_off'), (10, 'scratch'), (12, 'maps'),
                    (14, 'counts')):
        a = list(args)
        a[k] = None
        rc = _lib.lib().omp_page_align(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page align refuses a null %s with an error code' % what, 0 if rc == -22 and 'null pointer' in msg else 1, 0, msg))
    for what, k, v in (('n_pairs 0', 8, 0), ('n_pairs -1', 8, -1), ('n_pairs 2^24 + 1', 8, (1 << 24) + 1), ('sigma 255', 9, 255), ('sigma -1', 9, -1),
                       ('pool_bytes -1', 1, -1), ('maps_len -1', 13, -1), ('a scratch that is not 8-byte aligned', 10, ctypes.c_void_p(scratch.data_ptr() + 4))):
        a = list(args)
        a[k] = v
        rc = _lib.lib().omp_page_align(*a)
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('page align refuses %s with an error code' % what, 0 if rc == -22 and 'omp_page_align' in msg else 1, 0, msg))
    try:
        ops.page_align(case['pool'], case['pool_bytes'], case['a_off'], case['a_len'], case['b_off'], case['b_len'], case['map_off'], case['scratch_off'], 255,
                       scratch, maps, counts=res)
        bad = 1
    except RuntimeError as e:
        bad = 0 if 'omp_page_align' in str(e) and '(-22)' in str(e) and 'sigma' in str(e) else 1
    out.append(rec('the wrapper raises on sigma 255', bad, 0))
    torch.cuda.synchronize()
    out.append(rec('page align: nothing was written by the refused calls', int((res != SENTINEL).sum().item()) + int((maps != SENTINEL).sum().item()), 0))
    # what only the device tables show: the pair is refused on the device, its neighbours are aligned
    last = P - 1
    for what, key, p, v in (('a length of 65536', 'a_len', 1, PT.LEN_MAX + 1), ('a negative length', 'b_len', 2, -1), ('a negative offset', 'a_off', 3, -1),
                            ('a range past pool_bytes', 'b_off', 0, h['pool_size'] - int(h['b_len'][0]) + 1), ('a length past pool_bytes', 'a_len', 4, h['pool_size']),
                            ('a map slice past maps_len', 'map_off', last, case['maps_len'] - int(h['n'][last]) + 1), ('a negative map_off', 'map_off', 0, -1),
                            ('a negative scratch_off', 'scratch_off', 1, -8), ('a scratch_off that is no multiple of 8', 'scratch_off', 3, int(h['scratch_off'][3]) + 4),
                            ('a scratch slice past scratch_bytes', 'scratch_off', last, case['declared'] - int(h['need'][last]) + 8)):
        tab = case[key].clone()
        tab[p] = v
        counts, got_maps, tail = _launch(case, **{key: tab})
        wc, wm = _refused(case, p)
        out.append(rec('page align refuses %s on the device: counts -1, its maps untouched, the other pairs aligned' % what,
                       _bad(counts, wc) + _bad(got_maps, wm) + int((tail != 0x5a).sum()), 0, str(counts[p].tolist())))
    # the device stage
    al = PA.PageAligner(DEV)
    for what, kw in (('a length above the limit', dict(a_len=[PT.LEN_MAX + 1])), ('a range outside the pool', dict(b_off=[1])), ('sigma 255', dict(sigma=255)),
                     ('a code at or above sigma', dict(sigma=2))):
        a = dict(pool=np.asarray([0, 1, 2], np.uint8), a_off=[0], a_len=[3], b_off=[0], b_len=[3], sigma=3)
        a.update(kw)
        try:
            al.run(**a)
            bad = 1
        except ValueError:
            bad = 0
        out.append(rec('the aligner refuses %s on the host' % what, bad, 0))
    empty = al.run(np.zeros(0, np.uint8), [], [], [], [], 0)
    out.append(rec('the aligner on no pairs: nothing', int(empty['counts'].size) + int(empty['maps'].size), 0))
    zero = al.run(np.zeros(0, np.uint8), [0, 0], [0, 0], [0, 0], [0, 0], 0)
    out.append(rec('the aligner on empty strings: zero counts, no maps', _bad(zero['counts'], np.zeros((2, 4), np.int32)) + int(zero['maps'].size), 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
def _same_report(got, want):
    bad = sum(_bad(got[k], want[k]) for k in ('dist', 'len_pred', 'len_gt', 'match', 'sub', 'ins', 'dele'))
    bad += int(got['cer'] != want['cer']) + int(got['word_precision'] != want['word_precision']) + int(got['word_recall'] != want['word_recall'])
    bad += int(got['confusions'] != want['confusions'])
    for g, w in zip(got['pages'], want['pages']):
        bad += _bad(g['pred_to_gt'], w['pred_to_gt']) + _bad(g['gt_to_pred'], w['gt_to_pred']) + int(g['words'] != w['words']) + int(g['gt_words'] != w['gt_words'])
        bad += int(g['pred'] != w['pred']) + int(g['gt'] != w['gt'])
    return bad + abs(len(got['pages']) - len(want['pages']))


def check_engine_page_align(dtype_name):
    """the fixture of gpu_checks_page_text.check_engine_page_text (spot_windows' image and weights, windows = [default, 2 x 2 grid],
    suppress=0.5): align_page_text on the device == the host aligner; a call against its own words is all MATCH; against the blocks=True
    ordering the distance is score_page_text's"""
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
    tag = 'page align engine[%s]' % dtype_name
    plain = inf.predict(model, nt, args, windows=wins, suppress=0.5)
    blocks = inf.predict(model, nt, args, windows=wins, suppress=0.5, reading_order=True, blocks=True)
    truth = [[str(r['rec']) for r in recs] for recs in blocks]              # the blocks=True ordering, word by word
    host = PA.HostPageAligner()
    got = EV.align_page_text(copy.deepcopy(plain), truth, device=DEV)
    want = EV.align_page_text(copy.deepcopy(plain), truth, aligner=host)
    note = '%d records, %s characters, distances %s' % (sum(len(r) for r in plain), got['len_gt'].tolist(), got['dist'].tolist())
    out = [rec(tag + ' plain against the blocks=True ordering: every integer and status == the host aligner', _same_report(got, want), 0, note)]
    score = EV.score_page_text(copy.deepcopy(plain), truth, device=DEV)
    out.append(rec(tag + ' dist, len_pred, len_gt, score == score_page_text', _bad(got['dist'], score['dist']) + _bad(got['len_pred'], score['len_pred']) +
                   _bad(got['len_gt'], score['len_gt']) + int(not (got['score'] == score['score']).all()) + int(got['mean'] != score['mean']), 0))
    own = [[str(r['rec']) for r in recs] for recs in plain]
    me = EV.align_page_text(copy.deepcopy(plain), own, device=DEV)
    words = [w['status'] for p in me['pages'] for w in p['words'] if w['status'] != 'empty']
    gt_words = [w['status'] for p in me['pages'] for w in p['gt_words'] if w['status'] != 'empty']
    ok = (me['dist'] == 0).all() and (me['match'] == me['len_gt']).all() and int(me['len_gt'].sum()) > 0 and all(c in (0.0, None) for c in me['cer'])
    ok = ok and me['cer_micro'] == 0.0 and words and set(words) == {'correct'} and set(gt_words) == {'correct'} and me['word_precision'] == 1.0
    ok = ok and me['word_recall'] == 1.0 and all((p['pred_to_gt'] == np.arange(len(p['pred']))).all() for p in me['pages'])
    out.append(rec(tag + ' a call against its own words: all MATCH, every word CORRECT, cer 0', 0 if ok else 1, 0, '%d words' % len(words)))
    return out
