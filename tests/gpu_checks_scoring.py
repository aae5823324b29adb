"""GPU checks of scoring: omp_spotting_match against match_pages_cpu (utils/scoring.py) on every output
integer -- counts and both assignment arrays --, SpottingScorer against the specification with and without chunks, what the entry
point refuses, score_records on the device against score_records with the host scorer on the records of a real engine call, and the
structural time gate.  Every check returns records {name, err, tol, ok, note} like tests/gpu_checks.py."""
import copy
import statistics
import time

import numpy as np
import torch

from advancedliteratemachinery_amd.utils import overlap as OV
from advancedliteratemachinery_amd.utils import scoring as SC
from tests.scoring_cases import SIZES, pages

COMBOS = tuple((ti, td) for ti in (1, 500, 1000) for td in (1, 500, 1000))


def mixed40(seed=5):
    """40 images mixing SIZES: the two large ones a few times, the empty and one-sided ones often"""
    rng = np.random.RandomState(seed)
    pick = rng.choice(len(SIZES), 40, p=[0.1, 0.1, 0.1, 0.25, 0.2, 0.2, 0.05])
    pick[[3, 17, 39]] = [6, 0, 6]                # the 257-detection image inside and at the end, an empty one between others
    return tuple(SIZES[k] for k in pick)


class _Device(object):
    """one case on the device: the tables uploaded once, the intersections computed once (omp_polygon_overlap, tested on its own in
    tests/gpu_checks_overlap.py) and downloaded for the specification"""

    def __init__(self, case, grid, dev):
        from advancedliteratemachinery_amd import ops
        gs = case['group_start']
        self.n, self.G = int(gs[-1]), len(gs) - 1
        ms, ist = OV.mask_layout(gs)
        self.ist = ist
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)      # noqa: E731
        self.d = dict(inter_start=t(ist, torch.int64), group_start=t(gs, torch.int32), n_gt=t(case['n_gt'], torch.int32),
                      gt_dc=t(case['gt_dc'], torch.int32), text=t(case['text'], torch.int32), level=t(case['level'], torch.int32))
        self.inter = None
        self.flat = np.zeros(0, np.int32)
        if self.n:
            res = ops.polygon_overlap(t(case['polys'], torch.int32), self.d['group_start'], t(np.arange(self.n), torch.int32), t(ms, torch.int64),
                                      max(int(ms[-1]), 1), grid, 500, 0, inter_start=self.d['inter_start'], inter_total=int(ist[-1]))
            self.inter = res['inter']
            self.flat = self.inter.cpu().numpy()

    def match(self, n_thr, t_iou, t_dc, report):
        from advancedliteratemachinery_amd import ops
        d = self.d
        out = ops.spotting_match(self.inter, d['inter_start'], d['group_start'], d['n_gt'], d['gt_dc'], d['text'], d['level'], n_thr, t_iou, t_dc, report)
        return ops.split_match_ints(out.cpu().numpy(), self.n, self.G, n_thr)


def _diff(got, want):
    return sum(int((np.asarray(a) != np.asarray(b)).sum()) if np.asarray(a).shape == np.asarray(b).shape else 1 << 20 for a, b in zip(got, want))


def _op_cases():
    """(name, sizes, grid, n_thr, all_dc, [(t_iou, t_dc, report)]): every combination of the two thresholds on the single images,
    three of them on the 40-image mixes (the specification's time is what limits those)"""
    for k, size in enumerate(SIZES):
        yield 'G=1 %s grid=1000' % (size,), (size,), 1000, 2, False, [(ti, td, (0, 1, -1)[j % 3]) for j, (ti, td) in enumerate(COMBOS)]
    few = [(500, 500, 0), (1, 1000, None), (1000, 1, -1)]                 # report None: the last threshold
    yield 'G=40 grid=64 n_thr=64', mixed40(), 64, 64, False, few
    yield 'G=40 grid=1000 n_thr=1', mixed40(6), 1000, 1, False, few + [(500, 1, 0), (1, 500, 0)]
    yield 'G=1 (130, 257) grid=64 n_thr=64', (SIZES[-1],), 64, 64, False, few
    yield 'G=40 grid=64 n_thr=2, all ground truth don\'t-care', mixed40(7), 64, 2, True, few


def check_match_op():
    from tests.gpu_checks import DEV, rec
    out = []
    for c, (name, sizes, grid, n_thr, all_dc, combos) in enumerate(_op_cases()):
        case = pages(100 + c, sizes, grid, n_thr, all_dc=all_dc)
        dev = _Device(case, grid, DEV)
        matched = dc = 0
        for t_iou, t_dc, report in combos:
            report = n_thr - 1 if report is None else min(report, n_thr - 1)
            want = SC.match_pages_cpu(dev.flat, dev.ist, case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], n_thr, t_iou, t_dc,
                                      report)
            got = dev.match(n_thr, t_iou, t_dc, report)
            matched += int(want[0][..., 2].sum())
            dc += int((want[1] == SC.DET_DONT_CARE).sum())
            out.append(rec('match[%s] t_iou=%d t_dc=%d report=%d: counts, det_gt, gt_det' % (name, t_iou, t_dc, report), _diff(got, want), 0,
                           '%d polygons, %d matched over the sweep' % (dev.n, int(want[0][..., 2].sum()))))
        if any(min(m, nd) >= 60 for m, nd in sizes) and not all_dc:          # the small images are there for their shapes
            out.append(rec('match[%s] the case exercises matching' % name, 0 if matched > 0 else 1, 0, '%d matched, %d don\'t-care' % (matched, dc)))
        if all_dc and dev.n:
            out.append(rec('match[%s] the case exercises don\'t-care detections' % name, 0 if dc > 0 and matched == 0 else 1, 0, '%d don\'t-care' % dc))
        # the device stage as a whole on the same inputs: its intersections are the same kernel's
        t_iou, t_dc, report = combos[0]
        want = SC.match_pages_cpu(dev.flat, dev.ist, case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], n_thr, t_iou, t_dc, report)
        r = SC.SpottingScorer(DEV, grid).run(case['polys'], case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], n_thr, t_iou, t_dc,
                                             report)
        out.append(rec('match[%s] SpottingScorer.run == match_pages_cpu' % name, _diff((r['counts'], r['det_gt'], r['gt_det']), want), 0))
    return out


LARGE_PAGES = ((40, 1100), (1100, 40), (300, 700))      # up to 18 words of the free set: a wave owns words w, w + 4, w + 8, ...


def _stride_events(gt_det):
    """the matched detections of one image at the reported threshold (the REFERENCE's gt_det) -> (matches taken out of a free-set word
    >= 5, waves that take matches out of two or more different words of their own stride)"""
    d = gt_det[gt_det >= 0].astype(np.int64)
    words = d >> 6
    return int((words >= 5).sum()), sum(1 for w in range(4) if len(set(words[words % 4 == w].tolist())) >= 2)


def check_match_large():
    """pages of (40, 1100), (1100, 40) and (300, 700) (ground truth, detections), built like the smaller ones: the three in one call at
    n_thr = 2 against match_pages_cpu and, image by image, against the naive matcher (which is too slow for the sweep of 64); each
    alone at n_thr = 64 against match_pages_cpu.  Preconditions from the reference: on the two pages with more than 256 detections some
    combination matches out of a free-set word >= 5, and has a wave that matches out of two words of its own stride."""
    from tests.gpu_checks import DEV, rec
    from tests.scoring_cases import naive_match
    out = []
    grid = 1000
    held = {size: False for size in LARGE_PAGES if size[1] > 256}

    def events(name, want, case, sizes):
        for g, size in enumerate(sizes):
            lo = int(case['group_start'][g])
            high, waves = _stride_events(want[2][lo:lo + size[0]])
            if size in held:
                held[size] = held[size] or (high > 0 and waves > 0)
                out.append(rec('%s page %s: figures of the reference' % (name, size), 0, 0, '%d matches in words >= 5, %d waves with two words' % (high, waves)))

    # the three pages in one call, n_thr = 2: the specification and the naive matcher
    case = pages(120, LARGE_PAGES, grid, 2)
    dev = _Device(case, grid, DEV)
    gs = case['group_start']
    for t_iou, t_dc, report in ((500, 500, 0), (1000, 500, 1), (1, 1000, 1), (1000, 1, -1)):
        name = 'match[G=3 %s n_thr=2] t_iou=%d t_dc=%d report=%d' % (list(LARGE_PAGES), t_iou, t_dc, report)
        want = SC.match_pages_cpu(dev.flat, dev.ist, gs, case['n_gt'], case['gt_dc'], case['text'], case['level'], 2, t_iou, t_dc, report)
        got = dev.match(2, t_iou, t_dc, report)
        out.append(rec(name + ': counts, det_gt, gt_det', _diff(got, want), 0, '%d polygons, %d matched over the sweep' % (dev.n, int(want[0][..., 2].sum()))))
        bad = 0
        for g, (m, nd) in enumerate(LARGE_PAGES):
            lo, hi = int(gs[g]), int(gs[g + 1])
            mat = dev.flat[int(dev.ist[g]):int(dev.ist[g + 1])].reshape(hi - lo, hi - lo)
            naive = naive_match(mat, m, case['gt_dc'][lo:hi], case['text'][lo:hi], case['level'][lo:hi], 2, t_iou, t_dc, report)
            bad += _diff((got[0][g], got[1][lo + m:hi], got[2][lo:lo + m]), naive)
        out.append(rec(name + ': the device against the naive matcher, image by image', bad, 0))
        if report >= 0:
            events(name, want, case, LARGE_PAGES)
    # each page alone under the sweep of 64
    for c, size in enumerate(LARGE_PAGES):
        case = pages(130 + c, (size,), grid, 64)
        dev = _Device(case, grid, DEV)
        for t_iou, t_dc, report in ((500, 500, 0), (1000, 500, 63), (1, 1000, 40), (1000, 1, -1)):
            name = 'match[G=1 %s n_thr=64] t_iou=%d t_dc=%d report=%d' % (size, t_iou, t_dc, report)
            want = SC.match_pages_cpu(dev.flat, dev.ist, case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], 64, t_iou, t_dc, report)
            got = dev.match(64, t_iou, t_dc, report)
            out.append(rec(name + ': counts, det_gt, gt_det', _diff(got, want), 0, '%d polygons, %d matched over the sweep' % (dev.n, int(want[0][..., 2].sum()))))
            if report >= 0:
                events(name, want, case, (size,))
        r = SC.SpottingScorer(DEV, grid).run(case['polys'], case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], 64, 500, 500, 0)
        want = SC.match_pages_cpu(dev.flat, dev.ist, case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], 64, 500, 500, 0)
        out.append(rec('match[G=1 %s n_thr=64] SpottingScorer.run == match_pages_cpu' % (size,), _diff((r['counts'], r['det_gt'], r['gt_det']), want), 0))
    for size, ok in held.items():
        out.append(rec('precondition: page %s matches out of a free-set word >= 5, and one wave out of two words of its stride' % (size,), 0 if ok else 1, 0))
    return out


def check_chunked():
    """40 small images, the entry cap lowered so that they split into at least 3 chunks == pair_overlap_cpu + match_pages_cpu unchunked"""
    from tests.gpu_checks import DEV, rec
    rng = np.random.RandomState(11)
    sizes = tuple((int(rng.randint(0, 7)), int(rng.randint(0, 9))) for _ in range(40))
    case = pages(12, sizes, 64, 3)
    want = SC.HostScorer(64).run(case['polys'], case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], 3, 500, 500, 1)
    total = int(SC.inter_layout(case['group_start'])[-1])
    out = []
    for cap in (total // 3, max(m + d for m, d in sizes) ** 2, SC.ENTRY_CAP):
        sc = SC.SpottingScorer(DEV, 64, entry_cap=cap)
        got = sc.run(case['polys'], case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], 3, 500, 500, 1)
        bad = _diff([got[k] for k in ('counts', 'det_gt', 'gt_det')], [want[k] for k in ('counts', 'det_gt', 'gt_det')])
        out.append(rec('chunked scorer cap=%d == the unchunked specification' % cap, bad, 0, '%d chunks, %d matched' % (sc.chunks, int(want['counts'][..., 2].sum()))))
        if cap < total:
            out.append(rec('chunked scorer cap=%d splits into at least 3 chunks' % cap, 0 if sc.chunks >= 3 else 1, 0, '%d chunks' % sc.chunks))
        else:
            out.append(rec('scorer with the default cap: one chunk', abs(sc.chunks - 1), 0))
    try:
        SC.SpottingScorer(DEV, 64, entry_cap=max(m + d for m, d in sizes) ** 2 - 1).run(case['polys'], case['group_start'], case['n_gt'], case['gt_dc'],
                                                                                       case['text'], case['level'], 3)
        bad = 1
    except ValueError as e:
        bad = 0 if 'exceeds' in str(e) else 1
    out.append(rec('scorer refuses an image above the entry cap with a message', bad, 0))
    return out


def check_refusals():
    """what the entry point refuses comes back as an error code and a message, and what only the device tables show as counts of -1;
    nothing aborts"""
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    case = pages(1, ((2, 3), (1, 2)), 64, 2)
    dev = _Device(case, 64, DEV)
    d = dev.d
    good = dev.match(2, 500, 500, 0)
    out = []
    for what, kw in (('n_thr 0', dict(n_thr=0)), ('n_thr 65', dict(n_thr=65)), ('t_iou 0', dict(t_iou=0)), ('t_iou 1001', dict(t_iou=1001)),
                     ('t_dc 0', dict(t_dc=0)), ('t_dc 1001', dict(t_dc=1001)), ('report -2', dict(report=-2)), ('report n_thr', dict(report=2))):
        a = dict(n_thr=2, t_iou=500, t_dc=500, report=-1)
        a.update(kw)
        try:
            ops.spotting_match(dev.inter, d['inter_start'], d['group_start'], d['n_gt'], d['gt_dc'], d['text'], d['level'], a['n_thr'], a['t_iou'], a['t_dc'],
                               a['report'])
            bad = 1
        except RuntimeError as e:
            bad = 0 if 'omp_spotting_match' in str(e) and '(-22)' in str(e) else 1
        out.append(rec('match refuses %s with an error code' % what, bad, 0))
    res = torch.zeros(4 * 2 * 2 + 2 * dev.n, dtype=torch.int32, device=DEV)
    ptrs = [ops.ptr(dev.inter), ops.ptr(d['inter_start']), ops.ptr(d['group_start']), ops.ptr(d['n_gt']), ops.ptr(d['gt_dc']), ops.ptr(d['text']),
            ops.ptr(d['level'])]
    outs = [ops.ptr(res), ops.ptr(res[16:16 + dev.n]), ops.ptr(res[16 + dev.n:])]
    for k, what in enumerate(('inter', 'inter_start', 'group_start', 'n_gt', 'gt_dc', 'text', 'level', 'counts')):
        p, o = list(ptrs), list(outs)
        if k < 7:
            p[k] = None
        else:
            o[0] = None
        rc = _lib.lib().omp_spotting_match(*(p + [dev.n, dev.G, 2, 500, 500, -1] + o + [ops.stream()]))
        msg = _lib.lib().omp_last_error().decode()
        out.append(rec('match refuses a null %s with an error code' % what, 0 if rc == -22 and 'null pointer' in msg else 1, 0, msg))
    rc = _lib.lib().omp_spotting_match(*(ptrs + [dev.n, dev.G, 2, 500, 500, 0, outs[0], None, None, ops.stream()]))
    out.append(rec('match refuses a report without the assignment arrays', 0 if rc == -22 else 1, 0))
    torch.cuda.synchronize()
    out.append(rec('match: nothing was written by the refused calls', int(res.abs().sum().item()), 0))
    # what only the device tables show: the image is refused on the device, the others are scored
    n_gt = d['n_gt'].clone()
    n_gt[1] = 4                                                             # the second image holds 3 polygons
    got = ops.split_match_ints(ops.spotting_match(dev.inter, d['inter_start'], d['group_start'], n_gt, d['gt_dc'], d['text'], d['level'], 2, 500, 500,
                                                  0).cpu().numpy(), dev.n, dev.G, 2)
    bad = int((got[0][1] != -1).sum()) + int((got[0][0] != good[0][0]).sum()) + int((got[1][:5] != good[1][:5]).sum()) + int((got[1][5:] != -4).sum())
    out.append(rec('match refuses n_gt above the image\'s size on the device: counts -1, the other image scored', bad, 0))
    big = SC.GROUP_MAX + 1
    gs = torch.tensor([0, 5, 5 + big], dtype=torch.int32, device=DEV)
    ist = torch.tensor([0, 25, 25 + big * big], dtype=torch.int64, device=DEV)
    inter = torch.empty(25 + big * big, dtype=torch.int32, device=DEV)      # never read beyond the first image's 25 entries
    inter[:25] = dev.inter[:25]
    z = torch.zeros(5 + big, dtype=torch.int32, device=DEV)
    tab = {k: torch.cat([d[k][:5], z[5:]]) for k in ('gt_dc', 'text', 'level')}
    got = ops.split_match_ints(ops.spotting_match(inter, ist, gs, torch.tensor([2, 1], dtype=torch.int32, device=DEV), tab['gt_dc'], tab['text'], tab['level'],
                                                  2, 500, 500, 0).cpu().numpy(), 5 + big, 2, 2)
    bad = int((got[0][1] != -1).sum()) + int((got[0][0] != good[0][0]).sum()) + int((got[1][:5] != good[1][:5]).sum()) + int((got[1][5:] != -4).sum())
    out.append(rec('match refuses an image of %d polygons on the device: counts -1, the other image scored' % big, bad, 0))
    del inter
    try:
        SC.SpottingScorer(DEV, 64).run(np.zeros((big, 32), np.int32), [0, big], [1], np.zeros(big), np.zeros(big), np.zeros(big), 1)
        bad = 1
    except ValueError:
        bad = 0
    out.append(rec('the scorer refuses an image of %d polygons on the host' % big, bad, 0))
    r = SC.SpottingScorer(DEV, 64).run(np.zeros((0, 32), np.int32), [0, 0, 0], [0, 0], [], [], [], 3)
    out.append(rec('the scorer on images without polygons: zero counts', int(np.abs(r['counts']).sum()) + int(r['counts'].shape != (2, 3, 4)), 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
def check_engine_score(dtype_name):
    """spot_windows' image and weights, windows = [default, default, 2 x 2 grid]: score_records on the device == score_records with the
    host scorer, on ground truth made of the suppress=0.5 call's own records, for the plain and the suppressed records"""
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
    wins = [WN.default_window(args), WN.default_window(args)] + WN.grid_windows(2, 2, args.num_bins)
    sizes = [(int(img.shape[2]), int(img.shape[3]))] * int(img.shape[0])
    tag = 'score engine[%s]' % dtype_name
    plain = inf.predict(model, nt, args, windows=wins)
    kept = inf.predict(model, nt, args, windows=wins, suppress=0.5)
    # The ground truth is made of the suppress=0.5 call's own records.  Windows 0 and 1 are the same window, so the plain call returns
    # every word of it twice; ground truth made of THOSE records would hold every such word twice as well, and a one-to-one matching
    # must then lose a match for every duplicate that suppression removes, whatever the matcher does.  Made of the survivors, every
    # ground-truth word is a distinct word, no two of them overlap at 0.5, and each has its own exact copy among the suppressed call's
    # detections: that call's matches are the most the words allow, and the plain call's cannot exceed them.
    truth = []
    for recs in kept:
        words = []
        for k, r in enumerate(recs):
            if k % 3 == 2:
                continue                                                    # every third dropped
            words.append(dict(poly=r['polys'], text=r['rec'] + ('#' if k % 7 == 6 else ''), dc=k % 5 == 4))
        truth.append(words)
    altered = sum(1 for words in truth for w in words if w['text'].endswith('#') and not w['dc'])
    scores = sorted(set(float(r['score']) for recs in plain for r in recs))
    th = [0.0] + [s for s in (scores[len(scores) // 3], scores[2 * len(scores) // 3]) if s > 0.0]
    th = sorted(set(th))
    out = []
    results = {}
    for name, recs in (('plain', plain), ('suppress=0.5', kept)):
        on_dev, on_host = copy.deepcopy(recs), copy.deepcopy(recs)
        got = EV.score_records(on_dev, truth, sizes, args.num_bins, thresholds=th, report=len(th) - 1, device=DEV)
        want = EV.score_records(on_host, truth, sizes, args.num_bins, thresholds=th, report=len(th) - 1, scorer=SC.HostScorer(args.num_bins))
        results[name] = got
        note = '%d records, %d words, thresholds %s, totals %s' % (sum(len(r) for r in recs), sum(len(w) for w in truth), [round(t, 3) for t in th],
                                                                got['total'].tolist())
        out.append(rec('%s %s: counts == the host scorer' % (tag, name), _diff([got['counts'], got['total']], [want['counts'], want['total']]), 0, note))
        out.append(rec('%s %s: best and matches' % (tag, name), 0 if got['best'] == want['best'] and got['matches'] == want['matches'] else 1, 0))
        same = all('gt' in a and a['gt'] == b['gt'] and a['gt_text'] == b['gt_text'] for ra, rb in zip(on_dev, on_host) for a, b in zip(ra, rb))
        out.append(rec('%s %s: gt on every record' % (tag, name), 0 if same else 1, 0))
    p, s = results['plain']['total'][0], results['suppress=0.5']['total'][0]
    out.append(rec(tag + ' something is matched, and an altered text costs an end-to-end match', 0 if s[2] > 0 and (s[3] < s[2] if altered else s[3] <= s[2]) else 1, 0,
                   'suppressed totals %s, %d care words with an altered text' % (s.tolist(), altered)))
    out.append(rec(tag + ' suppress=0.5: the care detections fall', 0 if s[1] < p[1] else 1, 0, '%d -> %d' % (p[1], s[1])))
    out.append(rec(tag + ' suppress=0.5: matched does not fall', 0 if s[2] >= p[2] else 1, 0, '%d -> %d' % (p[2], s[2])))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the structural time gate
# ---------------------------------------------------------------------------------------------------------------------------------
def check_timing():
    """G = 40, n_thr = 64: the median of 3 whole SpottingScorer.run calls (upload, intersections, matching, download) at or below ONE
    match_pages_cpu call on the same inputs, which is handed its intersections.  No margin: it catches a launch or a synchronisation
    per image, not a tuning."""
    from tests.gpu_checks import DEV, rec
    case = pages(107, mixed40(), 64, 64)
    args = (case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], 64, 500, 500, 0)
    sc = SC.SpottingScorer(DEV, 64)
    got = sc.run(case['polys'], *args)                                      # warm: library load, allocator
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = sc.run(case['polys'], *args)
        ms.append((time.perf_counter() - t0) * 1e3)
    flat = np.concatenate([m.reshape(-1) for m in OV.pair_overlap_cpu(case['polys'], case['group_start'], 64)])
    t0 = time.perf_counter()
    want = SC.match_pages_cpu(flat, SC.inter_layout(case['group_start']), *args)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    note = 'device run %s ms (median %.3f), match_pages_cpu %.1f ms, %d polygons in 40 images' % ([round(v, 3) for v in ms], statistics.median(ms), cpu_ms,
                                                                                             int(case['group_start'][-1]))
    print(note)
    return [rec('scoring: G=40, n_thr=64, median of 3 device runs <= one match_pages_cpu call', statistics.median(ms), cpu_ms, note),
            rec('scoring: the timed outputs are equal', _diff((got['counts'], got['det_gt'], got['gt_det']), want), 0)]
