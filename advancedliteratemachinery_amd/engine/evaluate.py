"""Scoring spotting results against ground truth: precision, recall and h-mean for detection and end-to-end reading over a sweep of
score thresholds (utils/scoring.py holds the protocol and its specification, csrc/score.hip the matcher).

    score_records      the records any entry point returns + ground-truth words -> counts and metrics, ONE device flow per call
    evaluate_spotting  images + ground truth -> predict_images / spot_and_recognize in calls of `batch`, scored as they come
    score_page_text    the records of every image as ONE string against the page's ground-truth text: the normalised edit distance, which
                       depends on the order of the records (utils/page_text.py holds the specification)
    sweep_reading      the same records re-ordered under every candidate setting of the reading stage, all scored in ONE device call
    evaluate_reading   images + ground-truth texts -> engine calls of `batch`, then score_page_text or sweep_reading
    align_page_text    the edit script behind score_page_text's distance: S / D / I counts, CER, confusions, per-word status and the boxes
                       of the records that carry each ground-truth word (utils/page_align.py holds the specification)

Agreement with the official ICDAR / Total-Text evaluation scripts has not been checked (they are not part of this project)."""
import inspect

import numpy as np

from ..utils import scoring as SC

TEXT_KEYS = {'rec': None, 'lex': 'rec', 'mgp_text': None, 'mgp_lex': 'mgp_text'}     # key -> the key a None value falls back to


def _text_of(record, key):
    v = record.get(key)
    if v is None and TEXT_KEYS[key] is not None:
        v = record.get(TEXT_KEYS[key])
    if v is None:
        raise KeyError('a record has no %r%s' % (key, '' if TEXT_KEYS[key] is None else ' and no %r' % TEXT_KEYS[key]))
    return v


def summarise(counts, thresholds):
    """counts [G, T, 4] -> the part of score_records' result that follows from them"""
    counts = np.asarray(counts, dtype=np.int32).reshape(-1, len(thresholds), 4)
    total = counts.astype(np.int64).sum(0)
    m = SC.metrics(total)
    return dict(counts=counts, total=total, det=m['det'], e2e=m['e2e'], best=dict(det=m['det']['best'], e2e=m['e2e']['best']),
                thresholds=[float(t) for t in thresholds])


def score_records(records, ground_truth, sizes, bins, thresholds=(0.0,), iou=0.5, dc_overlap=0.5, text_key='rec', normalise=str.casefold,
                  min_len=0, report=None, scorer=None, device=None):
    """records: per image the list of record dicts any entry point returns (`polys`: 16 [x, y] pairs in original pixels, `score`, and
    the text under `text_key`).  ground_truth: per image a list of {'poly': [[x, y], ...] (3 .. 16 vertices, original pixels), 'text':
    str, 'dc': bool} (utils/ground_truth.py reads two layouts).  sizes: (h, w) per image.  bins: the grid both sides are quantised to
    (utils.scoring.quantise; 2 .. 4096, e.g. args.num_bins).
    thresholds: 1 .. 64 strictly ascending score thresholds; a record counts at a threshold when its `score` is at or above it.
    iou, dc_overlap: floats in (0, 1], taken at permille resolution with >=: a detection matches a word at IoU >= iou, and is don't-care
    when a don't-care word covers at least dc_overlap of it.  text_key: 'rec', 'lex', 'mgp_text' or 'mgp_lex' (a None `lex` /
    `mgp_lex` falls back to `rec` / `mgp_text`); normalise: a callable applied to both sides' strings before they are compared, or
    None.  min_len > 0: ground-truth words shorter than that become don't-care.
    report: a threshold index whose assignment is written back -- every record gains `gt` (the matched ground-truth index inside its
    image, -1 unmatched, -2 don't-care, -3 below the threshold) and `gt_text` (the matched word's text or None).
    scorer: a utils.scoring.SpottingScorer, or anything with its `run` (HostScorer: the specification); default: one on `device`
    (default 'cuda').  All images go through the scorer in one call.
    -> dict(counts int32 [G, T, 4] = per image and threshold (care ground truth, care detections, matched, matched with equal text),
    total [T, 4], det / e2e = dict(precision, recall, hmean: lists of T floats; best), best = dict(det, e2e: the threshold index of the
    highest h-mean, ties to the lowest), thresholds, matches: with report, per image the matched detection index of every ground-truth
    word (-1 unmatched, -2 don't-care), else None)."""
    if text_key not in TEXT_KEYS:
        raise ValueError('text_key must be one of %s, got %r' % (sorted(TEXT_KEYS), text_key))
    if not (len(records) == len(ground_truth) == len(sizes)):
        raise ValueError('records, ground_truth and sizes are per image: got %d, %d and %d' % (len(records), len(ground_truth), len(sizes)))
    th = SC.check_thresholds(thresholds)
    t_iou, t_dc = SC.permille(iou, 'iou'), SC.permille(dc_overlap, 'dc_overlap')
    rep = -1 if report is None else int(report)
    if rep < -1 or rep >= th.size:
        raise ValueError('report must be None or a threshold index below %d, got %r' % (th.size, report))
    polys, gs, n_gt, dc, scores, gt_texts, det_texts = [], [0], [], [], [], [], []
    for b, (recs, words, size) in enumerate(zip(records, ground_truth, sizes)):
        for r in recs:
            if not isinstance(r, dict) or 'polys' not in r:
                raise ValueError('image %d: score_records needs text-spotting records (dicts with `polys`)' % b)
        polys.append(SC.quantise([w['poly'] for w in words], size, bins))
        polys.append(SC.quantise([r['polys'] for r in recs], size, bins))
        n_gt.append(len(words))
        gs.append(gs[-1] + len(words) + len(recs))
        dc += [1 if (w.get('dc', False) or len(w['text']) < int(min_len)) else 0 for w in words] + [0] * len(recs)
        scores += [0.0] * len(words) + [float(r['score']) for r in recs]
        gt_texts.append([w['text'] for w in words])
        det_texts.append([_text_of(r, text_key) for r in recs])
    ids_gt, ids_det = SC.text_ids([t for ts in gt_texts for t in ts], [t for ts in det_texts for t in ts], normalise)
    text, a, c = [], 0, 0
    for ts_gt, ts_det in zip(gt_texts, det_texts):
        text += [ids_gt[a:a + len(ts_gt)], ids_det[c:c + len(ts_det)]]
        a, c = a + len(ts_gt), c + len(ts_det)
    text = np.concatenate(text + [np.zeros(0, np.int32)]).astype(np.int32)
    polys = np.concatenate(polys + [np.zeros((0, 32), np.int32)])
    if scorer is None:
        scorer = SC.SpottingScorer('cuda' if device is None else device, bins)
    res = scorer.run(polys, np.asarray(gs, np.int32), np.asarray(n_gt, np.int32), np.asarray(dc, np.int32), text, SC.levels(scores, th), int(th.size),
                     t_iou, t_dc, rep)
    out = summarise(res['counts'], th)
    out['matches'] = None
    if rep >= 0:
        out['matches'] = []
        for b, (recs, words) in enumerate(zip(records, ground_truth)):
            lo, m = gs[b], n_gt[b]
            out['matches'].append([int(v) for v in res['gt_det'][lo:lo + m]])
            for r, i in zip(recs, res['det_gt'][lo + m:gs[b + 1]].tolist()):
                r['gt'] = int(i)
                r['gt_text'] = words[i]['text'] if i >= 0 else None
    return out


_SCORE_ARGS = tuple(p for p in inspect.signature(score_records).parameters if p not in ('records', 'ground_truth', 'sizes', 'bins'))


def evaluate_spotting(model, images_u8, ground_truth, args, batch=8, mgp=None, bins=None, **kw):
    """images_u8: uint8 RGB [H, W, 3] arrays / tensors; ground_truth: per image the list of words (score_records).  The images go through
    predict_images -- spot_and_recognize(model, mgp, ...) when a recogniser `mgp` is given -- in calls of `batch`; every keyword
    argument that score_records takes (thresholds, iou, dc_overlap, text_key, normalise, min_len, report, scorer, device) goes there,
    every other one (ragged, windows / grid, suppress, reading_order, lexicon, tiles, crop, ...) to the engine call.  Each call is scored
    as it comes (bins: the scoring grid, default args.num_bins) and the counts are put together at the end.
    -> score_records' result over all images, plus `records`: the records per image.  KIE is refused: entity tuples are not words."""
    if args.infer_vie:
        raise ValueError('evaluate_spotting scores text-spotting records; with args.infer_vie the engine returns entity tuples')
    if len(images_u8) != len(ground_truth):
        raise ValueError('%d images for %d ground-truth lists' % (len(images_u8), len(ground_truth)))
    batch = int(batch)
    if batch < 1:
        raise ValueError('batch must be at least 1, got %d' % batch)
    skw = {k: kw.pop(k) for k in _SCORE_ARGS if k in kw}
    if mgp is None and skw.get('text_key', 'rec') in ('mgp_text', 'mgp_lex'):
        raise ValueError('text_key=%r needs a recogniser: pass mgp=' % skw['text_key'])
    bins = int(args.num_bins if bins is None else bins)
    th = SC.check_thresholds(skw.get('thresholds', (0.0,)))
    if skw.get('scorer') is None:
        dev = skw.get('device')
        skw['scorer'] = SC.SpottingScorer(next(model.parameters()).device if dev is None else dev, bins)
    from . import inference as inf
    pre, resizer, records, counts, matches = kw.pop('preprocessor', None), kw.pop('resizer', None), [], [], []
    names = kw.pop('file_names', None)
    if names is None:
        names = [str(b) for b in range(len(images_u8))]           # as ONE call over all images would name them
    for lo in range(0, len(images_u8), batch):
        imgs = list(images_u8[lo:lo + batch])
        if mgp is None:
            recs, pre = inf.predict_images(model, imgs, args, file_names=names[lo:lo + batch], preprocessor=pre, **kw)
        else:
            from .two_stage import spot_and_recognize
            recs, pre, resizer = spot_and_recognize(model, mgp, imgs, args, file_names=names[lo:lo + batch], preprocessor=pre, resizer=resizer, **kw)
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
        part = score_records(recs, ground_truth[lo:lo + batch], sizes, bins, **skw)
        records.extend(recs)
        counts.append(part['counts'])
        if part['matches'] is not None:
            matches.extend(part['matches'])
    out = summarise(np.concatenate(counts + [np.zeros((0, th.size, 4), np.int32)]), th)
    out['matches'] = matches if skw.get('report') is not None else None
    out['records'] = records
    return out


# ---------------------------------------------------------------------------------------------
# page text: the normalised edit distance of whole pages
# ---------------------------------------------------------------------------------------------
READING_KEYS = ('line_gap', 'line_back', 'line_offset', 'blocks', 'block_gap_x', 'block_gap_y', 'block_depth')


def _check_page_records(records, gt_texts, text_key, what):
    if text_key not in TEXT_KEYS:
        raise ValueError('text_key must be one of %s, got %r' % (sorted(TEXT_KEYS), text_key))
    if len(records) != len(gt_texts):
        raise ValueError('records and gt_texts are per image: got %d and %d' % (len(records), len(gt_texts)))
    for b, recs in enumerate(records):
        for r in recs:
            if not isinstance(r, dict) or 'polys' not in r:
                raise ValueError('image %d: %s needs text-spotting records (dicts with `polys`)' % (b, what))


def _gt_string(gt, strip, normalise):
    from ..utils import page_text as PT
    return PT.page_string(gt, 'text', strip, normalise)


def _page_summary(dist, a_len, b_len):
    from ..utils import page_text as PT
    s = PT.page_scores(dist, a_len, b_len)
    return dict(dist=np.asarray(dist, dtype=np.int32), len_pred=np.asarray(a_len, dtype=np.int32), len_gt=np.asarray(b_len, dtype=np.int32),
                score=s['score'], mean=s['mean'], micro=s['micro'])


def score_page_text(records, gt_texts, text_key='rec', strip=' \n', normalise=str.casefold, scorer=None, device=None):
    """records: per image the list of record dicts any entry point returns, IN THE ORDER IT RETURNED THEM (the text under `text_key`,
    with the fallbacks of score_records).  gt_texts: per image the page's text -- one string, or the list of its words in reading
    order (strings, or dicts with `text`); whether the annotation's order is the reading order is the caller's responsibility.
    Every image becomes one prediction string and one ground-truth string (utils.page_text.page_string: concatenated, the characters
    of `strip` removed, `normalise` applied or None) and is scored by the reference's normalised edit distance.
    scorer: a utils.page_text.PageTextScorer, or anything with its `run` (HostPageScorer: the specification); default: one on `device`
    (default 'cuda').  All images go through the scorer in one call.
    -> dict(dist int32 [G] = the Levenshtein distance per image, len_pred, len_gt int32 [G], score float64 [G] = 1 - dist / max(len_pred,
    len_gt) (1.0 for two empty strings), mean = the average of score (the reference's figure), micro = 1 - sum(dist) / sum(max))."""
    from ..utils import page_text as PT
    _check_page_records(records, gt_texts, text_key, 'score_page_text')
    pred = [PT.page_string(recs, text_key, strip, normalise) for recs in records]
    truth = [_gt_string(gt, strip, normalise) for gt in gt_texts]
    pool, a_off, a_len, b_off, b_len, sigma = PT.encode_pairs(pred, truth)
    if scorer is None:
        scorer = PT.PageTextScorer('cuda' if device is None else device)
    dist = scorer.run(pool, a_off, a_len, b_off, b_len, sigma)
    return _page_summary(dist, a_len, b_len)


def sweep_reading(records, sizes, bins, gt_texts, settings, text_key='rec', strip=' \n', normalise=str.casefold, reader=None, scorer=None,
                  device=None):
    """The reading stage's knobs against ground-truth page texts, without running the model again.  records, gt_texts: as
    score_page_text; sizes: (h, w) per image; settings: a list whose entries are None ("as given, not re-ordered") or dicts of
    utils.reading.order_records' keywords line_gap, line_back, line_offset, blocks, block_gap_x, block_gap_y, block_depth.
    Every setting re-orders COPIES of the records with order_records (one reading call per setting: `reader`, a
    utils.reading.ReadingOrder or anything with its __call__; default: one on `device`).  The polygons are
    utils.scoring.quantise(r['polys'], size, bins): the grid of DESIGN.md section 21, computed from the records' pixels, which can sit
    one bin below the ids the polygon decoder itself produced -- no private engine state is needed.
    All images x settings are scored in ONE scorer.run; a page's ground truth is stored once and shared by its settings.
    -> dict(settings = per setting score_page_text's result, best = the index of the highest mean, ties to the lowest)."""
    import torch

    from ..utils import page_text as PT
    from ..utils import reading as RD
    _check_page_records(records, gt_texts, text_key, 'sweep_reading')
    if len(sizes) != len(records):
        raise ValueError('records and sizes are per image: got %d and %d' % (len(records), len(sizes)))
    settings = list(settings)
    if not settings:
        raise ValueError('settings must hold at least one entry')
    for k, st in enumerate(settings):
        if st is not None and (not isinstance(st, dict) or any(key not in READING_KEYS for key in st)):
            raise ValueError('setting %d must be None or a dict with keys among %s, got %r' % (k, list(READING_KEYS), st))
    G = len(records)
    polys = None
    pred = []
    for st in settings:
        if st is None:
            ordered = records
        else:
            if polys is None:
                polys = [torch.from_numpy(SC.quantise([r['polys'] for r in recs], size, bins)) for recs, size in zip(records, sizes)]
            copies = [[dict(r) for r in recs] for recs in records]
            ordered = RD.order_records(copies, polys, sizes, int(bins), reader=reader, device='cuda' if device is None and reader is None else device, **st)
        pred += [PT.page_string(recs, text_key, strip, normalise) for recs in ordered]
    truth = [_gt_string(gt, strip, normalise) for gt in gt_texts]
    pool, a_off, a_len, b_off, b_len, sigma = PT.encode_pairs(pred, truth * len(settings))
    if scorer is None:
        scorer = PT.PageTextScorer('cuda' if device is None else device)
    dist = scorer.run(pool, a_off, a_len, b_off, b_len, sigma)
    out = [_page_summary(dist[k * G:(k + 1) * G], a_len[k * G:(k + 1) * G], b_len[k * G:(k + 1) * G]) for k in range(len(settings))]
    means = [s['mean'] for s in out]
    return dict(settings=out, best=means.index(max(means)))


_PAGE_ARGS = ('text_key', 'strip', 'normalise', 'scorer', 'device', 'reader')


def evaluate_reading(model, images_u8, gt_texts, args, batch=8, mgp=None, settings=None, **kw):
    """images_u8: uint8 RGB [H, W, 3] arrays / tensors; gt_texts: per image the page's text (score_page_text).  The images go through
    predict_images -- spot_and_recognize(model, mgp, ...) when a recogniser `mgp` is given -- in calls of `batch`; text_key, strip,
    normalise, scorer, device and reader go to the scoring, `bins` (default args.num_bins) is sweep_reading's grid, every other
    keyword (ragged, windows / grid, suppress, reading_order, blocks, lexicon, tiles, ...) to the engine call.  The records are
    collected and the distances are put together at the end: score_page_text over all images, or, with `settings`, sweep_reading.
    -> that function's result, plus `records`: the records per image.  KIE is refused: entity tuples are not words."""
    if args.infer_vie:
        raise ValueError('evaluate_reading scores text-spotting records; with args.infer_vie the engine returns entity tuples')
    if len(images_u8) != len(gt_texts):
        raise ValueError('%d images for %d ground-truth texts' % (len(images_u8), len(gt_texts)))
    batch = int(batch)
    if batch < 1:
        raise ValueError('batch must be at least 1, got %d' % batch)
    skw = {k: kw.pop(k) for k in _PAGE_ARGS if k in kw}
    if mgp is None and skw.get('text_key', 'rec') in ('mgp_text', 'mgp_lex'):
        raise ValueError('text_key=%r needs a recogniser: pass mgp=' % skw['text_key'])
    bins = kw.pop('bins', None)
    bins = int(args.num_bins if bins is None else bins)
    if skw.get('device') is None and skw.get('scorer') is None:
        skw['device'] = next(model.parameters()).device
    from . import inference as inf
    pre, resizer, records = kw.pop('preprocessor', None), kw.pop('resizer', None), []
    names = kw.pop('file_names', None)
    if names is None:
        names = [str(b) for b in range(len(images_u8))]
    for lo in range(0, len(images_u8), batch):
        imgs = list(images_u8[lo:lo + batch])
        if mgp is None:
            recs, pre = inf.predict_images(model, imgs, args, file_names=names[lo:lo + batch], preprocessor=pre, **kw)
        else:
            from .two_stage import spot_and_recognize
            recs, pre, resizer = spot_and_recognize(model, mgp, imgs, args, file_names=names[lo:lo + batch], preprocessor=pre, resizer=resizer, **kw)
        records.extend(recs)
    if settings is None:
        skw.pop('reader', None)
        out = score_page_text(records, gt_texts, **skw)
    else:
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images_u8]
        out = sweep_reading(records, sizes, bins, gt_texts, settings, **skw)
    out['records'] = records
    return out


# ---------------------------------------------------------------------------------------------
# page text alignment
# ---------------------------------------------------------------------------------------------
def _union_box(records):
    pts = [p for r in records for p in r['polys']]
    if not pts:
        return None
    xs, ys = [float(p[0]) for p in pts], [float(p[1]) for p in pts]
    return (min(xs), min(ys), max(xs), max(ys))


def _top(table, top):
    """a {key: n} table -> the `top` most frequent as [(key, n)], ties by key"""
    return sorted(table.items(), key=lambda kv: (-kv[1], kv[0]))[:max(int(top), 0)]


def align_page_text(records, gt_texts, text_key='rec', strip=' \n', normalise=str.casefold, top=20, aligner=None, device=None):
    """records and gt_texts: as score_page_text takes them.  Every image becomes one prediction string and one ground-truth string
    (utils.page_align.page_words: every word stripped and normalised on its own, then concatenated) and the two are aligned by the
    canonical optimal edit script (utils.page_align holds the rule).  aligner: a utils.page_align.PageAligner, or anything with its
    `run` (HostPageAligner: the specification); default: one on `device` (default 'cuda').  All images go through ONE aligner.run.
    -> dict(dist, len_pred, len_gt, match, sub, ins, dele int32 [G]; score, mean, micro as score_page_text gives them; cer = per image
    (sub + ins + dele) / len_gt, None for an empty ground truth; cer_micro = the same over all images; word_precision = the CORRECT
    prediction words over the non-empty ones; word_recall = the same over ground-truth words, None when every page's ground truth is one
    string; confusions = dict(sub=[((pred_char, gt_char), n)], ins=[(char, n)], dele=[(char, n)]), the `top` most frequent over all
    images; pages = per image dict(pred, gt = the aligned strings, pred_to_gt, gt_to_pred = the maps (-1: no partner), words = per
    record dict(chars=(start, end) in pred, status, span = its images in gt or (-1, -1)), gt_words = per ground-truth word dict(text,
    chars, status, span in pred, records=(first, last) = the records whose characters carry that span -- first the first record with
    start + len > span[0], last the last with start < span[1] -- and box = (x0, y0, x1, y1), the union of their `polys` in pixels;
    records and box are None for an ABSENT or EMPTY word)).  Statuses are utils.page_align.STATUS_NAMES."""
    from ..utils import page_align as PA
    from ..utils import page_text as PT
    _check_page_records(records, gt_texts, text_key, 'align_page_text')
    records = [list(recs) for recs in records]
    pred = [PA.page_words(recs, text_key, strip, normalise) for recs in records]
    truth = [PA.page_words(gt, 'text', strip, normalise) for gt in gt_texts]
    pool, a_off, a_len, b_off, b_len, sigma = PT.encode_pairs([p[0] for p in pred], [t[0] for t in truth])
    if aligner is None:
        aligner = PA.PageAligner('cuda' if device is None else device)
    res = aligner.run(pool, a_off, a_len, b_off, b_len, sigma)
    counts = np.asarray(res['counts'], dtype=np.int32).reshape(-1, 4)
    dist = counts[:, PA.SUB] + counts[:, PA.INS] + counts[:, PA.DEL]
    out = _page_summary(dist, a_len, b_len)
    out.update(match=counts[:, PA.MATCH].copy(), sub=counts[:, PA.SUB].copy(), ins=counts[:, PA.INS].copy(), dele=counts[:, PA.DEL].copy())
    out['cer'] = [int(d) / int(n) if n else None for d, n in zip(dist.tolist(), b_len.tolist())]
    out['cer_micro'] = int(dist.sum()) / int(b_len.sum()) if int(b_len.sum()) else None
    conf = dict(sub={}, ins={}, dele={})
    tally = dict(pred=[0, 0], gt=[0, 0])                                      # correct words, non-empty words
    pages = []
    for g, (recs, (ptext, p_start, p_len), (ttext, t_start, t_len)) in enumerate(zip(records, pred, truth)):
        a_map, b_map = PA.split_maps(res, a_len, b_len, g)
        for kind, table in PA.confusions(ptext, ttext, a_map, b_map).items():
            for key, n in table.items():
                conf[kind][key] = conf[kind].get(key, 0) + n
        p_status, p_span = PA.word_report_cpu(a_map, p_start, p_len, ptext, ttext)
        t_status, t_span = PA.word_report_cpu(b_map, t_start, t_len, ttext, ptext)
        for side, status in (('pred', p_status), ('gt', t_status)):
            tally[side][0] += int((status == PA.CORRECT).sum())
            tally[side][1] += int((status != PA.EMPTY).sum())
        p_end = p_start + p_len
        words = [dict(chars=(int(s), int(e)), status=PA.STATUS_NAMES[st], span=(int(sp[0]), int(sp[1])))
                 for s, e, st, sp in zip(p_start.tolist(), p_end.tolist(), p_status.tolist(), p_span.tolist())]
        gt_words = []
        for s, n, st, sp in zip(t_start.tolist(), t_len.tolist(), t_status.tolist(), t_span.tolist()):
            w = dict(text=ttext[s:s + n], chars=(s, s + n), status=PA.STATUS_NAMES[st], span=(int(sp[0]), int(sp[1])), records=None, box=None)
            if sp[0] >= 0:
                first = int(np.searchsorted(p_end, sp[0], side='right'))         # the first record with start + len > span[0]
                last = int(np.searchsorted(p_start, sp[1], side='left')) - 1    # the last record with start < span[1]
                w['records'] = (first, last)
                w['box'] = _union_box(recs[first:last + 1])
            gt_words.append(w)
        pages.append(dict(pred=ptext, gt=ttext, pred_to_gt=np.asarray(a_map, dtype=np.int32), gt_to_pred=np.asarray(b_map, dtype=np.int32), words=words,
                          gt_words=gt_words))
    out['word_precision'] = tally['pred'][0] / tally['pred'][1] if tally['pred'][1] else None
    one_string = all(isinstance(gt, str) for gt in gt_texts)
    out['word_recall'] = None if one_string or not tally['gt'][1] else tally['gt'][0] / tally['gt'][1]
    out['confusions'] = {kind: _top(table, top) for kind, table in conf.items()}
    out['pages'] = pages
    return out
