"""Scoring spotting results against ground truth: precision, recall and h-mean for detection and end-to-end reading over a sweep of
score thresholds (utils/scoring.py holds the protocol and its specification, csrc/score.hip the matcher).

    score_records      the records any entry point returns + ground-truth words -> counts and metrics, ONE device flow per call
    evaluate_spotting  images + ground truth -> predict_images / spot_and_recognize in calls of `batch`, scored as they come

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
