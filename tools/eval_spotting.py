"""Score a text-spotting checkpoint, or a results file, against ground truth (engine/evaluate.py).

  python tools/eval_spotting.py --resume CKPT --images DIR --anno FILE [--format coco|icdar] [--thresholds lo:hi:step]
        [--iou 0.5] [--dc_overlap 0.5] [--min_len 0] [--text_key rec|lex] [--case_sensitive] [--bins N] [--eval_batch 8]
        [stage options: --ragged --grid NX,NY --suppress 0.5 --suppress_measure iou --suppress_order first --reading_order --blocks
         --tiles NX,NY --tile_size S --lexicon FILE --lexicon_max_dist D] [the model's own flags, as the reference's parser takes them]
  python tools/eval_spotting.py --results FILE --anno FILE [--format coco|icdar] [--images DIR] ...          (no model)

--format coco   --anno is the reference's annotation JSON (COCO layout with bezier_pts, rec, iscrowd); image sizes come from it.
--format icdar  --anno is a folder of gt_<stem>.txt / <stem>.txt files (x1,y1,...,xk,yk,transcription; ### = don't-care), one per
                image of --images (sorted by name); --points K fixes the vertex count.  Sizes come from the image files.
--results FILE  a results JSON as engine.inference.validate writes it (a flat list of records whose image_id is the file name): the
                records are grouped by image_id and scored without a model.
--thresholds    lo:hi:step over the records' `score` (inclusive, at most 64 values; default 0:0 = the single threshold 0).
--lexicon FILE  one word per line, shared by all images (records gain `lex`; score it with --text_key lex).
Prints ONE JSON object: per threshold precision / recall / h-mean for detection and end-to-end, the best thresholds, the totals.
Agreement with the official ICDAR / Total-Text scripts has not been checked."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGE_EXT = ('.jpg', '.jpeg', '.png', '.bmp', '.tif', '.tiff', '.webp')


def parse_thresholds(spec):
    lo, hi, step = (float(v) for v in (spec.split(':') + ['0', '0'])[:3]) if ':' in spec else (float(spec), float(spec), 0.0)
    if step <= 0 or hi <= lo:
        return [lo]
    n = int(np.floor((hi - lo) / step + 1e-9)) + 1
    return [round(lo + k * step, 10) for k in range(n)]


def pair(spec):
    return None if spec is None else tuple(int(v) for v in spec.split(','))


def load_image(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))


def image_size(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.height, im.width


def report(res, extra):
    doc = dict(extra, thresholds=res['thresholds'], total=np.asarray(res['total']).tolist(), det=res['det'], e2e=res['e2e'], best=res['best'],
               best_threshold=dict(det=res['thresholds'][res['best']['det']], e2e=res['thresholds'][res['best']['e2e']]),
               best_hmean=dict(det=res['det']['hmean'][res['best']['det']], e2e=res['e2e']['hmean'][res['best']['e2e']]),
               note='agreement with the official evaluation scripts has not been checked')
    print(json.dumps(doc))
    return doc


def main(argv=None, scorer=None):
    """scorer: anything with SpottingScorer's `run`, in place of the device stage (the host tests pass utils.scoring.HostScorer)"""
    from advancedliteratemachinery_amd.engine import evaluate as EV
    from advancedliteratemachinery_amd.utils import ground_truth as GT
    from advancedliteratemachinery_amd.utils.parser import DefaultParser
    p = DefaultParser()
    for flag, kw in (('--images', dict(type=str)), ('--anno', dict(type=str, required=True)), ('--format', dict(type=str, default='coco', choices=['coco', 'icdar'])),
                     ('--points', dict(type=int)), ('--results', dict(type=str)), ('--thresholds', dict(type=str, default='0:0')),
                     ('--iou', dict(type=float, default=0.5)), ('--dc_overlap', dict(type=float, default=0.5)), ('--min_len', dict(type=int, default=0)),
                     ('--text_key', dict(type=str, default='rec')), ('--case_sensitive', dict(action='store_true')), ('--bins', dict(type=int)),
                     ('--eval_batch', dict(type=int, default=8)), ('--ragged', dict(action='store_true')), ('--grid', dict(type=str)),
                     ('--suppress', dict(type=float)), ('--suppress_measure', dict(type=str, default='iou')),
                     ('--suppress_order', dict(type=str, default='first')), ('--reading_order', dict(action='store_true')),
                     ('--blocks', dict(action='store_true')), ('--tiles', dict(type=str)), ('--tile_size', dict(type=int)),
                     ('--lexicon', dict(type=str)), ('--lexicon_max_dist', dict(type=int))):
        p.add_argument(flag, **kw)
    a = p.parse_args(argv)
    # ground truth, image names and sizes
    if a.format == 'coco':
        images, truth = GT.load_coco_bezier(a.anno, a)
        names = [im['file_name'] for im in images]
        sizes = [(im['height'], im['width']) for im in images]
    else:
        if not a.images:
            raise SystemExit('--format icdar reads the image names and sizes from --images')
        names = sorted(f for f in os.listdir(a.images) if f.lower().endswith(IMAGE_EXT))
        truth = GT.load_icdar_dir(a.anno, names, a.points)
        sizes = [image_size(os.path.join(a.images, f)) for f in names]
    skw = dict(thresholds=parse_thresholds(a.thresholds), iou=a.iou, dc_overlap=a.dc_overlap, min_len=a.min_len, text_key=a.text_key,
               normalise=None if a.case_sensitive else str.casefold, scorer=scorer)
    bins = a.bins if a.bins else a.num_bins
    if a.results:
        with open(a.results) as f:
            flat = json.load(f)
        by_name = {n: [] for n in names}
        stems = {os.path.splitext(os.path.basename(n))[0]: n for n in names}
        for r in flat:
            key = r['image_id'] if r['image_id'] in by_name else stems.get(os.path.splitext(os.path.basename(str(r['image_id'])))[0])
            if key is None:
                raise SystemExit('results name image %r, which the ground truth does not list' % (r['image_id'],))
            by_name[key].append(r)
        res = EV.score_records([by_name[n] for n in names], truth, sizes, bins, device='cuda', **skw)
        return report(res, dict(results=a.results, images=len(names), records=len(flat), bins=bins))
    if not a.resume or not a.images:
        raise SystemExit('pass --resume CKPT and --images DIR, or --results FILE')
    from advancedliteratemachinery_amd.model import build_model
    from advancedliteratemachinery_amd.utils.checkpointer import Checkpointer
    model = build_model(a)
    Checkpointer(allow_unsafe_pickle=a.allow_unsafe_pickle).load(a.resume, model, a)
    model.eval()
    stage = dict(ragged=a.ragged)
    if a.grid:
        stage['grid'] = pair(a.grid)
    if a.suppress is not None:
        stage.update(suppress=a.suppress, suppress_measure=a.suppress_measure, suppress_order=a.suppress_order)
    if a.reading_order:
        stage.update(reading_order=True, blocks=a.blocks)
    if a.tiles or a.tile_size:
        stage.update(tiles=pair(a.tiles), tile_size=a.tile_size)
    if a.lexicon:
        with open(a.lexicon, encoding='utf-8') as f:
            stage.update(lexicon=[w.strip() for w in f if w.strip()], lexicon_max_dist=a.lexicon_max_dist)
    imgs = [load_image(os.path.join(a.images, n)) for n in names]
    res = EV.evaluate_spotting(model, imgs, truth, a, batch=a.eval_batch, bins=bins, file_names=names, **dict(stage, **skw))
    return report(res, dict(resume=a.resume, images=len(names), records=sum(len(r) for r in res['records']), bins=bins, stage={
        k: v for k, v in stage.items() if k != 'lexicon'}))


if __name__ == '__main__':
    main()
