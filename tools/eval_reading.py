"""Score the page text of a checkpoint, or of a results file, against ground-truth page texts by the normalised edit distance
(engine/evaluate.py: score_page_text, sweep_reading, evaluate_reading).

  python tools/eval_reading.py --results FILE --gt FILE [--settings JSON] [--text_key rec|lex] [--case_sensitive] [--bins N]    (no model)
  python tools/eval_reading.py --resume CKPT --images DIR --gt FILE [--settings JSON] [--eval_batch 8]
        [stage options: --ragged --grid NX,NY --suppress 0.5 --reading_order --blocks --tiles NX,NY --tile_size S]
        [the model's own flags, as the reference's parser takes them]

--gt FILE       a JSON object {"images": [{"file_name": ..., "text": STRING or [WORD, ...], "height": H, "width": W}, ...]}: the page's
                text in reading order (blanks and newlines do not count).  height and width are needed with --results --settings only.
--results FILE  a results JSON as engine.inference.validate writes it (a flat list of records whose image_id is the file name): the
                records are grouped by image_id, kept in the file's order, and scored without a model.
--settings JSON a JSON list, inline or a file: each entry null ("as given") or an object with keys among line_gap, line_back,
                line_offset, blocks, block_gap_x, block_gap_y, block_depth.  The records are re-ordered under every entry
                (utils/reading.py: order_records) and all pages x settings are scored in one device call; `best` names the winner.
Prints ONE JSON object.  The score is the reference's 1 - edit_distance / max(len) per page, averaged over pages (`mean`); `micro` pools
the characters of all pages."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGE_EXT = ('.jpg', '.jpeg', '.png', '.bmp', '.tif', '.tiff', '.webp')


def pair(spec):
    return None if spec is None else tuple(int(v) for v in spec.split(','))


def load_image(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))


def load_settings(spec):
    if spec is None:
        return None
    if os.path.exists(spec):
        with open(spec) as f:
            return json.load(f)
    return json.loads(spec)


def summary(res):
    return dict(mean=res['mean'], micro=res['micro'], dist=np.asarray(res['dist']).tolist(), len_pred=np.asarray(res['len_pred']).tolist(),
                len_gt=np.asarray(res['len_gt']).tolist(), score=np.asarray(res['score']).tolist())


def report(res, settings, extra):
    if settings is None:
        doc = dict(extra, **summary(res))
    else:
        doc = dict(extra, settings=[dict(setting=st, **summary(s)) for st, s in zip(settings, res['settings'])], best=res['best'],
                   best_setting=settings[res['best']], best_mean=res['settings'][res['best']]['mean'])
    print(json.dumps(doc))
    return doc


def main(argv=None, scorer=None, reader=None):
    """scorer / reader: anything with PageTextScorer's `run` / ReadingOrder's __call__, in place of the device stages (the host tests
    pass utils.page_text.HostPageScorer and a reader over the numpy specification)"""
    from advancedliteratemachinery_amd.engine import evaluate as EV
    from advancedliteratemachinery_amd.utils.parser import DefaultParser
    p = DefaultParser()
    for flag, kw in (('--images', dict(type=str)), ('--gt', dict(type=str, required=True)), ('--results', dict(type=str)), ('--settings', dict(type=str)),
                     ('--text_key', dict(type=str, default='rec')), ('--case_sensitive', dict(action='store_true')), ('--bins', dict(type=int)),
                     ('--eval_batch', dict(type=int, default=8)), ('--ragged', dict(action='store_true')), ('--grid', dict(type=str)),
                     ('--suppress', dict(type=float)), ('--reading_order', dict(action='store_true')), ('--blocks', dict(action='store_true')),
                     ('--tiles', dict(type=str)), ('--tile_size', dict(type=int))):
        p.add_argument(flag, **kw)
    a = p.parse_args(argv)
    with open(a.gt, encoding='utf-8') as f:
        pages = json.load(f)['images']
    names = [im['file_name'] for im in pages]
    truth = [im['text'] for im in pages]
    settings = load_settings(a.settings)
    skw = dict(text_key=a.text_key, normalise=None if a.case_sensitive else str.casefold, scorer=scorer)
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
        records = [by_name[n] for n in names]
        if settings is None:
            res = EV.score_page_text(records, truth, device='cuda', **skw)
        else:
            if any('height' not in im or 'width' not in im for im in pages):
                raise SystemExit('--settings re-orders the records by their polygons: every image of --gt needs height and width')
            res = EV.sweep_reading(records, [(im['height'], im['width']) for im in pages], bins, truth, settings, reader=reader,
                                   device='cuda', **skw)
        return report(res, settings, dict(results=a.results, images=len(names), records=len(flat), bins=bins))
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
        stage['suppress'] = a.suppress
    if a.reading_order:
        stage.update(reading_order=True, blocks=a.blocks)
    if a.tiles or a.tile_size:
        stage.update(tiles=pair(a.tiles), tile_size=a.tile_size)
    imgs = [load_image(os.path.join(a.images, n)) for n in names]
    res = EV.evaluate_reading(model, imgs, truth, a, batch=a.eval_batch, settings=settings, bins=bins, file_names=names, reader=reader, **dict(stage, **skw))
    return report(res, settings, dict(resume=a.resume, images=len(names), records=sum(len(r) for r in res['records']), bins=bins, stage=stage))


if __name__ == '__main__':
    main()
