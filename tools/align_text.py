"""Align the page text of a results file with ground-truth page texts: S / D / I counts, CER, the most frequent confusions, word
precision and recall, and per ground-truth word its status and the box of the records that carry it (DESIGN.md section 26;
engine/evaluate.py: align_page_text).  No model is needed.

  python tools/align_text.py --results FILE --gt FILE [--text-key rec|lex|mgp_text|mgp_lex] [--top 20] [--case-sensitive] [--host]

--gt FILE       a JSON object {"images": [{"file_name": ..., "text": STRING or [WORD, ...]}, ...]}, as tools/eval_reading.py reads it
--results FILE  a results JSON as engine.inference.validate writes it (a flat list of records whose image_id is the file name): the
                records are grouped by image_id and kept in the file's order
--host          align with utils.page_align.HostPageAligner (the numpy definition) instead of the device stage
Prints ONE JSON object: the totals, the confusions, and per image its counts and its ground-truth words (text, status, span, records,
box).  The character maps are left out of the print; call align_page_text for them."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def group_records(flat, names):
    by_name = {n: [] for n in names}
    stems = {os.path.splitext(os.path.basename(n))[0]: n for n in names}
    for r in flat:
        key = r['image_id'] if r['image_id'] in by_name else stems.get(os.path.splitext(os.path.basename(str(r['image_id'])))[0])
        if key is None:
            raise SystemExit('results name image %r, which the ground truth does not list' % (r['image_id'],))
        by_name[key].append(r)
    return [by_name[n] for n in names]


def main(argv=None, aligner=None):
    """aligner: anything with PageAligner's `run`, in place of the device stage"""
    from advancedliteratemachinery_amd.engine import evaluate as EV
    from advancedliteratemachinery_amd.utils import page_align as PA
    p = argparse.ArgumentParser()
    p.add_argument('--results', required=True)
    p.add_argument('--gt', required=True)
    p.add_argument('--text-key', '--text_key', dest='text_key', default='rec')
    p.add_argument('--top', type=int, default=20)
    p.add_argument('--case-sensitive', '--case_sensitive', dest='case_sensitive', action='store_true')
    p.add_argument('--host', action='store_true')
    a = p.parse_args(argv)
    with open(a.gt, encoding='utf-8') as f:
        images = json.load(f)['images']
    with open(a.results) as f:
        flat = json.load(f)
    names = [im['file_name'] for im in images]
    records = group_records(flat, names)
    if aligner is None and a.host:
        aligner = PA.HostPageAligner()
    res = EV.align_page_text(records, [im['text'] for im in images], text_key=a.text_key, normalise=None if a.case_sensitive else str.casefold, top=a.top,
                             aligner=aligner, device='cuda')
    ints = lambda v: np.asarray(v).tolist()                                 # noqa: E731
    doc = dict(results=a.results, images=len(names), records=len(flat), host=bool(a.host),
               mean=res['mean'], micro=res['micro'], cer_micro=res['cer_micro'], word_precision=res['word_precision'], word_recall=res['word_recall'],
               match=int(res['match'].sum()), sub=int(res['sub'].sum()), ins=int(res['ins'].sum()), dele=int(res['dele'].sum()),
               confusions=dict(sub=[[k[0], k[1], n] for k, n in res['confusions']['sub']], ins=[[k, n] for k, n in res['confusions']['ins']],
                               dele=[[k, n] for k, n in res['confusions']['dele']]),
               pages=[dict(file_name=n, dist=int(res['dist'][g]), len_pred=int(res['len_pred'][g]), len_gt=int(res['len_gt'][g]), match=int(res['match'][g]),
                           sub=int(res['sub'][g]), ins=int(res['ins'][g]), dele=int(res['dele'][g]), cer=res['cer'][g], score=float(res['score'][g]),
                           words=[dict(status=w['status'], chars=ints(w['chars']), span=ints(w['span'])) for w in res['pages'][g]['words']],
                           gt_words=[dict(text=w['text'], status=w['status'], chars=ints(w['chars']), span=ints(w['span']),
                                          records=None if w['records'] is None else ints(w['records']), box=None if w['box'] is None else list(w['box']))
                                     for w in res['pages'][g]['gt_words']])
                      for g, n in enumerate(names)])
    print(json.dumps(doc))
    return doc


if __name__ == '__main__':
    main()
