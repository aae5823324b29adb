"""Find expressions -- amounts with thousands groups, currencies, dates with month names, ids of unknown length -- in the text of read pages:
where each stands and which words carry it (engine/search.py: find_regex).

  python tools/find_regex.py --results FILE --expressions FILE [--field rec] [--max-hits 16] [--max-dist N] [--max-ratio R] [--host]

--results FILE      a results JSON as engine.inference.validate writes it (a flat list of records whose image_id names the image): the
                    records are grouped by image_id, kept in the file's order -- write it with reading_order=True, the tool does not reorder.
--expressions FILE  a JSON list of expressions, searched on every image, or a JSON object {image_id: [expression, ...]} with one list per
                    image.  An expression is a string (utils.page_regex.parse_regex: find_pattern's atoms with groups, `|` and the
                    quantifiers ? * + {n} {a,b} {a,}) or a {"name": ..., "expression": ...} object.  It is matched exactly.
--max-dist N, --max-ratio R   search WITH ERRORS: an expression whose shortest word holds min_len characters gets
                    the tolerance min(min_len - 1, 4, N, R * min_len), a bound that is not given left out; every expression object of the
                    output gains `k` and a hit's `dist` is its distance.  Without both the search is exact, as before.
--host              utils.page_regex.HostRegexSearcher, or HostFuzzyRegexSearcher with errors (the numpy definitions) in place of the
                    device stage: no GPU is needed.
Prints ONE JSON object: per image and expression whether it stands on the page, the number of hits and the kept hits with their characters,
words and box; the records of a hit are named by their indices (`words`), not repeated.  No model is needed."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from find_text import group_records  # noqa: E402


def _expression(p):
    """a JSON expression -> a string or a (name, string) tuple"""
    if isinstance(p, dict):
        if set(p) != {'name', 'expression'}:
            raise SystemExit('an expression object holds `name` and `expression`, got %r' % (p,))
        return (str(p['name']), p['expression'])
    return p


def main(argv=None, searcher=None):
    """searcher: anything with RegexSearcher's `run` (with --max-dist or --max-ratio: FuzzyRegexSearcher's), in place of the device stage"""
    from advancedliteratemachinery_amd.engine.search import find_regex
    from advancedliteratemachinery_amd.utils import page_regex as PR
    p = argparse.ArgumentParser()
    p.add_argument('--results', required=True)
    p.add_argument('--expressions', required=True)
    p.add_argument('--field', default='rec')
    p.add_argument('--max-hits', type=int, default=16)
    p.add_argument('--max-dist', type=int, default=None)
    p.add_argument('--max-ratio', type=float, default=0.0)
    p.add_argument('--host', action='store_true')
    a = p.parse_args(argv)
    fuzzy = a.max_dist is not None or a.max_ratio != 0.0
    with open(a.results, encoding='utf-8') as f:
        names, records = group_records(json.load(f))
    with open(a.expressions, encoding='utf-8') as f:
        expressions = json.load(f)
    if isinstance(expressions, dict):
        stems = {os.path.splitext(os.path.basename(n))[0]: n for n in names}
        per = {n: [] for n in names}
        for key, ps in expressions.items():
            name = key if key in per else stems.get(os.path.splitext(os.path.basename(str(key)))[0])
            if name is None:
                raise SystemExit('expressions name image %r, which the results do not list' % (key,))
            per[name] = [_expression(q) for q in ps]
        expressions = [per[n] for n in names]
    else:
        expressions = [[_expression(q) for q in expressions] for _ in names]
    if searcher is None and a.host:
        searcher = PR.HostFuzzyRegexSearcher() if fuzzy else PR.HostRegexSearcher()
    found = find_regex(records, expressions, field=a.field, max_hits=a.max_hits, searcher=searcher, device='cuda', max_dist=a.max_dist, max_ratio=a.max_ratio)
    images = []
    for name, per_expression in zip(names, found):
        for d in per_expression:
            for h in d['hits']:
                del h['records']
        images.append(dict(image_id=name, expressions=per_expression))
    doc = dict(results=a.results, images=images, records=sum(len(r) for r in records), field=a.field, max_hits=a.max_hits,
               searcher='host' if a.host else 'device')
    if fuzzy:
        doc.update(max_dist=a.max_dist, max_ratio=a.max_ratio)
    print(json.dumps(doc))
    return doc


if __name__ == '__main__':
    main()
