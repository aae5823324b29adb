"""Find shapes -- dates, amounts, ids -- in the text of read pages: where each stands, which words carry it and how badly it was misread
(engine/search.py: find_pattern).

  python tools/find_pattern.py --results FILE --patterns FILE [--field rec] [--max-ratio 0] [--max-dist N] [--rep-max N] [--max-hits 16] [--host]

--results FILE   a results JSON as engine.inference.validate writes it (a flat list of records whose image_id names the image): the
                 records are grouped by image_id, kept in the file's order -- write it with reading_order=True, the tool does not reorder.
--patterns FILE  a JSON list of patterns, searched on every image, or a JSON object {image_id: [pattern, ...]} with one list per image.
                 A pattern is a string (utils.page_pattern.parse_pattern: classes with ?, {n}, {a,b}) or a {"name": ..., "pattern": ...}
                 object.
--max-ratio R    a pattern with Mand mandatory positions tolerates (1000 R * Mand) // 1000 errors; --max-dist N caps that, and Mand - 1
                 and 8 cap both.  The default is 0: exact shapes.
--rep-max N      what `*` and `+` repeat to at the most; without it they are refused.
--host           utils.page_pattern.HostPatternSearcher (the numpy definition) in place of the device stage: no GPU is needed.
Prints ONE JSON object: per image and pattern the best distance, the number of hits and the kept hits with their characters, words and
box; the records of a hit are named by their indices (`words`), not repeated.  No model is needed."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from find_text import group_records  # noqa: E402


def _pattern(p):
    """a JSON pattern -> a string or a (name, string) tuple"""
    if isinstance(p, dict):
        if set(p) != {'name', 'pattern'}:
            raise SystemExit('a pattern object holds `name` and `pattern`, got %r' % (p,))
        return (str(p['name']), p['pattern'])
    return p


def main(argv=None, searcher=None):
    """searcher: anything with PatternSearcher's `run`, in place of the device stage"""
    from advancedliteratemachinery_amd.engine.search import find_pattern
    from advancedliteratemachinery_amd.utils import page_pattern as PP
    p = argparse.ArgumentParser()
    p.add_argument('--results', required=True)
    p.add_argument('--patterns', required=True)
    p.add_argument('--field', default='rec')
    p.add_argument('--max-ratio', type=float, default=0.0)
    p.add_argument('--max-dist', type=int)
    p.add_argument('--rep-max', type=int)
    p.add_argument('--max-hits', type=int, default=16)
    p.add_argument('--host', action='store_true')
    a = p.parse_args(argv)
    with open(a.results, encoding='utf-8') as f:
        names, records = group_records(json.load(f))
    with open(a.patterns, encoding='utf-8') as f:
        patterns = json.load(f)
    if isinstance(patterns, dict):
        stems = {os.path.splitext(os.path.basename(n))[0]: n for n in names}
        per = {n: [] for n in names}
        for key, ps in patterns.items():
            name = key if key in per else stems.get(os.path.splitext(os.path.basename(str(key)))[0])
            if name is None:
                raise SystemExit('patterns name image %r, which the results do not list' % (key,))
            per[name] = [_pattern(q) for q in ps]
        patterns = [per[n] for n in names]
    else:
        patterns = [[_pattern(q) for q in patterns] for _ in names]
    if searcher is None and a.host:
        searcher = PP.HostPatternSearcher()
    found = find_pattern(records, patterns, field=a.field, max_dist=a.max_dist, max_ratio=a.max_ratio, rep_max=a.rep_max, max_hits=a.max_hits,
                         searcher=searcher, device='cuda')
    images = []
    for name, per_pattern in zip(names, found):
        for d in per_pattern:
            for h in d['hits']:
                del h['records']
        images.append(dict(image_id=name, patterns=per_pattern))
    doc = dict(results=a.results, images=images, records=sum(len(r) for r in records), field=a.field, max_ratio=a.max_ratio, max_dist=a.max_dist,
               rep_max=a.rep_max, max_hits=a.max_hits, searcher='host' if a.host else 'device')
    print(json.dumps(doc))
    return doc


if __name__ == '__main__':
    main()
