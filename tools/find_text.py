"""Find phrases in the text of read pages: where each stands, which words carry it and how badly it was misread (DESIGN.md section 25;
engine/search.py: find_text).

  python tools/find_text.py --results FILE --queries FILE [--field rec] [--max-ratio 0.2] [--max-dist N] [--max-hits 16] [--host]

--results FILE  a results JSON as engine.inference.validate writes it (a flat list of records whose image_id names the image): the
                records are grouped by image_id, kept in the file's order -- write it with reading_order=True, the tool does not reorder.
--queries FILE  a JSON list of phrases, searched on every image, or a JSON object {image_id: [phrase, ...]} with one list per image.
--max-ratio R   a query of m characters tolerates (1000 R * m) // 1000 edits, --max-dist N caps that, and m - 1 caps both.
--host          utils.page_search.HostSearcher (the numpy definition) in place of the device stage: no GPU is needed.
Prints ONE JSON object: per image and query the best distance, the number of hits and the kept hits with their characters, words and
box; the records of a hit are named by their indices (`words`), not repeated."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def group_records(flat):
    """a results list -> (image ids in the order of first appearance, the records of each in the file's order)"""
    by_name = {}
    for r in flat:
        by_name.setdefault(str(r['image_id']), []).append(r)
    return list(by_name), list(by_name.values())


def main(argv=None, searcher=None):
    """searcher: anything with PageSearcher's `run`, in place of the device stage"""
    from advancedliteratemachinery_amd.engine.search import find_text
    from advancedliteratemachinery_amd.utils import page_search as PS
    p = argparse.ArgumentParser()
    p.add_argument('--results', required=True)
    p.add_argument('--queries', required=True)
    p.add_argument('--field', default='rec')
    p.add_argument('--max-ratio', type=float, default=0.2)
    p.add_argument('--max-dist', type=int)
    p.add_argument('--max-hits', type=int, default=16)
    p.add_argument('--host', action='store_true')
    a = p.parse_args(argv)
    with open(a.results, encoding='utf-8') as f:
        names, records = group_records(json.load(f))
    with open(a.queries, encoding='utf-8') as f:
        queries = json.load(f)
    if isinstance(queries, dict):
        stems = {os.path.splitext(os.path.basename(n))[0]: n for n in names}
        per = {n: [] for n in names}
        for key, qs in queries.items():
            name = key if key in per else stems.get(os.path.splitext(os.path.basename(str(key)))[0])
            if name is None:
                raise SystemExit('queries name image %r, which the results do not list' % (key,))
            per[name] = list(qs)
        queries = [per[n] for n in names]
    if searcher is None and a.host:
        searcher = PS.HostSearcher()
    found = find_text(records, queries, field=a.field, max_dist=a.max_dist, max_ratio=a.max_ratio, max_hits=a.max_hits, searcher=searcher, device='cuda')
    images = []
    for name, per_query in zip(names, found):
        for d in per_query:
            for h in d['hits']:
                del h['records']
        images.append(dict(image_id=name, queries=per_query))
    doc = dict(results=a.results, images=images, records=sum(len(r) for r in records), field=a.field, max_ratio=a.max_ratio, max_dist=a.max_dist,
               max_hits=a.max_hits, searcher='host' if a.host else 'device')
    print(json.dumps(doc))
    return doc


if __name__ == '__main__':
    main()
