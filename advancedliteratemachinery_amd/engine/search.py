"""Page search on records: where a phrase stands on a read page, which words carry it and how badly it was misread (DESIGN.md section 25;
utils/page_search.py holds the definition, csrc/page_search.hip the kernel)."""
import numpy as np


def _per_image(queries, n_images):
    """one list of strings for all images, or one list per image -> one list per image"""
    queries = list(queries)
    if queries and all(isinstance(q, (list, tuple)) for q in queries):
        if len(queries) != n_images:
            raise ValueError('queries holds %d lists for %d images' % (len(queries), n_images))
        return [list(q) for q in queries]
    return [queries] * n_images


def _box(records):
    pts = [p for r in records for p in r['polys']]
    if not pts:
        return None
    xs, ys = [float(p[0]) for p in pts], [float(p[1]) for p in pts]
    return (min(xs), min(ys), max(xs), max(ys))


def find_text(records, queries, field='rec', max_dist=None, max_ratio=0.2, sep=' ', normalise=str.casefold, max_hits=16, searcher=None,
              device=None):
    """records: per image the list of record dicts any text-spotting entry point returns, IN THE ORDER TO BE READ (pass
    reading_order=True upstream; this function does not reorder).  queries: a list of strings for all images, or one list per image.
    Every image becomes one text (utils.page_search.page_index: the words' texts under `field`, normalised per word and joined by
    `sep`), every query is normalised the same way (normalise_query) and gets the tolerance k = tolerance(len, max_dist, max_ratio).
    searcher: a utils.page_search.PageSearcher, or anything with its `run` (HostSearcher: the specification); default: one on `device`
    (default 'cuda').  All images and queries go through ONE searcher.run.
    -> per image a list with one dict per query: query (as given), normalised, k, best (the least distance of the query against any
    stretch of the text; None when nothing beats the empty match), n_hits (all hits, as the definition counts them), dropped, hits.
    A hit is dict(dist, chars=(start, end) in the page's text, text = that stretch, words=(first, last) = the records that carry it --
    first is the first word with word_start + word_len > start, last the last word with word_start < end --, records = those records,
    box = (x0, y0, x1, y1), the union bounding box of their `polys` in pixels).  At most max_hits hits per query are kept, in ascending
    end; a hit that touches no word (first > last: it lies in a separator) is dropped and counted in `dropped`."""
    from ..utils import page_search as PS
    records = [list(recs) for recs in records]
    for b, recs in enumerate(records):
        for r in recs:
            if not isinstance(r, dict) or 'polys' not in r:
                raise ValueError('image %d: find_text needs text-spotting records (dicts with `polys`)' % b)
    lists = _per_image(queries, len(records))
    pages = [PS.page_index(recs, field, sep, normalise) for recs in records]
    table, k, jobs = {}, [], []
    for b, qs in enumerate(lists):
        for q in qs:
            s = PS.normalise_query(q, sep, normalise)
            if s not in table:
                table[s] = len(table)
                k.append(PS.tolerance(len(s), max_dist, max_ratio))
            jobs.append((b, table[s]))
    out = [[] for _ in records]
    if not jobs:
        return out
    pool, page_off, page_len, query_off, query_len, sigma = PS.encode_search([p[0] for p in pages], list(table))
    if searcher is None:
        searcher = PS.PageSearcher('cuda' if device is None else device)
    res = searcher.run(pool, page_off, page_len, query_off, query_len, np.asarray(jobs, dtype=np.int32), np.asarray(k, dtype=np.int32), int(max_hits),
                       sigma=sigma)
    names = list(table)
    at = 0
    for b, qs in enumerate(lists):
        text, w_start, w_len = pages[b]
        w_end = w_start + w_len
        for q in qs:
            dist, end = (int(v) for v in res['best'][at])
            hits, dropped = [], 0
            for e, d, s in res['hits'][at].tolist():
                if e < 0:
                    break
                first = int(np.searchsorted(w_end, s, side='right'))           # the first word with word_start + word_len > start
                last = int(np.searchsorted(w_start, e, side='left')) - 1      # the last word with word_start < end
                if first > last:
                    dropped += 1
                    continue
                carried = records[b][first:last + 1]
                hits.append(dict(dist=d, chars=(s, e), text=text[s:e], words=(first, last), records=carried, box=_box(carried)))
            out[b].append(dict(query=q, normalised=names[jobs[at][1]], k=k[jobs[at][1]], best=None if end == 0 else dist, n_hits=int(res['n_hits'][at]),
                               dropped=dropped, hits=hits))
            at += 1
    return out
