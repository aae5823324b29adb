"""Page search on records: where a phrase (find_text: DESIGN.md section 25, utils/page_search.py, csrc/page_search.hip) or a shape such as a
date, an amount or an id (find_pattern: DESIGN.md section 29, utils/page_pattern.py, csrc/page_pattern.hip; find_regex: the same with
groups, alternation and real loops, exactly: DESIGN.md section 30, utils/page_regex.py, csrc/page_regex.hip; with max_dist or max_ratio
within up to 4 errors: section 31, the same unit) stands on a read page, which words carry it and how badly it was misread."""
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


def _carried(recs, text, w_start, w_end, rows):
    """the (end, dist, start) rows of one job -> (the hits that touch a word, as dicts with the words that carry them; how many touch
    none).  first is the first word with word_start + word_len > start, last the last word with word_start < end."""
    hits, dropped = [], 0
    for e, d, s in np.asarray(rows).tolist():
        if e < 0:
            break
        first = int(np.searchsorted(w_end, s, side='right'))               # the first word with word_start + word_len > start
        last = int(np.searchsorted(w_start, e, side='left')) - 1          # the last word with word_start < end
        if first > last:
            dropped += 1
            continue
        carried = recs[first:last + 1]
        hits.append(dict(dist=d, chars=(s, e), text=text[s:e], words=(first, last), records=carried, box=_box(carried)))
    return hits, dropped


def _shape_jobs(records, shapes, caller, plural, a_shape, field, sep, normalise, parse):
    """what find_pattern and find_regex share: the record check, one list of shapes per image (a tuple is a (name, string) pair, so
    per-image lists are LISTS), the (name, string) unpacking, and the table of distinct strings, each parsed once by `parse` in the order
    they first occur -> (records as lists, pages = page_index per image, parsed, jobs = [(image, shape)], named = [(name, string)] per
    job)"""
    from ..utils.page_search import page_index
    records = [list(recs) for recs in records]
    for b, recs in enumerate(records):
        for r in recs:
            if not isinstance(r, dict) or 'polys' not in r:
                raise ValueError('image %d: %s needs text-spotting records (dicts with `polys`)' % (b, caller))
    shapes = list(shapes)
    if shapes and all(isinstance(p, list) for p in shapes):
        if len(shapes) != len(records):
            raise ValueError('%s holds %d lists for %d images' % (plural, len(shapes), len(records)))
        lists = [list(p) for p in shapes]
    else:
        lists = [shapes] * len(records)
    pages = [page_index(recs, field, sep, normalise) for recs in records]
    table, parsed, jobs, named = {}, [], [], []
    for b, ps in enumerate(lists):
        for p in ps:
            name, src = (None, p) if isinstance(p, str) else p if isinstance(p, tuple) and len(p) == 2 else (None, None)
            if not isinstance(src, str) or not (name is None or isinstance(name, str)):
                raise ValueError('%s is a string or a (name, string) pair, got %r' % (a_shape, p))
            if src not in table:
                table[src] = len(table)
                parsed.append(parse(src))
            jobs.append((b, table[src]))
            named.append((name, src))
    return records, pages, parsed, jobs, named


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
            hits, dropped = _carried(records[b], text, w_start, w_end, res['hits'][at])
            out[b].append(dict(query=q, normalised=names[jobs[at][1]], k=k[jobs[at][1]], best=None if end == 0 else dist, n_hits=int(res['n_hits'][at]),
                               dropped=dropped, hits=hits))
            at += 1
    return out


def find_pattern(records, patterns, field='rec', max_dist=None, max_ratio=0.0, sep=' ', normalise=None, rep_max=None, max_hits=16, searcher=None,
                 device=None):
    """records: as find_text takes them, IN THE ORDER TO BE READ.  patterns: a list for all images, or one list (not tuple) per image; a
    pattern is a string in the syntax of utils.page_pattern.parse_pattern (character classes with ?, {n} and {a,b}; `*` and `+` repeat up to
    rep_max and are refused without it) or a (name, string) tuple.  Every image becomes one text (page_index); `normalise` is applied to
    the page words ONLY, never to a pattern, and defaults to None because patterns are case-sensitive shapes.  A pattern with Mand
    mandatory positions gets the tolerance k = utils.page_pattern.tolerance(Mand, max_dist, max_ratio); max_ratio defaults to 0, exact
    shapes, and errors are opt-in.  Both defaults are choices that no data set has tested.
    searcher: a utils.page_pattern.PatternSearcher, or anything with its `run` (HostPatternSearcher: the specification); default: one on
    `device` (default 'cuda').  All images and patterns go through ONE searcher.run.
    -> per image a list with one dict per pattern: pattern (the string), name (None for a bare string), P, k, best (the least distance of
    the pattern against any stretch of the text; None when nothing is within k), n_hits, dropped, hits.  A hit is find_text's dict
    (dist, chars, text, words, records, box), with one difference: chars starts at the LEAST start that attains dist, the longest match
    (`\\d{1,4}` in `12345` is `2345`, not `5`), where find_text reports the shortest.  A hit that touches no word is dropped and counted."""
    from ..utils import page_pattern as PP
    k = []

    def parse(src):
        pattern = PP.parse_pattern(src, rep_max)
        k.append(PP.tolerance(pattern.Mand, max_dist, max_ratio))
        return pattern
    records, pages, parsed, jobs, named = _shape_jobs(records, patterns, 'find_pattern', 'patterns', 'a pattern', field, sep, normalise, parse)
    out = [[] for _ in records]
    if not jobs:
        return out
    pool, page_off, page_len, masks, opt, pat_len, _ = PP.encode_patterns([p[0] for p in pages], parsed)
    if searcher is None:
        searcher = PP.PatternSearcher('cuda' if device is None else device)
    res = searcher.run(pool, page_off, page_len, masks, opt, pat_len, np.asarray(jobs, dtype=np.int32), np.asarray(k, dtype=np.int32), int(max_hits))
    for at, ((b, q), (name, src)) in enumerate(zip(jobs, named)):
        text, w_start, w_len = pages[b]
        dist, end = (int(v) for v in res['best'][at])
        hits, dropped = _carried(records[b], text, w_start, w_start + w_len, res['hits'][at])
        out[b].append(dict(pattern=src, name=name, P=parsed[q].P, k=k[q], best=None if end == 0 else dist, n_hits=int(res['n_hits'][at]), dropped=dropped,
                           hits=hits))
    return out


def find_regex(records, expressions, field='rec', sep=' ', normalise=None, max_hits=16, searcher=None, device=None, max_dist=None, max_ratio=0.0):
    """records: as find_text takes them, IN THE ORDER TO BE READ.  expressions: a list for all images, or one list (not tuple) per image;
    an expression is a string in the syntax of utils.page_regex.parse_regex (find_pattern's atoms with groups, `|` at any depth and the
    quantifiers ? * + {n} {a,b} {a,}; `*`, `+` and `{a,}` are real loops) or a (name, string) tuple.  Every image becomes one text
    (page_index); `normalise` is applied to the page words ONLY, never to an expression.  With the defaults (max_dist=None, max_ratio=0.0)
    an expression is matched exactly, through a RegexSearcher, and the result dicts are those described below.
    WITH ERRORS: when max_dist or max_ratio is given, an expression whose shortest word holds min_len characters gets the tolerance
    k = utils.page_regex.regex_tolerance(min_len, max_dist, max_ratio) <= min(min_len - 1, 4) (max_dist alone bounds k by max_dist,
    max_ratio alone by the ratio, both by the lesser), ALL jobs (those with k = 0 included) go
    through one utils.page_regex.FuzzyRegexSearcher.run (searcher= then takes one, or a HostFuzzyRegexSearcher), every result dict gains
    `k`, best is the least distance within k or None, and a hit's dist is its distance (`(EUR|USD) ?\\d+` finds `EUP 120` at dist 1).
    searcher: a utils.page_regex.RegexSearcher, or anything with its `run` (HostRegexSearcher: the specification); default: one on
    `device` (default 'cuda').  All images and expressions go through ONE searcher.run.
    -> per image a list with one dict per expression: pattern (the string), name (None for a bare string), P (its positions), best (0
    when the expression stands somewhere on the page, else None), n_hits, dropped, hits.  A hit is find_pattern's dict (dist = 0, chars,
    text, words, records, box): it ends at the LAST column of a run of consecutive ends and starts at the LEAST start, the longest match
    (`\\d+` in `12345 ` is `12345`).  An expression in find_pattern's subset gets the hits find_pattern gives it at k = 0.  A hit that touches
    no word is dropped and counted."""
    from ..utils import page_regex as PR
    records, pages, parsed, jobs, named = _shape_jobs(records, expressions, 'find_regex', 'expressions', 'an expression', field, sep, normalise,
                                                      PR.parse_regex)
    fuzzy = max_dist is not None or (max_ratio is not None and float(max_ratio) != 0.0)
    out = [[] for _ in records]
    if not jobs:
        return out
    pool, page_off, page_len, masks, first, last, follow, pred, pat_len, _ = PR.encode_regex([p[0] for p in pages], parsed)
    if fuzzy:
        ratio = None if max_dist is not None and not max_ratio else max_ratio  # max_dist alone: the ratio's default of 0 is no bound
        k = [PR.regex_tolerance(r.min_len, max_dist, ratio) for r in parsed]
        if searcher is None:
            searcher = PR.FuzzyRegexSearcher('cuda' if device is None else device)
        res = searcher.run(pool, page_off, page_len, masks, first, last, follow, pred, pat_len, np.asarray(jobs, dtype=np.int32), np.asarray(k, dtype=np.int32),
                           int(max_hits))
    else:
        if searcher is None:
            searcher = PR.RegexSearcher('cuda' if device is None else device)
        res = searcher.run(pool, page_off, page_len, masks, first, last, follow, pred, pat_len, np.asarray(jobs, dtype=np.int32), int(max_hits))
    for at, ((b, q), (name, src)) in enumerate(zip(jobs, named)):
        text, w_start, w_len = pages[b]
        dist, end = (int(v) for v in res['best'][at])
        hits, dropped = _carried(records[b], text, w_start, w_start + w_len, res['hits'][at])
        out[b].append(dict(pattern=src, name=name, P=parsed[q].P, best=None if end == 0 else dist, n_hits=int(res['n_hits'][at]), dropped=dropped, hits=hits))
        if fuzzy:
            out[b][-1]['k'] = k[q]
    return out
