"""Page search: fuzzy phrase matches in the text of read pages.

A page's words, in the order an entry point returned them, are one text; a query is a phrase of 1 .. 64 characters; a job is one
(page, query) pair.  The answer per job is where the phrase stands in the text and how badly it was misread: Sellers' approximate
string matching, insert / delete / substitute cost 1.  The numpy / Python functions here are the DEFINITION; csrc/page_search.hip
(omp_page_search) equals search_cpu on every integer.

Text        page_index(): the records' texts, normalised PER WORD (casefold changes lengths) and joined by `sep`, with every word's
            offset and length in the text.
Queries     normalise_query(): normalised, every whitespace run one `sep`, both ends stripped; 1 .. QUERY_MAX characters.
Codes       encode_search(): one uint8 pool for all pages and queries of a call.  The characters that occur in ANY QUERY get the dense
            codes 0 .. sigma - 1 (sigma <= 254); every other page character gets 255, and 255 equals nothing, itself included.  That
            is exact: a character no query holds can never be part of a match.  Equal strings share one pool range.
Table       D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (q_i != t_j), D[i-1][j] + 1, D[i][j-1] + 1); v_j = D[m][j], j = 0 .. n.
best        (dist, end): dist = min_j v_j, end the least j that attains it; (m, 0) when nothing beats the empty match.
A hit       an end j in 1 .. n with v_j <= k, v_j <= v_{j-1} and (j == n or v_j < v_{j+1}): the LAST column of a valley floor within
            the tolerance.  In a run such as `aa` in `aaaa` only the last occurrence is a hit.  Two hits may overlap.
n_hits      counts all hits; hits int32 [J, H, 3] holds (end, dist, start) of the first min(n_hits, H) in ascending end, the rest -1.
start       the greatest s <= end with edit_distance(q, t[s:end]) == dist (the shortest match); end - start <= m + dist.
Lengths     a page 0 .. 65535 characters, a query 1 .. 64, 0 <= k <= m - 1, 1 .. 2^20 jobs a call, 1 .. 64 hits kept per job.
"""
import numpy as np

from .page_text import LEN_MAX, NONE, SIGMA_MAX, _DeviceStage, _encode, _rows

QUERY_MAX = 64                  # characters a query (csrc/page_search.hip: PS_QUERY_MAX): one 64-bit word of Myers' column
CHUNK = 128                     # text columns per lane (csrc/page_frame.h: PG_CHUNK)
HITS_MAX = 64                   # hits kept per job at the most
JOBS_MAX = 1 << 20
SCRATCH_CAP = 1 << 28           # device scratch per chunk of jobs


# ---------------------------------------------------------------------------------------------
# text, queries, codes
# ---------------------------------------------------------------------------------------------
def page_index(records, field='rec', sep=' ', normalise=str.casefold):
    """one image's records, IN THE ORDER GIVEN -> (text, word_start int32 [n], word_len int32 [n]).  Every word's text is taken by the
    fallback rule of engine/evaluate.py: TEXT_KEYS (any other `field` is read as it is); `normalise` is applied PER WORD (None: skipped),
    so word_start and word_len are offsets in the normalised text; the words are joined by `sep`.  An empty word has length 0."""
    from ..engine.evaluate import TEXT_KEYS, _text_of
    words = []
    for r in records:
        if isinstance(r, str):
            w = r
        elif isinstance(r, dict):
            w = str(_text_of(r, field) if field in TEXT_KEYS else r[field])
        else:
            raise ValueError('page_index takes record dicts or strings, got %s' % type(r).__name__)
        words.append(normalise(w) if normalise is not None else w)
    start, at = [], 0
    for w in words:
        start.append(at)
        at += len(w) + len(sep)
    return sep.join(words), np.asarray(start, dtype=np.int32).reshape(-1), np.asarray([len(w) for w in words], dtype=np.int32).reshape(-1)


def normalise_query(q, sep=' ', normalise=str.casefold):
    """a phrase as the caller wrote it -> the string that is searched: `normalise` applied (None: skipped), every whitespace run one
    `sep`, both ends stripped.  1 .. QUERY_MAX characters, or a ValueError that names the query."""
    if not isinstance(q, str):
        raise ValueError('a query must be a string, got %r' % (q,))
    s = sep.join((normalise(q) if normalise is not None else q).split())
    if not 1 <= len(s) <= QUERY_MAX:
        raise ValueError('query %r holds %d characters after normalisation; a query takes 1 .. %d' % (q, len(s), QUERY_MAX))
    return s


def tolerance(m, max_dist=None, max_ratio=0.2):
    """the tolerance k of a query of m characters: min(m - 1, (permille(max_ratio) * m) // 1000, max_dist); None leaves a bound out"""
    m = int(m)
    if not 1 <= m <= QUERY_MAX:
        raise ValueError('a query takes 1 .. %d characters, got %d' % (QUERY_MAX, m))
    k = m - 1
    if max_ratio is not None:
        r = float(max_ratio)
        if not 0.0 <= r <= 1.0:
            raise ValueError('max_ratio must be a float in [0, 1], got %r' % (max_ratio,))
        k = min(k, (int(round(1000 * r)) * m) // 1000)
    if max_dist is not None:
        if int(max_dist) < 0:
            raise ValueError('max_dist must be at least 0, got %r' % (max_dist,))
        k = min(k, int(max_dist))
    return k


def encode_search(page_texts, queries):
    """P page texts and Q queries (already normalised) -> (pool uint8, page_off, page_len int32 [P], query_off, query_len int32 [Q],
    sigma).  The queries' characters get the codes 0 .. sigma - 1, every other page character 255; equal strings of one side share one
    pool range."""
    page_texts, queries = list(page_texts), list(queries)
    for q in queries:
        if not 1 <= len(q) <= QUERY_MAX:
            raise ValueError('query %r holds %d characters; a query takes 1 .. %d' % (q, len(q), QUERY_MAX))
    for t in page_texts:
        if len(t) > LEN_MAX:
            raise ValueError('a page text holds %d characters; the limit is %d' % (len(t), LEN_MAX))
    pool, ((page_off, page_len), (query_off, query_len)), sigma = _encode(
        queries, page_texts, queries, too_many='the queries hold %d distinct characters; a call takes %d')
    return pool, page_off, page_len, query_off, query_len, sigma


# ---------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------
def _differs(a, b):
    """a != b under the rule that 255 equals nothing, itself included"""
    return a != b or a == NONE


def row_py(q, t):
    """v_0 .. v_n of Sellers' table by the plain double loop -- for tiny cases only"""
    q, t = [int(c) for c in q], [int(c) for c in t]
    prev = [0] * (len(t) + 1)
    for i, qi in enumerate(q, 1):
        cur = [i] + [0] * len(t)
        for j, tj in enumerate(t, 1):
            cur[j] = min(prev[j - 1] + int(_differs(qi, tj)), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return np.asarray(prev, dtype=np.int32)


def row_cpu(q, t, anchored=False):
    """v_0 .. v_n of Sellers' table, int32 [n + 1]: by rows of the query, vectorised over the text (page_text._rows, the recurrence of
    page_text.distance_cpu).  anchored: row 0 is 0, 1, 2, ... (the plain edit distance of q against every prefix of t) instead of zeros."""
    q, t = np.asarray(q, dtype=np.uint8).reshape(-1), np.asarray(t, dtype=np.uint8).reshape(-1)
    if not 1 <= q.size <= QUERY_MAX:
        raise ValueError('a query takes 1 .. %d codes, got %d' % (QUERY_MAX, q.size))
    if t.size > LEN_MAX:
        raise ValueError('a text holds %d codes; the limit is %d' % (t.size, LEN_MAX))
    for row in _rows(q, t, None if anchored else np.zeros(t.size + 1, dtype=np.int32)):
        pass
    return row


def hit_ends(v, k):
    """the ends of all hits of a row v_0 .. v_n under the tolerance k, ascending"""
    v = np.asarray(v, dtype=np.int32)
    n = v.size - 1
    if n < 1:
        return np.zeros(0, dtype=np.int32)
    nxt = np.append(v[2:], np.int32(QUERY_MAX + 1))                          # j == n: no next column
    ok = (v[1:] <= k) & (v[1:] <= v[:-1]) & (v[1:] < nxt)
    return (np.flatnonzero(ok) + 1).astype(np.int32)


def match_start(q, t, end, dist):
    """the greatest s <= end with edit_distance(q, t[s:end]) == dist: the anchored row of the reversed query over t[end-1], t[end-2], ...;
    the first l whose score equals dist (l = 0 allowed)"""
    q = np.asarray(q, dtype=np.uint8).reshape(-1)
    lo = max(0, int(end) - (q.size + int(dist)))
    r = row_cpu(q[::-1], np.asarray(t, dtype=np.uint8)[lo:int(end)][::-1], anchored=True)
    at = np.flatnonzero(r == dist)
    if at.size == 0:
        raise AssertionError('no start within m + dist characters of end %d' % end)
    return int(end) - int(at[0])


def _check_search(pool, page_off, page_len, query_off, query_len, jobs, k, max_hits):
    pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1)
    po, pl, qo, ql, k = [np.asarray(t, dtype=np.int64).reshape(-1) for t in (page_off, page_len, query_off, query_len, k)]
    jobs = np.asarray(jobs, dtype=np.int64).reshape(-1, 2)
    if po.size != pl.size:
        raise ValueError('page_off and page_len hold one entry per page, got %d and %d' % (po.size, pl.size))
    if not (qo.size == ql.size == k.size):
        raise ValueError('query_off, query_len and k hold one entry per query, got %d, %d and %d' % (qo.size, ql.size, k.size))
    max_hits = int(max_hits)
    if not 1 <= max_hits <= HITS_MAX:
        raise ValueError('max_hits must be 1 .. %d, got %d' % (HITS_MAX, max_hits))
    if jobs.shape[0] > JOBS_MAX:
        raise ValueError('a call takes %d jobs, got %d' % (JOBS_MAX, jobs.shape[0]))
    if pl.size and ((pl < 0).any() or (pl > LEN_MAX).any()):
        raise ValueError('a page length is outside 0 .. %d' % LEN_MAX)
    if ql.size and ((ql < 1).any() or (ql > QUERY_MAX).any()):
        raise ValueError('a query length is outside 1 .. %d' % QUERY_MAX)
    for off, ln in ((po, pl), (qo, ql)):
        if off.size and ((off < 0).any() or (off + ln > pool.size).any()):
            raise ValueError('a range lies outside the pool of %d codes' % pool.size)
    if k.size and ((k < 0).any() or (k >= ql).any()):
        raise ValueError('a tolerance is outside 0 .. m - 1')
    if jobs.size and ((jobs < 0).any() or (jobs[:, 0] >= pl.size).any() or (jobs[:, 1] >= ql.size).any()):
        raise ValueError('a job names a page or a query that is not there')
    return [pool] + [t.astype(np.int32) for t in (po, pl, qo, ql)] + [np.ascontiguousarray(jobs.astype(np.int32)), k.astype(np.int32), max_hits]


def search_cpu(pool, page_off, page_len, query_off, query_len, jobs, k, max_hits):
    """the definition, for the flat inputs omp_page_search takes -> dict(best int32 [J, 2] = (dist, end), n_hits int32 [J],
    hits int32 [J, max_hits, 3] = (end, dist, start), -1 where there is no hit)"""
    pool, po, pl, qo, ql, jobs, k, H = _check_search(pool, page_off, page_len, query_off, query_len, jobs, k, max_hits)
    J = jobs.shape[0]
    best = np.zeros((J, 2), dtype=np.int32)
    n_hits = np.zeros(J, dtype=np.int32)
    hits = np.full((J, H, 3), -1, dtype=np.int32)
    done = {}
    for j, (p, qi) in enumerate(jobs.tolist()):
        key = (po[p], pl[p], qo[qi], ql[qi], k[qi])
        if key not in done:
            q, t = pool[qo[qi]:qo[qi] + ql[qi]], pool[po[p]:po[p] + pl[p]]
            v = row_cpu(q, t)
            end = int(np.argmin(v))                                           # the least j that attains the minimum
            ends = hit_ends(v, int(k[qi]))
            rows = [(int(e), int(v[e]), match_start(q, t, int(e), int(v[e]))) for e in ends[:H].tolist()]
            done[key] = ((int(v[end]), end), int(ends.size), rows)
        b, c, rows = done[key]
        best[j] = b
        n_hits[j] = c
        if rows:
            hits[j, :len(rows)] = rows
    return dict(best=best, n_hits=n_hits, hits=hits)


def chunk_jobs(n_jobs, max_hits, scratch_cap=SCRATCH_CAP):
    """-> [(lo, hi)]: consecutive jobs whose scratch stays at or below scratch_cap bytes"""
    from ..ops import page_search_scratch_bytes
    one = page_search_scratch_bytes(1, max_hits)
    per = int(scratch_cap) // one
    if per < 1:
        raise ValueError('scratch_cap must hold one job (%d bytes at max_hits %d), got %d' % (one, max_hits, scratch_cap))
    return [(lo, min(lo + per, int(n_jobs))) for lo in range(0, int(n_jobs), per)]


class HostSearcher(object):
    """PageSearcher's `run` from the specification (search_cpu): what the device stage must equal"""

    def __init__(self):
        self.calls = 0

    def run(self, pool, page_off, page_len, query_off, query_len, jobs, k, max_hits, sigma=None):
        self.calls += 1
        return search_cpu(pool, page_off, page_len, query_off, query_len, jobs, k, max_hits)


# ---------------------------------------------------------------------------------------------
# the device stage
# ---------------------------------------------------------------------------------------------
class PageSearcher(_DeviceStage):
    """search_cpu on the device.  A call is ONE packed upload of the tables and the pool, one omp_page_search launch per chunk of jobs
    (a chunk's scratch stays at or below scratch_cap; the scratch is cached and grown), and ONE download of best, n_hits and hits.
    There is no CPU fallback: HostSearcher is the specification."""
    HOST = 'HostSearcher'

    def __init__(self, device, scratch_cap=SCRATCH_CAP):
        super().__init__(device, scratch_cap)
        chunk_jobs(1, 1, self.scratch_cap)       # the cap holds one job that keeps one hit; run() checks it against its max_hits

    def run(self, pool, page_off, page_len, query_off, query_len, jobs, k, max_hits, sigma=None):
        """the inputs of search_cpu (sigma: the number of dense codes; None: the largest code of the pool below 255, plus one) -> the
        dict of search_cpu, as numpy"""
        from .. import ops
        pool, po, pl, qo, ql, jobs, k, H = _check_search(pool, page_off, page_len, query_off, query_len, jobs, k, max_hits)
        dense = pool[pool != NONE]
        top = int(dense.max()) + 1 if dense.size else 0
        sigma = top if sigma is None else int(sigma)
        if sigma < top or sigma > SIGMA_MAX:
            raise ValueError('sigma must be %d .. %d for this pool, got %d' % (top, SIGMA_MAX, sigma))
        return self._search(ops.page_search, (po, pl, qo, ql, k), pool, jobs, sigma, H, chunk_jobs(jobs.shape[0], H, self.scratch_cap),
                            'omp_page_search refused a job (a length above the limits, a range outside the pool, or k >= m)', ops.page_search_scratch_bytes)
