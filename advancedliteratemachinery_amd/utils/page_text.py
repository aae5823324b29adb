"""Page text scoring: the normalised edit distance of whole pages.

A page's words, in the order an entry point returned them, are one string; the score of a page is the reference's
1 - edit_distance(pred, gt) / max(len(pred), len(gt)) after blanks and newlines are removed
(Benchmarks/CC-OCR/evaluation/evaluator/doc_parsing_evaluator.py:223-238).  Unlike the IoU protocol of utils/scoring.py this measure
depends on the ORDER of the words, so it can tell a two-column page read column by column from one read across the gutter.
The numpy functions here are the DEFINITION; csrc/page_text.hip (omp_page_edit_distance) equals pairs_cpu on every integer.

Strings     page_string(): the records' texts concatenated, the characters of `strip` removed, then `normalise` applied; predictions
            and ground truth go through the same function.
Codes       encode_pairs(): one uint8 pool for all strings of a call.  The characters that occur in ANY PREDICTION string get the dense
            codes 0 .. sigma - 1 (sigma <= 254); a ground-truth character outside that set gets 255, and 255 equals nothing, itself
            included.  That is exact: a character no prediction holds can never be part of a match.
Distance    distance_cpu(): Levenshtein, insert / delete / substitute cost 1, by rows of the table:
            new[j] = min(prev[j] + 1, prev[j - 1] + (a_i != b_j)), then new[j] = min_k<=j (new[k] + j - k), the left dependency, as
            minimum.accumulate(new - arange) + arange.  Integers only.
Lengths     0 .. LEN_MAX = 65535 characters a side.
Scores      page_scores(): per pair 1 - d / max(la, lb) in float64; mean (the reference's average over pages) and micro =
            1 - sum(d) / sum(max(la, lb)).  Two empty strings score 1.0 -- the reference would divide by zero there.
"""
import numpy as np

LEN_MAX = 65535                 # characters a side (csrc/myers.h: PT_LEN_MAX, and PT_BLOCK .. PT_NONE below)
BLOCK = 64                      # pattern characters per lane
STRIPE = 4096                   # pattern characters per pass over the text
SIGMA_MAX = 254
NONE = 255                      # the code that equals nothing
SCRATCH_CAP = 1 << 28           # device scratch per chunk of pairs (256 MiB = 8192 pairs)


# ---------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------
def page_string(records, field='rec', strip=' \n', normalise=str.casefold):
    """one image's records, IN THE ORDER GIVEN, as one string.  records: a list of record dicts (the text of each is taken by the
    fallback rule of engine/evaluate.py: TEXT_KEYS -- a None `lex` falls back to `rec`, a None `mgp_lex` to `mgp_text`; any other
    `field` is read as it is), a list of strings (ground-truth words), or one string (a ground-truth page).  The texts are
    concatenated, every character of `strip` is removed (the reference's .replace(' ', '').replace('\\n', '')), and `normalise` is
    applied to the result (None: skipped).  Ground truth goes through this function too; the order of its words is the annotation's,
    and whether that order is the reading order is the caller's responsibility."""
    from ..engine.evaluate import TEXT_KEYS, _text_of
    if isinstance(records, str):
        records = [records]
    parts = []
    for r in records:
        if isinstance(r, str):
            parts.append(r)
        elif isinstance(r, dict):
            parts.append(str(_text_of(r, field) if field in TEXT_KEYS else r[field]))
        else:
            raise ValueError('page_string takes record dicts or strings, got %s' % type(r).__name__)
    s = ''.join(parts)
    if strip:
        s = s.translate({ord(ch): None for ch in strip})
    return normalise(s) if normalise is not None else s


def _encode(code_strings, *sides, too_many):
    """the codes of a call: the characters of `code_strings` get the dense codes 0 .. sigma - 1 in the order they first occur, every
    other character NONE; each of `sides` (a list of strings) is placed in ONE pool, equal strings of one side sharing one range
    -> (pool uint8, [(off, len) int32 per side], sigma).  too_many: the message for more than SIGMA_MAX distinct characters."""
    table = {}
    for s in code_strings:
        for ch in s:
            table.setdefault(ch, len(table))
    sigma = len(table)
    if sigma > SIGMA_MAX:
        raise ValueError(too_many % (sigma, SIGMA_MAX))
    chunks, total, placed = [], 0, []
    for strings in sides:
        seen, off = {}, []
        for s in strings:
            if s not in seen:
                seen[s] = total
                chunks.append(np.fromiter((table.get(ch, NONE) for ch in s), dtype=np.uint8, count=len(s)))
                total += len(s)
            off.append(seen[s])
        placed.append((np.asarray(off, dtype=np.int32).reshape(-1), np.asarray([len(s) for s in strings], dtype=np.int32).reshape(-1)))
    if total > 0x7fffffff:
        raise ValueError('the strings of a call hold %d characters; a pool takes 2^31 - 1' % total)
    return np.concatenate(chunks + [np.zeros(0, np.uint8)]).astype(np.uint8), placed, sigma


def encode_pairs(pred_strings, gt_strings):
    """P prediction strings against P ground-truth strings -> (pool uint8, a_off, a_len, b_off, b_len int32 [P], sigma): pair p is
    pool[a_off[p] : a_off[p] + a_len[p]] (the prediction) against pool[b_off[p] : ...] (the ground truth).  Equal strings of one side
    share one pool range, so one ground-truth page can face many settings at the cost of one copy."""
    pred_strings, gt_strings = list(pred_strings), list(gt_strings)
    if len(pred_strings) != len(gt_strings):
        raise ValueError('%d prediction strings for %d ground-truth strings' % (len(pred_strings), len(gt_strings)))
    for s in pred_strings + gt_strings:
        if len(s) > LEN_MAX:
            raise ValueError('a page string holds %d characters; the limit is %d' % (len(s), LEN_MAX))
    pool, ((a_off, a_len), (b_off, b_len)), sigma = _encode(
        pred_strings, pred_strings, gt_strings, too_many='the prediction strings hold %d distinct characters; a call takes %d -- score '
        'such pages on the host with utils.lexicon.edit_distance_cpu')
    return pool, a_off, a_len, b_off, b_len, sigma


def _rows(a, b, first=None):
    """rows 0 .. la of the edit-distance table of the code sequences a (rows) and b (columns), int32 [lb + 1] each: THE row recurrence
    (the module docstring's).  first: row 0 (None: 0, 1, 2, ..., the Levenshtein table); column 0 is 0, 1, 2, ... either way."""
    ar = np.arange(b.size + 1, dtype=np.int32)
    prev = ar if first is None else first
    yield prev
    b_none = b == NONE
    rows = {NONE: np.ones(b.size, dtype=np.int32)}                            # a_i != b, per code of a: computed once
    for i, ai in enumerate(a.tolist(), 1):
        differs = rows.get(ai)
        if differs is None:
            differs = rows[ai] = ((b != ai) | b_none).astype(np.int32)
        new = np.empty(b.size + 1, dtype=np.int32)
        new[0] = i
        np.minimum(prev[1:] + 1, prev[:-1] + differs, out=new[1:])
        prev = np.minimum.accumulate(new - ar) + ar
        yield prev


def distance_cpu(a, b):
    """the Levenshtein distance of two code sequences (uint8; 255 equals nothing, itself included): the definition.  The table is walked
    by rows of the shorter sequence, vectorised over the longer (the distance is symmetric)."""
    a, b = np.asarray(a, dtype=np.uint8).reshape(-1), np.asarray(b, dtype=np.uint8).reshape(-1)
    if a.size > LEN_MAX or b.size > LEN_MAX:
        raise ValueError('a sequence holds %d codes; the limit is %d' % (max(a.size, b.size), LEN_MAX))
    if a.size > b.size:
        a, b = b, a
    for row in _rows(a, b):
        pass
    return int(row[-1])


def _check_pairs(pool, a_off, a_len, b_off, b_len):
    pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1)
    tabs = [np.asarray(t, dtype=np.int64).reshape(-1) for t in (a_off, a_len, b_off, b_len)]
    P = tabs[1].size
    if any(t.size != P for t in tabs):
        raise ValueError('a_off, a_len, b_off and b_len hold one entry per pair, got %s' % [t.size for t in tabs])
    for off, ln in ((tabs[0], tabs[1]), (tabs[2], tabs[3])):
        if P and ((ln < 0).any() or (ln > LEN_MAX).any()):
            raise ValueError('a length is outside 0 .. %d' % LEN_MAX)
        if P and ((off < 0).any() or (off + ln > pool.size).any()):
            raise ValueError('a range lies outside the pool of %d codes' % pool.size)
    return [pool] + [t.astype(np.int32) for t in tabs]


def pairs_cpu(pool, a_off, a_len, b_off, b_len):
    """distance_cpu over the pairs of a call, for the flat inputs omp_page_edit_distance takes -> int32 [P]"""
    pool, a_off, a_len, b_off, b_len = _check_pairs(pool, a_off, a_len, b_off, b_len)
    out = np.zeros(a_len.size, dtype=np.int32)
    done = {}
    for p, key in enumerate(zip(a_off.tolist(), a_len.tolist(), b_off.tolist(), b_len.tolist())):
        if key not in done:
            ao, la, bo, lb = key
            done[key] = distance_cpu(pool[ao:ao + la], pool[bo:bo + lb])
        out[p] = done[key]
    return out


def page_scores(dist, a_len, b_len):
    """-> dict(score float64 [P] = 1 - d / max(la, lb), mean = the average of score (the reference's figure), micro =
    1 - sum(d) / sum(max(la, lb))).  A pair of two empty strings scores 1.0; the reference would divide by zero there.  By the same
    convention no pairs at all give mean = micro = 1.0."""
    d = np.asarray(dist, dtype=np.int64).reshape(-1)
    longer = np.maximum(np.asarray(a_len, dtype=np.int64).reshape(-1), np.asarray(b_len, dtype=np.int64).reshape(-1))
    if longer.size != d.size:
        raise ValueError('%d distances for %d pairs' % (d.size, longer.size))
    if (d < 0).any() or (d > longer).any():
        raise ValueError('a distance lies outside 0 .. max(la, lb)')
    score = np.ones(d.size, dtype=np.float64)
    some = longer > 0
    score[some] = 1.0 - d[some] / longer[some]
    total = int(longer.sum())
    return dict(score=score, mean=float(score.mean()) if d.size else 1.0, micro=1.0 - int(d.sum()) / total if total else 1.0)


def chunk_pairs(n_pairs, scratch_cap=SCRATCH_CAP):
    """-> [(lo, hi)]: consecutive pairs whose scratch stays at or below scratch_cap bytes"""
    from ..ops import PAGE_TEXT_SLICE_BYTES
    per = int(scratch_cap) // PAGE_TEXT_SLICE_BYTES
    if per < 1:
        raise ValueError('scratch_cap must hold one pair (%d bytes), got %d' % (PAGE_TEXT_SLICE_BYTES, scratch_cap))
    return [(lo, min(lo + per, int(n_pairs))) for lo in range(0, int(n_pairs), per)]


class HostPageScorer(object):
    """PageTextScorer's `run` from the specification (pairs_cpu): what the device stage must equal"""

    def __init__(self):
        self.calls = 0

    def run(self, pool, a_off, a_len, b_off, b_len, sigma):
        self.calls += 1
        return pairs_cpu(pool, a_off, a_len, b_off, b_len)


# ---------------------------------------------------------------------------------------------
# the device stage
# ---------------------------------------------------------------------------------------------
def _check_sigma(pool, sigma):
    """sigma as an int in 0 .. SIGMA_MAX with every code of the pool below it or NONE"""
    sigma = int(sigma)
    if sigma < 0 or sigma > SIGMA_MAX:
        raise ValueError('sigma must be 0 .. %d, got %d' % (SIGMA_MAX, sigma))
    if pool.size and int((pool + np.uint8(1)).max()) > sigma:                # uint8 wraps: 255 -> 0, a code c -> c + 1 <= sigma
        raise ValueError('the pool holds a code at or above sigma (%d) that is not %d' % (sigma, NONE))
    return sigma


class _DeviceStage(object):
    """what PageTextScorer, page_align.PageAligner and the searchers of page_search, page_pattern and page_regex share: the device check,
    the cached scratch and the packed upload; the searchers also the whole device half of their `run` (_search).  HOST names the host
    twin, the specification."""
    HOST = None

    def __init__(self, device, scratch_cap):
        import torch
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('%s runs on MI355X only (got device %s); there is no CPU fallback -- '
                               '%s is the host specification' % (type(self).__name__, self.device, self.HOST))
        self.scratch_cap = int(scratch_cap)
        self.scratch = None
        self.chunks = 0             # chunks of the last run
        self.calls = 0

    def _grow(self, need):
        """the cached scratch, at least `need` bytes"""
        import torch
        if self.scratch is None or self.scratch.numel() < need:
            self.scratch = None                                              # let go of the old one before the larger one is made
            self.scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.scratch

    def _upload(self, tables, pool):
        """the one upload: the tables, the widest first (each lands on a multiple of its own width), then the pool -> (the tables as
        device tensors of their own types, the pool)"""
        import torch
        blob = torch.from_numpy(np.concatenate([t.view(np.uint8) for t in tables] + [pool, np.zeros(1, np.uint8)])).to(self.device)
        ends = np.cumsum([t.nbytes for t in tables]).tolist()
        return [blob[e - t.nbytes:e].view(getattr(torch, t.dtype.name)) for t, e in zip(tables, ends)], blob[ends[-1]:]

    def _search(self, op, tables, pool, jobs, sigma, H, parts, refused, scratch_bytes=None):
        """the device half of a page search's `run` (page_search, page_pattern and page_regex).  op: the ops wrapper, which takes (pool,
        pool_bytes, *tables, jobs, sigma, max_hits[, scratch], best=, n_hits=, hits=); tables: numpy, in the wrapper's order (64-bit words
        travel as int64: the same bytes); jobs int32 [J, 2].  ONE packed upload, the widest tables first; the cached scratch grown to
        scratch_bytes(the jobs of the largest part, H) when a per-job scratch size is given; one op per (lo, hi) of `parts` with that
        part's jobs and its slices of the outputs; ONE download -> dict(best int32 [J, 2], n_hits int32 [J], hits int32 [J, H, 3]) as
        numpy.  A refused job (n_hits < 0) raises RuntimeError(refused)."""
        import torch
        J = jobs.shape[0]
        self.calls += 1
        self.chunks = len(parts)
        if J == 0:
            return dict(best=np.zeros((0, 2), np.int32), n_hits=np.zeros(0, np.int32), hits=np.zeros((0, H, 3), np.int32))
        flat = [t.reshape(-1).view(np.int64) if t.dtype == np.uint64 else t.reshape(-1) for t in tables] + [jobs.reshape(-1)]
        order = sorted(range(len(flat)), key=lambda i: -flat[i].itemsize)     # stable
        with torch.cuda.device(self.device):
            sent, d_pool = self._upload([flat[i] for i in order], pool)
            tabs = [None] * len(flat)
            for i, d in zip(order, sent):
                tabs[i] = d                                                   # back in the wrapper's order
            d_jobs = tabs.pop()
            tail = () if scratch_bytes is None else (self._grow(scratch_bytes(max(hi - lo for lo, hi in parts), H)),)
            out = torch.empty(J * (3 + 3 * H), dtype=torch.int32, device=self.device)     # best [J, 2] | n_hits [J] | hits [J, H, 3]
            for lo, hi in parts:
                op(d_pool, pool.size, *tabs, d_jobs[2 * lo:2 * hi], sigma, H, *tail, best=out[2 * lo:2 * hi], n_hits=out[2 * J + lo:2 * J + hi],
                   hits=out[3 * J + 3 * H * lo:3 * J + 3 * H * hi])
            host = out.cpu().numpy()                                          # the one download
        res = dict(best=host[:2 * J].reshape(J, 2), n_hits=host[2 * J:3 * J], hits=host[3 * J:].reshape(J, H, 3))
        if (res['n_hits'] < 0).any():
            raise RuntimeError(refused)
        return res


class PageTextScorer(_DeviceStage):
    """pairs_cpu on the device.  A call is ONE packed upload of the tables and the pool, one omp_page_edit_distance launch per chunk of
    pairs (a chunk's scratch stays at or below scratch_cap; the scratch is cached and grown), and ONE download of the distances.
    There is no CPU fallback: HostPageScorer is the specification."""
    HOST = 'HostPageScorer'

    def __init__(self, device, scratch_cap=SCRATCH_CAP):
        super().__init__(device, scratch_cap)
        chunk_pairs(1, self.scratch_cap)

    def run(self, pool, a_off, a_len, b_off, b_len, sigma):
        """pool uint8, a_off / a_len / b_off / b_len int32 [P] as encode_pairs gives them -> int32 [P] as numpy"""
        import torch

        from .. import ops
        pool, a_off, a_len, b_off, b_len = _check_pairs(pool, a_off, a_len, b_off, b_len)
        sigma = _check_sigma(pool, sigma)
        P = a_len.size
        self.calls += 1
        parts = chunk_pairs(P, self.scratch_cap)
        self.chunks = len(parts)
        if P == 0:
            return np.zeros(0, dtype=np.int32)
        with torch.cuda.device(self.device):
            (d_ao, d_al, d_bo, d_bl), d_pool = self._upload((a_off, a_len, b_off, b_len), pool)
            scratch = self._grow(ops.page_scratch_bytes(max(hi - lo for lo, hi in parts)))
            dist = torch.empty(P, dtype=torch.int32, device=self.device)
            for lo, hi in parts:
                ops.page_edit_distance(d_pool, pool.size, d_ao[lo:hi], d_al[lo:hi], d_bo[lo:hi], d_bl[lo:hi], sigma, scratch, dist=dist[lo:hi])
            out = dist.cpu().numpy()                                          # the one download
        if (out < 0).any():
            raise RuntimeError('omp_page_edit_distance refused a pair (a length above %d, or a range outside the pool)' % LEN_MAX)
        return out
