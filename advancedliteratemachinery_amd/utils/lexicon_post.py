"""Posterior lexicon decoding: the lexicon word MGP-STR's character head itself finds most likely.

`lexicon=` (utils/lexicon.py, section 15) snaps a reading to the nearest word under the edit distance of the GREEDY string.
The character head knows more: a posterior over 38 classes ([GO], [s], then CHARACTER) at each of its 27 positions.  The
head is non-autoregressive, so for a word w of n characters

    P(w) = prod_{i < n} p_i(w[i]) * p_n([s])

is exactly the probability that the reference's decoding rule (test_final.py:172-181: per-position choice, cut at the first
[s]) yields w, were the choice sampled instead of taken greedily.  The lexicon protocols named at the top of
utils/lexicon.py are normally run by scoring every lexicon word under the recogniser and taking the most probable.

Floats end at the COSTS; everything after them is integer, so host and device agree on every output:

    costs_cpu(logits fp32 [N, 27, 38]) -> int32 [N, 26, 38]: position 0 is dropped (as recognize does with [:, 1:]), the
        log-softmax of each row is taken in float64 from the fp32 logits, and
            cost = clip(floor(-logp * 1024 + 0.5), 0, COST_CAP),   COST_CAP = 2^20 - 1
        One unit is 1/1024 nat; 26 capped terms stay far below 2^31.  Worked values: 38 equal logits give
        floor(ln 38 * 1024 + 0.5) = 3725 everywhere; one class at +20 over zeros gives 0 for that class
        (-logp = ln(1 + 37 e^-20) = 7.6e-8 nat) and 20480 for the others.
    class_table(alphabet, fold_case) -> uint8 [256]: lexicon code (utils/lexicon.py: code_table) -> class index
        2 + CHARACTER.index(ch); 255 = "unscorable" (a character MGP-STR cannot emit, and the codes 254 / 255).
    score of a word of n codes for query q:  sum_{i < n} cost[q, i, class(w[i])] + cost[q, n, 1]   (class 1 is [s]).
        A word with n > 25, or with any unscorable code, has no score and is never returned.  The empty word scores
        cost[q, 0, 1].
    score_cpu(costs, pool, offsets, table, ranges) -> best uint64 [N, 2]: column 0 the least key (score << 32) | index
        over the query's half-open range of lexicon indices, column 1 the least key among the OTHER indices (the
        runner-up; a duplicate spelling at another index counts); NONE_KEY = there is none.  Ties go to the lowest index
        because the index is the low half of the key.  Ranges are clamped to [0, L]; an inverted range is empty.  The
        offsets are clamped into the pool exactly as the kernel clamps them (word w is pool[s, e) with
        s = clip(offsets[w], 0, pool_bytes), e = clip(offsets[w + 1], s, pool_bytes)), so a damaged table has a defined
        answer.
    greedy_cpu(costs) -> int32 [N, 2] (greedy_cost, greedy_len) on the QUANTISED costs: per position the least cost, the
        lowest class among equals; greedy_len is the first position whose class is 1 ([s]), or 26 if there is none; the
        cost is the sum of the minima through that position (26 terms without an [s]).  Informational: records report
        gap = score - greedy_cost.  The gap may be negative: a shorter word has fewer factors, so the greedy string is not
        the MAP string (a word that ends where greedy reads on pays one [s] term instead of several character terms).
    accept_post(score, second, min_prob, min_margin): the host's acceptance rule, in integer units.

`score_py` is the definition (a pure-Python double loop); `score_cpu` is the numpy specification the kernel is held to.
`PosteriorMatcher` runs it on the device (csrc/lexicon_post.hip: omp_logprob_costs, omp_lexicon_posterior); there is no
CPU fallback.  OmniParser's own `rec` is autoregressive -- rescoring it needs teacher-forced decoder runs per candidate --
so `lex*` from `rec` stays edit-distance.
"""
import math

import numpy as np

from .lexicon import NONE_KEY, _check_ranges

POSITIONS = 26            # scored positions: the head's 27 minus position 0
CLASSES = 38              # [GO], [s], then the 36 characters
EOS_CLASS = 1
WORD_MAX_POST = 25        # a word and its [s] fit the 26 positions
UNSCORABLE = 255
UNIT = 1024               # cost units per nat
COST_CAP = (1 << 20) - 1
WORK_SLICES = 4096        # omp_lexicon_posterior: work holds 2 * (n + WORK_SLICES) uint64 (include/omp355.h)


def _mgp_characters():
    from ..model.mgp_str import CHARACTER
    return CHARACTER


def costs_cpu(logits):
    """fp32 [N, 27, 38] logits -> int32 [N, 26, 38] costs: clip(floor(-log_softmax * 1024 + 0.5), 0, COST_CAP) with the
    log-softmax in float64 from the fp32 values, position 0 dropped.  38 equal logits give 3725 everywhere; one class at
    +20 over zeros gives 0 for that class and 20480 for the others."""
    x = np.asarray(logits, dtype=np.float32)
    if x.ndim != 3 or x.shape[1] != POSITIONS + 1 or x.shape[2] != CLASSES:
        raise ValueError('logits are [N, %d, %d], got %s' % (POSITIONS + 1, CLASSES, x.shape))
    x = x[:, 1:].astype(np.float64)
    m = x.max(axis=2, keepdims=True)
    logp = (x - m) - np.log(np.exp(x - m).sum(axis=2, keepdims=True))
    return np.clip(np.floor(-logp * UNIT + 0.5), 0, COST_CAP).astype(np.int32)


def class_table(alphabet, fold_case, characters=None):
    """uint8 [256]: the lexicon code of utils/lexicon.py: code_table(alphabet, fold_case) -> 2 + characters.index(ch), compared
    after lower-casing when fold_case is set (the codes are made with upper()); 255 for a code whose character MGP-STR cannot
    emit, for unused codes and for 254 / 255."""
    from .lexicon import code_table
    characters = _mgp_characters() if characters is None else characters
    out = np.full(256, UNSCORABLE, dtype=np.uint8)
    for ch, code in code_table(alphabet, fold_case).items():
        c = ch.lower() if fold_case else ch
        if len(c) == 1 and c in characters:
            out[code] = 2 + characters.index(c)
    return out


def _check_costs(costs):
    c = np.asarray(costs)
    if c.ndim != 3 or c.shape[1] != POSITIONS or c.shape[2] != CLASSES:
        raise ValueError('costs are [N, %d, %d], got %s' % (POSITIONS, CLASSES, c.shape))
    return c.astype(np.int64)


def _word_bounds(offsets, L, pool_bytes):
    """the kernel's clamping: word w is pool[s, e), s = clip(offsets[w], 0, pool_bytes), e = clip(offsets[w + 1], s, pool_bytes)"""
    off = np.asarray(offsets, dtype=np.int64)[:L + 1]
    s = np.clip(off[:-1], 0, pool_bytes)
    e = np.minimum(np.maximum(off[1:], s), pool_bytes)
    return s, e


def word_score_py(cost_q, codes, table):
    """the score of one word (a sequence of lexicon codes) under one query's [26][38] costs, or None"""
    n = len(codes)
    if n > WORD_MAX_POST:
        return None
    total = 0
    for i, code in enumerate(codes):
        cls = int(table[int(code)])
        if cls == UNSCORABLE:
            return None
        total += int(cost_q[i][cls])
    return total + int(cost_q[n][EOS_CLASS])


def score_py(costs, pool, offsets, table, ranges=None, pool_bytes=None):
    """The definition: a double loop over queries and words -> best uint64 [N, 2] as score_cpu."""
    c = _check_costs(costs)
    L = len(offsets) - 1
    pool = np.asarray(pool, dtype=np.uint8)
    pool_bytes = int(pool.size) if pool_bytes is None else max(min(int(pool_bytes), int(pool.size)), 0)
    s, e = _word_bounds(offsets, L, pool_bytes)
    rng = _check_ranges(ranges, c.shape[0], L)
    best = np.full((c.shape[0], 2), NONE_KEY, dtype=np.uint64)
    for q in range(c.shape[0]):
        lo, hi = (0, L) if rng is None else (int(rng[q, 0]), int(rng[q, 1]))
        a = b = NONE_KEY
        rows = c[q].tolist()
        for w in range(lo, hi):
            sc = word_score_py(rows, pool[int(s[w]):int(e[w])].tolist(), table)
            if sc is None:
                continue
            key = (sc << 32) | w
            if key < a:
                a, b = key, a
            elif key < b:
                b = key
        best[q, 0], best[q, 1] = a, b
    return best


class _Classes(object):
    """the lexicon as score_cpu walks it: which words can be scored (ok), and for those, in index order, the flat indices
    position * 38 + class of their characters into one query's costs (a dead position points at a zero appended behind the
    costs) and of their [s] term"""

    def __init__(self, pool, offsets, table, pool_bytes=None):
        pool = np.asarray(pool, dtype=np.uint8)
        pool_bytes = int(pool.size) if pool_bytes is None else max(min(int(pool_bytes), int(pool.size)), 0)
        self.L = len(offsets) - 1
        s, e = _word_bounds(offsets, self.L, pool_bytes)
        self.lens = e - s
        fits = self.lens <= WORD_MAX_POST
        n = np.where(fits, self.lens, 0)
        col = np.arange(WORD_MAX_POST)[None, :]
        live = col < n[:, None]
        src = np.minimum(s[:, None] + col, max(pool_bytes - 1, 0))
        cls = np.asarray(table, dtype=np.uint8)[pool[src]] if pool_bytes > 0 else np.zeros(live.shape, dtype=np.uint8)
        scorable = cls < CLASSES                                     # 255 by convention; the kernel refuses 38..254 too
        self.ok = fits & ~(~scorable & live).any(axis=1)
        self.sel = np.nonzero(self.ok)[0].astype(np.int64)
        flat = np.where(live & scorable, col * CLASSES + cls, POSITIONS * CLASSES)
        self.flat = flat[self.sel].astype(np.int32)
        self.eos = (n[self.sel] * CLASSES + EOS_CLASS).astype(np.int32)


def score_cpu(costs, pool, offsets, table, ranges=None, pool_bytes=None):
    """The specification of omp_lexicon_posterior: -> best uint64 [N, 2]; column 0 the least key (score << 32) | index of
    the query's range, column 1 the least key among the other indices, NONE_KEY where there is none."""
    c = _check_costs(costs)
    lex = _Classes(pool, offsets, table, pool_bytes)
    N = c.shape[0]
    rng = _check_ranges(ranges, N, lex.L)
    best = np.full((N, 2), NONE_KEY, dtype=np.uint64)
    for q in range(N):
        lo, hi = (0, lex.L) if rng is None else (int(rng[q, 0]), int(rng[q, 1]))
        a, b = (int(v) for v in np.searchsorted(lex.sel, [lo, max(hi, lo)]))
        if a >= b:
            continue
        cq = np.append(c[q].reshape(-1), 0)
        score = cq[lex.flat[a:b]].sum(axis=1) + cq[lex.eos[a:b]]
        key = ((score << 32) | lex.sel[a:b]).astype(np.uint64)
        k = int(key.argmin())
        best[q, 0] = key[k]
        if key.size > 1:
            key[k] = np.uint64(NONE_KEY)
            best[q, 1] = key.min()
    return best


def greedy_cpu(costs):
    """int32 [N, 2] (greedy_cost, greedy_len) on the quantised costs: the least cost per position (lowest class among equals), cut
    at the first position whose class is [s] (that position's cost included); 26 positions and length 26 without one."""
    c = _check_costs(costs)
    key = (c << 6) | np.arange(CLASSES, dtype=np.int64)[None, None, :]
    k = key.min(axis=2)
    cls, mn = k & 63, k >> 6
    out = np.zeros((c.shape[0], 2), dtype=np.int32)
    for q in range(c.shape[0]):
        eos = np.nonzero(cls[q] == EOS_CLASS)[0]
        n = int(eos[0]) if eos.size else POSITIONS
        out[q, 0] = int(mn[q, :min(n + 1, POSITIONS)].sum())
        out[q, 1] = n
    return out


def unpack_post(best):
    """uint64 [N, 2] keys -> (idx int64 [N, 2], score int64 [N, 2]) with (-1, -1) for NONE_KEY"""
    b = np.ascontiguousarray(best).view(np.uint64).reshape(-1, 2)
    none = b == np.uint64(NONE_KEY)
    idx = (b & np.uint64(0xffffffff)).astype(np.int64)
    score = (b >> np.uint64(32)).astype(np.int64)
    idx[none], score[none] = -1, -1
    return idx, score


def accept_post(score, second, min_prob=None, min_margin=None):
    """the host's acceptance rule in integer units (1/1024 nat).  score: the best word's, None or negative = no word (never
    accepted); second: the runner-up's, None or negative = none.  Rejected when min_prob is given and
    score > floor(-ln(min_prob) * 1024), or when min_margin (nats) is given, a runner-up exists and
    second - score < ceil(min_margin * 1024)."""
    if score is None or score < 0:
        return False
    if min_prob is not None:
        if min_prob > 0 and score > int(math.floor(-math.log(min_prob) * UNIT)):
            return False
    if min_margin is not None and second is not None and second >= 0:
        if second - score < int(math.ceil(min_margin * UNIT)):
            return False
    return True


def check_post_args(min_prob, min_margin):
    if min_prob is not None and not (0.0 < float(min_prob) <= 1.0):
        raise ValueError('lexicon_min_prob is a probability in (0, 1], got %r' % (min_prob,))
    if min_margin is not None and not float(min_margin) >= 0.0:
        raise ValueError('lexicon_min_margin is a log-probability margin in nats, >= 0, got %r' % (min_margin,))


class PosteriorMatcher(object):
    """Posterior decoding on the device, around a utils.lexicon.LexiconMatcher whose uploaded pool and offsets it reuses; the
    class table is built from the matcher's alphabet once.  A call takes the character head's fp32 logits [N, 27, 38] ON THE
    DEVICE and answers per row.  Per chunk of `matcher.chunk` rows: at most one upload (the ranges), one omp_logprob_costs,
    one omp_lexicon_posterior, one download (keys and greedy path in one block)."""

    def __init__(self, matcher, characters=None):
        import torch
        self.device = torch.device(matcher.device)
        if self.device.type != 'cuda':
            raise RuntimeError('PosteriorMatcher runs on MI355X only (got device %s); there is no CPU fallback -- '
                               'score_cpu is the host specification' % (self.device,))
        self.matcher = matcher
        self.words = matcher.words
        self.table_host = class_table(matcher.alphabet, matcher.fold_case, characters)
        self.table = torch.from_numpy(self.table_host).to(self.device)
        self.chunk = int(matcher.chunk)
        self.keep_costs = False      # tests: keep every chunk's device costs in last_costs
        self.last_costs = []
        self.last_chunks = 0

    @property
    def n_lists(self):
        return self.matcher.n_lists

    def range_of(self, i):
        return self.matcher.range_of(i)

    def score(self, logits, ranges=None):
        """-> (best uint64 [N, 2] as score_cpu, greedy int32 [N, 2] as greedy_cpu), numpy"""
        import torch

        from .. import ops
        m = self.matcher
        if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3
                and logits.shape[1] == POSITIONS + 1 and logits.shape[2] == CLASSES):
            raise ValueError('logits are a device fp32 tensor [N, %d, %d]' % (POSITIONS + 1, CLASSES))
        N = int(logits.shape[0])
        rng = _check_ranges(ranges, N, m.L)
        best = np.full((N, 2), NONE_KEY, dtype=np.uint64)
        greedy = np.zeros((N, 2), dtype=np.int32)
        self.last_chunks, self.last_costs = 0, []
        with torch.cuda.device(self.device):
            for i0 in range(0, N, self.chunk):
                i1 = min(N, i0 + self.chunk)
                n = i1 - i0
                lo = hi = None
                hint = 0
                if rng is not None:
                    both = torch.from_numpy(np.ascontiguousarray(rng[i0:i1].T)).to(self.device)   # the chunk's one upload
                    lo, hi = both[0], both[1]
                    hint = max(int((rng[i0:i1, 1] - rng[i0:i1, 0]).max()), 0)
                out = torch.empty(3 * n, dtype=torch.int64, device=self.device)
                costs, g = ops.logprob_costs(logits[i0:i1].contiguous(), greedy=out[2 * n:].view(torch.int32).view(n, 2))
                ops.lexicon_posterior(costs, lo, hi, m.pool, m.pool_bytes, m.offsets, m.L, self.table, range_hint=hint,
                                      best=out[:2 * n].view(n, 2))
                host = out.cpu().numpy()                                                            # the chunk's one download
                best[i0:i1] = host[:2 * n].view(np.uint64).reshape(n, 2)
                greedy[i0:i1] = host[2 * n:].view(np.int32).reshape(n, 2)
                if self.keep_costs:
                    self.last_costs.append(costs)
                self.last_chunks += 1
        return best, greedy

    def __call__(self, logits, ranges=None, min_prob=None, min_margin=None):
        """-> list of dicts: word (None when there is none or the match is rejected), index, score, second = (index, score) or
        None, greedy_cost, greedy_len -- indices into the whole lexicon, scores in integer units"""
        best, greedy = self.score(logits, ranges)
        return describe(best, greedy, self.words, min_prob, min_margin)


def describe(best, greedy, words, min_prob=None, min_margin=None):
    idx, score = unpack_post(best)
    out = []
    for (i, j), (s, t), (gc, gl) in zip(idx.tolist(), score.tolist(), np.asarray(greedy).tolist()):
        second = (j, t) if j >= 0 else None
        ok = i >= 0 and accept_post(s, t if j >= 0 else None, min_prob, min_margin)
        out.append(dict(word=words[i] if ok else None, index=i, score=s if i >= 0 else None, second=second, greedy_cost=gc, greedy_len=gl))
    return out


def result_keys(d, prefix, base=0):
    """one describe() entry -> the public keys: prefix (the accepted word or None), prefix_index (-1: no word), prefix_logp
    (-score / 1024), prefix_second ((index, logp) or None), prefix_gap ((score - greedy_cost) / 1024 nats; may be negative).
    base: the first index of the record's own list (per-image lexicons)."""
    none = d['index'] < 0
    sec = d['second']
    return {prefix: d['word'], prefix + '_index': -1 if none else d['index'] - base,
            prefix + '_logp': None if none else -d['score'] / float(UNIT),
            prefix + '_second': None if sec is None else (sec[0] - base, -sec[1] / float(UNIT)),
            prefix + '_gap': None if none else (d['score'] - d['greedy_cost']) / float(UNIT)}


def posterior_of(matcher):
    """the PosteriorMatcher of a lexicon matcher, built once and cached on it"""
    post = getattr(matcher, '_posterior', None)
    if post is None:
        post = PosteriorMatcher(matcher)
        matcher._posterior = post
    return post


def annotate_posterior(records, matcher, logits, prefix='mgp_lex', min_prob=None, min_margin=None):
    """records: per image a list of record dicts; logits: the character head's logits of all records, in record order, on the
    device.  Every record gains prefix, prefix_index (in its image's own list for per-image lexicons), prefix_logp,
    prefix_second and prefix_gap.  ALL words of the call go through ONE posterior call."""
    per_image = getattr(matcher, 'n_lists', None) is not None
    owners, ranges = [], []
    for b, recs in enumerate(records):
        for r in recs:
            owners.append(r)
            if per_image:
                ranges.append(tuple(matcher.range_of(b)))
    if not owners:
        return records
    if logits is None or int(logits.shape[0]) != len(owners):
        raise ValueError('%d records but %s rows of character logits' % (len(owners), None if logits is None else int(logits.shape[0])))
    res = posterior_of(matcher)(logits, ranges=ranges if per_image else None, min_prob=min_prob, min_margin=min_margin)
    for k, (r, d) in enumerate(zip(owners, res)):
        r.update(result_keys(d, prefix, ranges[k][0] if per_image else 0))
    return records
