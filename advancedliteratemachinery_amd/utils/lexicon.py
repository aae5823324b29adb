"""Lexicon correction: snap every word a reader returns to the nearest word of a word list.

The protocols text spotters report under hand each image (or each test set) a lexicon and take the nearest entry of it:
Total-Text / CTW1500 "Full", ICDAR-15 strong / weak / generic, closed-vocabulary KIE fields.  The distance is plain
Levenshtein -- insert, delete and substitute cost 1, no transpositions -- which is what the reference's recogniser
evaluation uses (OCR/MGP-STR/test_final.py:14, nltk's edit_distance with its defaults).

Characters become CODES before anything is compared:

    alphabet, fold_case -> table: each character's index at its first occurrence in the alphabet; with fold_case the
        alphabet and every word go through str.upper() first (so 'a' and 'A' share the code of whichever comes first)
    a character outside the alphabet -> UNKNOWN_WORD (255) in a lexicon word, UNKNOWN_QUERY (254) in a query: two
        unknown characters never compare equal, and an alphabet has at most 254 symbols
    lexicon  -> (pool uint8 [sum of lengths], offsets int32 [L + 1]): word i is pool[offsets[i] : offsets[i + 1]], at most
        WORD_MAX = 255 codes
    queries  -> (codes uint8 [N, 64], q_len int32 [N]): at most QUERY_MAX = 64 codes (OmniParser reads 25 characters,
        MGP-STR 27); bytes beyond q_len are 0

which is the layout of omp_lexicon_nearest (include/omp355.h, csrc/lexicon.hip).  The answer for a query and a half-open
range [lo, hi) of lexicon indices is the word of least distance, the lowest index among equals; (-1, -1) for an empty
range.  An empty query is legal: its distance to a word is the word's length.

`edit_distance_cpu` is the definition (the two-row dynamic programme).  `nearest_cpu` is the specification of the kernel:
Myers' bit-parallel recurrence on numpy uint64 arrays across the lexicon, one query at a time,

    Peq[c] = bits i with query[i] == c;  Pv = all ones, Mv = 0, score = m;  per lexicon character c:
        Eq = Peq[c];  Xv = Eq | Mv;  Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq
        Ph = Mv | ~(Xh | Pv);  Mh = Pv & Xh
        score += (Ph >> (m - 1)) & 1;  score -= (Mh >> (m - 1)) & 1
        Ph = (Ph << 1) | 1;  Mh <<= 1;  Pv = Mh | ~(Xv | Ph);  Mv = Ph & Xv

with m == 0 apart (the word's length).  Integers only, so host and device agree on every output.  `LexiconMatcher` runs
it on the device; there is no CPU fallback.
"""
import numpy as np

QUERY_MAX = 64
WORD_MAX = 255
ALPHABET_MAX = 254
UNKNOWN_QUERY = 254
UNKNOWN_WORD = 255
NONE_KEY = (1 << 64) - 1


def edit_distance_cpu(a, b):
    """Levenshtein distance of two sequences (strings, lists, arrays of codes): insert / delete / substitute cost 1."""
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, cb in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb))
        prev = cur
    return prev[len(b)]


def default_alphabet():
    """OmniParser's character set (utils/parser.py: DEFAULT_CHARS, what args.chars defaults to)"""
    from .parser import DEFAULT_CHARS
    return DEFAULT_CHARS


def _fold(s, fold_case):
    return s.upper() if fold_case else s


def code_table(alphabet, fold_case=True):
    """character -> code: its index at its first occurrence in the (folded) alphabet"""
    table = {}
    for ch in _fold(''.join(alphabet), fold_case):
        if ch not in table:
            table[ch] = len(table)
    if len(table) > ALPHABET_MAX:
        raise ValueError('an alphabet holds at most %d symbols, got %d' % (ALPHABET_MAX, len(table)))
    return table


def _codes(word, table, fold_case, unknown):
    return [table.get(ch, unknown) for ch in _fold(word, fold_case)]


def encode_words(words, alphabet, fold_case=True):
    """lexicon words -> (pool uint8, offsets int32 [L + 1]); characters outside the alphabet become UNKNOWN_WORD"""
    table = code_table(alphabet, fold_case)
    rows = [_codes(w, table, fold_case, UNKNOWN_WORD) for w in words]
    for w, r in zip(words, rows):
        if len(r) > WORD_MAX:
            raise ValueError('a lexicon word holds at most %d characters, got %d: %r' % (WORD_MAX, len(r), w[:40]))
    lens = np.asarray([len(r) for r in rows], dtype=np.int64)
    if len(rows) >= 1 << 31 or int(lens.sum()) >= 1 << 31:
        raise ValueError('a lexicon holds fewer than 2^31 words and characters')
    offsets = np.zeros(len(rows) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(lens)
    pool = np.asarray([c for r in rows for c in r], dtype=np.uint8)
    return pool, offsets


def encode_queries(queries, alphabet, fold_case=True):
    """query strings -> (codes uint8 [N, 64], q_len int32 [N]); characters outside the alphabet become UNKNOWN_QUERY"""
    table = code_table(alphabet, fold_case)
    codes = np.zeros((len(queries), QUERY_MAX), dtype=np.uint8)
    q_len = np.zeros(len(queries), dtype=np.int32)
    for i, q in enumerate(queries):
        r = _codes(q, table, fold_case, UNKNOWN_QUERY)
        if len(r) > QUERY_MAX:
            raise ValueError('a query holds at most %d characters, got %d: %r' % (QUERY_MAX, len(r), q[:80]))
        codes[i, :len(r)] = r
        q_len[i] = len(r)
    return codes, q_len


def _union_alphabet(queries, lexicon, fold_case):
    seen = {}
    for w in list(lexicon) + list(queries):
        for ch in _fold(w, fold_case):
            seen.setdefault(ch, None)
    return ''.join(seen)


def _check_ranges(ranges, n, L):
    """None or N (lo, hi) pairs -> int32 [N, 2] inside [0, L] (an inverted range counts as empty) or None"""
    if ranges is None:
        return None
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    if r.shape[0] != n:
        raise ValueError('%d ranges for %d queries' % (r.shape[0], n))
    return np.clip(r, 0, L).astype(np.int32)


class _Padded(object):
    """the lexicon as the numpy oracle walks it: a [L, longest] code matrix and the words ordered by falling length, so that
    the words still running at character j are a prefix of that order"""

    def __init__(self, pool, offsets):
        offsets = np.asarray(offsets, dtype=np.int64)
        self.lens = (offsets[1:] - offsets[:-1]).astype(np.int64)
        self.L = int(self.lens.size)
        width = int(self.lens.max()) if self.L else 0
        self.mat = np.zeros((self.L, max(width, 1)), dtype=np.uint8)
        if width:
            col = np.arange(width)[None, :]
            live = col < self.lens[:, None]
            self.mat[live] = np.asarray(pool, dtype=np.uint8)[:int(offsets[-1])]
        self.order = np.argsort(-self.lens, kind='stable')

    def distances(self, q, sel=None):
        """q: the query's codes (uint8 [m]).  sel: word indices ordered by falling length (default: all).  -> int64 [len(sel)]
        distances, in the order of sel"""
        sel = self.order if sel is None else sel
        lens = self.lens[sel]
        m = int(len(q))
        if m == 0 or sel.size == 0:
            return lens.copy()
        peq = np.zeros(256, dtype=np.uint64)
        for i, c in enumerate(np.asarray(q).tolist()):
            if c < UNKNOWN_QUERY:
                peq[c] |= np.uint64(1 << i)
        one, top = np.uint64(1), np.uint64(m - 1)
        Pv = np.full(sel.size, ~np.uint64(0), dtype=np.uint64)
        Mv = np.zeros(sel.size, dtype=np.uint64)
        score = np.full(sel.size, m, dtype=np.int64)
        alive = np.searchsorted(-lens, -np.arange(int(lens[0])), side='left')   # words longer than j
        for j in range(int(lens[0])):
            n = int(alive[j])
            pv, mv = Pv[:n], Mv[:n]
            Eq = peq[self.mat[sel[:n], j]]
            Xv = Eq | mv
            Xh = (((Eq & pv) + pv) ^ pv) | Eq
            Ph = mv | ~(Xh | pv)
            Mh = pv & Xh
            score[:n] += ((Ph >> top) & one).astype(np.int64)
            score[:n] -= ((Mh >> top) & one).astype(np.int64)
            Ph = (Ph << one) | one
            Mh = Mh << one
            Pv[:n] = Mh | ~(Xv | Ph)
            Mv[:n] = Ph & Xv
        return score


def nearest_encoded_cpu(q_codes, q_len, pool, offsets, ranges=None, with_distances=False):
    """The specification on encoded operands: -> (idx int32 [N], dist int32 [N]); (-1, -1) for an empty range.
    with_distances: also a list with every query's distances to its whole range (int64 [hi - lo], lexicon order)."""
    lex = _Padded(pool, offsets)
    N = len(q_len)
    rng = _check_ranges(ranges, N, lex.L)
    idx = np.full(N, -1, dtype=np.int32)
    dist = np.full(N, -1, dtype=np.int32)
    every = []
    for i in range(N):
        m = int(q_len[i])
        if m < 0 or m > QUERY_MAX:
            raise ValueError('query %d holds %d codes' % (i, m))
        if rng is None:
            sel = lex.order
        else:
            lo, hi = int(rng[i, 0]), int(rng[i, 1])
            sel = lex.order[(lex.order >= lo) & (lex.order < hi)]
        d = lex.distances(np.asarray(q_codes[i][:m]), sel)
        if with_distances:
            full = np.empty(sel.size, dtype=np.int64)
            full[np.argsort(np.argsort(sel, kind='stable'), kind='stable')] = d
            every.append(full)
        if sel.size:
            key = (d << 32) | sel           # the kernel's key: least distance, then least index
            k = int(key.min())
            idx[i], dist[i] = k & 0xffffffff, k >> 32
    return (idx, dist, every) if with_distances else (idx, dist)


def nearest_cpu(queries, lexicon, ranges=None, fold_case=True, alphabet=None):
    """For each query string the nearest lexicon word inside its range [lo, hi) of lexicon indices (default: the whole
    lexicon), ties to the lowest index -> (idx int32 [N], dist int32 [N]); an empty range gives (-1, -1).
    alphabet=None: every character that occurs is its own symbol; with an alphabet, characters outside it match nothing."""
    queries, lexicon = list(queries), list(lexicon)
    if alphabet is None:
        alphabet = _union_alphabet(queries, lexicon, fold_case)
    pool, offsets = encode_words(lexicon, alphabet, fold_case)
    q_codes, q_len = encode_queries(queries, alphabet, fold_case)
    return nearest_encoded_cpu(q_codes, q_len, pool, offsets, ranges)


def accept(dist, q_len, max_dist=None, max_ratio=None):
    """the host's acceptance rule: a match is rejected when dist > max_dist or dist > floor(max_ratio * len(query));
    len(query) counts the query's codes.  No match (dist < 0) is never accepted."""
    if dist < 0:
        return False
    if max_dist is not None and dist > max_dist:
        return False
    if max_ratio is not None and dist > int(np.floor(max_ratio * q_len)):
        return False
    return True


def unpack_best(best):
    """uint64 keys (dist << 32) | idx, all ones = none -> (idx int32, dist int32) with (-1, -1) for none"""
    b = np.asarray(best).view(np.uint64)
    none = b == np.uint64(NONE_KEY)
    idx = (b & np.uint64(0xffffffff)).astype(np.int64)
    dist = (b >> np.uint64(32)).astype(np.int64)
    idx[none], dist[none] = -1, -1
    return idx.astype(np.int32), dist.astype(np.int32)


class LexiconMatcher(object):
    """A lexicon on the device.  The constructor encodes and uploads it once and keeps the spellings; a call takes query
    strings and answers, per query, (word or None, idx, dist) -- the nearest word of the query's range, the lowest index
    among equals; (None, -1, -1) for an empty range.  Per chunk of `chunk` queries (65 536 by default): one upload (lengths,
    ranges and codes in one block), one omp_lexicon_nearest, one download."""

    def __init__(self, device, words, alphabet=None, fold_case=True, chunk=65536):
        import torch
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('LexiconMatcher runs on MI355X only (got device %s); there is no CPU fallback -- '
                               'nearest_cpu is the host specification' % (self.device,))
        self.words = list(words)
        if not self.words:
            raise ValueError('an empty lexicon')
        self.alphabet = default_alphabet() if alphabet is None else alphabet
        self.fold_case = bool(fold_case)
        self.chunk = int(chunk)
        pool, offsets = encode_words(self.words, self.alphabet, self.fold_case)
        self.pool_bytes = int(pool.size)
        # eight spare bytes so that an all-empty-word lexicon still owns an allocation; the kernel is told pool_bytes
        self.pool = torch.from_numpy(np.concatenate([pool, np.zeros(8, dtype=np.uint8)])).to(self.device)
        self.offsets = torch.from_numpy(offsets).to(self.device)
        self.L = len(self.words)
        self._ranges = None
        self.last_chunks = 0

    @classmethod
    def from_lists(cls, device, lists, alphabet=None, fold_case=True, chunk=65536):
        """one lexicon per image: the lists back to back in one device lexicon; range_of(i) is list i's [lo, hi)"""
        lists = [list(w) for w in lists]
        m = cls(device, [w for ws in lists for w in ws], alphabet, fold_case, chunk)
        m._ranges = list_ranges(lists)
        return m

    @property
    def n_lists(self):
        return None if self._ranges is None else len(self._ranges)

    def range_of(self, i):
        if self._ranges is None:
            raise ValueError('this matcher was not built from per-image lists (LexiconMatcher.from_lists)')
        return self._ranges[i]

    def nearest(self, queries, ranges=None):
        """-> (idx int32 [N], dist int32 [N], q_len int32 [N]) as nearest_cpu"""
        import torch

        from .. import ops
        queries = list(queries)
        N = len(queries)
        codes, q_len = encode_queries(queries, self.alphabet, self.fold_case)
        rng = _check_ranges(ranges, N, self.L)
        idx = np.full(N, -1, dtype=np.int32)
        dist = np.full(N, -1, dtype=np.int32)
        self.last_chunks = 0
        with torch.cuda.device(self.device):
            for i0 in range(0, N, self.chunk):
                i1 = min(N, i0 + self.chunk)
                n = i1 - i0
                parts = [q_len[i0:i1].view(np.uint8)]
                if rng is not None:
                    parts += [np.ascontiguousarray(rng[i0:i1, 0]).view(np.uint8), np.ascontiguousarray(rng[i0:i1, 1]).view(np.uint8)]
                parts.append(codes[i0:i1].reshape(-1))
                blob = torch.from_numpy(np.concatenate(parts)).to(self.device)        # the chunk's one upload
                ints = blob[:(4 * n) * (3 if rng is not None else 1)].view(torch.int32)
                q_codes = blob[blob.numel() - n * QUERY_MAX:].view(n, QUERY_MAX)
                hint = int((rng[i0:i1, 1] - rng[i0:i1, 0]).max()) if rng is not None else 0
                best = ops.lexicon_nearest(q_codes, ints[:n], ints[n:2 * n] if rng is not None else None,
                                           ints[2 * n:3 * n] if rng is not None else None, self.pool, self.pool_bytes, self.offsets,
                                           self.L, range_hint=max(hint, 0))
                idx[i0:i1], dist[i0:i1] = unpack_best(best.cpu().numpy())            # the chunk's one download
                self.last_chunks += 1
        return idx, dist, q_len

    def __call__(self, queries, ranges=None, max_dist=None, max_ratio=None):
        """-> list of (word | None, idx, dist).  The nearest word is always reported by idx and dist; the word itself is
        None when the match is rejected: dist > max_dist, or dist > floor(max_ratio * len(query))."""
        idx, dist, q_len = self.nearest(queries, ranges)
        out = []
        for i, d, m in zip(idx.tolist(), dist.tolist(), q_len.tolist()):
            out.append((self.words[i] if accept(d, m, max_dist, max_ratio) else None, i, d))
        return out


def list_ranges(lists):
    """per-image word lists laid back to back -> [(lo, hi)] per list"""
    out, lo = [], 0
    for ws in lists:
        out.append((lo, lo + len(ws)))
        lo += len(ws)
    return out


# ---------------------------------------------------------------------------------------------
# the engine's side: `lexicon=` of predict / predict_images / spot_and_recognize
# ---------------------------------------------------------------------------------------------
def is_matcher(obj):
    return callable(obj) and hasattr(obj, 'range_of')


def resolve_lexicon(lexicon, n_images, device, alphabet, fold_case=True):
    """`lexicon=` as the engine entry points take it -> a matcher.  A matcher passes through (one built from per-image
    lists must hold one list per image of the call); a list of words becomes a matcher shared by all images; a list of
    word lists, one per image, becomes LexiconMatcher.from_lists.  Built on `device` with `alphabet` for this call."""
    if is_matcher(lexicon):
        m = lexicon
    else:
        items = list(lexicon)
        if items and all(isinstance(w, str) for w in items):
            m = LexiconMatcher(device, items, alphabet, fold_case)
        elif items and not any(isinstance(w, str) for w in items):
            m = LexiconMatcher.from_lists(device, items, alphabet, fold_case)
        else:
            raise ValueError('lexicon is a LexiconMatcher, a non-empty list of words or a list of word lists (one per image)')
    n = getattr(m, 'n_lists', None)
    if n is not None and n != n_images:
        raise ValueError('%d per-image lexicons for %d images' % (n, n_images))
    return m


def annotate_records(records, matcher, source='rec', prefix='lex', max_dist=None, max_ratio=None):
    """records: per image a list of record dicts.  Every record gains `prefix` (the accepted word or None),
    `prefix_index` (the nearest word's index -- in its image's own list for per-image lexicons -- or -1) and
    `prefix_dist`, from its `source` string.  ALL words of the call go through ONE matcher call."""
    per_image = getattr(matcher, 'n_lists', None) is not None
    owners, queries, ranges = [], [], []
    for b, recs in enumerate(records):
        for r in recs:
            owners.append(r)
            queries.append(r[source])
            if per_image:
                ranges.append(tuple(matcher.range_of(b)))
    if not owners:
        return records
    res = matcher(queries, ranges=ranges if per_image else None, max_dist=max_dist, max_ratio=max_ratio)
    for k, (r, (word, idx, dist)) in enumerate(zip(owners, res)):
        r[prefix] = word
        r[prefix + '_index'] = idx - ranges[k][0] if per_image and idx >= 0 else idx
        r[prefix + '_dist'] = dist
    return records
