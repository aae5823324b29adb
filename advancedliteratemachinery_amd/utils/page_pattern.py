"""Page patterns: dates, amounts and ids in the text of read pages.

utils/page_search.py finds a literal phrase; this module finds a SHAPE: a sequence of 1 .. 64 positions, each a character class, each
mandatory or optional, with up to k errors (insert / delete / substitute cost 1; skipping an optional position is free).  A job is one
(page, pattern) pair.  The numpy / Python functions here are the DEFINITION; csrc/page_pattern.hip (omp_page_pattern_search) equals
search_cpu on every integer.

Syntax      parse_pattern(): atoms are a literal, an escaped literal, `.`, \\d \\D \\w \\W \\s \\S and [...] / [^...]; one atom takes one
            of the quantifiers ?, {n}, {a,b}; * and + mean {0,rep_max} / {1,rep_max} and need rep_max.  x{a,b} becomes a mandatory and
            b - a optional positions.  Groups, |, anchors, back-references and lazy quantifiers are refused.  1 <= P <= 64 positions
            after expansion, Mand >= 1 of them mandatory.  The parser tokenises only: whether a character is in an atom is decided by
            Python's re (re.compile(atom, re.DOTALL).fullmatch(ch)).
Codes       encode_patterns(): a page character's signature is the tuple of its memberships in every distinct atom of the call;
            signatures get the dense codes 0 .. sigma - 1 (sigma <= 254) in order of first appearance.  Per pattern mask uint64
            [sigma + 1]: bit i of mask[c] says that code c is in the class of position i; row sigma is 0 and stands for every code at
            or above sigma.  opt uint64: bit i says that position i is optional.
Table       D[0][j] = 0, D[i][0] = D[i-1][0] + skip_i, D[i][j] = min(D[i-1][j-1] + (t_j not in C_i), D[i-1][j] + skip_i, D[i][j-1] + 1)
            with skip_i = 0 for an optional position and 1 for a mandatory one; v_j = min(D[P][j], k + 1): clipped, so what lies above
            the tolerance is never compared.
Tolerance   tolerance(): k = min(Mand - 1, (permille(max_ratio) * Mand) // 1000, max_dist, K_MAX = 8): the empty match never qualifies.
A hit       page_search's rule on the clipped v: an end j in 1 .. n with v_j <= k, v_j <= v_{j-1} and (j == n or v_j < v_{j+1}).
best        (min v, the least end that attains it), or (k + 1, 0) when nothing is within k.
hits        int32 [J, H, 3] = (end, dist, start) in ascending end, -1 beyond the hits; n_hits counts all hits.
start       the LEAST s >= end - (P + dist) whose anchored cost (the same table with D[0][j] = j) of the pattern against t[s:end] equals
            dist: the LONGEST match, the POSIX convention.  This deliberately differs from page_search's shortest match, which would
            return 5 for \\d{1,4} in `12345`: a field's value is wanted whole.
Limits      a page 0 .. 65535 characters, 1 .. 2^20 jobs a call, 1 .. 64 hits kept per job.
"""
import re
import warnings

import numpy as np

from .page_search import HITS_MAX, JOBS_MAX, SCRATCH_CAP, hit_ends
from .page_text import LEN_MAX, SIGMA_MAX, _DeviceStage

POS_MAX = 64                    # positions a pattern (csrc/page_frame.h: PG_POS_MAX): one 64-bit word per row
K_MAX = 8                       # errors at the most (csrc/page_pattern.hip: PP_K_MAX): k + 1 <= 9 rows live in registers
CHUNK = 128                     # text columns per lane (csrc/page_frame.h: PG_CHUNK)
_FULL = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------
# syntax
# ---------------------------------------------------------------------------------------------
class Pattern(object):
    """a parsed pattern: src, atoms (one re source per position), optional (one bool per position), P, Mand, opt (the bit word)"""

    def __init__(self, src, atoms, optional):
        self.src, self.atoms, self.optional = src, tuple(atoms), tuple(bool(o) for o in optional)
        self.P = len(self.atoms)
        self.Mand = self.P - sum(self.optional)
        self.opt = sum(1 << i for i, o in enumerate(self.optional) if o)

    def __repr__(self):
        return 'Pattern(%r, P=%d, Mand=%d)' % (self.src, self.P, self.Mand)


_CLASS_ESCAPES = 'dDwWsS'
_ANCHOR_ESCAPES = 'bBAZ'


def _compiled(atom):
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        return re.compile(atom, re.DOTALL)


def parse_pattern(src, rep_max=None):
    """a pattern as the caller wrote it -> Pattern.  rep_max: what `*`, `+` and `{a,}` repeat to at the most (None: they are refused).
    Every refusal is a ValueError that names the pattern and the offset."""
    if isinstance(src, Pattern):
        return src
    if not isinstance(src, str):
        raise ValueError('a pattern must be a string, got %r' % (src,))
    if rep_max is not None and int(rep_max) < 1:
        raise ValueError('rep_max must be at least 1, got %r' % (rep_max,))

    def bad(at, what):
        return ValueError('pattern %r, offset %d: %s' % (src, at, what))

    atoms, optional = [], []
    i, n = 0, len(src)
    while i < n:
        at, ch = i, src[i]
        if ch == '\\':
            if i + 1 >= n:
                raise bad(at, 'a backslash at the end')
            e = src[i + 1]
            if e.isdigit():
                raise bad(at, 'back-references are not supported')
            if e in _ANCHOR_ESCAPES:
                raise bad(at, 'anchors and word boundaries are not supported')
            atom = src[i:i + 2]
            if e not in _CLASS_ESCAPES:                                          # an escaped literal, \n, \t, ...: re says which exist
                try:
                    _compiled(atom)
                except (re.error, Warning):
                    raise bad(at, 'the escape %r is not supported' % atom)
            i += 2
        elif ch == '[':
            j = i + 1
            if j < n and src[j] == '^':
                j += 1
            if j < n and src[j] == ']':
                j += 1
            while j < n and src[j] != ']':
                j += 2 if src[j] == '\\' else 1
            if j >= n:
                raise bad(at, 'a character class that is not closed')
            atom = src[i:j + 1]
            try:
                _compiled(atom)
            except (re.error, Warning) as e:
                raise bad(at, 'the character class %r is refused by re: %s' % (atom, e))
            i = j + 1
        elif ch in '()':
            raise bad(at, 'groups and captures are not supported')
        elif ch == '|':
            raise bad(at, 'alternation is not supported')
        elif ch in '^$':
            raise bad(at, 'anchors are not supported')
        elif ch in '*+?{':
            raise bad(at, 'a quantifier with nothing to repeat')
        elif ch == '}':
            raise bad(at, 'a brace that closes nothing (write \\})')
        else:
            atom = '\\' + ch if ch in ']' else ch
            i += 1
        # ---- the quantifier of this atom ----
        lo, hi = 1, 1
        if i < n and src[i] in '*+?{':
            qat, q = i, src[i]
            if q == '?':
                lo, hi, i = 0, 1, i + 1
            elif q in '*+':
                if rep_max is None:
                    raise bad(qat, '`%s` is unbounded repetition: give rep_max, or write {a,b}' % q)
                lo, hi, i = (0 if q == '*' else 1), int(rep_max), i + 1
            else:
                m = re.compile(r'\{(\d*)(,?)(\d*)\}').match(src, i)
                if m is None or (m.group(1) == '' and m.group(3) == ''):
                    raise bad(qat, 'a brace that is no {n} or {a,b} quantifier (write \\{)')
                a, comma, b = m.groups()
                lo = int(a) if a else 0
                if not comma:
                    hi = lo
                elif b:
                    hi = int(b)
                elif rep_max is None:
                    raise bad(qat, '`{%s,}` is unbounded repetition: give rep_max, or write {a,b}' % a)
                else:
                    hi = max(lo, int(rep_max))
                if hi < lo:
                    raise bad(qat, 'a quantifier {a,b} with b < a')
                i = m.end()
            if i < n and src[i] in '?+':
                raise bad(i, 'lazy and possessive quantifiers are not supported')
            if i < n and src[i] in '*{':
                raise bad(i, 'a quantifier on a quantifier')
        if len(atoms) + hi > POS_MAX:
            raise bad(at, 'the pattern holds more than %d positions after expansion' % POS_MAX)
        atoms += [atom] * hi
        optional += [False] * lo + [True] * (hi - lo)
    if not atoms:
        raise bad(0, 'the pattern holds no position')
    if all(optional):
        raise bad(0, 'every position is optional: the pattern would match the empty string')
    return Pattern(src, atoms, optional)


def tolerance(mand, max_dist=None, max_ratio=0.0):
    """the tolerance k of a pattern with `mand` mandatory positions: min(mand - 1, (permille(max_ratio) * mand) // 1000, max_dist, K_MAX);
    None leaves a bound out"""
    mand = int(mand)
    if not 1 <= mand <= POS_MAX:
        raise ValueError('a pattern holds 1 .. %d mandatory positions, got %d' % (POS_MAX, mand))
    k = min(mand - 1, K_MAX)
    if max_ratio is not None:
        r = float(max_ratio)
        if not 0.0 <= r <= 1.0:
            raise ValueError('max_ratio must be a float in [0, 1], got %r' % (max_ratio,))
        k = min(k, (int(round(1000 * r)) * mand) // 1000)
    if max_dist is not None:
        if int(max_dist) < 0:
            raise ValueError('max_dist must be at least 0, got %r' % (max_dist,))
        k = min(k, int(max_dist))
    return k


# ---------------------------------------------------------------------------------------------
# codes
# ---------------------------------------------------------------------------------------------
def encode_classes(page_texts, atom_rows):
    """what encode_patterns and page_regex.encode_regex share: page texts and, per pattern, the re sources of its positions -> (pool uint8,
    page_off, page_len int32 [pages], masks uint64 [Q, sigma + 1], sigma).  A page character's signature is the tuple of its memberships in
    every distinct atom of the call; signatures get the dense codes in order of first appearance.  Equal page texts share one pool range."""
    page_texts, atom_rows = list(page_texts), [tuple(r) for r in atom_rows]
    for t in page_texts:
        if len(t) > LEN_MAX:
            raise ValueError('a page text holds %d characters; the limit is %d' % (len(t), LEN_MAX))
    atoms = {}
    for row in atom_rows:
        for a in row:
            if a not in atoms:
                atoms[a] = (len(atoms), _compiled(a))
    tests = [rx for _, rx in atoms.values()]
    code_of, sigs = {}, {}
    for t in page_texts:
        for ch in t:
            if ch not in code_of:
                sig = tuple(rx.fullmatch(ch) is not None for rx in tests)
                code_of[ch] = sigs.setdefault(sig, len(sigs))
    sigma = len(sigs)
    if sigma > SIGMA_MAX:
        raise ValueError('the page characters fall into %d classes under these patterns; a call takes %d' % (sigma, SIGMA_MAX))
    chunks, total, seen, off = [], 0, {}, []
    for t in page_texts:
        if t not in seen:
            seen[t] = total
            chunks.append(np.fromiter((code_of[ch] for ch in t), dtype=np.uint8, count=len(t)))
            total += len(t)
        off.append(seen[t])
    if total > 0x7fffffff:
        raise ValueError('the pages of a call hold %d characters; a pool takes 2^31 - 1' % total)
    member = np.zeros((sigma + 1, max(len(atoms), 1)), dtype=bool)                # [code, atom]; row sigma: in no class
    for sig, c in sigs.items():
        member[c, :len(sig)] = sig
    masks = np.zeros((len(atom_rows), sigma + 1), dtype=np.uint64)
    for q, row in enumerate(atom_rows):
        for i, a in enumerate(row):
            masks[q] |= member[:, atoms[a][0]].astype(np.uint64) << np.uint64(i)
    i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(-1)                   # noqa: E731
    return np.concatenate(chunks + [np.zeros(0, np.uint8)]).astype(np.uint8), i32(off), i32([len(t) for t in page_texts]), masks, sigma


def encode_patterns(page_texts, patterns):
    """page texts and Q patterns (Pattern objects, or strings parsed without rep_max) -> (pool uint8, page_off, page_len int32 [pages],
    masks uint64 [Q, sigma + 1], opt uint64 [Q], pat_len int32 [Q], sigma).  Equal page texts share one pool range."""
    patterns = [parse_pattern(p) for p in patterns]
    pool, page_off, page_len, masks, sigma = encode_classes(page_texts, [p.atoms for p in patterns])
    return (pool, page_off, page_len, masks, np.asarray([p.opt for p in patterns], dtype=np.uint64).reshape(-1),
            np.asarray([p.P for p in patterns], dtype=np.int32).reshape(-1), sigma)


# ---------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------
def _pattern(mask, opt, P):
    mask, opt, P = np.asarray(mask, dtype=np.uint64).reshape(-1), int(opt), int(P)
    if not 1 <= P <= POS_MAX:
        raise ValueError('a pattern takes 1 .. %d positions, got %d' % (POS_MAX, P))
    if mask.size < 1:
        raise ValueError('a mask table holds sigma + 1 >= 1 words')
    if opt >> P or opt < 0:
        raise ValueError('opt holds bits at or above P = %d' % P)
    if bin(opt).count('1') >= P:
        raise ValueError('every position is optional')
    return mask, opt, P


def _classes(mask, t):
    """the class word of every text character: codes at or above sigma read row sigma"""
    t = np.asarray(t, dtype=np.uint8).reshape(-1)
    if t.size > LEN_MAX:
        raise ValueError('a text holds %d codes; the limit is %d' % (t.size, LEN_MAX))
    return mask[np.minimum(t.astype(np.int64), mask.size - 1)]


def row_py(mask, opt, P, t, anchored=False):
    """D[P][0 .. n], unclipped, by the plain double loop -- the ground truth, for tiny cases only"""
    mask, opt, P = _pattern(mask, opt, P)
    B = [int(b) for b in _classes(mask, t)]
    prev = list(range(len(B) + 1)) if anchored else [0] * (len(B) + 1)
    for i in range(P):
        skip = 0 if (opt >> i) & 1 else 1
        cur = [prev[0] + skip] + [0] * len(B)
        for j, b in enumerate(B, 1):
            cur[j] = min(prev[j - 1] + (0 if (b >> i) & 1 else 1), prev[j] + skip, cur[j - 1] + 1)
        prev = cur
    return np.asarray(prev, dtype=np.int32)


def row_cpu(mask, opt, P, t, anchored=False, reverse=False):
    """D[P][0 .. n], unclipped, int32 [n + 1]: by rows of the pattern, vectorised over the text; the left dependency closes with
    minimum.accumulate(a - j) + j, as in page_text._rows.  anchored: row 0 is 0, 1, 2, ... instead of zeros.  reverse: the positions
    are taken from the last to the first (the caller reverses the text)."""
    mask, opt, P = _pattern(mask, opt, P)
    B = _classes(mask, t)
    ar = np.arange(B.size + 1, dtype=np.int32)
    prev = ar if anchored else np.zeros(B.size + 1, dtype=np.int32)
    for i in (range(P - 1, -1, -1) if reverse else range(P)):
        skip = 0 if (opt >> i) & 1 else 1
        differs = 1 - ((B >> np.uint64(i)) & np.uint64(1)).astype(np.int32)
        new = np.empty(B.size + 1, dtype=np.int32)
        new[0] = prev[0] + skip
        np.minimum(prev[1:] + skip, prev[:-1] + differs, out=new[1:])
        prev = np.minimum.accumulate(new - ar) + ar
    return prev


def closure_words(opt):
    """the words of the closure over optional positions -> (lead, A, I, F): the leading optional run; the optional bits; the bit
    before each run -- for the leading run, which has none, its own first bit --; the last bit of each run.  Df = X | F;
    X |= A & (~(Df - I) ^ Df) sets, per run, every bit above the lowest one that X holds in it or just before it: the borrow of a
    run stops at its F bit.  The search sets the leading run outright (the empty prefix stands at every column); the anchored walk
    does not, and there the leading run is a run like the others."""
    opt = int(opt)
    return opt & ~(opt + 1), opt, ((opt >> 1) & ~opt) | (opt & 1), opt & ~(opt >> 1)


def row_bits(mask, opt, P, t, k):
    """v_0 .. v_n, CLIPPED at k + 1, by the column step the kernel runs: Wu and Manber's rows R_0 .. R_k, one 64-bit word each (bit i
    of R_d: a prefix of i + 1 positions ends here with at most d errors), closed over the optional positions with Navarro and
    Raffinot's three words.  Python integers; equals minimum(row_py, k + 1)."""
    mask, opt, P = _pattern(mask, opt, P)
    lead, A, I, F = closure_words(opt)
    k = int(k)

    def cl(X):
        X |= lead
        Df = X | F
        return (X | (A & ((~(Df - I)) ^ Df))) & _FULL

    def value(R):
        return next((d for d in range(k + 1) if (R[d] >> (P - 1)) & 1), k + 1)

    R = [cl(0)]
    for d in range(1, k + 1):
        R.append(cl(R[d - 1] | ((R[d - 1] << 1) | 1)))
    out = [value(R)]
    for b in _classes(mask, t).tolist():
        b = int(b)
        new = [cl(((R[0] << 1) | 1) & b)]
        for d in range(1, k + 1):
            new.append(cl((((R[d] << 1) | 1) & b) | R[d - 1] | ((R[d - 1] << 1) | 1) | ((new[d - 1] << 1) | 1)))
        R = new
        out.append(value(R))
    return np.asarray(out, dtype=np.int32)


def _reverse_bits(x, P):
    return int(bin(int(x) | (1 << P))[:2:-1], 2) & ((1 << P) - 1)


def start_bits(mask, opt, P, t, end, dist):
    """match_start by the walk the kernel runs: the rows of the REVERSED pattern over t[end-1], t[end-2], ..., anchored.  The fresh
    column is the search's; its empty prefix feeds the first step's match and substitution and nothing after that -- neither a `| 1` nor
    the leading run: a match that ends in an inserted character costs more than dist at a hit, because v_end <= v_{end-1}.  The anchored
    cost is never below dist, so `R_dist holds bit P - 1` says that it equals dist; the LAST such l within min(end, P + dist) is kept."""
    mask, opt, P = _pattern(mask, opt, P)
    end, dist = int(end), int(dist)
    lead, A, I, F = closure_words(_reverse_bits(opt, P))

    def cl(X, first=False):
        if first:
            X |= lead
        Df = X | F
        return (X | (A & ((~(Df - I)) ^ Df))) & _FULL

    R = [cl(0, True)]
    for d in range(1, dist + 1):
        R.append(cl(R[d - 1] | ((R[d - 1] << 1) | 1), True))
    found = 0
    back = _classes(mask, np.asarray(t, dtype=np.uint8).reshape(-1)[max(0, end - (P + dist)):end][::-1]).tolist()
    for l, b in enumerate(back, 1):
        b, e = _reverse_bits(b, P), int(l == 1)
        new = [cl(((R[0] << 1) | e) & b)]
        for d in range(1, dist + 1):
            new.append(cl((((R[d] << 1) | e) & b) | R[d - 1] | ((R[d - 1] << 1) | e) | (new[d - 1] << 1)))
        R = new
        if (R[dist] >> (P - 1)) & 1:
            found = l
    if not found:
        raise AssertionError('no start within P + dist characters of end %d' % end)
    return end - found


def match_start(mask, opt, P, t, end, dist):
    """the least s >= end - (P + dist) whose anchored cost of the pattern against t[s:end] equals dist (the longest match): the anchored
    row of the reversed pattern over t[end-1], t[end-2], ...; the LAST l whose value equals dist"""
    end, dist = int(end), int(dist)
    lo = max(0, end - (int(P) + dist))
    r = row_cpu(mask, opt, P, np.asarray(t, dtype=np.uint8).reshape(-1)[lo:end][::-1], anchored=True, reverse=True)
    at = np.flatnonzero(r == dist)
    if at.size == 0:
        raise AssertionError('no start within P + dist characters of end %d' % end)
    return end - int(at[-1])


def _check_search(pool, page_off, page_len, masks, opt, pat_len, jobs, k, max_hits):
    pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1)
    po, pl, P, k = [np.asarray(t, dtype=np.int64).reshape(-1) for t in (page_off, page_len, pat_len, k)]
    opt = np.ascontiguousarray(opt, dtype=np.uint64).reshape(-1)
    masks = np.ascontiguousarray(masks, dtype=np.uint64)
    jobs = np.asarray(jobs, dtype=np.int64).reshape(-1, 2)
    if po.size != pl.size:
        raise ValueError('page_off and page_len hold one entry per page, got %d and %d' % (po.size, pl.size))
    if masks.ndim != 2 or masks.shape[1] < 1 or masks.shape[1] > SIGMA_MAX + 1 or not (masks.shape[0] == opt.size == P.size == k.size):
        raise ValueError('masks [Q, sigma + 1], opt, pat_len and k hold one entry per pattern, got %s, %d, %d and %d'
                         % (masks.shape, opt.size, P.size, k.size))
    max_hits = int(max_hits)
    if not 1 <= max_hits <= HITS_MAX:
        raise ValueError('max_hits must be 1 .. %d, got %d' % (HITS_MAX, max_hits))
    if jobs.shape[0] > JOBS_MAX:
        raise ValueError('a call takes %d jobs, got %d' % (JOBS_MAX, jobs.shape[0]))
    if pl.size and ((pl < 0).any() or (pl > LEN_MAX).any()):
        raise ValueError('a page length is outside 0 .. %d' % LEN_MAX)
    if po.size and ((po < 0).any() or (po + pl > pool.size).any()):
        raise ValueError('a range lies outside the pool of %d codes' % pool.size)
    if P.size and ((P < 1).any() or (P > POS_MAX).any()):
        raise ValueError('a pattern length is outside 1 .. %d' % POS_MAX)
    mand = np.asarray([int(p) - bin(int(o)).count('1') for p, o in zip(P.tolist(), opt.tolist())], dtype=np.int64)
    if any(int(o) >> int(p) for p, o in zip(P.tolist(), opt.tolist())) or (mand < 1).any():
        raise ValueError('an opt word holds bits at or above P, or leaves no mandatory position')
    if k.size and ((k < 0).any() or (k > np.minimum(mand - 1, K_MAX)).any()):
        raise ValueError('a tolerance is outside 0 .. min(Mand - 1, %d)' % K_MAX)
    if jobs.size and ((jobs < 0).any() or (jobs[:, 0] >= pl.size).any() or (jobs[:, 1] >= P.size).any()):
        raise ValueError('a job names a page or a pattern that is not there')
    return [pool, po.astype(np.int32), pl.astype(np.int32), masks, opt, P.astype(np.int32), np.ascontiguousarray(jobs.astype(np.int32)), k.astype(np.int32),
            max_hits]


def search_cpu(pool, page_off, page_len, masks, opt, pat_len, jobs, k, max_hits):
    """the definition, for the flat inputs omp_page_pattern_search takes -> dict(best int32 [J, 2] = (dist, end), n_hits int32 [J],
    hits int32 [J, max_hits, 3] = (end, dist, start), -1 where there is no hit)"""
    pool, po, pl, masks, opt, P, jobs, k, H = _check_search(pool, page_off, page_len, masks, opt, pat_len, jobs, k, max_hits)
    J = jobs.shape[0]
    best = np.zeros((J, 2), dtype=np.int32)
    n_hits = np.zeros(J, dtype=np.int32)
    hits = np.full((J, H, 3), -1, dtype=np.int32)
    done = {}
    for j, (p, q) in enumerate(jobs.tolist()):
        key = (po[p], pl[p], q)
        if key not in done:
            t = pool[po[p]:po[p] + pl[p]]
            kq = int(k[q])
            v = np.minimum(row_cpu(masks[q], opt[q], P[q], t), kq + 1)
            end = int(np.argmin(v))                                           # the least j that attains the minimum; v_0 = k + 1
            ends = hit_ends(v, kq)
            rows = [(int(e), int(v[e]), match_start(masks[q], opt[q], P[q], t, int(e), int(v[e]))) for e in ends[:H].tolist()]
            done[key] = ((int(v[end]), end), int(ends.size), rows)
        b, c, rows = done[key]
        best[j] = b
        n_hits[j] = c
        if rows:
            hits[j, :len(rows)] = rows
    return dict(best=best, n_hits=n_hits, hits=hits)


def chunk_jobs(n_jobs, max_hits, scratch_cap=SCRATCH_CAP):
    """-> [(lo, hi)]: consecutive jobs whose scratch stays at or below scratch_cap bytes"""
    from ..ops import page_pattern_scratch_bytes
    one = page_pattern_scratch_bytes(1, max_hits)
    per = int(scratch_cap) // one
    if per < 1:
        raise ValueError('scratch_cap must hold one job (%d bytes at max_hits %d), got %d' % (one, max_hits, scratch_cap))
    return [(lo, min(lo + per, int(n_jobs))) for lo in range(0, int(n_jobs), per)]


class HostPatternSearcher(object):
    """PatternSearcher's `run` from the specification (search_cpu): what the device stage must equal"""

    def __init__(self):
        self.calls = 0

    def run(self, pool, page_off, page_len, masks, opt, pat_len, jobs, k, max_hits):
        self.calls += 1
        return search_cpu(pool, page_off, page_len, masks, opt, pat_len, jobs, k, max_hits)


# ---------------------------------------------------------------------------------------------
# the device stage
# ---------------------------------------------------------------------------------------------
class PatternSearcher(_DeviceStage):
    """search_cpu on the device.  A call is ONE packed upload of the tables and the pool, one omp_page_pattern_search launch per chunk
    of jobs (a chunk's scratch stays at or below scratch_cap; the scratch is cached and grown), and ONE download of best, n_hits and
    hits.  There is no CPU fallback: HostPatternSearcher is the specification."""
    HOST = 'HostPatternSearcher'

    def __init__(self, device, scratch_cap=SCRATCH_CAP):
        super().__init__(device, scratch_cap)
        chunk_jobs(1, 1, self.scratch_cap)       # the cap holds one job that keeps one hit; run() checks it against its max_hits

    def run(self, pool, page_off, page_len, masks, opt, pat_len, jobs, k, max_hits):
        """the inputs of search_cpu -> the dict of search_cpu, as numpy.  sigma is masks.shape[1] - 1."""
        from .. import ops
        pool, po, pl, masks, opt, P, jobs, k, H = _check_search(pool, page_off, page_len, masks, opt, pat_len, jobs, k, max_hits)
        return self._search(ops.page_pattern_search, (po, pl, masks, opt, P, k), pool, jobs, masks.shape[1] - 1, H,
                            chunk_jobs(jobs.shape[0], H, self.scratch_cap),
                            'omp_page_pattern_search refused a job (a length above the limits, a range outside the pool, opt bits at or above P, '
                            'or k above min(Mand - 1, %d))' % K_MAX, ops.page_pattern_scratch_bytes)
