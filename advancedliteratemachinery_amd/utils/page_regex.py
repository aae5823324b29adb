"""Page expressions: alternation, groups and unbounded repeats in the text of read pages.

utils/page_pattern.py finds a flat row of character classes with up to k errors; this module finds a regular EXPRESSION over the same
atoms, exactly (k = 0): groups, `|` at any depth and real loops.  A job is one (page, expression) pair.  The numpy / Python functions here
are the DEFINITION; csrc/page_regex.hip (omp_page_regex_search) equals search_cpu on every integer.

Syntax      parse_regex(): the atoms of parse_pattern (a literal, an escaped literal, `.`, \\d \\D \\w \\W \\s \\S, [...] / [^...]); groups
            ( ) and (?: ), both non-capturing; `|` at any depth; the quantifiers ? * + {n} {a,b} {a,} on an atom or a group.  * + and {a,}
            are real loops.  x{a,b} copies the positions of x: a mandatory copies and b - a optional ones; x{a,} is a copies with the loop
            on the last one (x* for a = 0).  Anchors, \\b \\B \\A \\Z, back-references, lazy and possessive quantifiers, a quantifier on a
            quantifier, empty groups or branches, any other (?...) extension, more than 64 positions after expansion and an expression
            that matches the empty string are refused.  Whether a character is in an atom is decided by Python's re
            (re.compile(atom, re.DOTALL).fullmatch(ch)).
Automaton   Glushkov's position automaton: one state per position 0 .. P - 1, P <= 64, no epsilon moves.  first / last: the positions a
            match can begin / end with; follow[i]: the positions that can come after position i; pred is follow transposed.  Bit i of
            the state word D says that a match prefix has just consumed a character at position i.
Codes       encode_regex(): the signature coding of page_pattern.encode_patterns (sigma <= 254, row sigma of a mask is 0).
Step        D_0 = 0, D_j = (Follow(D_{j-1}) | first) & B(t_j), Follow(D) = OR of follow[i] over the bits i of D, B(c) = mask[c].
            Column j (1-based) is an END iff D_j & last != 0.
A hit       page_search's rule on v_j = 0 at an end, else 1, v_0 = 1, k = 0: the LAST column of a run of consecutive ends.  `\\d+` on
            `12345 ` is one hit at 5.
best        (0, the least end), or (1, 0) when there is no end.
hits        int32 [J, H, 3] = (end, 0, start) in ascending end, -1 beyond the hits; n_hits counts all hits.
start       the LEAST s with t[s:end] in the language (the longest match, find_pattern's convention), by the reverse walk
            R = last & B(t_end); while R != 0: if R & first remember s; R = Pred(R) & B(t_{s-1}).  There is no span cap.
Split       ends_chunked(): the kernel's way over a page.  The step is linear over union, so a lane runs its chunk from D = 0 (the
            speculative pass), then takes the exit state of the lane before it and runs the bits it has not carried yet through its
            chunk WITHOUT injecting first, until no lane gets a new bit.
Limits      a page 0 .. 65535 characters, 1 .. 2^20 jobs a call, 1 .. 64 hits kept per job.

With errors (csrc/page_regex.hip, omp_page_regex_fuzzy_search, equals fuzzy_search_cpu on every integer):
Tolerance   k = regex_tolerance(min_len, max_dist, max_ratio) = min(page_pattern.tolerance(min_len, ...), K_MAX), min_len the length of the
            shortest word of the language: k <= min_len - 1, so deleting the whole expression never qualifies.
Rows        R_0 .. R_k, one word each.  Bit p of R_i after column j: some t[s:j] aligns, with at most i insertions, deletions and
            substitutions of cost 1, to a path of the automaton from first that ends at position p.  Fol(X) = Follow(X) | first:
              before any text  R_0 = 0, R_i = Fol(R_{i-1})
              column j         R'_0 = Fol(R_0) & B
                               R'_i = (Fol(R_i) & B) | Fol(R_{i-1}) | R_{i-1} | Fol(R'_{i-1})     match, substitution, insertion, deletion
            v_j = the least i with R'_i & last != 0, else k + 1; v_0 = k + 1.  dist_py is the same on sets of positions.
A hit       page_search.hit_ends(v, k); best = (min v, the least end that attains it) or (k + 1, 0); hits = (end, dist, start).
start       fuzzy_start(): the least s whose anchored distance of t[s:end] to the language equals dist: the same step backwards from
            `end` with rows 0 .. dist, Pred for Follow and last for first, the injection of row i gated by a flag G_i (the walk's own
            start state: 1 at `end`, G'_0 = 0, G'_i = G_{i-1}: it has consumed that many characters as insertions).  No span cap.
Split       dist_chunked(): the step is R' = L(R) | constant with L linear over union, so ends_chunked's speculative pass and carry
            rounds carry over with k + 1 words where there was one.
"""
import re
from collections import namedtuple

import numpy as np

from .page_pattern import _ANCHOR_ESCAPES, _CLASS_ESCAPES, _compiled, encode_classes
from .page_search import HITS_MAX, JOBS_MAX, hit_ends
from .page_text import LEN_MAX, SIGMA_MAX, _DeviceStage

POS_MAX = 64                    # positions an expression (csrc/page_frame.h: PG_POS_MAX): one 64-bit state word
CHUNK = 128                     # text columns per lane (csrc/page_frame.h: PG_CHUNK)
LANES = 64
ROUND = CHUNK * LANES           # text columns per round of the wave
K_MAX = 4                       # errors at the most under an expression (csrc/page_regex.hip: PR_K_MAX): k + 1 <= 5 rows in registers
_FULL = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------
# syntax
# ---------------------------------------------------------------------------------------------
class Regex(object):
    """a parsed expression: src, atoms (one re source per position), P, first, last (the bit words), follow and pred (uint64 [64], rows
    at or above P zero; pred is follow transposed), min_len (the length of the shortest word of the language)"""

    def __init__(self, src, atoms, first, last, follow):
        self.src, self.atoms = src, tuple(atoms)
        self.P = len(self.atoms)
        self.first, self.last = int(first), int(last)
        rows = [int(f) for f in follow] + [0] * (POS_MAX - len(follow))
        self.follow = np.asarray(rows, dtype=np.uint64)
        self.pred = np.asarray(_transpose(rows), dtype=np.uint64)
        self.min_len = min_len(self.first, self.last, rows)

    def __repr__(self):
        return 'Regex(%r, P=%d)' % (self.src, self.P)


def _transpose(rows):
    out = [0] * POS_MAX
    for i, f in enumerate(rows):
        f = int(f)
        while f:
            j = (f & -f).bit_length() - 1
            out[j] |= 1 << i
            f &= f - 1
    return out


def _bits(x):
    x = int(x)
    while x:
        yield (x & -x).bit_length() - 1
        x &= x - 1


def min_len(first, last, follow):
    """the length of the shortest word of the language: a breadth-first walk from first through follow to last.  POS_MAX + 1 when no
    position of last can be reached (the language is empty; parse_regex builds no such automaton)"""
    first, last = int(first), int(last)
    seen, front, depth = 0, first, 1
    while front:
        if front & last:
            return depth
        seen |= front
        nxt = 0
        for i in _bits(front):
            nxt |= int(follow[i])
        front, depth = nxt & ~seen, depth + 1
    return POS_MAX + 1


_BRACE = re.compile(r'\{(\d*)(,?)(\d*)\}')


class _Parser(object):
    """recursive descent: alt := seq ('|' seq)*; seq := item+; item := (atom | group) quantifier?.  A node is ('atom', source),
    ('cat', [nodes]), ('alt', [nodes]), ('opt', node), ('star', node) or ('plus', node); a counted repeat lists the same node several times,
    and the positions are numbered when the automaton is built, so every listing gets positions of its own."""

    def __init__(self, src):
        self.src, self.n, self.i = src, len(src), 0

    def bad(self, at, what):
        return ValueError('expression %r, offset %d: %s' % (self.src, at, what))

    def alt(self, depth):
        at = self.i
        branches = [self.seq(depth)]
        while self.i < self.n and self.src[self.i] == '|':
            self.i += 1
            branches.append(self.seq(depth))
            if sum(b[1] for b in branches) > POS_MAX:
                raise self.bad(at, 'the expression holds more than %d positions after expansion' % POS_MAX)
        return branches[0] if len(branches) == 1 else (('alt', [b[0] for b in branches]), sum(b[1] for b in branches))

    def seq(self, depth):
        src, n, at = self.src, self.n, self.i
        items, size = [], 0
        while self.i < n and src[self.i] != '|' and not (src[self.i] == ')' and depth):
            node, s = self.item(depth)
            items.append(node)
            size += s
            if size > POS_MAX:
                raise self.bad(at, 'the expression holds more than %d positions after expansion' % POS_MAX)
        if not items:
            raise self.bad(at, 'an empty group or branch')
        return (items[0] if len(items) == 1 else ('cat', items)), size

    def atom(self, depth):
        src, n, at = self.src, self.n, self.i
        ch = src[at]
        if ch == '\\':
            if at + 1 >= n:
                raise self.bad(at, 'a backslash at the end')
            e = src[at + 1]
            if e.isdigit():
                raise self.bad(at, 'back-references are not supported')
            if e in _ANCHOR_ESCAPES:
                raise self.bad(at, 'anchors and word boundaries are not supported')
            atom = src[at:at + 2]
            if e not in _CLASS_ESCAPES:                                          # an escaped literal, \n, \t, ...: re says which exist
                try:
                    _compiled(atom)
                except (re.error, Warning):
                    raise self.bad(at, 'the escape %r is not supported' % atom)
            self.i = at + 2
            return ('atom', atom), 1
        if ch == '[':
            j = at + 1
            if j < n and src[j] == '^':
                j += 1
            if j < n and src[j] == ']':
                j += 1
            while j < n and src[j] != ']':
                j += 2 if src[j] == '\\' else 1
            if j >= n:
                raise self.bad(at, 'a character class that is not closed')
            atom = src[at:j + 1]
            try:
                _compiled(atom)
            except (re.error, Warning) as e:
                raise self.bad(at, 'the character class %r is refused by re: %s' % (atom, e))
            self.i = j + 1
            return ('atom', atom), 1
        if ch == '(':
            self.i = at + 1
            if src.startswith('(?', at):
                if not src.startswith('(?:', at):
                    raise self.bad(at, 'the extension %r is not supported; only (?: ) is' % src[at:at + 3])
                self.i = at + 3
            node = self.alt(depth + 1)
            if self.i >= n or src[self.i] != ')':
                raise self.bad(at, 'a group that is not closed')
            self.i += 1
            return node
        if ch == ')':
            raise self.bad(at, 'a parenthesis that closes nothing (write \\))')
        if ch in '^$':
            raise self.bad(at, 'anchors are not supported')
        if ch in '*+?{':
            raise self.bad(at, 'a quantifier with nothing to repeat')
        if ch == '}':
            raise self.bad(at, 'a brace that closes nothing (write \\})')
        self.i = at + 1
        return ('atom', '\\' + ch if ch in ']' else ch), 1

    def item(self, depth):
        src, n, at = self.src, self.n, self.i
        node, size = self.atom(depth)
        i = self.i
        if i >= n or src[i] not in '*+?{':
            return node, size
        qat, q = i, src[i]
        if q == '?':
            lo, hi, i = 0, 1, i + 1
        elif q == '*':
            lo, hi, i = 0, None, i + 1
        elif q == '+':
            lo, hi, i = 1, None, i + 1
        else:
            m = _BRACE.match(src, i)
            if m is None or (m.group(1) == '' and m.group(3) == ''):
                raise self.bad(qat, 'a brace that is no {n}, {a,b} or {a,} quantifier (write \\{)')
            a, comma, b = m.groups()
            lo = int(a) if a else 0
            hi = lo if not comma else int(b) if b else None
            if hi is not None and hi < lo:
                raise self.bad(qat, 'a quantifier {a,b} with b < a')
            if hi == 0:
                raise self.bad(qat, 'a quantifier that repeats nothing')
            i = m.end()
        if i < n and src[i] in '?+':
            raise self.bad(i, 'lazy and possessive quantifiers are not supported')
        if i < n and src[i] in '*{':
            raise self.bad(i, 'a quantifier on a quantifier')
        self.i = i
        copies = max(lo, 1) if hi is None else hi
        if copies * size > POS_MAX:
            raise self.bad(at, 'the expression holds more than %d positions after expansion' % POS_MAX)
        if hi is None:                                                           # x{a,}: a copies, the loop on the last one; x* for a = 0
            parts = [node] * (lo - 1) + [('plus', node)] if lo else [('star', node)]
        else:
            parts = [node] * lo + [('opt', node)] * (hi - lo)
        return (parts[0] if len(parts) == 1 else ('cat', parts)), copies * size


def _glushkov(node, atoms, follow):
    """number the positions of `node` after those in `atoms`, fill their follow words -> (nullable, first, last)"""
    kind, arg = node
    if kind == 'atom':
        atoms.append(arg)
        follow.append(0)
        return False, 1 << (len(atoms) - 1), 1 << (len(atoms) - 1)
    if kind == 'cat':
        null, first, last = True, 0, 0
        for child in arg:
            n, f, l = _glushkov(child, atoms, follow)
            for i in _bits(last):
                follow[i] |= f
            first |= f if null else 0
            last = l | (last if n else 0)
            null = null and n
        return null, first, last
    if kind == 'alt':
        parts = [_glushkov(child, atoms, follow) for child in arg]
        return any(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts)
    n, f, l = _glushkov(arg, atoms, follow)
    if kind in ('star', 'plus'):
        for i in _bits(l):
            follow[i] |= f
    return (n if kind == 'plus' else True), f, l


def parse_regex(src):
    """an expression as the caller wrote it -> Regex.  Every refusal is a ValueError that names the expression and the offset."""
    if isinstance(src, Regex):
        return src
    if not isinstance(src, str):
        raise ValueError('an expression must be a string, got %r' % (src,))
    p = _Parser(src)
    if not src:
        raise p.bad(0, 'the expression holds no position')
    node, size = p.alt(0)
    assert p.i == p.n and size <= POS_MAX
    atoms, follow = [], []
    null, first, last = _glushkov(node, atoms, follow)
    if null:
        raise p.bad(0, 'the expression matches the empty string')
    return Regex(src, atoms, first, last, follow)


# ---------------------------------------------------------------------------------------------
# codes
# ---------------------------------------------------------------------------------------------
def encode_regex(page_texts, regexes):
    """page texts and Q expressions (Regex objects or strings) -> (pool uint8, page_off, page_len int32 [pages], masks uint64
    [Q, sigma + 1], first, last uint64 [Q], follow, pred uint64 [Q, 64], pat_len int32 [Q], sigma).  The coding is encode_patterns'."""
    regexes = [parse_regex(r) for r in regexes]
    pool, page_off, page_len, masks, sigma = encode_classes(page_texts, [r.atoms for r in regexes])
    u64 = lambda v: np.asarray(v, dtype=np.uint64)                              # noqa: E731
    return (pool, page_off, page_len, masks, u64([r.first for r in regexes]).reshape(-1), u64([r.last for r in regexes]).reshape(-1),
            u64([r.follow for r in regexes]).reshape(-1, POS_MAX), u64([r.pred for r in regexes]).reshape(-1, POS_MAX),
            np.asarray([r.P for r in regexes], dtype=np.int32).reshape(-1), sigma)


# ---------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------
Tables = namedtuple('Tables', 'mask first last follow pred P')


def tables(masks, first, last, follow, pred, pat_len, q=0):
    """expression q of encode_regex's outputs, checked -> Tables(mask uint64 [sigma + 1], first, last, follow [64], pred [64], P) with
    Python integers"""
    mask = np.asarray(masks, dtype=np.uint64)[q].reshape(-1)
    P = int(np.asarray(pat_len).reshape(-1)[q])
    fi, la = int(np.asarray(first).reshape(-1)[q]), int(np.asarray(last).reshape(-1)[q])
    fo = [int(v) for v in np.asarray(follow, dtype=np.uint64).reshape(-1, POS_MAX)[q]]
    pr = [int(v) for v in np.asarray(pred, dtype=np.uint64).reshape(-1, POS_MAX)[q]]
    if not 1 <= P <= POS_MAX:
        raise ValueError('an expression takes 1 .. %d positions, got %d' % (POS_MAX, P))
    if mask.size < 1:
        raise ValueError('a mask table holds sigma + 1 >= 1 words')
    if any(w >> P for w in [fi, la] + fo + pr) or any(fo[P:]) or any(pr[P:]):
        raise ValueError('first, last, follow or pred hold bits or rows at or above P = %d' % P)
    if fi == 0 or la == 0:
        raise ValueError('first or last is empty: the expression matches nothing')
    return Tables(mask, fi, la, fo, pr, P)


def _classes(mask, t):
    """the class word of every text character, as Python integers: codes at or above sigma read row sigma"""
    t = np.asarray(t, dtype=np.uint8).reshape(-1)
    if t.size > LEN_MAX:
        raise ValueError('a text holds %d codes; the limit is %d' % (t.size, LEN_MAX))
    return mask[np.minimum(t.astype(np.int64), mask.size - 1)].tolist()


def _byte_tables(rows, P):
    """T[b][v] = OR of rows[8 b + i] over the bits i of v, for b < ceil(P / 8): Follow (or Pred) of a state word by one lookup per byte"""
    out = []
    for b in range((P + 7) // 8):
        T = [0] * 256
        for v in range(1, 256):
            low = v & -v
            T[v] = T[v ^ low] | rows[8 * b + low.bit_length() - 1]
        out.append(T)
    return out


def _move(T, D):
    F, b = 0, 0
    while D:
        F |= T[b][D & 255]
        D >>= 8
        b += 1
    return F


def ends_py(tab, t):
    """the end columns of text t, ascending, int32: sets of positions, no bit tricks -- the ground truth of the step"""
    B = [frozenset(_bits(b)) for b in _classes(tab.mask, t)]
    first, last = frozenset(_bits(tab.first)), frozenset(_bits(tab.last))
    follow = [frozenset(_bits(f)) for f in tab.follow]
    D, out = frozenset(), []
    for j, b in enumerate(B, 1):
        reach = set(first)
        for i in D:
            reach |= follow[i]
        D = frozenset(reach) & b
        if D & last:
            out.append(j)
    return np.asarray(out, dtype=np.int32)


def _end_flags(tab, t):
    """bool [n + 1]: column j is an end (column 0 never is)"""
    B = _classes(tab.mask, t)
    T, first, last = _byte_tables(tab.follow, tab.P), tab.first, tab.last
    flags = np.zeros(len(B) + 1, dtype=bool)
    D = 0
    for j, b in enumerate(B, 1):
        D = (_move(T, D) | first) & b
        if D & last:
            flags[j] = True
    return flags


def ends_cpu(tab, t):
    """the end columns of text t, ascending, int32, by the words: D_j = (Follow(D_{j-1}) | first) & B(t_j); j is an end iff D_j & last"""
    return np.flatnonzero(_end_flags(tab, t)).astype(np.int32)


def match_start(tab, t, end):
    """the least s with t[s:end] in the language, by the reverse walk; `end` must be an end column"""
    end = int(end)
    B = _classes(tab.mask, np.asarray(t, dtype=np.uint8).reshape(-1)[:end])
    T = _byte_tables(tab.pred, tab.P)
    s, found = end - 1, None
    R = tab.last & B[s]
    while R:
        if R & tab.first:
            found = s
        if s == 0:
            break
        s -= 1
        R = _move(T, R) & B[s]
    if found is None:
        raise AssertionError('column %d is no end: the reverse walk found no start' % end)
    return found


def ends_chunked(tab, t, chunk=CHUNK, lanes=LANES):
    """ends_cpu by the split the kernel runs, with `lanes` lanes of `chunk` columns a round of the wave.  Per round: lane l runs its chunk
    from D = 0 (lane 0: from the exact exit state of the round before) with first injected at every column, and keeps its end bits and
    its exit state X.  Then, until no lane gets a new bit: every lane l >= 1 that holds text takes X of lane l - 1, keeps the bits it
    has not carried yet, runs them through its chunk WITHOUT injection (C = Follow(C) & B), ORs C & last into its end bits and C after
    its last column into X, and leaves the chunk as soon as C == 0.  -> (ends int32 ascending, the carry rounds of every wave round)"""
    chunk, lanes = int(chunk), int(lanes)
    B = _classes(tab.mask, t)
    n = len(B)
    T, first, last = _byte_tables(tab.follow, tab.P), tab.first, tab.last
    flags = np.zeros(n + 1, dtype=bool)
    carry_in, rounds = 0, []
    for r0 in range(0, n, chunk * lanes):
        lo = [min(r0 + l * chunk, n) for l in range(lanes + 1)]                   # lane l owns the characters lo[l] .. lo[l + 1] - 1
        X = [0] * lanes
        for l in range(lanes):
            D = carry_in if l == 0 else 0
            for c in range(lo[l], lo[l + 1]):
                D = (_move(T, D) | first) & B[c]
                if D & last:
                    flags[c + 1] = True
            X[l] = D
        carried, count = [0] * lanes, 0
        while True:
            new = [0] + [X[l - 1] & ~carried[l] if lo[l + 1] > lo[l] else 0 for l in range(1, lanes)]     # all lanes read before any writes
            if not any(new):
                break
            count += 1
            for l in range(1, lanes):
                C = new[l]
                carried[l] |= C
                for c in range(lo[l], lo[l + 1]):
                    if not C:
                        break
                    C = _move(T, C) & B[c]
                    if C & last:
                        flags[c + 1] = True
                X[l] |= C
        rounds.append(count)
        carry_in = X[lanes - 1]
    return np.flatnonzero(flags).astype(np.int32), rounds


def _check_search(pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, max_hits):
    pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1)
    po, pl, P = [np.asarray(t, dtype=np.int64).reshape(-1) for t in (page_off, page_len, pat_len)]
    first, last = [np.ascontiguousarray(t, dtype=np.uint64).reshape(-1) for t in (first, last)]
    masks = np.ascontiguousarray(masks, dtype=np.uint64)
    follow, pred = [np.ascontiguousarray(t, dtype=np.uint64) for t in (follow, pred)]
    jobs = np.asarray(jobs, dtype=np.int64).reshape(-1, 2)
    if po.size != pl.size:
        raise ValueError('page_off and page_len hold one entry per page, got %d and %d' % (po.size, pl.size))
    Q = P.size
    if masks.ndim != 2 or masks.shape[1] < 1 or masks.shape[1] > SIGMA_MAX + 1 or not (masks.shape[0] == first.size == last.size == Q):
        raise ValueError('masks [Q, sigma + 1], first, last and pat_len hold one entry per expression, got %s, %d, %d and %d'
                         % (masks.shape, first.size, last.size, Q))
    if follow.shape != (Q, POS_MAX) or pred.shape != (Q, POS_MAX):
        raise ValueError('follow and pred are [Q, %d], got %s and %s' % (POS_MAX, follow.shape, pred.shape))
    max_hits = int(max_hits)
    if not 1 <= max_hits <= HITS_MAX:
        raise ValueError('max_hits must be 1 .. %d, got %d' % (HITS_MAX, max_hits))
    if jobs.shape[0] > JOBS_MAX:
        raise ValueError('a call takes %d jobs, got %d' % (JOBS_MAX, jobs.shape[0]))
    if pl.size and ((pl < 0).any() or (pl > LEN_MAX).any()):
        raise ValueError('a page length is outside 0 .. %d' % LEN_MAX)
    if po.size and ((po < 0).any() or (po + pl > pool.size).any()):
        raise ValueError('a range lies outside the pool of %d codes' % pool.size)
    if Q and ((P < 1).any() or (P > POS_MAX).any()):
        raise ValueError('an expression length is outside 1 .. %d' % POS_MAX)
    if Q:
        below = np.where(P >= POS_MAX, np.uint64(_FULL), (np.uint64(1) << np.minimum(P, POS_MAX - 1).astype(np.uint64)) - np.uint64(1))   # the bits below P
        rows = np.arange(POS_MAX)[None, :] < P[:, None]                                                  # the rows below P
        allowed = np.where(rows, below[:, None], np.uint64(0))
        if ((first | last) & ~below).any() or ((follow | pred) & ~allowed).any():
            raise ValueError('first, last, follow or pred hold bits or rows at or above P')
        if (first == 0).any() or (last == 0).any():
            raise ValueError('first or last of an expression is empty')
        bits = lambda w: np.unpackbits(w.view(np.uint8).reshape(Q, POS_MAX, 8), axis=2, bitorder='little')  # noqa: E731  [q, row, bit]
        if (bits(follow) != bits(pred).transpose(0, 2, 1)).any():
            raise ValueError('pred is not follow transposed')
    if jobs.size and ((jobs < 0).any() or (jobs[:, 0] >= pl.size).any() or (jobs[:, 1] >= Q).any()):
        raise ValueError('a job names a page or an expression that is not there')
    return [pool, po.astype(np.int32), pl.astype(np.int32), masks, first, last, follow, pred, P.astype(np.int32),
            np.ascontiguousarray(jobs.astype(np.int32)), max_hits]


def search_cpu(pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, max_hits):
    """the definition, for the flat inputs omp_page_regex_search takes -> dict(best int32 [J, 2] = (0, the least end) or (1, 0),
    n_hits int32 [J], hits int32 [J, max_hits, 3] = (end, 0, start), -1 where there is no hit)"""
    pool, po, pl, masks, first, last, follow, pred, P, jobs, H = _check_search(pool, page_off, page_len, masks, first, last, follow, pred,
                                                                               pat_len, jobs, max_hits)
    J = jobs.shape[0]
    best = np.zeros((J, 2), dtype=np.int32)
    n_hits = np.zeros(J, dtype=np.int32)
    hits = np.full((J, H, 3), -1, dtype=np.int32)
    done, tabs = {}, {}
    for j, (p, q) in enumerate(jobs.tolist()):
        key = (po[p], pl[p], q)
        if key not in done:
            if q not in tabs:
                tabs[q] = tables(masks, first, last, follow, pred, P, q)
            t = pool[po[p]:po[p] + pl[p]]
            v = 1 - _end_flags(tabs[q], t).astype(np.int32)                    # v_0 = 1: column 0 is never an end
            ends = hit_ends(v, 0)
            least = np.flatnonzero(v == 0)
            rows = [(int(e), 0, match_start(tabs[q], t, int(e))) for e in ends[:H].tolist()]
            done[key] = ((0, int(least[0])) if least.size else (1, 0), int(ends.size), rows)
        b, c, rows = done[key]
        best[j] = b
        n_hits[j] = c
        if rows:
            hits[j, :len(rows)] = rows
    return dict(best=best, n_hits=n_hits, hits=hits)


class HostRegexSearcher(object):
    """RegexSearcher's `run` from the specification (search_cpu): what the device stage must equal"""

    def __init__(self):
        self.calls = 0

    def run(self, pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, max_hits):
        self.calls += 1
        return search_cpu(pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, max_hits)


# ---------------------------------------------------------------------------------------------
# the device stage
# ---------------------------------------------------------------------------------------------
def _job_parts(n_jobs):
    """-> [(lo, hi)]: the kernels need no scratch, so a launch takes JOBS_MAX jobs"""
    return [(lo, min(lo + JOBS_MAX, n_jobs)) for lo in range(0, n_jobs, JOBS_MAX)]


class RegexSearcher(_DeviceStage):
    """search_cpu on the device.  A call is ONE packed upload of the tables and the pool, one omp_page_regex_search launch per JOBS_MAX
    jobs (the kernel needs no scratch), and ONE download of best, n_hits and hits.  There is no CPU fallback: HostRegexSearcher is the
    specification."""
    HOST = 'HostRegexSearcher'

    def __init__(self, device):
        super().__init__(device, 0)

    def run(self, pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, max_hits):
        """the inputs of search_cpu -> the dict of search_cpu, as numpy.  sigma is masks.shape[1] - 1."""
        from .. import ops
        pool, po, pl, masks, first, last, follow, pred, P, jobs, H = _check_search(pool, page_off, page_len, masks, first, last, follow, pred,
                                                                                   pat_len, jobs, max_hits)
        return self._search(ops.page_regex_search, (po, pl, masks, first, last, follow, pred, P), pool, jobs, masks.shape[1] - 1, H,
                            _job_parts(jobs.shape[0]),
                            'omp_page_regex_search refused a job (a length above the limits, a range outside the pool, or first, last, follow '
                            'or pred words with bits or rows at or above P)')


# ---------------------------------------------------------------------------------------------
# with errors: the specification
# ---------------------------------------------------------------------------------------------
def regex_tolerance(shortest, max_dist=None, max_ratio=0.0):
    """the tolerance k of an expression whose shortest word holds `shortest` characters (Regex.min_len):
    min(page_pattern.tolerance(shortest, max_dist, max_ratio), K_MAX), so k <= shortest - 1"""
    from .page_pattern import tolerance
    return min(tolerance(min(int(shortest), POS_MAX), max_dist, max_ratio), K_MAX)


def _tolerance_of(k):
    k = int(k)
    if not 0 <= k <= K_MAX:
        raise ValueError('a tolerance is 0 .. %d, got %d' % (K_MAX, k))
    return k


def dist_py(tab, t, k, rows=False):
    """v_0 .. v_n, clipped at k + 1, int32: sets of positions per row, no bit tricks -- the ground truth of the step with errors.
    rows=True: -> (v, per column 0 .. n the k + 1 rows as frozensets)"""
    k = _tolerance_of(k)
    B = [frozenset(_bits(b)) for b in _classes(tab.mask, t)]
    first, last = frozenset(_bits(tab.first)), frozenset(_bits(tab.last))
    follow = [frozenset(_bits(f)) for f in tab.follow]

    def fol(X):
        reach = set(first)
        for p in X:
            reach |= follow[p]
        return frozenset(reach)
    R = [frozenset()]
    for i in range(1, k + 1):
        R.append(fol(R[i - 1]))                                               # deletions only
    v, kept = [k + 1], [list(R)]
    for b in B:
        new = [fol(R[0]) & b]
        for i in range(1, k + 1):
            new.append((fol(R[i]) & b) | fol(R[i - 1]) | R[i - 1] | fol(new[i - 1]))
        R = new
        v.append(next((i for i in range(k + 1) if R[i] & last), k + 1))
        kept.append(list(R))
    v = np.asarray(v, dtype=np.int32)
    return (v, kept) if rows else v


def _fuzzy_step(T, inject, R, b):
    """one column of the step on words: T the byte tables of follow (or pred), inject[i] the word injected into row i (first, or 0)"""
    new = [(_move(T, R[0]) | inject[0]) & b]
    for i in range(1, len(R)):
        new.append(((_move(T, R[i]) | inject[i]) & b) | _move(T, R[i - 1]) | inject[i - 1] | R[i - 1] | _move(T, new[i - 1]) | inject[i - 1])
    return new


def _fuzzy_init(T, first, k):
    R = [0]
    for i in range(1, k + 1):
        R.append(_move(T, R[i - 1]) | first)
    return R


def _value(R, last, k):
    return next((i for i in range(k + 1) if R[i] & last), k + 1)


def dist_cpu(tab, t, k):
    """v_0 .. v_n, clipped at k + 1, int32, by the words: R'_0 = Fol(R_0) & B, R'_i = (Fol(R_i) & B) | Fol(R_{i-1}) | R_{i-1} | Fol(R'_{i-1})"""
    k = _tolerance_of(k)
    T, first, last = _byte_tables(tab.follow, tab.P), tab.first, tab.last
    R = _fuzzy_init(T, first, k)
    inject = [first] * (k + 1)
    v = [k + 1]
    for b in _classes(tab.mask, t):
        R = _fuzzy_step(T, inject, R, b)
        v.append(_value(R, last, k))
    return np.asarray(v, dtype=np.int32)


def fuzzy_start(tab, t, end, dist):
    """the least s whose anchored distance of t[s:end] to the language equals dist (the longest match); (end, dist) must be a hit.  The
    step backwards from `end` with rows 0 .. dist over pred; last is injected into row i while G_i holds: G_i = 1 at `end`, G'_0 = 0,
    G'_i = G_{i-1} after every character"""
    end, dist = int(end), int(dist)
    if not 0 <= dist <= K_MAX:
        raise ValueError('a distance is 0 .. %d, got %d' % (K_MAX, dist))
    B = _classes(tab.mask, np.asarray(t, dtype=np.uint8).reshape(-1)[:end])
    T, first, last = _byte_tables(tab.pred, tab.P), tab.first, tab.last
    R, G = _fuzzy_init(T, last, dist), [1] * (dist + 1)
    s, found = end, None
    while s > 0 and (any(R) or any(G)):
        s -= 1
        new_g = [0] + G[:-1]
        b = B[s]
        new = [(_move(T, R[0]) | (last if G[0] else 0)) & b]
        for i in range(1, dist + 1):
            below = _move(T, R[i - 1]) | (last if G[i - 1] else 0)
            new.append(((_move(T, R[i]) | (last if G[i] else 0)) & b) | below | R[i - 1] | _move(T, new[i - 1]) | (last if new_g[i - 1] else 0))
        R, G = new, new_g
        if R[dist] & first:
            found = s
    if found is None:
        raise AssertionError('column %d is no end at distance %d: the reverse walk found no start' % (end, dist))
    return found


def dist_chunked(tab, t, k, chunk=CHUNK, lanes=LANES):
    """dist_cpu by the split the kernel runs.  Per round: lane l runs its chunk from the deletion-only rows (lane 0: from the exact exit
    rows of the round before) with first injected, and keeps k + 1 end planes (plane i holds column j iff R_i & last != 0 there) and its
    exit rows X.  Then, until no lane gets a new bit in any row: every lane l >= 1 that holds text takes the rows X of lane l - 1, keeps
    new_i = in_i & ~carried_i, runs them through the step WITHOUT any first, ORs the ends into the planes and the rows after its last
    column into X, and leaves the chunk as soon as every row is 0.  v_j is the number of planes without column j.
    -> (v int32 [n + 1], the carry rounds of every wave round)"""
    k = _tolerance_of(k)
    chunk, lanes = int(chunk), int(lanes)
    B = _classes(tab.mask, t)
    n = len(B)
    T, first, last = _byte_tables(tab.follow, tab.P), tab.first, tab.last
    with_first, without = [first] * (k + 1), [0] * (k + 1)
    init = _fuzzy_init(T, first, k)
    planes = np.zeros((k + 1, n + 1), dtype=bool)

    def mark(R, col):
        for i in range(k + 1):
            if R[i] & last:
                planes[i, col] = True
    carry_in, rounds = list(init), []
    for r0 in range(0, n, chunk * lanes):
        lo = [min(r0 + l * chunk, n) for l in range(lanes + 1)]                   # lane l owns the characters lo[l] .. lo[l + 1] - 1
        X = []
        for l in range(lanes):
            R = list(carry_in if l == 0 else init)
            for c in range(lo[l], lo[l + 1]):
                R = _fuzzy_step(T, with_first, R, B[c])
                mark(R, c + 1)
            X.append(R)
        carried, count = [[0] * (k + 1) for _ in range(lanes)], 0
        while True:
            new = [[0] * (k + 1)] + [[X[l - 1][i] & ~carried[l][i] if lo[l + 1] > lo[l] else 0 for i in range(k + 1)] for l in range(1, lanes)]
            if not any(any(r) for r in new):
                break
            count += 1
            for l in range(1, lanes):
                C = new[l]
                carried[l] = [a | b for a, b in zip(carried[l], C)]
                for c in range(lo[l], lo[l + 1]):
                    if not any(C):
                        break
                    C = _fuzzy_step(T, without, C, B[c])
                    mark(C, c + 1)
                X[l] = [a | b for a, b in zip(X[l], C)]
        rounds.append(count)
        carry_in = X[lanes - 1]
    return (k + 1 - planes.sum(axis=0)).astype(np.int32), rounds


def _check_fuzzy(pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, k, max_hits):
    out = _check_search(pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, max_hits)
    first, last, follow = out[4], out[5], out[6]
    k = np.asarray(k, dtype=np.int64).reshape(-1)
    if k.size != first.size:
        raise ValueError('k holds one entry per expression, got %d for %d' % (k.size, first.size))
    if k.size and ((k < 0).any() or (k > K_MAX).any()):
        raise ValueError('a tolerance is outside 0 .. %d' % K_MAX)
    # k >= min_len iff a word of at most k <= K_MAX characters exists: the positions reached by exactly `depth` characters, all expressions at once
    front, top = first.copy(), int(k.max()) if k.size else 0
    for depth in range(1, top + 1):
        short = (k >= depth) & ((front & last) != 0)
        if short.any():
            q = int(np.flatnonzero(short)[0])
            raise ValueError('expression %d: the tolerance %d is not below the length of its shortest word, %d' % (q, k[q], depth))
        nxt = np.zeros_like(front)
        for i in range(int(out[8].max())):
            nxt |= np.where((front >> np.uint64(i)) & np.uint64(1) != 0, follow[:, i], np.uint64(0))
        front = nxt
    return out[:10] + [k.astype(np.int32), out[10]]


def fuzzy_search_cpu(pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, k, max_hits):
    """the definition with errors, for the flat inputs omp_page_regex_fuzzy_search takes; k int32 [Q], one tolerance per expression
    -> dict(best int32 [J, 2] = (the least distance, the least end that attains it) or (k + 1, 0), n_hits int32 [J], hits int32
    [J, max_hits, 3] = (end, dist, start), -1 where there is no hit)"""
    pool, po, pl, masks, first, last, follow, pred, P, jobs, k, H = _check_fuzzy(pool, page_off, page_len, masks, first, last, follow, pred,
                                                                                 pat_len, jobs, k, max_hits)
    J = jobs.shape[0]
    best = np.zeros((J, 2), dtype=np.int32)
    n_hits = np.zeros(J, dtype=np.int32)
    hits = np.full((J, H, 3), -1, dtype=np.int32)
    done, tabs = {}, {}
    for j, (p, q) in enumerate(jobs.tolist()):
        key = (po[p], pl[p], q)
        if key not in done:
            if q not in tabs:
                tabs[q] = tables(masks, first, last, follow, pred, P, q)
            t = pool[po[p]:po[p] + pl[p]]
            kq = int(k[q])
            v = dist_cpu(tabs[q], t, kq)
            end = int(np.argmin(v))                                           # the least j that attains the minimum; v_0 = k + 1
            ends = hit_ends(v, kq)
            rows = [(int(e), int(v[e]), fuzzy_start(tabs[q], t, int(e), int(v[e]))) for e in ends[:H].tolist()]
            done[key] = ((int(v[end]), end), int(ends.size), rows)
        b, c, rows = done[key]
        best[j] = b
        n_hits[j] = c
        if rows:
            hits[j, :len(rows)] = rows
    return dict(best=best, n_hits=n_hits, hits=hits)


class HostFuzzyRegexSearcher(object):
    """FuzzyRegexSearcher's `run` from the specification (fuzzy_search_cpu): what the device stage must equal"""

    def __init__(self):
        self.calls = 0

    def run(self, pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, k, max_hits):
        self.calls += 1
        return fuzzy_search_cpu(pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, k, max_hits)


class FuzzyRegexSearcher(_DeviceStage):
    """fuzzy_search_cpu on the device.  A call is ONE packed upload of the tables and the pool, one omp_page_regex_fuzzy_search launch per
    JOBS_MAX jobs (the kernel needs no scratch), and ONE download of best, n_hits and hits.  There is no CPU fallback:
    HostFuzzyRegexSearcher is the specification."""
    HOST = 'HostFuzzyRegexSearcher'

    def __init__(self, device):
        super().__init__(device, 0)

    def run(self, pool, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, k, max_hits):
        """the inputs of fuzzy_search_cpu -> the dict of fuzzy_search_cpu, as numpy.  sigma is masks.shape[1] - 1."""
        from .. import ops
        pool, po, pl, masks, first, last, follow, pred, P, jobs, k, H = _check_fuzzy(pool, page_off, page_len, masks, first, last, follow, pred,
                                                                                     pat_len, jobs, k, max_hits)
        return self._search(ops.page_regex_fuzzy_search, (po, pl, masks, first, last, follow, pred, P, k), pool, jobs, masks.shape[1] - 1, H,
                            _job_parts(jobs.shape[0]),
                            'omp_page_regex_fuzzy_search refused a job (a length above the limits, a range outside the pool, first, last, '
                            'follow or pred words with bits or rows at or above P, or k outside 0 .. %d)' % K_MAX)
