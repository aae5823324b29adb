"""Page text alignment: the optimal edit script of whole pages.

utils/page_text.py says how far a read page is from its ground truth; this module says WHERE: which characters match, which are
substituted, which the prediction holds in excess (INS) and which it lacks (DEL).  Codes, equality and lengths are page_text's
(encode_pairs; 255 equals nothing, itself included; sigma <= 254; 0 .. 65535 characters a side).  a is the prediction (rows i), b the
ground truth (columns j).  The numpy / Python functions here are the DEFINITION; csrc/page_align.hip (omp_page_align) equals
pairs_align_cpu on every integer.

Script      align_cpu(): D is the full Levenshtein table (D[i][0] = i, D[0][j] = j).  The walk runs from (la, lb) to (0, 0) and takes at
            (i, j) the FIRST rule that applies:
              1. i > 0, j > 0 and D[i-1][j-1] + (a_i != b_j) == D[i][j]: the diagonal, a MATCH when the characters are equal, otherwise
                 a SUB; a_map[i-1] = j-1, b_map[j-1] = i-1
              2. i > 0 and D[i-1][j] + 1 == D[i][j]: INS, a_map[i-1] = -1
              3. otherwise DEL, b_map[j-1] = -1
            so the script is unique.  counts = (match, sub, ins, del); sub + ins + del == dist, match + sub + ins == la,
            match + sub + del == lb; the mapped entries of a_map increase strictly and b_map is their inverse.
Words       page_words(): the records' texts, each stripped and normalised PER WORD, concatenated, with every word's start and length.
            word_report_cpu(): per word CORRECT / WRONG / ABSENT / EMPTY and the span of its images on the other side.
            confusions(): which characters were taken for which.
Stage       PageAligner: one packed upload, one omp_page_align launch per chunk of pairs, one download.  HostPageAligner is its host
            twin, built from pairs_align_cpu.
"""
import numpy as np

from .page_text import LEN_MAX, NONE, _check_pairs, _check_sigma, _DeviceStage, _rows

SCRATCH_CAP = 1 << 30           # device scratch per chunk of pairs
MAPS_CAP = (1 << 31) - 1        # map entries per chunk
MATCH, SUB, INS, DEL = 0, 1, 2, 3                                          # the columns of counts
CORRECT, WRONG, ABSENT, EMPTY = 0, 1, 2, 3                                 # word statuses
STATUS_NAMES = ('correct', 'wrong', 'absent', 'empty')
GAP = -2                        # what pairs_align_cpu leaves in map entries that no pair owns


# ---------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------
def table_cpu(a, b):
    """the full Levenshtein table int32 [la + 1, lb + 1] of two code sequences, by rows as page_text.distance_cpu builds them (rows of
    the shorter sequence, vectorised over the longer; the table of (b, a) is the transpose)"""
    a, b = np.asarray(a, dtype=np.uint8).reshape(-1), np.asarray(b, dtype=np.uint8).reshape(-1)
    if a.size > LEN_MAX or b.size > LEN_MAX:
        raise ValueError('a sequence holds %d codes; the limit is %d' % (max(a.size, b.size), LEN_MAX))
    if a.size > b.size:
        return np.ascontiguousarray(table_cpu(b, a).T)
    D = np.empty((a.size + 1, b.size + 1), dtype=np.int32)
    for i, row in enumerate(_rows(a, b)):
        D[i] = row
    return D


def align_cpu(a, b):
    """-> (dist, counts int32 [4] = (match, sub, ins, del), a_map int32 [la], b_map int32 [lb]): the definition (the module docstring
    holds the rule)"""
    a, b = np.asarray(a, dtype=np.uint8).reshape(-1), np.asarray(b, dtype=np.uint8).reshape(-1)
    D = table_cpu(a, b)
    la, lb = a.size, b.size
    a_map, b_map = np.full(la, -1, dtype=np.int32), np.full(lb, -1, dtype=np.int32)
    counts = [0, 0, 0, 0]
    al, bl = a.tolist(), b.tolist()
    i, j = la, lb
    while i > 0 or j > 0:
        here = int(D[i, j])
        if i > 0 and j > 0:
            same = al[i - 1] == bl[j - 1] and al[i - 1] != NONE
            if int(D[i - 1, j - 1]) + (0 if same else 1) == here:
                a_map[i - 1], b_map[j - 1] = j - 1, i - 1
                counts[MATCH if same else SUB] += 1
                i, j = i - 1, j - 1
                continue
        if i > 0 and int(D[i - 1, j]) + 1 == here:
            counts[INS] += 1
            i -= 1
            continue
        counts[DEL] += 1
        j -= 1
    return int(D[la, lb]), np.asarray(counts, dtype=np.int32), a_map, b_map


def _check_offsets(map_off, a_len, b_len):
    map_off = np.asarray(map_off, dtype=np.int64).reshape(-1)
    if map_off.size != a_len.size:
        raise ValueError('map_off holds one entry per pair, got %d for %d pairs' % (map_off.size, a_len.size))
    if map_off.size and (map_off < 0).any():
        raise ValueError('a map offset is negative')
    return map_off


def pairs_align_cpu(pool, a_off, a_len, b_off, b_len, map_off):
    """align_cpu over the pairs of a call, for the flat inputs omp_page_align takes -> (counts int32 [P, 4], maps int32): pair p owns
    maps[map_off[p] : map_off[p] + la + lb], a_map first and b_map after it; entries no pair owns hold GAP"""
    pool, a_off, a_len, b_off, b_len = _check_pairs(pool, a_off, a_len, b_off, b_len)
    map_off = _check_offsets(map_off, a_len, b_len)
    P = a_len.size
    size = int((map_off + a_len + b_len).max()) if P else 0
    counts = np.zeros((P, 4), dtype=np.int32)
    maps = np.full(size, GAP, dtype=np.int32)
    done = {}
    for p, key in enumerate(zip(a_off.tolist(), a_len.tolist(), b_off.tolist(), b_len.tolist())):
        if key not in done:
            ao, la, bo, lb = key
            done[key] = align_cpu(pool[ao:ao + la], pool[bo:bo + lb])
        _, c, am, bm = done[key]
        la, lb, at = key[1], key[3], int(map_off[p])
        counts[p] = c
        maps[at:at + la] = am
        maps[at + la:at + la + lb] = bm
    return counts, maps


def dense_map_off(a_len, b_len):
    """the map offsets of pairs laid out back to back -> int64 [P]"""
    n = np.asarray(a_len, dtype=np.int64).reshape(-1) + np.asarray(b_len, dtype=np.int64).reshape(-1)
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(n)])[:n.size]


def page_words(records, field='rec', strip=' \n', normalise=str.casefold):
    """one image's words, IN THE ORDER GIVEN -> (text, w_start int32 [n], w_len int32 [n]).  records: a list of record dicts (the text
    of each taken as page_text.page_string takes it), a list of strings, or one string = one word.  Every word has the characters of
    `strip` removed and is then normalised ON ITS OWN; text is the concatenation, and word k is text[w_start[k] : w_start[k] + w_len[k]].
    For a `normalise` that works character by character (str.casefold) text == page_string(records, ...); for any other callable the
    two may differ, and the string that is aligned is THIS one, the concatenation of the per-word results."""
    from .page_text import page_string
    if isinstance(records, str):
        records = [records]
    words = [page_string([r], field, strip, normalise) for r in records]
    w_len = np.asarray([len(w) for w in words], dtype=np.int32).reshape(-1)
    w_start = (np.cumsum(w_len) - w_len).astype(np.int32)
    return ''.join(words), w_start, w_len


def word_report_cpu(x_map, w_start, w_len, x, y):
    """the words of side x (w_start, w_len into x) under x_map (x's characters -> positions of y, -1 = none) -> (status int8 [n],
    span int32 [n, 2]).  CORRECT: every character mapped, every mapped pair equal and the images consecutive (x_map[s + k] ==
    x_map[s] + k); ABSENT: no character mapped (a spurious prediction word, or a missed ground-truth word); EMPTY: w_len == 0; WRONG:
    everything else.  span = (min image, max image + 1) on the other side, or (-1, -1).  x and y: strings or code sequences."""
    x_map = np.asarray(x_map, dtype=np.int64).reshape(-1)
    w_start, w_len = np.asarray(w_start, dtype=np.int64).reshape(-1), np.asarray(w_len, dtype=np.int64).reshape(-1)
    x, y = list(x), list(y)
    if len(x) != x_map.size:
        raise ValueError('x_map holds %d entries for %d characters' % (x_map.size, len(x)))
    status = np.zeros(w_start.size, dtype=np.int8)
    span = np.full((w_start.size, 2), -1, dtype=np.int32)
    for k, (s, n) in enumerate(zip(w_start.tolist(), w_len.tolist())):
        if n == 0:
            status[k] = EMPTY
            continue
        img = x_map[s:s + n]
        hit = img >= 0
        if not hit.any():
            status[k] = ABSENT
            continue
        span[k] = (int(img[hit].min()), int(img[hit].max()) + 1)
        ok = bool(hit.all()) and bool((img == img[0] + np.arange(n)).all())
        ok = ok and all(x[s + t] == y[int(img[t])] and x[s + t] != NONE for t in range(n))
        status[k] = CORRECT if ok else WRONG
    return status, span


def confusions(pred, gt, a_map, b_map):
    """-> dict(sub={(pred_char, gt_char): n}, ins={char: n}, dele={char: n}) on the Python strings of one page"""
    sub, ins, dele = {}, {}, {}
    for i, j in enumerate(np.asarray(a_map).tolist()):
        if j < 0:
            ins[pred[i]] = ins.get(pred[i], 0) + 1
        elif pred[i] != gt[j]:
            sub[(pred[i], gt[j])] = sub.get((pred[i], gt[j]), 0) + 1
    for j, i in enumerate(np.asarray(b_map).tolist()):
        if i < 0:
            dele[gt[j]] = dele.get(gt[j], 0) + 1
    return dict(sub=sub, ins=ins, dele=dele)


def chunk_pairs(a_len, b_len, scratch_cap=SCRATCH_CAP, maps_cap=MAPS_CAP):
    """-> [(lo, hi)]: consecutive pairs whose scratch stays at or below scratch_cap bytes and whose maps stay at or below maps_cap
    entries.  A pair that alone needs more scratch raises ValueError."""
    from ..ops import page_align_scratch_bytes
    parts, lo, used, ents = [], 0, 0, 0
    for p, (la, lb) in enumerate(zip(np.asarray(a_len).reshape(-1).tolist(), np.asarray(b_len).reshape(-1).tolist())):
        need = page_align_scratch_bytes(la, lb)
        if need > scratch_cap:
            raise ValueError('pair %d (%d x %d characters) needs %d bytes of scratch; scratch_cap is %d' % (p, la, lb, need, scratch_cap))
        if la + lb > maps_cap:
            raise ValueError('pair %d needs %d map entries; a chunk holds %d' % (p, la + lb, maps_cap))
        if p > lo and (used + need > scratch_cap or ents + la + lb > maps_cap):
            parts.append((lo, p))
            lo, used, ents = p, 0, 0
        used += need
        ents += la + lb
    if lo < len(np.asarray(a_len).reshape(-1)):
        parts.append((lo, len(np.asarray(a_len).reshape(-1))))
    return parts


class HostPageAligner(object):
    """PageAligner's `run` from the specification (pairs_align_cpu): what the device stage must equal"""

    def __init__(self):
        self.calls = 0

    def run(self, pool, a_off, a_len, b_off, b_len, sigma):
        self.calls += 1
        map_off = dense_map_off(a_len, b_len)
        counts, maps = pairs_align_cpu(pool, a_off, a_len, b_off, b_len, map_off)
        return dict(counts=counts, map_off=map_off, maps=maps)


def split_maps(res, a_len, b_len, p):
    """pair p of a `run` result -> (a_map, b_map)"""
    at, la, lb = int(res['map_off'][p]), int(a_len[p]), int(b_len[p])
    return res['maps'][at:at + la], res['maps'][at + la:at + la + lb]


# ---------------------------------------------------------------------------------------------
# the device stage
# ---------------------------------------------------------------------------------------------
class PageAligner(_DeviceStage):
    """pairs_align_cpu on the device.  A call is ONE packed upload of the tables and the pool, one omp_page_align launch per chunk of
    pairs (a chunk's scratch stays at or below scratch_cap and its maps below 2^31 entries; the scratch is cached and grown), and ONE
    download of the counts and the maps.  A pair that alone needs more than scratch_cap raises ValueError.  There is no CPU fallback:
    HostPageAligner is the specification."""
    HOST = 'HostPageAligner'

    def __init__(self, device, scratch_cap=SCRATCH_CAP):
        super().__init__(device, scratch_cap)

    def run(self, pool, a_off, a_len, b_off, b_len, sigma):
        """pool uint8, a_off / a_len / b_off / b_len int32 [P] as encode_pairs gives them -> dict(counts int32 [P, 4], map_off int64 [P],
        maps int32) as numpy: pair p's a_map and b_map lie back to back from maps[map_off[p]]"""
        import torch

        from .. import ops
        pool, a_off, a_len, b_off, b_len = _check_pairs(pool, a_off, a_len, b_off, b_len)
        sigma = _check_sigma(pool, sigma)
        P = a_len.size
        parts = chunk_pairs(a_len, b_len, self.scratch_cap)
        self.calls += 1
        self.chunks = len(parts)
        map_off = dense_map_off(a_len, b_len)
        if P == 0:
            return dict(counts=np.zeros((0, 4), np.int32), map_off=map_off, maps=np.zeros(0, np.int32))
        total = int(map_off[-1]) + int(a_len[-1]) + int(b_len[-1])
        need = np.asarray([ops.page_align_scratch_bytes(la, lb) for la, lb in zip(a_len.tolist(), b_len.tolist())], dtype=np.int64)
        scratch_off = np.zeros(P, dtype=np.int64)
        rel_off = np.zeros(P, dtype=np.int64)                                # map offsets inside the chunk's slice of maps
        for lo, hi in parts:
            scratch_off[lo:hi] = np.cumsum(need[lo:hi]) - need[lo:hi]
            rel_off[lo:hi] = map_off[lo:hi] - map_off[lo]
        most = max(int(scratch_off[hi - 1] + need[hi - 1]) for lo, hi in parts)
        with torch.cuda.device(self.device):
            (d_rel, d_so, d_ao, d_al, d_bo, d_bl), d_pool = self._upload((rel_off, scratch_off, a_off, a_len, b_off, b_len), pool)
            scratch = self._grow(most)
            out = torch.empty(4 * P + max(total, 1), dtype=torch.int32, device=self.device)
            for lo, hi in parts:
                m0 = 4 * P + int(map_off[lo])
                m1 = 4 * P + (int(map_off[hi]) if hi < P else total)
                ops.page_align(d_pool, pool.size, d_ao[lo:hi], d_al[lo:hi], d_bo[lo:hi], d_bl[lo:hi], d_rel[lo:hi], d_so[lo:hi], sigma, scratch,
                               out[m0:max(m1, m0 + 1)], m1 - m0, counts=out[4 * lo:4 * hi])
            host = out.cpu().numpy()                                          # the one download
        counts = host[:4 * P].reshape(P, 4)
        if (counts < 0).any():
            raise RuntimeError('omp_page_align refused a pair (a length above %d, a range outside the pool, or a slice outside maps or scratch)' % LEN_MAX)
        return dict(counts=counts, map_off=map_off, maps=host[4 * P:4 * P + total])
