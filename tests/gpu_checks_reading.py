"""GPU checks of the reading-order stage: omp_reading_links / omp_reading_lines against their numpy
specification (utils/reading.py) on every output integer -- succ0, cost0, succ, pred, line, line_pos, rank, n_lines -- and
`reading_order=` of predict / spot_and_recognize against lines_cpu applied on the host to the same call's records.  Every check
returns records {name, err, tol, ok, note} like tests/gpu_checks.py."""
import copy

import numpy as np
import torch

from advancedliteratemachinery_amd.utils import overlap as OV
from advancedliteratemachinery_amd.utils import reading as RD
from advancedliteratemachinery_amd.utils import synthetic as weights
from advancedliteratemachinery_amd.utils import windows as WN
from advancedliteratemachinery_amd.utils.parser import make_args
from tests import reading_cases as RC

GROUP_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513)   # the wave and the links kernel's tile of 256 from both sides, two tiles and a word
LARGE_SIZES = (1023, 1024, 1025, 2049)                     # the lines kernel's 1024 threads from both sides, a third word for one thread
LARGE_KINDS = ('rotated', 'ring', 'duplicates', 'rows')
ASPECTS = ((256, 256), (256, 128), (37, 256), (1, 1))
PARAMS = ((2000, 500, 500), (0, 0, 0), (10000, 10000, 10000))
KINDS = ('rows', 'rotated', 'ring', 'random', 'duplicates', 'degenerate')
OUTS = ('succ', 'pred', 'line', 'line_pos', 'rank', 'n_lines')


# ---------------------------------------------------------------------------------------------------------------------------------
# words
# ---------------------------------------------------------------------------------------------------------------------------------
def group_words(rng, n, grid, kind):
    """n words of one group -> int32 [n, 32]; tokens may leave [0, grid - 1]: both sides clamp"""
    if n == 0:
        return np.zeros((0, 32), np.int32)
    s = grid / 1000.0
    c = (grid / 2.0, grid / 2.0)
    if kind == 'ring':
        w = max(2, int(2 * np.pi * 0.4 * grid / n * 0.85))
        return RC.ring(n, r=0.4 * grid, w=w, h=max(1, w // 4), centre=c)
    if kind == 'random':
        return rng.randint(-grid // 50 - 1, grid + grid // 50 + 1, size=(n, 32)).astype(np.int32)
    if kind == 'degenerate':
        pts = rng.randint(0, grid, size=(max(1, n // 3), 2))
        return np.tile(pts[rng.randint(len(pts), size=n)], (1, 16)).astype(np.int32)      # all 16 points equal, many words on one point
    cols = max(1, int(np.ceil(np.sqrt(n / 2.0))) * 2)
    rows = (n + cols - 1) // cols
    w, h, gap = max(2, int(700 * s / cols * 0.8)), max(2, int(700 * s / max(rows, cols / 3.0) * 0.45)), max(1, int(700 * s / cols * 0.2))
    pts = RC.page_points(rows, cols, w=w, h=h, gap=gap, pitch=max(h + 1, int(h * 1.7)), centre=c, jitter=rng.uniform(0, h / 4.0))
    pts = RC.rotate(pts, rng.uniform(-180, 180) if kind == 'rotated' else rng.uniform(-3, 3), np.asarray(c))
    p = RC.to_bins(pts[rng.permutation(rows * cols)[:n]])
    if kind == 'duplicates' and n > 1:
        p[1::3] = p[0::3][:len(p[1::3])]                                                   # exact duplicates: ties everywhere
        p[-1] = p[0]
    return p


def _case(rng, sizes, grid, kinds=KINDS):
    gs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    polys = np.concatenate([group_words(rng, int(n), grid, kinds[g % len(kinds)]) for g, n in enumerate(sizes)] + [np.zeros((0, 32), np.int32)])
    aspect = np.asarray([ASPECTS[(g // 2) % len(ASPECTS)] for g in range(len(sizes))], dtype=np.int32).reshape(-1, 2)
    return polys, gs, aspect


def _cases():
    """(name, polys, group_start, aspect, grid): the smallest shapes that can break the kernels"""
    rng = np.random.RandomState(18)
    for grid in (1000, 4096, 64):
        for shift in (0, 1):                                                 # every size meets two kinds of content and two aspects
            sizes = GROUP_SIZES[shift * 3:] + GROUP_SIZES[:shift * 3]
            yield ('grid=%d groups=%s' % (grid, list(sizes)),) + _case(rng, sizes, grid) + (grid,)
    for k, kind in enumerate(KINDS):                                         # G = 1, each content alone under each aspect
        polys, gs, _ = _case(rng, (257,), 1000, (kind,))
        yield 'G=1 n=257 %s' % kind, polys, gs, np.asarray([ASPECTS[k % 4]], np.int32), 1000
    sizes = rng.randint(0, 40, 40)
    sizes[[3, 4, 17, 39]] = 0                                                # empty groups between full ones, and at the end
    sizes[[5, 18]] = 300
    yield ('G=40 mixed',) + _case(rng, sizes, 1000) + (1000,)


def _compare(tag, got, want, links, out, note=''):
    bad = sum(int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else 10 ** 6 for k in OUTS)
    from tests.gpu_checks import rec
    out.append(rec(tag + ' succ, pred, line, line_pos, rank, n_lines', bad, 0, note))
    bad = int((got['succ0'] != links[0]).sum()) + int((got['cost0'] != links[1]).sum())
    out.append(rec(tag + ' succ0, cost0', bad, 0, '%d links' % int((links[0] >= 0).sum())))


def check_reading_op():
    from tests.gpu_checks import DEV, rec
    out = []
    linked = lines = 0
    for name, polys, gs, aspect, grid in _cases():
        reader = RD.ReadingOrder(DEV, grid)
        d_polys = torch.from_numpy(polys).to(DEV)
        for gap, back, offset in PARAMS:
            tag = 'reading[%s] gap=%d back=%d offset=%d' % (name, gap, back, offset)
            links = RD.links_cpu(polys, gs, aspect, gap, back, offset, grid)
            want = RD.lines_cpu(polys, gs, aspect, gap, back, offset, grid)
            got = reader.run(d_polys, gs, aspect, gap, back, offset, want_links=True)
            _compare(tag, got, want, links, out, '%d words, %d lines' % (len(polys), int(want['n_lines'].sum())))
            linked += int((want['succ'] >= 0).sum())
            lines += int(want['n_lines'].sum())
    out.append(rec('reading: the cases link words and cut cycles somewhere', 0 if linked > 1000 and lines > 1000 else 1, 0, '%d links, %d lines' % (linked, lines)))
    # links + lines where a thread of the lines kernel owns a second and a third word: one content kind per group, default parameters
    polys, gs, aspect = _case(np.random.RandomState(19), LARGE_SIZES, 4096, LARGE_KINDS)
    links = RD.links_cpu(polys, gs, aspect, grid=4096)
    want = RD.resolve_cpu(links[0], links[1], gs, RD.features_cpu(OV._check_polys(polys, 4096), RD._aspect_per_word(gs, aspect)))   # lines_cpu, its links shared
    got = RD.ReadingOrder(DEV, 4096).run(polys, gs, aspect, want_links=True)
    _compare('reading[grid=4096 groups=%s]' % (list(LARGE_SIZES),), got, want, links, out, '%d words, %d lines' % (len(polys), int(want['n_lines'].sum())))
    # the ring alone: one cycle, cut in front of word 0
    got = RD.ReadingOrder(DEV, 1000).run(RC.ring(), [0, 10], [[256, 256]])
    out.append(rec('reading: ring of 10 is one line from word 0', int(got['line_pos'].tolist() != list(range(10))) + int(got['n_lines'].tolist() != [1]), 0))
    r = RD.ReadingOrder(DEV, 1000).run(torch.zeros(0, 32, dtype=torch.int32), [0, 0, 0], [[1, 1], [2, 2]])
    out.append(rec('reading: no words, no launch', int(r['rank'].size) + int(r['n_lines'].tolist() != [0, 0]), 0))
    return out


def check_reading_largest_group():
    """one group of exactly 8192 words: a page of 128 rows of 64 on the 4096 grid"""
    from tests.gpu_checks import DEV
    rng = np.random.RandomState(5)
    pts = RC.page_points(128, 64, w=40, h=16, gap=12, pitch=30, centre=(2048.0, 2048.0), jitter=1.0)
    polys = RC.to_bins(RC.rotate(pts, 1.5, np.asarray((2048.0, 2048.0)))[rng.permutation(8192)])
    gs, aspect = np.asarray([0, 8192], np.int32), np.asarray([[256, 181]], np.int32)
    links = RD.links_cpu(polys, gs, aspect, grid=4096)
    want = RD.resolve_cpu(links[0], links[1], gs, RD.features_cpu(OV._check_polys(polys, 4096), np.repeat(aspect, 8192, 0)))   # lines_cpu, its links shared
    got = RD.ReadingOrder(DEV, 4096).run(polys, gs, aspect, want_links=True)
    out = []
    _compare('reading[n=8192]', got, want, links, out, '%d lines' % int(want['n_lines'][0]))
    from tests.gpu_checks import rec
    out.append(rec('reading[n=8192] the page is 128 lines of 64', 0 if int(want['n_lines'][0]) == 128 and int(want['line_pos'].max()) == 63 else 1, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# line resolution alone, on planted links: reading_lines_kernel with 2 .. 8 words per thread
# ---------------------------------------------------------------------------------------------------------------------------------
RESOLUTION_SIZES = (1023, 1024, 1025, 2048, 2049, 4097, 8191, 8192)       # 1 | 1 | 2 ragged | 2 | 3 ragged | 5 ragged | 8 ragged | 8 words per thread
MIXED_SIZES = (1025, 0, 1, 8192, 1023)                                    # the LDS layout follows cap = 8192 while ng differs
STRUCTURES = ('chain', 'cycle', 'many', 'stars equal', 'stars distinct', 'extremes', 'ignored')
COST_MAX = 2 ** 43 - 1                                                    # the bound of csrc/reading.hip's header


def _segments(n, rng):
    """lengths and kinds that fill n: cycles of exactly 1023, 1024 and 1025 where they fit beside a 2-cycle, two 2-cycles, then short
    cycles (2 or more members) and paths in turn -> [(length, is_cycle)]"""
    segs, used = [], 0
    for c in (1023, 1024, 1025):
        if used + c + 2 <= n:
            segs.append((c, True))
            used += c
    for _ in range(2):
        if used + 2 <= n:
            segs.append((2, True))
            used += 2
    while used < n:
        m = min(n - used, int(rng.randint(1, 40)))
        segs.append((m, m >= 2 and len(segs) % 2 == 0))
        used += m
    return segs


def _star(succ, cost, members, equal):
    """members[1:] all claim members[0]; equal costs (the lowest index wins), or distinct ones with the least at the highest index"""
    b, claim = int(members[0]), np.sort(members[1:])
    succ[claim] = b
    cost[claim] = 7 if equal else 1000 + (claim.max() - claim)


def group_links(kind, n, rng):
    """one group's planted links, local indices -> (succ0 int64 [n], cost0 int64 [n], ignored bool [n]: entries the kernel is documented
    to ignore; with kind 'ignored' some point outside 0 .. n - 1, which the caller turns into indices of a neighbouring group)"""
    succ = np.full(n, -1, dtype=np.int64)
    cost = rng.randint(0, COST_MAX + 1, n, dtype=np.int64)
    ignored = np.zeros(n, dtype=bool)
    if n == 0:
        return succ, cost, ignored
    perm = rng.permutation(n)
    if kind in ('chain', 'cycle'):
        succ[perm[:-1]] = perm[1:]
        if kind == 'cycle' and n > 1:
            succ[perm[-1]] = perm[0]
    elif kind in ('many', 'ignored'):
        at = 0
        for m, cyc in _segments(n, rng):
            seg = perm[at:at + m]
            succ[seg[:-1]] = seg[1:]
            if cyc:
                succ[seg[-1]] = seg[0]
            at += m
        if kind == 'ignored' and n >= 8:
            pick = rng.permutation(n)[:max(3, n // 6)]
            third = len(pick) // 3
            succ[pick[:third]] = pick[:third]                                # a word naming itself
            succ[pick[third:2 * third]] = np.where(rng.rand(third) < 0.5, -2 - rng.randint(0, 9, third), n + rng.randint(0, 9, third))   # outside its group
            succ[pick[2 * third:]] = -1                                      # no successor, and a garbage cost
            cost[pick[2 * third:]] = rng.randint(-2 ** 62, 2 ** 62, len(pick) - 2 * third, dtype=np.int64)
            ignored[pick[:2 * third]] = True
    else:                                                                    # stars of 2, 64 and 1025 claimants; the rest is one chain
        at = 0
        for m in (2, 64, 1025):
            if at + m + 1 <= n:
                _star(succ, cost, perm[at:at + m + 1], kind == 'stars equal')
                if kind == 'extremes':
                    cost[perm[at + 1:at + m + 1]] = np.where(rng.rand(m) < 0.5, 0, COST_MAX)
                at += m + 1
        rest = perm[at:]
        succ[rest[:-1]] = rest[1:]
        if kind == 'extremes':
            cost[rest] = np.where(rng.rand(len(rest)) < 0.5, 0, COST_MAX)
            if len(rest) > 1:
                succ[rest[-1]] = perm[0]                                     # a chain that ends in a star's centre: one more claimant
    return succ, cost, ignored


def planted_call(kind, sizes, rng):
    """-> (succ0 int32 [N] global, cost0 int64 [N], the same links with the ignored entries set to -1)"""
    gs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(gs[-1])
    succ0, clean, cost0 = np.full(N, -1, np.int64), np.full(N, -1, np.int64), np.zeros(N, np.int64)
    for g, n in enumerate(sizes):
        s, c, ign = group_links(kind, n, rng)
        lo = int(gs[g])
        inside = (s >= 0) & (s < n)
        # -2, -3, ...: the words in front of the group, from its neighbour's last; n, n + 1, ...: the words behind it.  At the ends of a
        # call these leave the call altogether (below 0 or from N on): the kernel compares them and never uses them as an index
        glob = np.where(s == -1, -1, np.where(s < -1, lo + s + 1, lo + s))
        assert (ign | inside | (s == -1)).all() and not (ign & (glob >= lo) & (glob < lo + n) & (glob != np.arange(lo, lo + n))).any()
        succ0[lo:lo + n] = glob
        clean[lo:lo + n] = np.where(ign, -1, glob)
        cost0[lo:lo + n] = c
    assert succ0.max() < 2 ** 31 and (clean < N).all()
    return succ0.astype(np.int32), cost0, clean.astype(np.int32)


def _cycle_lengths(succ):
    """the lengths of the cycles of links without contests (every word named at most once)"""
    succ = [int(v) for v in succ]
    seen, out = [False] * len(succ), []
    for i in range(len(succ)):
        j, m = i, 0
        while j >= 0 and not seen[j]:
            seen[j] = True
            j, m = succ[j], m + 1
        if j == i and m:
            out.append(m)
    return out


def _resolution_words(content, sizes, rng, grid):
    N = int(sum(sizes))
    if content == 'identical':                                               # every line ordering ties down to the head's index
        return np.tile(rng.randint(0, grid, size=(1, 32)), (N, 1)).astype(np.int32)
    if content == 'bottom':                                                  # every y at the last bin: the largest sum a line can hold
        p = rng.randint(0, grid, size=(N, 32)).astype(np.int32)
        p[:, 1::2] = grid - 1
        return p
    return rng.randint(0, grid, size=(N, 32)).astype(np.int32)


def _resolution_calls():
    """(name, structure, content, sizes, aspect)"""
    for n in RESOLUTION_SIZES:
        for kind in STRUCTURES:
            yield 'n=%d' % n, kind, 'random', (n,), ((256, 256),)
        for kind in ('chain', 'cycle', 'many', 'stars equal'):
            yield 'n=%d' % n, kind, 'identical', (n,), ((37, 256),)
    yield 'n=8192 every y = 4095', 'chain', 'bottom', (8192,), ((256, 256),)
    for kind in STRUCTURES:
        yield 'groups=%s' % (list(MIXED_SIZES),), kind, 'random', MIXED_SIZES, tuple(ASPECTS[g % 4] for g in range(len(MIXED_SIZES)))


def check_reading_resolution():
    """omp_reading_lines on links that no geometry produces == resolve_cpu on the same links, on succ, pred, line, line_pos, rank and
    n_lines: one chain through a whole group, the chain closed into a cycle, many cycles and paths (2-cycles, cycles of exactly 1023,
    1024 and 1025), stars of 2, 64 and 1025 claimants, the cost extremes 0 and 2^43 - 1; groups of 1023 .. 8192 words alone and mixed
    in one call.  The kernel is documented to ignore a word naming itself, a successor outside its group and succ0 = -1 whatever its
    cost; resolve_cpu is only defined for in-group links, so the expectation is resolve_cpu with exactly those entries set to -1."""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV, rec
    grid = 4096
    out = []
    rng = np.random.RandomState(21)
    seen = dict(longest=0, lines=0, losers=0, cut=0, ignored=0, big_cycles=set())
    for name, kind, content, sizes, aspect in _resolution_calls():
        gs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        N, G = int(gs[-1]), len(sizes)
        aspect = np.asarray(aspect, dtype=np.int32).reshape(G, 2)
        polys = _resolution_words(content, sizes, rng, grid)
        succ0, cost0, clean = planted_call(kind, sizes, rng)
        want = RD.resolve_cpu(clean, cost0, gs, RD.features_cpu(polys, RD._aspect_per_word(gs, aspect)))
        host = np.concatenate([gs, aspect.reshape(-1)]).astype(np.int32)
        d_polys, tables = torch.from_numpy(polys).to(DEV), torch.from_numpy(host).to(DEV)
        ints = ops.reading_lines(d_polys, tables, host, G, grid, torch.from_numpy(succ0).to(DEV), torch.from_numpy(cost0).to(DEV))
        got = dict(zip(OUTS, ops.split_reading_ints(ints.cpu().numpy(), N)))
        bad = sum(int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else 10 ** 6 for k in OUTS)
        out.append(rec('resolution[%s] %s, %s words: succ, pred, line, line_pos, rank, n_lines' % (name, kind, content), bad, 0,
                       '%d lines, longest %d' % (int(want['n_lines'].sum()), int(want['line_pos'].max()) + 1)))
        # what the reference says the planted links did
        linked = clean >= 0
        if kind == 'chain':
            out.append(rec('precondition: resolution[%s] chain, %s words: one line through every group' % (name, content),
                           int((want['n_lines'] != (np.diff(gs) > 0)).sum()) + int(int(want['line_pos'].max()) != max(sizes) - 1), 0))
        if kind == 'cycle':
            heads = [int(want['line_pos'][gs[g]]) for g in range(G) if sizes[g]]
            out.append(rec('precondition: resolution[%s] cycle, %s words: one line per group, cut in front of its least index' % (name, content),
                           int((want['n_lines'] != (np.diff(gs) > 0)).sum()) + int(any(heads)), 0))
        seen['longest'] = max(seen['longest'], int(want['line_pos'].max()) + 1)
        seen['lines'] += int(want['n_lines'].sum())
        seen['losers'] += int((linked & (want['succ'] != clean)).sum()) if kind.startswith('stars') or kind == 'extremes' else 0
        seen['cut'] += int((linked & (want['succ'] == -1)).sum()) if kind in ('cycle', 'many') else 0
        seen['ignored'] += int((succ0 != clean).sum())
        if kind == 'many':
            seen['big_cycles'] |= set(c for c in _cycle_lengths(clean) if c > 1000)
    ok = (seen['longest'] == 8192 and seen['losers'] > 5000 and seen['cut'] > 500 and seen['ignored'] > 1000 and seen['big_cycles'] == {1023, 1024, 1025})
    out.append(rec('precondition: the planted links hold a line of 8192, lost contests, cut cycles of 1023 / 1024 / 1025 and ignored entries', 0 if ok else 1, 0,
                   '%s' % (sorted(seen.items(), key=lambda kv: kv[0]),)))
    return out


def check_reading_refusals():
    """what the entry points refuse comes back as an error code and a message, before any launch; nothing aborts"""
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    polys = torch.zeros(2, 32, dtype=torch.int32, device=DEV)
    good = np.asarray([0, 2, 256, 256], dtype=np.int32)
    tables = torch.from_numpy(good).to(DEV)
    succ0 = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    cost0 = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    ints = torch.full((12,), -7, dtype=torch.int32, device=DEV)
    out = []

    def refused(what, fn, entry):
        try:
            fn()
            bad = 1
        except RuntimeError as e:
            bad = 0 if entry in str(e) else 1
        out.append(rec('%s refuses %s with an error code' % (entry, what), bad, 0))

    host_cases = (('aspect 0', [0, 2, 0, 256]), ('aspect 257', [0, 2, 256, 257]), ('group_start from 1', [1, 2, 256, 256]),
                  ('group_start to 3', [0, 3, 256, 256]))
    for entry in ('omp_reading_links', 'omp_reading_lines'):
        links = entry.endswith('links')

        def call(host=good, grid=1000, params=(2000, 500, 500), G=1, tab=tables):
            if links:
                return ops.reading_links(polys, tab, np.asarray(host, np.int32), G, grid, *params)
            return ops.reading_lines(polys, tab, np.asarray(host, np.int32), G, grid, succ0, cost0, out=ints[:10 + G])
        for what, grid in (('grid 4097', 4097), ('grid 1', 1)):
            refused(what, lambda: call(grid=grid), entry)
        for what, host in host_cases:
            refused(what, lambda: call(host=host), entry)
        t2 = torch.zeros(7, dtype=torch.int32, device=DEV)
        refused('a falling group_start', lambda: call(host=[0, 3, 2, 256, 256, 256, 256], G=2, tab=t2), entry)
        if links:
            for what, params in (('gap -1', (-1, 500, 500)), ('gap 10001', (10001, 500, 500)), ('back 10001', (2000, 10001, 500)),
                                 ('offset -1', (2000, 500, -1)), ('offset 10001', (2000, 500, 10001))):
                refused(what, lambda: call(params=params), entry)
        # n < 0 cannot come from a tensor: the C entry itself
        lib = _lib.lib()
        h = np.asarray([0, 0], np.int32)
        if links:
            rc = lib.omp_reading_links(None, -1, None, h.ctypes.data, 0, 1000, 2000, 500, 500, None, None, None)
        else:
            rc = lib.omp_reading_lines(None, -1, None, h.ctypes.data, 0, 1000, None, None, None, None, None, None, None, None, None)
        out.append(rec('%s refuses n = -1 with an error code' % entry, 0 if rc != 0 else 1, 0))
        h = np.asarray([0], np.int32)
        if links:
            rc = lib.omp_reading_links(None, 0, None, h.ctypes.data, 0, 1000, 2000, 500, 500, None, None, None)
        else:
            rc = lib.omp_reading_lines(None, 0, None, h.ctypes.data, 0, 1000, None, None, None, None, None, None, None, None, None)
        out.append(rec('%s: n = 0 is fine and launches nothing' % entry, abs(int(rc)), 0))
    torch.cuda.synchronize()
    untouched = int((succ0 != -7).sum()) + int((cost0 != -7).sum()) + int((ints != -7).sum())
    out.append(rec('reading: a refused call writes nothing', untouched, 0))
    # a group of 8193: the device refuses it -- n_lines = -1 and nothing else -- and the Python stage raises
    n = OV.GROUP_MAX + 1
    big = torch.zeros(n, 32, dtype=torch.int32, device=DEV)
    host = np.asarray([0, n, n, 256, 256, 256, 256], dtype=np.int32)
    t3 = torch.from_numpy(host).to(DEV)
    s0, c0 = ops.reading_links(big, t3, host, 2, 1000, 2000, 500, 500)
    res = ops.reading_lines(big, t3, host, 2, 1000, s0, c0, out=torch.full((5 * n + 2,), -7, dtype=torch.int32, device=DEV)).cpu().numpy()
    out.append(rec('reading: a group of 8193 gives n_lines = -1 and nothing else', int((res[:5 * n] != -7).sum()) + int(res[5 * n:].tolist() != [-1, 0]), 0))
    try:
        RD.ReadingOrder(DEV, 1000).run(big, [0, n], [[256, 256]])
        bad = 1
    except RuntimeError:
        bad = 0
    out.append(rec('reading: ReadingOrder raises on a group of 8193', bad, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
def _minus(r, keys=('line', 'line_pos')):
    return {k: v for k, v in r.items() if k not in keys}


def _expected(records, polys_per_image, sizes, grid):
    """lines_cpu on the host -> per image the records in reading order with `line` / `line_pos` attached (copies)"""
    out = []
    for recs, polys, hw in zip(records, polys_per_image, sizes):
        res = RD.lines_cpu(polys, [0, len(recs)], [RD.aspect_of(*hw)], grid=grid)
        order = np.argsort(res['rank'])
        out.append([dict(copy.deepcopy(recs[i]), line=int(res['line'][i]), line_pos=int(res['line_pos'][i])) for i in order])
    return out


def check_engine_reading(dtype_name):
    """spot_windows' image and weights, windows = [default, 2 x 2 grid], suppress=0.5: predict(reading_order=True) == lines_cpu on the
    survivors' raw polygon ids"""
    from advancedliteratemachinery_amd.engine import inference as inf
    from advancedliteratemachinery_amd.utils.nested_tensor import NestedTensor
    from tests.gpu_checks import DEV, ENGINES, build_model, golden, rec
    from tests.gpu_checks_windows import fixture_case
    gold = golden('spot_windows')
    args, sd, img, mask, _ = fixture_case(gold, 'eos')
    model = build_model(args, sd, gold['case']['depths'], ENGINES[dtype_name])
    nt = NestedTensor(img.to(DEV), mask.to(DEV))
    wins = [WN.default_window(args)] + WN.grid_windows(2, 2, args.num_bins)
    tag = 'reading engine[%s]' % dtype_name
    out = []
    unsup = inf.predict(model, nt, args, windows=wins)
    plain = inf.predict(model, nt, args, windows=wins, suppress=0.5)
    again = inf.predict(model, nt, args, windows=wins, suppress=0.5, reading_order=False, line_gap=3.0)
    out.append(rec(tag + ' reading_order=False is today\'s predict', 0 if again == plain and all('line' not in r for r in plain[0]) else 1, 0,
                   '%d records' % len(plain[0])))
    raw, _ = inf.predict_raw(model, nt, args, windows=WN.resolve_windows(wins, 1))
    raw_polys = [None if r is None else r[0][1] for r in raw]
    rows = []
    OV.suppress_records(copy.deepcopy(unsup), raw_polys, args.num_bins, 0.5, device=DEV, kept_rows=rows)
    sizes = [(int(nt.tensors.shape[2]), int(nt.tensors.shape[3]))] * len(plain)
    surv = [torch.as_tensor(p).reshape(-1, 32)[rows[b]].cpu().numpy() if p is not None else np.zeros((0, 32), np.int64) for b, p in enumerate(raw_polys)]
    for kw in (dict(), dict(line_gap=0.5, line_back=0.0, line_offset=0.25)):
        got = inf.predict(model, nt, args, windows=wins, suppress=0.5, reading_order=True, **kw)
        name = '%s %s' % (tag, kw or 'defaults')
        for b in range(len(plain)):
            perm = sorted(map(repr, map(_minus, got[b]))) == sorted(map(repr, plain[b]))
            out.append(rec(name + ' the records are a permutation of the call without reading_order', 0 if perm else 1, 0, '%d records' % len(got[b])))
        gap, back, offset = RD.check_reading_args(kw.get('line_gap', 2.0), kw.get('line_back', 0.5), kw.get('line_offset', 0.5))
        want = []
        for recs, polys, hw in zip(plain, surv, sizes):
            res = RD.lines_cpu(polys, [0, len(recs)], [RD.aspect_of(*hw)], gap, back, offset, args.num_bins)
            want.append([dict(recs[i], line=int(res['line'][i]), line_pos=int(res['line_pos'][i])) for i in np.argsort(res['rank'])])
        out.append(rec(name + ' order, line, line_pos == lines_cpu on the survivors\' polygon ids', 0 if got == want else 1, 0,
                       '%d lines' % (max(r['line'] for r in got[0]) + 1 if got[0] else 0)))
        out.append(rec(name + ' the fixture has words to order', 0 if len(got[0]) >= 2 else 1, 0))
    # no suppress=, no windows, with lexicon=: every row, lexicon on the reordered records
    plain = inf.predict(model, nt, args)
    raw, _ = inf.predict_raw(model, nt, args)
    got = inf.predict(model, nt, args, reading_order=True, lexicon=['word', 'text'])
    want = _expected(plain, [r[0][1].reshape(-1, 32).cpu().numpy() for r in raw], sizes, args.num_bins)
    same = [[_minus(r, ('lex', 'lex_index', 'lex_dist')) for r in recs] for recs in got] == want and all('lex_dist' in r for r in got[0])
    out.append(rec(tag + ' no windows, no suppress: every row, lexicon on the reordered records', 0 if same else 1, 0, '%d records' % len(got[0])))
    return out


def check_two_stage_reading():
    """spot_and_recognize(crop='polygon', reading_order=True): the records are ordered before the crops; every mgp_* stays with the
    record whose crop it read"""
    from advancedliteratemachinery_amd.engine.two_stage import spot_and_recognize
    from oracle import mgp_str_ref as R
    from tests.gpu_checks import build_model, rec
    from tests.gpu_checks_mgp import build
    depths = (2, 2, 2, 2)
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, pt_seq_length=6, test_min_size=64, test_max_size=112)
    sd = weights.make_state_dict(args, seed=5, depths=depths)
    omni = build_model(args, sd, depths, torch.float32)
    c = R.cfg(depth=2)
    mgp = build(c, R.make_state_dict(c, seed=17), torch.float32)
    rng = np.random.RandomState(3)
    images = [torch.from_numpy(rng.randint(0, 256, (90, 140, 3), dtype=np.uint8)), torch.from_numpy(rng.randint(0, 256, (70, 100, 3), dtype=np.uint8))]
    wins = [WN.default_window(args)] + WN.grid_windows(2, 2, args.num_bins)
    out = []
    plain, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon', windows=wins, ragged=True)
    got, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon', windows=wins, ragged=True, reading_order=True)
    out.append(rec('two-stage reading: there are words', 0 if sum(len(p) for p in plain) >= 2 else 1, 0, '%d records' % sum(len(p) for p in plain)))
    bad = 0
    for b, (recs, before) in enumerate(zip(got, plain)):
        bad += int(sorted(map(repr, map(_minus, recs))) != sorted(map(repr, before)))        # crop i of the plain call is on the same record
        bad += int(any('mgp_text' not in r or 'line' not in r for r in recs))
        bad += int(sorted((r['line'], r['line_pos']) for r in recs) != [(r['line'], r['line_pos']) for r in recs])   # in reading order
    out.append(rec('two-stage reading: every mgp_* stays with the record whose crop it read, records in reading order', bad, 0))
    bad = 0
    for recs in got:
        n_lines = len(set(r['line'] for r in recs))
        lines = RD.page_lines(recs, field='mgp_text')
        bad += int(len(lines) != n_lines) + int(n_lines != (max(r['line'] for r in recs) + 1 if recs else 0))
        bad += int(' '.join(lines).split(' ') != [str(r['mgp_text']) for r in recs]) if recs and all(' ' not in r['mgp_text'] and r['mgp_text'] for r in recs) else 0
    out.append(rec('two-stage reading: page_lines(field=mgp_text) has n_lines entries', bad, 0))
    return out
