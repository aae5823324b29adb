"""GPU checks of the block stage: omp_reading_blocks against its numpy specification (utils/reading.py:
blocks_cpu) on every output integer -- block, line, rank, n_blocks, levels -- and `blocks=` of predict / spot_and_recognize against
lines_cpu + blocks_cpu applied on the host to the same call's polygon ids.  Every check returns records {name, err, tol, ok, note}
like tests/gpu_checks.py."""
import copy

import numpy as np
import torch

from advancedliteratemachinery_amd.utils import overlap as OV
from advancedliteratemachinery_amd.utils import reading as RD
from advancedliteratemachinery_amd.utils import synthetic as weights
from advancedliteratemachinery_amd.utils import windows as WN
from advancedliteratemachinery_amd.utils.parser import make_args
from tests import blocks_cases as BC
from tests import reading_cases as RC

LINE_COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)   # the wave, the sort's sizes and the 8-per-thread chunks from both sides
ASPECTS = ((256, 256), (256, 128), (37, 256), (1, 1))
PARAMS = ((1000, 1500, 8), (0, 0, 16), (10000, 10000, 2), (1000, 1500, 1))   # gap_x, gap_y, depth
KINDS = ('columns', 'nested', 'random', 'duplicates', 'degenerate')
OUTS = ('block', 'line', 'rank', 'n_blocks', 'levels')


# ---------------------------------------------------------------------------------------------------------------------------------
# pages whose lines are GIVEN: the line counts are exact
# ---------------------------------------------------------------------------------------------------------------------------------
def group_lines(rng, n_lines, grid, kind):
    """-> (polys int32 [n, 32], line int32 [n], line_pos int32 [n]) of one group with exactly n_lines lines, words in shuffled order"""
    if n_lines == 0:
        return np.zeros((0, 32), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    if kind == 'nested':
        return BC.random_lines_page(rng, n_lines, grid)
    if kind == 'random':
        p = rng.randint(-grid // 50 - 1, grid + grid // 50 + 1, size=(n_lines, 32)).astype(np.int32)   # tokens may leave the grid: both sides clamp
        return p, rng.permutation(n_lines).astype(np.int32), np.zeros(n_lines, np.int32)
    if kind == 'degenerate':
        pts = rng.randint(0, grid, size=(max(1, n_lines // 3), 2))
        p = np.tile(pts[rng.randint(len(pts), size=n_lines)], (1, 16)).astype(np.int32)                 # all 16 points equal, many lines on one point
        return p, rng.permutation(n_lines).astype(np.int32), np.zeros(n_lines, np.int32)
    cols = 2 + int(rng.randint(0, 3))
    rows = (n_lines + cols - 1) // cols
    words = 1 + int(rng.randint(0, 2))
    cw = 0.9 * grid / cols
    w, h = max(1.0, 0.7 * cw / words), max(1.0, 0.5 * 0.9 * grid / rows)
    polys, line, pos = [], [], []
    for l in range(n_lines):
        c, r = l // rows, l % rows
        for k in range(words):
            polys.append(RC.word(0.05 * grid + c * cw + k * (w + 0.05 * cw / words), 0.05 * grid + r * 0.9 * grid / rows, w, h))
            line.append(l)
            pos.append(k)
    p = np.clip(RC.to_bins(np.stack(polys)), 0, grid - 1)
    line, pos = np.asarray(line, np.int32), np.asarray(pos, np.int32)
    renumber = rng.permutation(n_lines).astype(np.int32)                    # line numbers carry no geometry
    line = renumber[line]
    if kind == 'duplicates' and n_lines > 1:
        src = rng.randint(0, len(p), size=len(p) // 3)
        p[rng.randint(0, len(p), size=len(src))] = p[src]                   # exact duplicates: ties go to the line number
    order = rng.permutation(len(p))
    return p[order], line[order], pos[order]


def _case(rng, counts, grid, kinds=KINDS):
    parts = [group_lines(rng, int(n), grid, kinds[g % len(kinds)]) for g, n in enumerate(counts)]
    gs = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int32)
    aspect = np.asarray([ASPECTS[(g // 2) % len(ASPECTS)] for g in range(len(counts))], dtype=np.int32).reshape(-1, 2)
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), gs, aspect,
            np.asarray(counts, np.int32))


def _cases():
    """(name, polys, line, line_pos, group_start, aspect, n_lines, grid): the smallest shapes that can break the kernel"""
    rng = np.random.RandomState(19)
    for grid in (1000, 4096, 64):
        for shift in (0, 1):                                                 # every count meets two kinds of content and two aspects
            counts = LINE_COUNTS[shift * 3:] + LINE_COUNTS[:shift * 3]
            yield ('grid=%d lines=%s' % (grid, list(counts)),) + _case(rng, counts, grid) + (grid,)
    for k, kind in enumerate(KINDS):                                         # G = 1, each content alone
        yield ('G=1 lines=257 %s' % kind,) + _case(rng, (257,), 1000, (kind,))[:4] + (np.asarray([ASPECTS[k % 4]], np.int32), np.asarray([257], np.int32), 1000)
    counts = rng.randint(0, 40, 40)
    counts[[3, 4, 17, 39]] = 0                                               # empty groups between full ones, and at the end
    counts[[5, 18]] = 300
    yield ('G=40 mixed',) + _case(rng, counts, 1000) + (1000,)


def device_blocks(polys, line, pos, gs, aspect, n_lines, grid, gap_x, gap_y, depth, fill=None):
    """ops.reading_blocks on given lines -> blocks_cpu's dict as numpy"""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV
    N, G = len(polys), len(gs) - 1
    host = np.concatenate([np.asarray(gs, np.int32), np.asarray(aspect, np.int32).reshape(-1)]).astype(np.int32)
    lines = np.zeros(5 * N + G, np.int32)
    lines[2 * N:3 * N], lines[3 * N:4 * N], lines[5 * N:] = line, pos, n_lines
    out = None if fill is None else torch.full((3 * N + 2 * G,), fill, dtype=torch.int32, device=DEV)
    d_polys = torch.from_numpy(np.ascontiguousarray(polys, dtype=np.int32)).to(DEV).reshape(N, 32)
    ints = ops.reading_blocks(d_polys, torch.from_numpy(host).to(DEV), host, G, grid, torch.from_numpy(lines).to(DEV), gap_x, gap_y, depth, out=out)
    return dict(zip(OUTS, (v.cpu().numpy() for v in ops.split_block_ints(ints, N, G))))


def _bad(got, want):
    return sum(int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else 10 ** 6 for k in OUTS)


def check_blocks_op():
    from tests.gpu_checks import rec
    out = []
    blocks, deep = 0, 0
    for name, polys, line, pos, gs, aspect, n_lines, grid in _cases():
        for gap_x, gap_y, depth in PARAMS:
            want = RD.blocks_cpu(polys, gs, aspect, line, pos, n_lines, gap_x, gap_y, depth, grid)
            got = device_blocks(polys, line, pos, gs, aspect, n_lines, grid, gap_x, gap_y, depth)
            out.append(rec('blocks[%s] gap_x=%d gap_y=%d depth=%d block, line, rank, n_blocks, levels' % (name, gap_x, gap_y, depth), _bad(got, want), 0,
                           '%d words, %d lines, %d blocks, levels up to %d' % (len(polys), int(n_lines.sum()), int(want['n_blocks'].sum()), int(want['levels'].max()))))
            blocks += int(want['n_blocks'].sum())
            deep = max(deep, int(want['levels'].max()))
    out.append(rec('blocks: the cases cut pages and nest', 0 if blocks > 1000 and deep >= 6 else 1, 0, '%d blocks, %d levels' % (blocks, deep)))
    return out


def check_blocks_pipeline():
    """ReadingOrder.run(blocks=...): links, lines and blocks in one call against lines_cpu + blocks_cpu, on column pages, the nested
    page, random 16-gons, duplicates and degenerate groups; the lines of the call stay lines_cpu's"""
    from tests.gpu_checks import DEV, rec
    from tests.gpu_checks_reading import group_words
    rng = np.random.RandomState(23)
    parts = [RC.to_bins(BC.column_page(cols=2, rows=5, words=2)[0]), RC.to_bins(BC.column_page(cols=3, rows=7, words=3, w=40, gap=8, gutter=60)[0]),
             RC.to_bins(BC.nested_page()[0]), np.zeros((0, 32), np.int32), group_words(rng, 257, 1000, 'random'), group_words(rng, 130, 1000, 'duplicates'),
             group_words(rng, 65, 1000, 'degenerate'), group_words(rng, 300, 1000, 'rows')]
    parts = [p[rng.permutation(len(p))] for p in parts]
    polys = np.concatenate(parts).astype(np.int32)
    gs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    aspect = np.asarray([ASPECTS[0]] * 4 + [ASPECTS[g % 4] for g in range(4)], np.int32)
    reader = RD.ReadingOrder(DEV, 1000)
    plain = reader.run(polys, gs, aspect)
    out = []
    for gap_x, gap_y, depth in PARAMS:
        lines = RD.lines_cpu(polys, gs, aspect, grid=1000)
        want = RD.blocks_cpu(polys, gs, aspect, lines['line'], lines['line_pos'], lines['n_lines'], gap_x, gap_y, depth, 1000)
        got = reader.run(polys, gs, aspect, blocks=(gap_x, gap_y, depth))
        tag = 'blocks pipeline gap_x=%d gap_y=%d depth=%d' % (gap_x, gap_y, depth)
        out.append(rec(tag + ' block, line, rank, n_blocks, levels', _bad(got['blocks'], want), 0, '%s blocks, %s levels' % (want['n_blocks'].tolist(), want['levels'].tolist())))
        same = all((got[k] == plain[k]).all() and (got[k] == lines[k]).all() for k in ('succ', 'pred', 'line', 'line_pos', 'rank', 'n_lines'))
        out.append(rec(tag + ' the lines of the call are lines_cpu\'s and the call\'s without blocks', 0 if same else 1, 0))
    want = RD.blocks_cpu(polys, gs, aspect, lines['line'], lines['line_pos'], lines['n_lines'], grid=1000)
    out.append(rec('blocks pipeline: the column pages are 4 and 5 blocks, the nested page 5', 0 if want['n_blocks'][:4].tolist() == [4, 5, 5, 0] else 1, 0,
                   str(want['n_blocks'].tolist())))
    # order_records on the real device stage: a two-column page under a headline comes headline, left column, right column, footer
    pts, names = BC.column_page(cols=2, rows=5, words=2)
    order = rng.permutation(len(pts))
    recs = RD.order_records([[dict(rec=str(names[i])) for i in order]], [torch.from_numpy(RC.to_bins(pts[order])).to(DEV)], [(1000, 1000)], 1000,
                            blocks=True, device=DEV)[0]
    names = [('head',)] + [('col', c, r, k) for c in range(2) for r in range(5) for k in range(2)] + [('foot',)]
    ok = ([r['rec'] for r in recs] == [str(n) for n in names] and [r['block'] for r in recs] == [0] + [1] * 10 + [2] * 10 + [3]
          and [r['line'] for r in recs] == [0] + [1 + l for l in range(10) for _ in range(2)] + [11])
    out.append(rec('blocks: order_records(blocks=True) reads a two-column page column by column', 0 if ok else 1, 0))
    r = reader.run(torch.zeros(0, 32, dtype=torch.int32), [0, 0, 0], [[1, 1], [2, 2]], blocks=(1000, 1500, 8))
    out.append(rec('blocks: no words, no launch', int(r['blocks']['rank'].size) + int(r['blocks']['n_blocks'].tolist() != [0, 0]), 0))
    return out


def check_blocks_largest_group():
    """one group of exactly 8192 single-word lines, 8 columns of 1024, on the 4096 grid: 128 KB of LDS, sorts of 8192"""
    from tests.gpu_checks import rec
    rng = np.random.RandomState(6)
    polys = RC.to_bins(np.stack([RC.word(40 + 500 * c, 2 + 4 * r, 300, 2) for c in range(8) for r in range(1024)]))
    order = rng.permutation(8192)
    polys = polys[order]
    line, pos = rng.permutation(8192).astype(np.int32), np.zeros(8192, np.int32)
    gs, aspect, n_lines = np.asarray([0, 8192], np.int32), np.asarray([[256, 181]], np.int32), np.asarray([8192], np.int32)
    out = []
    for gap_x, gap_y, depth in ((1000, 1500, 8), (0, 0, 3)):
        want = RD.blocks_cpu(polys, gs, aspect, line, pos, n_lines, gap_x, gap_y, depth, 4096)
        got = device_blocks(polys, line, pos, gs, aspect, n_lines, 4096, gap_x, gap_y, depth)
        out.append(rec('blocks[lines=8192] gap_x=%d gap_y=%d depth=%d' % (gap_x, gap_y, depth), _bad(got, want), 0,
                       '%d blocks, %d levels' % (int(want['n_blocks'][0]), int(want['levels'][0]))))
        if depth == 8:
            cols = (order // 1024)[np.argsort(want['rank'])]
            ok = int(want['n_blocks'][0]) == 8 and cols.tolist() == sorted(cols.tolist())
            out.append(rec('blocks[lines=8192] the page is 8 columns read one after the other', 0 if ok else 1, 0))
        else:
            out.append(rec('blocks[lines=8192] gap 0 cuts every row of every column', 0 if int(want['n_blocks'][0]) == 8192 else 1, 0))
    return out


def check_blocks_refusals():
    """what the entry point refuses comes back as an error code and a message, before any launch; nothing aborts"""
    from advancedliteratemachinery_amd import _lib, ops
    from tests.gpu_checks import DEV, rec
    polys = torch.zeros(2, 32, dtype=torch.int32, device=DEV)
    good = np.asarray([0, 2, 256, 256], dtype=np.int32)
    tables = torch.from_numpy(good).to(DEV)
    lines = torch.zeros(11, dtype=torch.int32, device=DEV)
    lines[10] = 1
    ints = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    out = []

    def refused(what, fn):
        try:
            fn()
            bad = 1
        except RuntimeError as e:
            bad = 0 if 'omp_reading_blocks' in str(e) else 1
        out.append(rec('omp_reading_blocks refuses %s with an error code' % what, bad, 0))

    def call(host=good, grid=1000, params=(1000, 1500, 8), G=1, tab=tables, ln=lines):
        return ops.reading_blocks(polys, tab, np.asarray(host, np.int32), G, grid, ln[:10 + G], *params, out=ints[:6 + 2 * G])

    for what, grid in (('grid 4097', 4097), ('grid 1', 1)):
        refused(what, lambda: call(grid=grid))
    for what, host in (('aspect 0', [0, 2, 0, 256]), ('aspect 257', [0, 2, 256, 257]), ('group_start from 1', [1, 2, 256, 256]),
                       ('group_start to 3', [0, 3, 256, 256])):
        refused(what, lambda: call(host=host))
    t2 = torch.zeros(7, dtype=torch.int32, device=DEV)
    l2 = torch.zeros(12, dtype=torch.int32, device=DEV)
    ints2 = torch.full((10,), -7, dtype=torch.int32, device=DEV)
    refused('a falling group_start', lambda: ops.reading_blocks(polys, t2, np.asarray([0, 3, 2, 256, 256, 256, 256], np.int32), 2, 1000, l2, 1000, 1500, 8, out=ints2))
    for what, params in (('gap_x -1', (-1, 1500, 8)), ('gap_x 10001', (10001, 1500, 8)), ('gap_y -1', (1000, -1, 8)), ('gap_y 10001', (1000, 10001, 8)),
                         ('depth 0', (1000, 1500, 0)), ('depth 17', (1000, 1500, 17)), ('depth -1', (1000, 1500, -1))):
        refused(what, lambda: call(params=params))
    lib = _lib.lib()
    h = np.asarray([0, 0], np.int32)
    rc = lib.omp_reading_blocks(None, -1, None, h.ctypes.data, 0, 1000, 1000, 1500, 8, None, None, None, None, None, None, None, None, None)
    out.append(rec('omp_reading_blocks refuses n = -1 with an error code', 0 if rc != 0 else 1, 0))
    h = np.asarray([0], np.int32)
    rc = lib.omp_reading_blocks(None, 0, None, h.ctypes.data, 0, 1000, 1000, 1500, 8, None, None, None, None, None, None, None, None, None)
    out.append(rec('omp_reading_blocks: n = 0 is fine and launches nothing', abs(int(rc)), 0))
    rc = lib.omp_reading_blocks(polys.data_ptr(), 2, tables.data_ptr(), good.ctypes.data, 1, 1000, 1000, 1500, 8, None, None, None, None, None, None, None, None, None)
    out.append(rec('omp_reading_blocks refuses null inputs with an error code', 0 if rc != 0 else 1, 0))
    torch.cuda.synchronize()
    out.append(rec('blocks: a refused call writes nothing', int((ints != -7).sum()) + int((ints2 != -7).sum()), 0))
    call()
    torch.cuda.synchronize()
    out.append(rec('blocks: the same call with good arguments runs', int(ints.cpu().tolist() != [0, 0, 0, 0, 0, 0, 1, 2]), 0, str(ints.cpu().tolist())))
    # a group of 8193: the device refuses it -- n_blocks = -1 and nothing else -- and the Python stage raises
    n = OV.GROUP_MAX + 1
    z = np.zeros(n, np.int32)
    res = device_blocks(np.zeros((n, 32), np.int32), z, z, [0, n, n], [[256, 256], [256, 256]], [1, 0], 1000, 1000, 1500, 8, fill=-7)
    bad = sum(int((res[k] != -7).sum()) for k in ('block', 'line', 'rank')) + int(res['n_blocks'].tolist() != [-1, 0]) + int(res['levels'].tolist() != [-7, 0])
    out.append(rec('blocks: a group of 8193 gives n_blocks = -1 and nothing else', bad, 0))
    try:
        RD.ReadingOrder(DEV, 1000).run(torch.zeros(n, 32, dtype=torch.int32, device=DEV), [0, n], [[256, 256]], blocks=(1000, 1500, 8))
        bad = 1
    except RuntimeError:
        bad = 0
    out.append(rec('blocks: ReadingOrder raises on a group of 8193', bad, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
def _minus(r, keys=('block',)):
    return {k: v for k, v in r.items() if k not in keys}


def check_engine_blocks(dtype_name):
    """spot_windows' image and weights, windows = [default, 2 x 2 grid], suppress=0.5: predict(reading_order=True, blocks=True) ==
    lines_cpu + blocks_cpu on the survivors' raw polygon ids"""
    from advancedliteratemachinery_amd.engine import inference as inf
    from advancedliteratemachinery_amd.utils.nested_tensor import NestedTensor
    from tests.gpu_checks import DEV, ENGINES, build_model, golden, rec
    from tests.gpu_checks_windows import fixture_case
    gold = golden('spot_windows')
    args, sd, img, mask, _ = fixture_case(gold, 'eos')
    model = build_model(args, sd, gold['case']['depths'], ENGINES[dtype_name])
    nt = NestedTensor(img.to(DEV), mask.to(DEV))
    wins = [WN.default_window(args)] + WN.grid_windows(2, 2, args.num_bins)
    kw = dict(windows=wins, suppress=0.5)
    tag = 'blocks engine[%s]' % dtype_name
    out = []
    unsup = inf.predict(model, nt, args, windows=wins)
    plain = inf.predict(model, nt, args, **kw)
    ordered = inf.predict(model, nt, args, reading_order=True, **kw)
    again = inf.predict(model, nt, args, reading_order=True, blocks=False, block_gap_x=3.0, block_depth=2, **kw)
    out.append(rec(tag + ' blocks=False is today\'s predict(reading_order=True)', 0 if again == ordered and all('block' not in r for r in ordered[0]) else 1, 0,
                   '%d records' % len(ordered[0])))
    raw, _ = inf.predict_raw(model, nt, args, windows=WN.resolve_windows(wins, 1))
    raw_polys = [None if r is None else r[0][1] for r in raw]
    rows = []
    OV.suppress_records(copy.deepcopy(unsup), raw_polys, args.num_bins, 0.5, device=DEV, kept_rows=rows)
    sizes = [(int(nt.tensors.shape[2]), int(nt.tensors.shape[3]))] * len(plain)
    surv = [torch.as_tensor(p).reshape(-1, 32)[rows[b]].cpu().numpy() if p is not None else np.zeros((0, 32), np.int64) for b, p in enumerate(raw_polys)]
    n_blocks = []
    for bkw in (dict(), dict(block_gap_x=0.0, block_gap_y=0.0, block_depth=16), dict(block_gap_x=0.25, block_gap_y=0.1, block_depth=1)):
        got = inf.predict(model, nt, args, reading_order=True, blocks=True, **dict(kw, **bkw))
        name = '%s %s' % (tag, bkw or 'defaults')
        for b in range(len(plain)):
            perm = sorted(map(repr, (_minus(r, ('block', 'line')) for r in got[b]))) == sorted(map(repr, (_minus(r, ('line',)) for r in ordered[b])))
            out.append(rec(name + ' the records are a permutation of the call without blocks (but for line)', 0 if perm else 1, 0, '%d records' % len(got[b])))
        cut = RD.check_block_args(True, bkw.get('block_gap_x', 1.0), bkw.get('block_gap_y', 1.5), bkw.get('block_depth', 8))
        want = []
        for recs, polys, hw in zip(plain, surv, sizes):
            asp = [RD.aspect_of(*hw)]
            res = RD.lines_cpu(polys, [0, len(recs)], asp, grid=args.num_bins)
            blk = RD.blocks_cpu(polys, [0, len(recs)], asp, res['line'], res['line_pos'], res['n_lines'], *cut, grid=args.num_bins)
            want.append([dict(recs[i], line=int(blk['line'][i]), line_pos=int(res['line_pos'][i]), block=int(blk['block'][i])) for i in np.argsort(blk['rank'])])
            n_blocks.append(int(blk['n_blocks'][0]))
        out.append(rec(name + ' order, block, line, line_pos == lines_cpu + blocks_cpu on the survivors\' polygon ids', 0 if got == want else 1, 0,
                       '%d blocks' % n_blocks[-1]))
    # how many blocks the three parameter sets give is the fixture's business (its random-weight polygons overlap: one block each)
    out.append(rec(tag + ' the fixture has words to put into blocks', 0 if len(plain[0]) >= 2 and min(n_blocks) >= 1 else 1, 0, 'blocks %s' % n_blocks))
    return out


def check_two_stage_blocks():
    """spot_and_recognize(crop='polygon', reading_order=True, blocks=True): the records are ordered before the crops; every mgp_*
    stays with the record whose crop it read"""
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
    got, _, _ = spot_and_recognize(omni, mgp, images, args, crop='polygon', windows=wins, ragged=True, reading_order=True, blocks=True, block_gap_x=0.0,
                                   block_gap_y=0.0)
    out.append(rec('two-stage blocks: there are words', 0 if sum(len(p) for p in plain) >= 2 else 1, 0, '%d records' % sum(len(p) for p in plain)))
    bad = 0
    for recs, before in zip(got, plain):
        bad += int(sorted(map(repr, (_minus(r, ('block', 'line', 'line_pos')) for r in recs))) != sorted(map(repr, before)))   # crop i of the plain call is on the same record
        bad += int(any('mgp_text' not in r or 'block' not in r for r in recs))
        keys = [(r['block'], r['line'], r['line_pos']) for r in recs]
        bad += int(sorted(keys) != keys) + int([r['line'] for r in recs] != sorted(r['line'] for r in recs))               # block by block, lines counting up
    out.append(rec('two-stage blocks: every mgp_* stays with the record whose crop it read, records block by block', bad, 0))
    bad = 0
    for recs in got:
        blocks = RD.page_blocks(recs, field='mgp_text')
        bad += int(len(blocks) != len(set(r['block'] for r in recs))) + int(sum(len(b.split('\n')) for b in blocks) != len(set(r['line'] for r in recs)) if recs else 0)
    out.append(rec('two-stage blocks: page_blocks(field=mgp_text) has one string per block and one row per line', bad, 0))
    return out
