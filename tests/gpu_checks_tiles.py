"""GPU checks of tiled pages: omp_tile_remap against its numpy specification (utils/tiles.py: remap_cpu) on every
output integer; tiled engine calls against every tile submitted alone, against the specification applied to the same ids, against
today's predict_images, with the page stages (suppress=, reading_order=) and through the two-stage reader.  Every check returns records
{name, err, tol, ok, note} like tests/gpu_checks.py; the GPU modules are imported inside the checks."""
import copy

import numpy as np
import torch

from advancedliteratemachinery_amd.utils import overlap as OV
from advancedliteratemachinery_amd.utils import reading as RD
from advancedliteratemachinery_amd.utils import synthetic as weights
from advancedliteratemachinery_amd.utils import tiles as TL
from advancedliteratemachinery_amd.utils.parser import make_args
from tests.tiles_cases import random_case

F32_GRADE = ('fp32', 'bf16x3')
NEW_KEYS = ('tile', 'tile_rect', 'tile_cut')


# ---------------------------------------------------------------------------------------------------------------------------------
# op level: omp_tile_remap == remap_cpu
# ---------------------------------------------------------------------------------------------------------------------------------
OP_WORDS = (1, 63, 64, 65, 1025, 5000)


def _want_ints(spec, cap):
    src = np.full(max(cap, 1) if cap else 0, -1, np.int32)
    n = min(cap, len(spec['src_row']))
    src[:n] = spec['src_row'][:n]
    return np.concatenate([spec['cut'], src, spec['tile_count'], spec['tile_dropped'], spec['out_start'], spec['page_count']])


def _run_op(case, nb, P, edge, drop, cap=None):
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV
    T, pages = len(case['tile_page']), len(case['page_size'])
    tables = np.concatenate([np.asarray(case[k], np.int64).reshape(-1) for k in ('row_start', 'tile_rect', 'tile_page', 'page_size')]).astype(np.int32)
    polys = torch.from_numpy(np.clip(case['polys'], -1, TL.BINS_MAX).astype(np.int32)).to(DEV)
    points = torch.from_numpy(np.clip(case['points'], -1, TL.BINS_MAX).astype(np.int32)).to(DEV)
    res = ops.tile_remap(polys, points, torch.from_numpy(tables).to(DEV), T, pages, nb, P, edge, drop, cap=cap)
    return res['ints'].cpu().numpy(), res['page_polys'].cpu().numpy(), res['page_points'].cpu().numpy()


def _compare(tag, case, nb, P, edge, drop, out):
    from tests.gpu_checks import rec
    spec = TL.remap_cpu(case['polys'], case['points'], case['row_start'], case['tile_rect'], case['tile_page'], case['page_size'], nb, P, edge, drop)
    N, total = len(case['polys']), len(spec['src_row'])
    ints, polys, points = _run_op(case, nb, P, edge, drop)
    want = _want_ints(spec, N)
    bad = int(ints.shape != want.shape) or int((ints != want).sum())
    out.append(rec(tag + ' cut | src_row | tile_count | tile_dropped | out_start | page_count', bad, 0, '%d of %d words kept' % (total, N)))
    bad = int((polys[:total] != spec['page_polys']).sum()) + int((points[:total] != spec['page_points']).sum())
    out.append(rec(tag + ' page_polys, page_points', bad, 0))
    return spec


def check_tile_remap_op():
    from tests.gpu_checks import rec
    out = []
    for i, n in enumerate(OP_WORDS):
        pages = 1 + i % 5
        for j, (nb, P, edge, drop, corner) in enumerate(((1000, 2000, 2, True, False), (1000, 1000, 0, False, False), (4096, 4096, 4096, True, False),
                                                         (1000, 2, 1000, True, False), (4096, 4096, 2, True, True), (4096, 4096, 0, False, True))):
            case = random_case(1000 * i + j, n, pages if not corner else 2, nb=nb, corner=corner)
            tag = 'tile_remap[n=%d,pages=%d,tiles=%d,nb=%d,P=%d,edge=%d,drop=%d%s]' % (n, len(case['page_size']), len(case['tile_page']), nb, P, edge, drop,
                                                                                     ',65535 px' if corner else '')
            spec = _compare(tag, case, nb, P, edge, drop, out)
            if j == 0:
                out.append(rec(tag + ' some tiles are empty and some words are cut', 0 if (n < 63 or ((spec['tile_count'] == 0).any() and
                                                                                             (spec['tile_dropped'] > 0).any())) else 1, 0))
                # a cap at half the total: the head of the list, the counts in full, nothing written beyond the cap
                cap = len(spec['src_row']) // 2
                ints, polys, points = _run_op(case, nb, P, edge, drop, cap=cap)
                want = _want_ints(spec, cap)
                bad = int(ints.shape != want.shape) or int((ints != want).sum())
                bad += int((polys != spec['page_polys'][:cap]).sum()) + int((points != spec['page_points'][:cap]).sum())
                out.append(rec(tag + ' cap=%d: the head of the list, counts in full' % cap, bad, 0))
    # refused descriptors, straight through ops: a rectangle that leaves its page, an empty one, pages outside the table, a page of 0
    # and of 65536 pixels, a row_start that falls and one that runs past the words -- each refuses its tile and nothing else
    case = random_case(77, 600, 4, empty=0.0)
    T = len(case['tile_page'])
    assert T >= 12
    rs, rect, page, size = (case[k].astype(np.int64).copy() for k in ('row_start', 'tile_rect', 'tile_page', 'page_size'))
    size = np.concatenate([size, [[0, 100], [65536, 100]]])
    rect[0, 2] = size[page[0], 0] + 1
    rect[1, 3] = rect[1, 1]
    rect[2, 0] = -1
    page[3], page[4], page[5], page[6] = -1, len(size), len(size) - 2, len(size) - 1
    rs[9] = rs[8] - 1 if rs[8] > 0 else rs[9]            # tile 8's range falls; tile 9, which would now reach back into tile 7's words, is refused too
    rect[9, 1] = size[page[9], 1]
    rs[T] = len(case['polys']) + 5                        # the last tile runs past the words
    bad_case = dict(case, row_start=rs, tile_rect=rect, tile_page=page, page_size=size)
    spec = _compare('tile_remap[refused descriptors]', bad_case, 1000, 2000, 2, True, out)
    refused = sorted(np.nonzero(spec['tile_count'] < 0)[0].tolist())
    out.append(rec('tile_remap[refused descriptors]: tiles %s refused, their words\' cut entries untouched (-1)' % refused,
                   0 if refused == [0, 1, 2, 3, 4, 5, 6, 8, 9, T - 1] and (spec['cut'] == -1).sum() > 0 and (spec['tile_count'] > 0).any() else 1, 0))
    # the stage object: the same answers through its one upload and one download; it raises on a refused tile; no words, no launch
    from tests.gpu_checks import DEV
    stage = TL.TileStage(DEV, 1000)
    keys = ('row_start', 'tile_rect', 'tile_page', 'page_size')
    res = stage.run(torch.from_numpy(case['polys']).long(), torch.from_numpy(case['points']).long(), *[case[k] for k in keys], 2000, 2, True)
    spec = TL.remap_cpu(case['polys'], case['points'], *[case[k] for k in keys], 1000, 2000, 2, True)
    bad = sum(int(np.asarray(res[k]).shape != spec[k].shape) or int((np.asarray(res[k]) != spec[k]).sum())
              for k in ('cut', 'src_row', 'tile_count', 'tile_dropped', 'out_start', 'page_count'))
    bad += int((res['page_polys'].cpu().numpy() != spec['page_polys']).sum()) + int((res['page_points'].cpu().numpy() != spec['page_points']).sum())
    out.append(rec('TileStage.run == remap_cpu (int64 ids from the host)', bad + int(not res['page_polys'].is_cuda), 0))
    try:
        stage.run(case['polys'], case['points'], case['row_start'], rect, case['tile_page'], case['page_size'], 2000)
        bad = 1
    except RuntimeError as e:
        bad = 0 if 'refused' in str(e) else 1
    out.append(rec('TileStage.run raises when the device refuses a tile', bad, 0))
    none = stage.run(np.zeros((0, 32), np.int32), np.zeros((0, 2), np.int32), np.zeros(T + 1, np.int32), *[case[k] for k in keys[1:]], 2000)
    bad = int(none['page_polys'].shape != (0, 32)) + int(not none['page_polys'].is_cuda) + int(none['tile_count'].tolist() != [0] * T) + int(none['out_start'].tolist() != [0] * (T + 1))
    out.append(rec('TileStage.run without words', bad, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------------------
PAGES = ((150, 220), (110, 160))     # (h, w)


def _model(dtype_name, seed=5):
    from tests.gpu_checks import ENGINES, build_model
    depths = (2, 2, 2, 2)
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, pt_seq_length=8, test_min_size=64, test_max_size=112)
    sd = weights.make_state_dict(args, seed=seed, depths=depths)
    return args, build_model(args, sd, depths, ENGINES[dtype_name])


def _pages():
    from tests.gpu_checks import DEV
    rng = np.random.RandomState(3)
    return [torch.from_numpy(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(DEV) for h, w in PAGES]


class _Spy(object):
    """records what a tiled call hands its tile stage and what comes back, and the per-tile records before they become page records"""

    def __enter__(self):
        spy = self
        self.calls, self.tile_recs = [], []
        self._stage, self._records = TL.TileStage, TL.tile_records

        class Stage(self._stage):
            def run(self, polys, points, row_start, tile_rect, tile_page, page_size, page_bins, edge=2, drop_cut=True):
                res = super().run(polys, points, row_start, tile_rect, tile_page, page_size, page_bins, edge, drop_cut)
                spy.calls.append(dict(polys=torch.as_tensor(polys).cpu().numpy(), points=torch.as_tensor(points).cpu().numpy(),
                                      row_start=np.asarray(row_start), rect=np.asarray(tile_rect), page=np.asarray(tile_page),
                                      size=np.asarray(page_size), page_bins=page_bins, edge=edge, drop_cut=drop_cut, res=res))
                return res

        def records(recs, *a, **kw):
            spy.tile_recs.append(copy.deepcopy(recs))
            return spy._records(recs, *a, **kw)
        TL.TileStage, TL.tile_records = Stage, records
        return self

    def __exit__(self, *exc):
        TL.TileStage, TL.tile_records = self._stage, self._records


def _strip(records, keys=NEW_KEYS):
    return [[{k: v for k, v in r.items() if k not in keys} for r in recs] for recs in records]


def _spec_of(call):
    return TL.remap_cpu(call['polys'], call['points'], call['row_start'], call['rect'], call['page'], call['size'], 1000, call['page_bins'],
                        call['edge'], call['drop_cut'])


def _stage_equals_spec(call):
    spec, res = _spec_of(call), call['res']
    bad = sum(int(np.asarray(res[k]).shape != spec[k].shape) or int((np.asarray(res[k]) != spec[k]).sum())
              for k in ('cut', 'src_row', 'tile_count', 'tile_dropped', 'out_start', 'page_count'))
    return bad + int((res['page_polys'].cpu().numpy() != spec['page_polys']).sum()) + int((res['page_points'].cpu().numpy() != spec['page_points']).sum())


def check_engine_tiles(dtype_name):
    """tiles=(2, 2) on two pages, ragged: every tile's ids == the tile view alone; the page records == tile_records(remap_cpu(ids))"""
    from advancedliteratemachinery_amd.engine.inference import predict_images, predict_raw
    from tests.gpu_checks import REPORT, rec
    from tests.gpu_checks_windows import _agree
    args, model = _model(dtype_name)
    pages = _pages()
    out, stats = [], [0, 0]
    cut_seen = 0
    for cut, edge in (('drop', 2), ('keep', 2), ('drop', 300), ('keep', 300)):     # edge 300: a third of a tile, so that words ARE cut
        with _Spy() as spy:
            got, pre = predict_images(model, pages, args, ragged=True, tiles=(2, 2), tile_cut=cut, tile_edge=edge, file_names=['p0', 'p1'])
        call, tile_recs = spy.calls[0], spy.tile_recs[0]
        tag = 'tiles engine[%s,%s,edge=%d]' % (dtype_name, cut, edge)
        cut_seen += int((call['res']['cut'] > 0).sum())
        out.append(rec(tag + ' ONE stage call for 8 tiles of 2 pages', abs(len(spy.calls) - 1) + abs(len(call['rect']) - 8), 0,
                       '%d words, %d kept' % (len(call['polys']), int(call['res']['out_start'][-1]))))
        out.append(rec(tag + ' words spotted, in more than one tile', 0 if (np.diff(call['row_start']) > 0).sum() > 1 else 1, 0))
        out.append(rec(tag + ' the stage == remap_cpu on the call\'s own ids', _stage_equals_spec(call), 0))
        # the page records == tile_records applied to remap_cpu of those ids
        want = TL.tile_records(copy.deepcopy(tile_recs), _spec_of(call), call['rect'], call['page'], 2, ['p0', 'p1'])
        out.append(rec(tag + ' page records == tile_records(remap_cpu(ids))', 0 if got == want else 1, 0))
        bad = sum(int(r['image_id'] != 'p%d' % p) + int(not set(NEW_KEYS) <= set(r)) + int(cut == 'drop' and r['tile_cut'] != 0)
                  for p, recs in enumerate(got) for r in recs)
        out.append(rec(tag + ' records carry the page\'s image_id and tile, tile_rect, tile_cut', bad, 0))
        if (cut, edge) != ('drop', 2):
            continue
        # every tile alone: its view through the same preprocessor and predict_raw (the ids), and through predict_images (the records)
        for k, (x0, y0, x1, y1) in enumerate(call['rect'].tolist()):
            view = pages[int(call['page'][k])][y0:y1, x0:x1]
            nt, _ = pre([view])
            raw, _ = predict_raw(model, nt, args, [(y1 - y0, x1 - x0)], ragged=True)
            lo, hi = int(call['row_start'][k]), int(call['row_start'][k + 1])
            mine = None if hi == lo else (torch.from_numpy(call['points'][lo:hi]).reshape(-1), torch.from_numpy(call['polys'][lo:hi]).reshape(-1))
            alone = None if raw[0] is None else (raw[0][0][0].reshape(-1).cpu(), raw[0][0][1].reshape(-1).cpu())
            if alone is not None and alone[0].numel() % 2:
                alone = (alone[0][:-1], alone[1])
            before = list(stats)
            _agree(mine, alone, stats)
            if dtype_name in F32_GRADE:
                out.append(rec('%s tile %d %s ids identical to the view alone' % (tag, k, [x0, y0, x1, y1]), (stats[1] - before[1]) - (stats[0] - before[0]), 0))
                recs_alone, _ = predict_images(model, [view], args, ragged=True, preprocessor=pre, file_names=['p%d' % int(call['page'][k])])
                out.append(rec('%s tile %d records == predict_images(view)' % (tag, k), 0 if recs_alone[0] == tile_recs[k] else 1, 0))
    out.append(rec('tiles engine[%s] words were cut at edge=300' % dtype_name, 0 if cut_seen > 0 else 1, 0, '%d cut flags' % cut_seen))
    frac = stats[0] / max(1, stats[1])
    REPORT.append(dict(name='tiles_equal_alone[%s]' % dtype_name, match=frac, tokens=stats[1]))
    out.append(rec('tiles engine[%s] token agreement with every tile alone' % dtype_name, 1.0 - frac, 0.0 if dtype_name in F32_GRADE else 0.05,
                   'agreement %.3f of %d' % (frac, stats[1])))
    return out


def check_identity_tiling(dtype_name):
    from advancedliteratemachinery_amd.engine.inference import predict_images
    from tests.gpu_checks import rec
    args, model = _model(dtype_name)
    pages = _pages()
    today, pre = predict_images(model, pages, args, ragged=True)
    n = sum(len(r) for r in today)
    out = [rec('tiles identity[%s]: words spotted' % dtype_name, 0 if n > 0 else 1, 0, '%d words' % n)]
    same, _ = predict_images(model, pages, args, ragged=True, preprocessor=pre, tiles=None, tile_size=None)
    out.append(rec('tiles identity[%s]: tiles=None is today\'s predict_images' % dtype_name, 0 if same == today else 1, 0))
    got, _ = predict_images(model, pages, args, ragged=True, preprocessor=pre, tiles=(1, 1), tile_overlap=0, page_bins=args.num_bins)
    out.append(rec('tiles identity[%s]: tiles=(1, 1), page_bins=num_bins records minus the new keys' % dtype_name, 0 if _strip(got) == today else 1, 0))
    bad = sum(int(r.get('tile') != 0 or r.get('tile_cut') != 0 or r.get('tile_rect') != [0, 0, w, h]) for recs, (h, w) in zip(got, PAGES) for r in recs)
    out.append(rec('tiles identity[%s]: tile = 0, tile_cut = 0, tile_rect = the page' % dtype_name, bad, 0))
    return out


def check_page_stages(dtype_name):
    """suppress= and reading_order= on a tiled call == suppress_cpu / lines_cpu run on page_polys at page_bins, one group per page"""
    from advancedliteratemachinery_amd.engine.inference import predict_images
    from tests.gpu_checks import rec
    args, model = _model(dtype_name)
    pages = _pages()
    out = []
    with _Spy() as spy:
        plain, pre = predict_images(model, pages, args, ragged=True, tiles=(2, 2), tile_cut='keep', tile_overlap=0.25)
    with _Spy() as spy:
        got, _ = predict_images(model, pages, args, ragged=True, preprocessor=pre, tiles=(2, 2), tile_cut='keep', tile_overlap=0.25, suppress=0.3,
                                suppress_measure='iomin', reading_order=True)
    call = spy.calls[0]
    P = call['page_bins']
    polys = call['res']['page_polys'].cpu().numpy()
    gs = np.concatenate([[0], np.cumsum(call['res']['page_count'])]).astype(np.int32)
    tag = 'tiles page stages[%s]' % dtype_name
    out.append(rec(tag + ' page_bins = min(4096, num_bins max(nx, ny))', abs(P - 2000), 0))
    owner, _ = OV.suppress_cpu(polys, gs, np.arange(len(polys)), OV.permille(0.3), 'iomin', P)
    keep = np.nonzero(owner == np.arange(len(polys)))[0]
    kgs = np.searchsorted(keep, gs).astype(np.int32)
    aspect = np.asarray([RD.aspect_of(h, w) for h, w in PAGES], np.int32)
    lines = RD.lines_cpu(polys[keep], kgs, aspect, 2000, 500, 500, P)
    bad = 0
    for p in range(2):
        lo = int(gs[p])
        want = [None] * int(kgs[p + 1] - kgs[p])
        for i in range(int(kgs[p]), int(kgs[p + 1])):
            r = dict(plain[p][int(keep[i]) - lo])
            r['merged'] = [int(n) - lo for n in np.nonzero((owner == keep[i]) & (np.arange(len(polys)) != keep[i]))[0]]
            r['line'], r['line_pos'] = int(lines['line'][i]), int(lines['line_pos'][i])
            want[int(lines['rank'][i])] = r
        bad += int(got[p] != want)
    out.append(rec(tag + ' merged, line, line_pos and the order == suppress_cpu / lines_cpu on page_polys', bad, 0,
                   '%d words, %d survive' % (len(polys), len(keep))))
    out.append(rec(tag + ' words on both pages', 0 if (np.diff(gs) > 0).all() else 1, 0))
    return out


def check_two_stage_tiles():
    from advancedliteratemachinery_amd.engine.two_stage import recognize_crops, spot_and_recognize
    from oracle import mgp_str_ref as R
    from tests.gpu_checks import rec
    from tests.gpu_checks_mgp import build
    args, omni = _model('fp32')
    c = R.cfg(depth=2)
    mgp = build(c, R.make_state_dict(c, seed=17), torch.float32)
    pages = [p.contiguous() for p in _pages()]
    out = []
    for mode in ('box', 'polygon'):
        got, _, _ = spot_and_recognize(omni, mgp, pages, args, crop=mode, ragged=True, tiles=(2, 2))
        flat = [(b, r) for b, recs in enumerate(got) for r in recs]
        out.append(rec('two-stage tiles[%s]: words spotted in several tiles' % mode, 0 if len(set((b, r['tile']) for b, r in flat)) > 1 else 1, 0,
                       '%d words' % len(flat)))
        keys = set(NEW_KEYS) | {'box', 'mgp_text', 'mgp_conf', 'mgp_choice', 'mgp_ids'}
        bad = sum(int(not keys <= set(r)) for _, r in flat)
        # the polygons are page pixels: inside the record's tile rectangle on the page
        for _, r in flat:
            x0, y0, x1, y1 = r['tile_rect']
            bad += sum(int(not (x0 <= q[0] <= x1 and y0 <= q[1] <= y1)) for q in r['polys'])
        out.append(rec('two-stage tiles[%s]: records carry the tile fields, the mgp_* fields and page-pixel polygons' % mode, bad, 0))
        if mode == 'polygon':
            reads, _ = recognize_crops(mgp, pages, None, polys=[(b, r['polys']) for b, r in flat])
        else:
            reads, _ = recognize_crops(mgp, pages, [(b,) + tuple(r['box']) for b, r in flat])
        bad = 0
        for (_, r), m in zip(flat, reads):
            bad += int(r['mgp_text'] != m['char_text']) + int(r['mgp_choice'] != m['choice']) + int(tuple(r['mgp_conf']) != tuple(m['conf']))
            bad += sum(int(list(r['mgp_ids'][k]) != list(m[k + '_ids'])) for k in ('char', 'bpe', 'wp'))
        out.append(rec('two-stage tiles[%s]: mgp_* == recognize_crops on the records\' page polygons' % mode, bad + int(len(reads) != len(flat)), 0))
    return out
