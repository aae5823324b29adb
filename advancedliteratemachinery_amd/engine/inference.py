"""Batched inference driver: the MI355X replacement for the reference's batch-1 `validate` loop
(OCR/OmniParser/engine/val.py:11-100), plus a `predict()` convenience API.

  * prompts are built exactly like val.py:25-33;
  * B images per call (the reference asserts 1).  Images of different sizes are padded to the largest and masked (the
    default), or with `ragged=True` each is encoded and decoded at its own size -- the answers of one call per image
    (OmniParser.infer);
  * `validate` is image-sharded: under torch.distributed every rank decodes a contiguous shard of the dataloader's
    items (utils/dist.py::shard_range), the decoded token tensors meet in ONE all-gather per tensor at the end
    (pack_results / all_gather_results: RCCL over xGMI on MI355X, gloo in the CPU tests) and rank 0 alone writes the
    JSON -- the reference writes the same file from every rank (val.py:64-68);
  * results are formatted like decode_pred_seq (val.py:70-100): {image_id, pts, score, polys, rec}; KIE results
    (`vie_categories > 0`) go to one <file_name>.json per image like val.py:39-43.
"""
import json
import os

import numpy as np
import torch
import torch.distributed as tdist

from ..utils import dist as udist
from ..utils.misc import decode_seq
from ..utils.nested_tensor import NestedTensor, nested_tensor_from_tensor_list


def build_prompts(args, device='cpu'):
    """val.py:25-33."""
    nb = args.num_bins
    if args.use_char_window_prompt:
        pt = [0, 0, nb - 1, nb - 1, nb, nb + len(args.chars), args.pt_sos_index]
    else:
        pt = [0, 0, nb - 1, nb - 1, args.pt_sos_index]
    mk = lambda v: torch.tensor([v], dtype=torch.long, device=device)  # noqa: E731
    return [mk(pt), mk([args.poly_sos_index]), mk([args.rec_sos_index])]


def decode_pred_seq(index_seqs, prob_seqs, target, args):
    """val.py:70-100: ids -> records in ORIGINAL image coordinates."""
    pt = index_seqs[0]
    if len(pt) % 2 != 0:
        pt = pt[:-1]
    pts = decode_seq(pt, args, 'pt')
    polys = decode_seq(index_seqs[1], args, 'poly')
    recs, confs = decode_seq(index_seqs[2], args, 'rec', prob_seqs)
    h, w = target['orig_size']
    h, w = float(h), float(w)
    scale = torch.tensor([w, h] * 16)
    out = []
    for p, poly, rec, conf in zip(pts, polys, recs, confs):
        out.append({'image_id': target['file_name'],
                    'pts': [[p['point'][0] * w, p['point'][1] * h]],
                    'score': conf,
                    'polys': (poly['polygon'] * scale).reshape(-1, 2).tolist(),
                    'rec': rec['rec']})
    return out


def _as_nested(images):
    """NestedTensor from whatever the caller has: anything with .tensors / .mask (ours OR the reference's class, as its
    dataloader collates), a (B,3,H,W) tensor, or a list of (3,H,W) tensors of possibly different sizes."""
    if hasattr(images, 'tensors'):
        mask = images.mask
        if mask is None:
            t = images.tensors
            mask = torch.zeros(t.shape[0], t.shape[2], t.shape[3], dtype=torch.bool, device=t.device)
        return NestedTensor(images.tensors, mask)
    if isinstance(images, torch.Tensor):
        return NestedTensor(images, torch.zeros(images.shape[0], images.shape[2], images.shape[3], dtype=torch.bool, device=images.device))
    return nested_tensor_from_tensor_list(list(images))


def _ragged_inputs(images, dev):
    """ragged calls: the unpadded images of whatever the caller has (a list of (3,H,W) tensors stays a list; a padded batch keeps its
    mask, from which OmniParser.infer reads every image's extent) -> (img, mask, [(h, w)] per image)"""
    from ..model.omniparser import mask_extents
    if isinstance(images, (list, tuple)):
        imgs = [torch.as_tensor(i).to(dev) for i in images]
        return imgs, None, [(int(i.shape[1]), int(i.shape[2])) for i in imgs]
    nt = _as_nested(images).to(dev)
    return nt.tensors, nt.mask, mask_extents(nt.mask)


@torch.no_grad()
def predict_raw(model, images, args, orig_sizes=None, ragged=False, windows=None, char_windows=None, clip_windows=False):
    """-> (per-image raw model outputs exactly as the reference's forward returns them, NestedTensor on the device).
    ragged=True: every image is decoded at its own size, no padding (OmniParser.infer(ragged=True)); the second value is then the
    list of (h, w) per image, and the KIE default orig_size is each image's own size.
    windows, char_windows, clip_windows: window prompts, as OmniParser.infer takes them (every image's result then carries a third
    entry, the window index per instance); without them the call is the plain one."""
    dev = next(model.parameters()).device
    seqs = build_prompts(args)
    wkw = {}
    if windows is not None or char_windows is not None:
        wkw = dict(windows=windows, char_windows=char_windows, clip_windows=clip_windows)
    if ragged:
        img, mask, sizes = _ragged_inputs(images, dev)
        if args.infer_vie:
            seqs.append([torch.as_tensor(s) for s in (orig_sizes if orig_sizes is not None else sizes)])
        return model.infer(img, mask, seqs, ragged=True, **wkw), sizes
    nt = _as_nested(images)
    B = nt.tensors.shape[0]
    has_padding = bool(nt.mask.any())
    nt = nt.to(dev)
    if args.infer_vie:
        if orig_sizes is None:
            orig_sizes = [(int(nt.tensors.shape[2]), int(nt.tensors.shape[3]))] * B
        seqs.append([torch.as_tensor(s) for s in orig_sizes])
    return model.infer(nt.tensors, nt.mask, seqs, has_padding=has_padding, **wkw), nt


def _n_images(images):
    if hasattr(images, 'tensors'):
        return int(images.tensors.shape[0])
    return int(images.shape[0]) if isinstance(images, torch.Tensor) else len(images)


@torch.no_grad()
def predict(model, images, args, targets=None, orig_sizes=None, ragged=False, lexicon=None, lexicon_max_dist=None, lexicon_max_ratio=None,
            windows=None, char_windows=None, clip_windows=False, grid=None, suppress=None, suppress_measure='iou', suppress_order='first',
            reading_order=False, line_gap=2.0, line_back=0.5, line_offset=0.5, blocks=False, block_gap_x=1.0, block_gap_y=1.5, block_depth=8):
    """images: list of (3,H,W) tensors, a (B,3,H,W) tensor or a NestedTensor (this package's or the reference's).
    Returns one entry per image: list of records (text spotting), list of tuples (KIE) or [].
    ragged=False: images of different sizes are padded to the largest and masked, and an image's tokens may then depend on the
    others in the call.  ragged=True: every image is decoded exactly as if it had been submitted alone; without targets its
    orig_size is its own (h, w), not the padded batch's.
    lexicon: a utils.lexicon.LexiconMatcher, a list of words shared by all images, or a list of word lists, one per image
    (a raw list is encoded with args.chars and uploaded for this call; pass a matcher to keep it on the device).  Every record
    then gains `lex` (the nearest word, or None when lexicon_max_dist / lexicon_max_ratio reject it), `lex_index` and
    `lex_dist`, from its `rec`, which stays as it is; all words of the call are matched in one device call.
    windows (a list of [x0, y0, x1, y1] in coordinate bins shared by all images, or one list per image), grid=(nx, ny) (shorthand
    for utils.windows.grid_windows(nx, ny, args.num_bins)), char_windows, clip_windows: window prompts (OmniParser.infer; DESIGN.md
    section 16) -- every window of an image is read under its own prompt in ONE engine call; an image's records are those of its
    windows in window order, and every record gains `window` (the index) and `window_bins` (its [x0, y0, x1, y1]).  Without these
    arguments the records are the plain call's.  Text spotting only; composes with ragged= and lexicon=.
    suppress (a float in (0, 1]), suppress_measure ('iou' | 'iomin'), suppress_order ('first' | 'score'): overlap suppression (DESIGN.md
    section 17; utils/overlap.py) -- records of one image whose decoded polygons overlap by at least `suppress` are the same word: the
    first in priority order ('first': record order, i.e. window order, then the decoder's; 'score': descending `score`, ties to the
    lower index) stays and gains `merged`, the list of (window, index) of the records it absorbed (plain indices without windows; an
    index counts the image's records before suppression), the others are removed.  The polygons are the raw ids on the device; all
    images go through ONE device call, before lexicon= annotates the survivors.  Without suppress= the records are the plain call's.
    reading_order=True, line_gap, line_back, line_offset (floats in [0, 10], in units of a word's height): reading order (DESIGN.md
    section 18; utils/reading.py) -- the words of an image are linked into text lines (a word follows another when it starts within
    line_gap heights after its end, at most line_back heights before it, and at most line_offset heights off its axis, in both words'
    frames), the lines are ordered top to bottom, every record gains `line` and `line_pos`, and each image's list is reordered
    accordingly (utils.reading.page_lines joins it into strings).  It runs on the raw polygon ids on the device, ONE device call for
    all images, after suppress= (on the survivors) and before lexicon=; `merged` indices keep counting the records before suppression.
    Without reading_order the records are the plain call's.
    blocks=True (needs reading_order=True), block_gap_x, block_gap_y (floats in [0, 10], in units of a word's height), block_depth (1 ..
    16): multi-column pages (utils/reading.py: blocks_cpu) -- a recursive XY-cut over the lines, in the same
    device call, directly after the lines: the page is cut into bands wherever a horizontal gap wider than block_gap_y heights
    crosses it, every band into columns at vertical gaps wider than block_gap_x heights, and so on, block_depth levels at most.
    Every record gains `block` (its block within the image, in reading order from 0), `line` counts up through block 0, then block
    1, ..., `line_pos` stays, and each image's list comes in that order (utils.reading.page_blocks gives one string per block).  The
    two gap defaults are choices that no data set has tested.  Without blocks no new code runs."""
    _check_stage_args(args, lexicon, suppress, suppress_measure, suppress_order, reading_order, line_gap, line_back, line_offset, blocks, block_gap_x,
                      block_gap_y, block_depth)
    out, raw_polys, sizes = _decode_records(model, images, args, targets, orig_sizes, ragged, windows, char_windows, clip_windows, grid)
    if args.infer_vie:
        return out
    return _finish_records(model, out, raw_polys, sizes, args.num_bins, args, lexicon, lexicon_max_dist, lexicon_max_ratio, suppress, suppress_measure,
                           suppress_order, reading_order, line_gap, line_back, line_offset, blocks, block_gap_x, block_gap_y, block_depth)


def _check_stage_args(args, lexicon, suppress, suppress_measure, suppress_order, reading_order, line_gap, line_back, line_offset, blocks, block_gap_x,
                      block_gap_y, block_depth):
    """the refusals of predict's post-processing arguments, ahead of any device work"""
    if blocks and not reading_order:
        raise ValueError('blocks=True orders the lines of reading_order=True: pass both')
    if reading_order:
        from ..utils import reading as RD
        RD.check_reading_args(line_gap, line_back, line_offset, args.infer_vie, blocks, block_gap_x, block_gap_y, block_depth)
    if suppress is not None:
        from ..utils import overlap as OV
        OV.check_suppress_args(suppress, suppress_measure, suppress_order, args.infer_vie)
    if lexicon is not None and args.infer_vie:
        raise ValueError('lexicon= needs text-spotting records; with args.infer_vie the engine returns entity tuples')


def _decode_records(model, images, args, targets, orig_sizes, ragged, windows, char_windows, clip_windows, grid, want_points=False):
    """predict's first part: the engine call and decode_pred_seq -> (records per image, the polygon decoder's raw ids per image -- device
    tensors, None for an image without a result --, orig_size per image); with args.infer_vie (the entity tuples per image, None, None).
    want_points: a fourth value, the point decoder's raw ids per image."""
    if orig_sizes is None and targets is not None and args.infer_vie:
        orig_sizes = [t['orig_size'] for t in targets]
    per_image = None
    if windows is not None or grid is not None or char_windows is not None:
        from ..utils import windows as WN
        if args.infer_vie:
            raise ValueError('windows= / grid= need text-spotting records; with args.infer_vie the engine returns entity tuples')
        per_image = WN.resolve_windows(windows, _n_images(images), grid=grid, num_bins=args.num_bins)
        if per_image is None:
            per_image = WN.resolve_windows([WN.default_window(args)], _n_images(images))
    wkw = {} if per_image is None else dict(windows=per_image, char_windows=char_windows, clip_windows=clip_windows)
    raw, nt = predict_raw(model, images, args, orig_sizes, ragged=ragged, **wkw)
    if args.infer_vie:
        return [r if r is not None else [] for r in raw], None, None
    out, sizes = [], []
    for b, r in enumerate(raw):
        tgt = (targets[b] if targets is not None else
               {'file_name': str(b), 'orig_size': nt[b] if ragged else (nt.tensors.shape[2], nt.tensors.shape[3])})
        sizes.append(tgt['orig_size'])
        if r is None:
            out.append([])
            continue
        seq_cpu = [t[0].cpu() for t in r[0]]
        out.append(decode_pred_seq(seq_cpu, r[1][0].cpu(), tgt, args))
        if per_image is not None:
            for rcd, w in zip(out[-1], r[2].tolist()):
                rcd['window'], rcd['window_bins'] = int(w), list(per_image[b][w])
    raw_polys = [None if r is None else r[0][1] for r in raw]
    if want_points:
        return out, raw_polys, sizes, [None if r is None else r[0][0] for r in raw]
    return out, raw_polys, sizes


def _finish_records(model, out, raw_polys, sizes, grid, args, lexicon=None, lexicon_max_dist=None, lexicon_max_ratio=None, suppress=None,
                    suppress_measure='iou', suppress_order='first', reading_order=False, line_gap=2.0, line_back=0.5, line_offset=0.5, blocks=False,
                    block_gap_x=1.0, block_gap_y=1.5, block_depth=8):
    """predict's second part: suppress=, reading_order= / blocks= and lexicon= on the records of one list per image, whose polygons are
    raw_polys on a grid of `grid` bins and whose sizes are `sizes` -- the images of a plain call, the pages of a tiled one"""
    rows = None
    if suppress is not None:
        from ..utils import overlap as OV
        rows = []
        out = OV.suppress_records(out, raw_polys, grid, suppress, suppress_measure, suppress_order,
                                  device=next(model.parameters()).device, kept_rows=rows)
    if reading_order:
        from ..utils import reading as RD
        out = RD.order_records(out, raw_polys, sizes, grid, line_gap, line_back, line_offset, rows=rows,
                               device=next(model.parameters()).device, blocks=blocks, block_gap_x=block_gap_x, block_gap_y=block_gap_y,
                               block_depth=block_depth)
    if lexicon is not None:
        from ..utils import lexicon as LX
        matcher = LX.resolve_lexicon(lexicon, len(out), next(model.parameters()).device, args.chars)
        LX.annotate_records(out, matcher, 'rec', 'lex', lexicon_max_dist, lexicon_max_ratio)
    return out


@torch.no_grad()
def predict_images(model, images_u8, args, file_names=None, preprocessor=None, ragged=False, lexicon=None, lexicon_max_dist=None,
                   lexicon_max_ratio=None, windows=None, char_windows=None, clip_windows=False, grid=None, suppress=None, suppress_measure='iou',
                   suppress_order='first', reading_order=False, line_gap=2.0, line_back=0.5, line_offset=0.5, blocks=False, block_gap_x=1.0,
                   block_gap_y=1.5, block_depth=8, tiles=None, tile_size=None, tile_overlap=0.125, tile_edge=2, tile_cut='drop', page_bins=None):
    """Raw images in, records out: uint8 RGB [H, W, 3] arrays / tensors -> the reference's val transform chain on the
    device (utils/preprocess.py: aspect-preserving Pillow-exact resize to test_min_size / test_max_size, ToTensor,
    Normalize, pad + mask) -> the hot path -> records in ORIGINAL image coordinates (val.py:70-100).
    ragged=True: the preprocessed images are decoded at their own sizes (predict), not padded to the largest of the call.
    lexicon, lexicon_max_dist, lexicon_max_ratio: as predict (records gain `lex`, `lex_index`, `lex_dist`).
    windows, char_windows, clip_windows, grid: as predict (window prompts; records gain `window`, `window_bins`).  The bins of a
    window are fractions of the RESIZED image the model sees, which is the original image scaled: the same fractions of both.
    suppress, suppress_measure, suppress_order: as predict (overlap suppression; survivors gain `merged`).
    reading_order, line_gap, line_back, line_offset: as predict (records gain `line`, `line_pos` and come in reading order); the
    aspect of every image is that of the ORIGINAL image, whose size scales the polygons.
    blocks, block_gap_x, block_gap_y, block_depth: as predict (records gain `block`; needs reading_order=True).
    tiles=(nx, ny) or tile_size=s (nx = ceil(width / s), ny = ceil(height / s) per page), tile_overlap, tile_edge, tile_cut, page_bins:
    tiled pages (utils/tiles.py) -- a page larger than the model's input is not scaled down as a whole: it is cut
    into nx * ny overlapping tiles (utils.tiles.plan_tiles: the cores partition the page, every tile is its core grown by ox =
    ceil(width / nx) * tile_overlap pixels and oy likewise, so neighbours share 2 ox pixels), every tile is resized on its own to
    test_min_size / test_max_size, and the tiles of ALL pages are read in ONE engine flow as views of the page images.  ragged= is
    honoured as given; ragged=True is recommended, since only then a tile's words do not depend on the other tiles of the call.  One
    device call (omp_tile_remap) then carries the words into page bins -- a grid of page_bins bins over the page, default min(4096,
    num_bins * max(nx, ny)) over the call's pages --, flags the words that reach within tile_edge tile bins of an INNER side of their
    tile (a fragment of a word the neighbouring tile sees whole) and, with tile_cut='drop', removes them; 'keep' returns them too.  The
    records come per PAGE, tiles in x-outer order and inside a tile in the decoder's order, `pts` / `polys` in page pixels, and gain
    `tile` (index within the page), `tile_rect` ([x0, y0, x1, y1], pixels) and `tile_cut` (bits 1 left, 2 top, 4 right, 8 bottom).
    suppress=, reading_order= / blocks= and lexicon= then run on the PAGES: on the page-bin polygons with grid = page_bins, the pages'
    sizes and one group per page; `merged` indices count a page's records after the tile stage.  suppress= removes the doubles of
    the words that lie whole in two tiles' shared strip.  A word longer than 2 ox pixels (2 oy for a vertical one) fits no shared
    strip: it is cut in BOTH of its tiles and is lost under 'drop'; 'keep' returns both fragments, flagged.  windows= / grid= compose
    in their shared form (every tile is read under the same windows; one window list per image is refused); KIE is refused.  The
    defaults of tile_overlap, tile_edge and page_bins are choices that no data set has tested.  Without tiles= / tile_size= no new
    code runs and the records are the plain call's.
    Returns (results per image, preprocessor) so the coefficient tables can be reused by the next call."""
    from ..utils.preprocess import DevicePreprocessor
    tkw = None
    if tiles is not None or tile_size is not None:
        from ..utils import tiles as TL
        tkw = TL.check_tile_args(tiles, tile_size, tile_overlap, tile_edge, tile_cut, page_bins, args.num_bins, args.infer_vie, windows)
    if lexicon is not None and args.infer_vie:
        raise ValueError('lexicon= needs text-spotting records; with args.infer_vie the engine returns entity tuples')
    skw = {}
    if suppress is not None:
        from ..utils import overlap as OV
        OV.check_suppress_args(suppress, suppress_measure, suppress_order, args.infer_vie)
        skw = dict(suppress=suppress, suppress_measure=suppress_measure, suppress_order=suppress_order)
    if blocks and not reading_order:
        raise ValueError('blocks=True orders the lines of reading_order=True: pass both')
    if reading_order:
        from ..utils import reading as RD
        RD.check_reading_args(line_gap, line_back, line_offset, args.infer_vie, blocks, block_gap_x, block_gap_y, block_depth)
        skw.update(reading_order=True, line_gap=line_gap, line_back=line_back, line_offset=line_offset)
        if blocks:
            skw.update(blocks=True, block_gap_x=block_gap_x, block_gap_y=block_gap_y, block_depth=block_depth)
    dev = next(model.parameters()).device
    if preprocessor is None:
        preprocessor = DevicePreprocessor(args.test_min_size, args.test_max_size, dev)
    imgs = [torch.as_tensor(i).to(dev) for i in images_u8]
    if tkw is not None:
        return _predict_tiled(model, imgs, args, file_names, preprocessor, ragged, lexicon, lexicon_max_dist, lexicon_max_ratio, windows, char_windows,
                              clip_windows, grid, skw, tiles, tile_size, tkw), preprocessor
    nt, _ = preprocessor(imgs)
    targets = [{'file_name': (file_names[b] if file_names is not None else str(b)),
                'orig_size': (int(im.shape[0]), int(im.shape[1]))} for b, im in enumerate(imgs)]
    return predict(model, nt, args, targets=targets, orig_sizes=[t['orig_size'] for t in targets], ragged=ragged, lexicon=lexicon,
                   lexicon_max_dist=lexicon_max_dist, lexicon_max_ratio=lexicon_max_ratio, windows=windows, char_windows=char_windows,
                   clip_windows=clip_windows, grid=grid, **skw), preprocessor


def _predict_tiled(model, imgs, args, file_names, preprocessor, ragged, lexicon, lexicon_max_dist, lexicon_max_ratio, windows, char_windows,
                   clip_windows, grid, skw, tiles, tile_size, tkw):
    """predict_images with tiles= / tile_size=: the tiles of all pages through predict's first part in ONE flow, the tile stage, predict's
    second part on the pages"""
    from ..utils import tiles as TL
    dev = next(model.parameters()).device
    page_hw = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
    names = [file_names[p] if file_names is not None else str(p) for p in range(len(imgs))]
    rect, owner, page_size, grids = TL.plan_pages(page_hw, tiles, tile_size, tkw['o'])
    P = tkw['page_bins'] if tkw['page_bins'] is not None else TL.default_page_bins(args.num_bins, grids)
    if len(imgs) == 0:
        return []
    views = [imgs[p][y0:y1, x0:x1] for p, (x0, y0, x1, y1) in zip(owner.tolist(), rect.tolist())]     # no copy: the preprocessor takes the pitch
    nt, _ = preprocessor(views)
    targets = [{'file_name': names[p], 'orig_size': (y1 - y0, x1 - x0)} for p, (x0, y0, x1, y1) in zip(owner.tolist(), rect.tolist())]
    recs, raw_polys, _, raw_points = _decode_records(model, nt, args, targets, [t['orig_size'] for t in targets], ragged, windows, char_windows,
                                                     clip_windows, grid, want_points=True)
    counts = [len(r) for r in recs]
    row_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    polys = [torch.as_tensor(raw_polys[k]).reshape(-1, 32)[:n] for k, n in enumerate(counts) if n]
    points = [torch.as_tensor(raw_points[k]).reshape(-1)[:2 * n].reshape(-1, 2) for k, n in enumerate(counts) if n]
    if polys:
        polys, points = torch.cat(polys, 0), torch.cat(points, 0)
    else:
        polys, points = torch.zeros(0, 32, dtype=torch.int32), torch.zeros(0, 2, dtype=torch.int32)
    res = TL.TileStage(dev, args.num_bins).run(polys, points, row_start, rect, owner, page_size, P, tkw['edge'], tkw['drop_cut'])   # ONE device call
    out = TL.tile_records(recs, res, rect, owner, len(imgs), names)
    page_start = np.concatenate([[0], np.cumsum(res['page_count'])]).astype(np.int64)       # tiles are sorted by page: a page's rows are contiguous
    page_polys = [res['page_polys'][int(page_start[p]):int(page_start[p + 1])] if len(out[p]) else None for p in range(len(imgs))]
    return _finish_records(model, out, page_polys, page_hw, P, args, lexicon, lexicon_max_dist, lexicon_max_ratio, **skw)


def _meta(t):
    """the (small, picklable) part of a dataloader target that result formatting needs"""
    h, w = t['orig_size']
    return {'file_name': t['file_name'], 'orig_size': (float(h), float(w)), 'dataset_name': t.get('dataset_name', 'results')}


def plan_eos_balance(pred, world, batch_size):
    """Straggler balance for EOS-honouring inference ("expected scaling loss comes from ragged decode length (straggler
    rank), not bandwidth -> balance by sorting / bucketing images by predicted N").  An image's decode time grows with its instance count
    (2 N point steps, then N polygon and N recognition rows); images of one engine call are decoded in lock-step, so a call costs its
    DENSEST image, and a rank costs the sum of its calls -- contiguous shards of a dataset whose dense pages sit together make one rank
    the straggler of every all-gather.
      pred: predicted instance count (any cost proxy) per image, dataset order -- annotation counts of a validation set, the previous
            epoch's decoded counts, a detector's proposals;
      -> plan[rank] = list of batches, each a list of GLOBAL image indices.
    (1) across ranks: longest-processing-time-first -- images by predicted cost, descending, each to the least-loaded rank that still has
        room; shard SIZES stay those of utils/dist.py::shard_range, so every rank makes the same number of engine calls (+-1) and the
        padded all-gather is unchanged;
    (2) inside a rank: by predicted cost, descending, cut into batches of `batch_size`: images that finish together are decoded together.
    Deterministic (ties by index): every rank computes the same plan without communicating."""
    n = len(pred)
    cap = [udist.shard_range(n, r, world)[1] - udist.shard_range(n, r, world)[0] for r in range(world)]
    load = [0.0] * world
    mine = [[] for _ in range(world)]
    for i in sorted(range(n), key=lambda i: (-float(pred[i]), i)):
        r = min((r for r in range(world) if len(mine[r]) < cap[r]), key=lambda r: (load[r], r))
        mine[r].append(i)
        load[r] += float(pred[i])
    bs = max(1, int(batch_size))
    plan = []
    for r in range(world):
        order = sorted(mine[r], key=lambda i: (-float(pred[i]), i))
        plan.append([order[o:o + bs] for o in range(0, len(order), bs)])
    return plan


def plan_cost(plan, pred):
    """lock-step cost model of a plan: per rank, the sum over its engine calls of the call's densest image -> list per rank"""
    return [sum(max(float(pred[i]) for i in b) for b in batches if b) for batches in plan]


def _items_by_index(dataloader, order):
    """the items of `dataloader` with the given GLOBAL indices, in that order, without touching the others (map-style DataLoader that walks
    its dataset in order: re-pointed at Subset(dataset, order); a sequence: indexed)."""
    ds = getattr(dataloader, 'dataset', None)
    if isinstance(dataloader, torch.utils.data.DataLoader) and ds is not None and hasattr(ds, '__getitem__') and \
            (dataloader.batch_size in (1, None)) and len(ds) == len(dataloader) and \
            isinstance(getattr(dataloader, 'sampler', None), torch.utils.data.SequentialSampler):
        kw = {}
        if dataloader.num_workers > 0:
            kw = dict(prefetch_factor=dataloader.prefetch_factor, persistent_workers=dataloader.persistent_workers)
        return torch.utils.data.DataLoader(torch.utils.data.Subset(ds, list(order)), batch_size=dataloader.batch_size, shuffle=False,
                                           num_workers=dataloader.num_workers, collate_fn=dataloader.collate_fn, pin_memory=dataloader.pin_memory,
                                           worker_init_fn=dataloader.worker_init_fn, **kw)
    if isinstance(dataloader, (list, tuple)):
        return [dataloader[i] for i in order]
    raise TypeError('EOS balancing (args.eos_pred_counts) needs a sized, index-addressable loader: a sequence or a DataLoader over a map-style dataset in order')


def _rank_items(dataloader, rank, ws, sharded):
    """This rank's part of the validation set WITHOUT decoding the other ranks' images (every rank used to iterate the
    whole loader and discard what was not its own).  A torch DataLoader with a map-style dataset is re-pointed at
    Subset(dataset, [lo, hi)) (same collate / workers / batch size 1 as the reference's val loader); a plain sequence is
    sliced; a generic iterable is consumed lazily with islice -- skipped items are still produced by the iterable, but never
    held: nothing is materialised with list().  -> (iterable of this rank's items, lo, hi)."""
    import itertools
    if ws == 1 or sharded:
        return dataloader, 0, None
    if not hasattr(dataloader, '__len__'):
        raise TypeError('validate over %d ranks needs a dataloader with a length (to cut contiguous shards); pass a sized loader or '
                        'one that is already rank-sharded (args.dataloader_is_sharded)' % ws)
    n_items = len(dataloader)
    lo, hi = udist.shard_range(n_items, rank, ws)
    ds = getattr(dataloader, 'dataset', None)
    # only a loader that walks its dataset IN ORDER may be re-pointed at a Subset: a full-length non-sequential sampler (a
    # permutation, a weighted sampler) defines the item order itself -- that falls through to islice below
    if isinstance(dataloader, torch.utils.data.DataLoader) and ds is not None and hasattr(ds, '__getitem__') and \
            (dataloader.batch_size in (1, None)) and len(ds) == n_items and \
            isinstance(getattr(dataloader, 'sampler', None), torch.utils.data.SequentialSampler):
        sub = torch.utils.data.Subset(ds, range(lo, hi))
        kw = {}
        if dataloader.num_workers > 0:   # these two are only legal with worker processes
            kw = dict(prefetch_factor=dataloader.prefetch_factor, persistent_workers=dataloader.persistent_workers)
        return torch.utils.data.DataLoader(sub, batch_size=dataloader.batch_size, shuffle=False, num_workers=dataloader.num_workers,
                                           collate_fn=dataloader.collate_fn, pin_memory=dataloader.pin_memory,
                                           worker_init_fn=dataloader.worker_init_fn, **kw), lo, hi
    if isinstance(dataloader, (list, tuple)):
        return dataloader[lo:hi], lo, hi
    return itertools.islice(iter(dataloader), lo, hi), lo, hi


@torch.no_grad()
def validate(model, dataloader, epoch, args, batch_size=1, ragged=False):
    """Drop-in for engine.validate (val.py:11-68), image-sharded over the ranks of torch.distributed.

    dataloader yields (samples, targets) as the reference's does (samples: NestedTensor of 1 or more images, targets:
    list of dicts with file_name / orig_size / dataset_name).  Rank r decodes items [lo, hi) = shard_range(len, r, W)
    -- a loader that is already rank-sharded (DistributedSampler: `args.dataloader_is_sharded`) is consumed whole --
    `batch_size` consecutive items are merged into one engine call, decoded token tensors are packed to fixed size and all-gathered ONCE at the end, and
    rank 0 formats and writes <output_folder>/results/epXXX/<dataset>.json (text spotting) or one <file_name>.json per
    image (KIE).  Returns the records on rank 0 (a list; per-image lists for KIE) and [] elsewhere.
    Images of different sizes in one engine call: ragged=False pads them to the largest and masks the padding, as the reference's
    collate would for a batch it never runs (val.py:22 asserts batch 1) -- an image's tokens may then depend on the others in its call.
    ragged=True hands the model the unpadded images (OmniParser.infer(ragged=True)): every image is decoded as at batch_size=1.
    args.eos_pred_counts (optional: one predicted instance count per dataloader item) switches the contiguous shards for plan_eos_balance's:
    cost-balanced across ranks, homogeneous inside an engine call; the output is the same, in dataset order."""
    model.eval()
    rank, ws = udist.world()
    dev = next(model.parameters()).device
    sharded = bool(getattr(args, 'dataloader_is_sharded', False))
    pred = getattr(args, 'eos_pred_counts', None)
    kie = args.vie_categories > 0
    local_raw, local_meta = [], []
    pend_imgs, pend_tg, pend_key = [], [], []
    if pred is not None and not sharded:
        # balanced shards + homogeneous batches (plan_eos_balance): this rank's images in plan order, engine calls cut where the plan cuts;
        # every meta carries its dataset index so that rank 0 restores dataset order before formatting (the JSON is the unbalanced run's)
        if len(pred) != len(dataloader):
            raise ValueError('args.eos_pred_counts holds %d entries for %d dataloader items' % (len(pred), len(dataloader)))
        my = plan_eos_balance(pred, ws, batch_size)[rank]
        order = [i for b in my for i in b]
        cuts = set()
        acc = 0
        for b in my:
            acc += len(b)
            cuts.add(acc)
        items, lo = _items_by_index(dataloader, order), 0
    else:
        items, lo, hi = _rank_items(dataloader, rank, ws, sharded)
        order, cuts = None, None
    seen = [0]

    def flush():
        if not pend_imgs:
            return
        raw, _ = predict_raw(model, list(pend_imgs), args, [t['orig_size'] for t in pend_tg] if args.infer_vie else None, ragged=ragged)
        local_raw.extend(raw)
        for t, key in zip(pend_tg, pend_key):
            m = _meta(t)
            m['_idx'] = key
            local_meta.append(m)
        del pend_imgs[:], pend_tg[:], pend_key[:]

    # Sort key of an image = (shard, ITEM index, image inside the item): `lo`, `order` and `cuts` count dataloader ITEMS, and an item may hold
    # several images (counting images there let the ranks' keys overlap and cut the balanced plan in the wrong places).  A loader that
    # is already rank-sharded has no global item index: its ranks' parts stay in rank order (shard = rank), as the gather delivers them.
    for it, (samples, targets) in enumerate(items):
        nt = _as_nested(samples)
        item = order[it] if order is not None else lo + it
        for k, (img, t) in enumerate(zip(nt.unpad_tensors(), targets)):
            pend_imgs.append(img)
            pend_tg.append(t)
            pend_key.append((rank if sharded else 0, item, k))
            if cuts is None and len(pend_imgs) >= max(1, int(batch_size)):
                flush()
        seen[0] += 1
        if cuts is not None and seen[0] in cuts:   # the plan cuts between ITEMS
            flush()
    flush()

    folder = os.path.join(args.output_folder, 'results', 'ep%03d' % epoch) if getattr(args, 'output_folder', None) else None
    if kie:
        # results are host objects (strings, class names): small, gathered as objects
        pairs = [(m, r) for m, r in zip(local_meta, local_raw) if r]
        if ws > 1:
            allp = [None] * ws
            tdist.all_gather_object(allp, pairs)
            pairs = [p for part in allp for p in part]
        if rank != 0:
            return []
        pairs.sort(key=lambda mr: mr[0]['_idx'])
        if folder is not None:
            for m, r in pairs:
                path = os.path.join(folder, m['file_name'] + '.json')
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with open(path, 'w') as f:
                    json.dump(r, f)
        return [r for _, r in pairs]

    # text spotting: fixed-size token tensors, one all-gather per tensor for the whole validation set
    n_loc = torch.tensor([len(local_raw), max([0] + [r[0][0].numel() // 2 for r in local_raw if r is not None])], dtype=torch.int64, device=dev)
    if ws > 1:
        tdist.all_reduce(n_loc, op=tdist.ReduceOp.MAX)
    n_max, inst_max = int(n_loc[0]), max(1, int(n_loc[1]))
    padded = list(local_raw) + [None] * (n_max - len(local_raw))
    ids, probs, n_inst = udist.pack_results(padded, inst_max, args.rec_length, dev)
    ids, probs, n_inst = udist.all_gather_results(ids, probs, n_inst)
    metas = local_meta
    if ws > 1:
        allm = [None] * ws
        tdist.all_gather_object(allm, local_meta)
        metas = allm
    if rank != 0:
        return []
    results, last = [], None
    per_rank = [metas] if ws == 1 else metas
    every = []
    for r_, ms in enumerate(per_rank):
        outs = udist.unpack_results(ids[r_ * n_max:r_ * n_max + len(ms)].cpu(), probs[r_ * n_max:r_ * n_max + len(ms)].cpu(),
                                    n_inst[r_ * n_max:r_ * n_max + len(ms)].cpu())
        every.extend(zip(ms, outs))
    every.sort(key=lambda mo: mo[0]['_idx'])     # dataset order, whatever the sharding was
    for m, o in every:
        last = m
        if o is None:       # the reference skips empty outputs (val.py:36-37)
            continue
        results.extend(decode_pred_seq([t[0] for t in o[0]], o[1][0], m, args))
    if folder is not None and last is not None:
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, last['dataset_name'] + '.json'), 'w') as f:
            f.write(json.dumps(results, indent=4))
    return results
