"""Two-stage reading: OmniParser detections -> word crops on the device -> MGP-STR recogniser ->
fused multi-granularity decoding.

The reference ships the two models as separate projects and no glue between them, so the interfaces on both sides are
the reference's own: detections are OmniParser's records in ORIGINAL image coordinates (engine/val.py:70-100,
`polys` = 16 points), a word crop is the axis-aligned bounding box of its polygon (the rectangle the reference's KIE
path derives from a polygon, transformer.py:186-196: min / max over the points), and the recogniser sees each crop the
way MGP-STR's own evaluation does (OCR/MGP-STR/dataset.py:462: `image.resize((128, 32), Image.BICUBIC)` + ToTensor;
test_final.py:145-240: greedy ids, max-softmax confidences cumprod-ed to the first EOS, the most confident of the
char / BPE / WordPiece heads wins).  Everything between the uint8 image and the token ids runs on the MI355X: no crop
ever visits the host.  crop='polygon' replaces the bounding box by the word rectified along its polygon
(utils/word_crops.py): rotated, vertical and curved words arrive upright and tight.
"""
import math

import torch

from ..utils.preprocess import CropResizer
from ..utils.word_crops import PolygonCropper, polygon_strip_size
from .inference import predict_images


def polygon_box(polys, width, height):
    """16 (x, y) points in original-image pixels -> integer box (x0, y0, x1, y1), x1 / y1 exclusive, clipped to the image and
    at least one pixel wide and high (min / max over the points as transformer.py:186-196, floor / ceil to whole pixels)."""
    xs = [p[0] for p in polys]
    ys = [p[1] for p in polys]
    x0 = max(0, min(int(math.floor(min(xs))), width - 1))
    y0 = max(0, min(int(math.floor(min(ys))), height - 1))
    x1 = max(x0 + 1, min(int(math.ceil(max(xs))), width))
    y1 = max(y0 + 1, min(int(math.ceil(max(ys))), height))
    return x0, y0, x1, y1


@torch.no_grad()
def recognize_crops(mgp_model, images_u8, boxes, resizer=None, chunk=512, polys=None, keep_logits=False):
    """boxes: (image index, x0, y0, x1, y1).  -> list of MGPSTR.recognize results (one dict per box).
    polys: (image index, 16 x 2 points) per crop instead of boxes (boxes is then ignored): the crops are rectified along
    their polygons (utils/word_crops.py: PolygonCropper), and `resizer` is a PolygonCropper.
    keep_logits=True: -> (results, resizer, logits): the character head's fp32 logits of all crops [n, 27, 38], kept on the
    device across the chunks (None without crops)."""
    crops = boxes if polys is None else polys
    if not crops:
        return ([], resizer, None) if keep_logits else ([], resizer)
    dev = images_u8[0].device
    if resizer is None:
        c = mgp_model.cfg
        resizer = (CropResizer if polys is None else PolygonCropper)(dev, c['img'][0], c['img'][1])
    out, kept = [], []
    for i in range(0, len(crops), chunk):
        batch = resizer(images_u8, crops[i:i + chunk])
        if keep_logits:
            res, logits = mgp_model.recognize(batch, char_logits=True)
            out.extend(res)
            kept.append(logits)
        else:
            out.extend(mgp_model.recognize(batch))
    if keep_logits:
        return out, resizer, kept[0] if len(kept) == 1 else torch.cat(kept, 0)
    return out, resizer


@torch.no_grad()
def spot_and_recognize(omni_model, mgp_model, images_u8, args, file_names=None, preprocessor=None, resizer=None, crop='box', ragged=False,
                       lexicon=None, lexicon_max_dist=None, lexicon_max_ratio=None, windows=None, char_windows=None, clip_windows=False,
                       grid=None, suppress=None, suppress_measure='iou', suppress_order='first', reading_order=False, line_gap=2.0, line_back=0.5,
                       line_offset=0.5, blocks=False, block_gap_x=1.0, block_gap_y=1.5, block_depth=8, tiles=None, tile_size=None, tile_overlap=0.125,
                       tile_edge=2, tile_cut='drop', page_bins=None, lexicon_mode='edit', lexicon_min_prob=None, lexicon_min_margin=None):
    """uint8 RGB [H, W, 3] images -> per image the OmniParser records, each extended by the recogniser's reading of its
    crop: `box` (x0, y0, x1, y1), `mgp_text` (character-head string up to its EOS), `mgp_conf` (char, bpe, wp),
    `mgp_choice` (0 char / 1 bpe / 2 wp / -1 none: the most confident head, test_final.py:172-236) and the raw ids of
    the three heads (the BPE / WordPiece STRINGS need the GPT-2 / BERT vocabulary files, which are not in the
    reference tree).  crop='box' reads the bounding box of each polygon; crop='polygon' reads the word rectified along
    its polygon (rotated, vertical and curved text arrives upright and tight; `resizer` is then a PolygonCropper) and the
    records gain `crop`: 'polygon' and `strip`: (sh, sw), the rectified word's own size.  `ragged` goes to predict_images.
    lexicon (a utils.lexicon.LexiconMatcher, a list of words, or a list of word lists, one per image), lexicon_max_dist,
    lexicon_max_ratio: records gain `lex`, `lex_index`, `lex_dist` from `rec` (predict_images) and `mgp_lex`, `mgp_lex_index`,
    `mgp_lex_dist` from `mgp_text`; a raw list is encoded with args.chars for the one and MGP-STR's character set for the
    other, a matcher serves both with its own alphabet.  One device call per source string for all words of all images.
    lexicon_mode='posterior', lexicon_min_prob, lexicon_min_margin: posterior lexicon decoding (DESIGN.md section 22;
    utils/lexicon_post.py): `mgp_lex` becomes the lexicon word of greatest probability under MGP-STR's character head instead
    of the nearest word of the greedy string.  The crops' character logits stay on the device, ONE posterior call scores all words
    of all images (per-image lists through ranges), and the records gain `mgp_lex`, `mgp_lex_index`, `mgp_lex_logp` (nats),
    `mgp_lex_second` ((index, logp) of the runner-up or None) and `mgp_lex_gap` (nats below the greedy path; may be negative) --
    no `mgp_lex_dist`.  A word is rejected (`mgp_lex` None) below lexicon_min_prob or when the runner-up is closer than
    lexicon_min_margin nats.  `lex*` from `rec` stays edit-distance under lexicon_max_dist / lexicon_max_ratio: OmniParser's
    recogniser is autoregressive.  'edit' (the default) is the behaviour described above.
    windows, char_windows, clip_windows, grid=(nx, ny): window prompts, as predict_images takes them: the
    spotter reads every window of every image in one engine call, the records gain `window` and `window_bins`, and the recogniser
    reads the crops of all windows' words exactly as it reads the plain call's.
    suppress, suppress_measure, suppress_order: overlap suppression, as predict_images takes it: duplicates are
    removed BEFORE the crops, so a duplicate is neither cropped nor recognised; survivors gain `merged`.
    reading_order, line_gap, line_back, line_offset: reading order, as predict_images takes it: the records are
    put into text lines and reading order BEFORE the crops, so the crops are read in that order and `mgp_*` land on the reordered
    records; utils.reading.page_lines(records, field='mgp_text') joins an image's lines.
    blocks, block_gap_x, block_gap_y, block_depth: multi-column pages, as predict_images takes them (needs
    reading_order=True): the records gain `block` and come block by block BEFORE the crops, so `mgp_*` land on the reordered records;
    utils.reading.page_blocks(records, field='mgp_text') gives one string per block.
    tiles=(nx, ny) or tile_size=, tile_overlap, tile_edge, tile_cut, page_bins: tiled pages, as predict_images takes them (DESIGN.md
    section 20): the spotter reads every page as overlapping full-resolution tiles, the records come per page in PAGE pixels with
    `tile`, `tile_rect` and `tile_cut`, and the crops are cut from the page images along those page-pixel polygons, at the page's
    resolution.  The three defaults are choices that no data set has tested.
    Returns (results, preprocessor, resizer) so the cached tables can be reused."""
    if crop not in ('box', 'polygon'):
        raise ValueError("crop must be 'box' or 'polygon', got %r" % (crop,))
    if lexicon is not None and args.infer_vie:
        raise ValueError('lexicon= needs text-spotting records; with args.infer_vie the engine returns entity tuples')
    if lexicon_mode not in ('edit', 'posterior'):
        raise ValueError("lexicon_mode must be 'edit' or 'posterior', got %r" % (lexicon_mode,))
    if lexicon_mode != 'posterior' and (lexicon_min_prob is not None or lexicon_min_margin is not None):
        raise ValueError("lexicon_min_prob / lexicon_min_margin belong to lexicon_mode='posterior'")
    if lexicon_mode == 'posterior':
        if args.infer_vie:
            raise ValueError("lexicon_mode='posterior' needs text-spotting records; with args.infer_vie the engine returns entity tuples")
        if lexicon is None:
            raise ValueError("lexicon_mode='posterior' needs lexicon=")
        from ..utils import lexicon_post as LP
        LP.check_post_args(lexicon_min_prob, lexicon_min_margin)
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
    if tiles is not None or tile_size is not None:
        from ..utils import tiles as TL
        TL.check_tile_args(tiles, tile_size, tile_overlap, tile_edge, tile_cut, page_bins, args.num_bins, args.infer_vie, windows)
        skw.update(tiles=tiles, tile_size=tile_size, tile_overlap=tile_overlap, tile_edge=tile_edge, tile_cut=tile_cut, page_bins=page_bins)
    dev = next(omni_model.parameters()).device
    imgs = [torch.as_tensor(i).to(dev).contiguous() for i in images_u8]
    if lexicon is not None:
        from ..utils import lexicon as LX
        if not LX.is_matcher(lexicon):
            lexicon = [list(w) if not isinstance(w, str) else w for w in lexicon]   # read a generator once, use it twice
    records, preprocessor = predict_images(omni_model, imgs, args, file_names=file_names, preprocessor=preprocessor, ragged=ragged,
                                           lexicon=lexicon, lexicon_max_dist=lexicon_max_dist, lexicon_max_ratio=lexicon_max_ratio,
                                           windows=windows, char_windows=char_windows, clip_windows=clip_windows, grid=grid, **skw)
    boxes, polys, owner = [], [], []
    for b, recs in enumerate(records):
        h, w = int(imgs[b].shape[0]), int(imgs[b].shape[1])
        for r in recs:
            r['box'] = polygon_box(r['polys'], w, h)
            boxes.append((b,) + r['box'])
            if crop == 'polygon':
                r['crop'], r['strip'] = 'polygon', polygon_strip_size(r['polys'])
                polys.append((b, r['polys']))
            owner.append(r)
    if lexicon_mode == 'posterior':
        reads, resizer, char_logits = recognize_crops(mgp_model, imgs, boxes, resizer, polys=polys if crop == 'polygon' else None, keep_logits=True)
    else:
        reads, resizer = recognize_crops(mgp_model, imgs, boxes, resizer, polys=polys if crop == 'polygon' else None)
    for r, m in zip(owner, reads):
        r['mgp_text'], r['mgp_conf'], r['mgp_choice'] = m['char_text'], m['conf'], m['choice']
        r['mgp_ids'] = dict(char=m['char_ids'], bpe=m['bpe_ids'], wp=m['wp_ids'])
    if lexicon is not None:
        from ..model.mgp_str import CHARACTER
        matcher = LX.resolve_lexicon(lexicon, len(records), dev, CHARACTER)
        if lexicon_mode == 'posterior':
            LP.annotate_posterior(records, matcher, char_logits, 'mgp_lex', lexicon_min_prob, lexicon_min_margin)
        else:
            LX.annotate_records(records, matcher, 'mgp_text', 'mgp_lex', lexicon_max_dist, lexicon_max_ratio)
    return records, preprocessor, resizer
