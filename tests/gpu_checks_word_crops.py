"""Polygon-rectified word crops: the case builders shared by the CPU tests
(tests/test_word_crops_host.py) and the GPU parity checks of PolygonCropper / spot_and_recognize(crop='polygon') against
rectify_polygon_cpu + the real Pillow.  Everything is integer on both sides, so every tolerance here is zero except the
confidences of the end-to-end check (1e-4, as check_two_stage).  Same record format as tests/gpu_checks.py; the GPU
modules are imported inside the checks so that the builders stay usable without a device."""
import math

import numpy as np
from PIL import Image, ImageDraw, ImageFont

from advancedliteratemachinery_amd.utils.word_crops import SMAX, polygon_strip_size, rectify_polygon_cpu

WORD_ANGLES = (35, 90, -60, 10)
WORD_BOX = (40, 48, 220, 72)          # x0, y0, x1, y1 of the upright word: 180 x 24


# ---------------------------------------------------------------------------------------------
# case builders (numpy / Pillow only)
# ---------------------------------------------------------------------------------------------
def rect_poly(x0, y0, x1, y1):
    """a horizontal rectangle as 16 evenly spaced points: top edge left to right, bottom edge walking back"""
    xs = np.linspace(x0, x1, 8)
    return [(float(x), float(y0)) for x in xs] + [(float(x), float(y1)) for x in xs[::-1]]


def vertical_poly(x0, y0, x1, y1):
    """the same rectangle read top-down: the top edge runs DOWN the right side, the bottom edge back up the left side;
    the strip is np.rot90 of the slice"""
    ys = np.linspace(y0, y1, 8)
    return [(float(x1), float(y)) for y in ys] + [(float(x0), float(y)) for y in ys[::-1]]


def random_rects(rng, H, W, n):
    """n integer-cornered rectangles inside an H x W image; the first ones are the edge cases nobody may drop: the whole
    image, single pixels in two corners, one pixel wide, one pixel high, and rectangles touching each border"""
    fixed = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, W, H), (W // 2, 0, W // 2 + 1, H), (0, H // 2, W, H // 2 + 1),
             (0, 3, 7, H), (W - 9, 0, W, 11), (5, 0, W - 3, 2), (3, H - 4, W, H), (0, 0, 1, H), (0, H - 1, W, H),
             (W - 2, 0, W, H)]   # two pixels wide: more than 100 times as high as wide from H = 201, where Image.resize swaps its passes
    out = list(fixed[:n])
    while len(out) < n:
        x0 = int(rng.randint(0, W))
        y0 = int(rng.randint(0, H))
        out.append((x0, y0, int(rng.randint(x0 + 1, W + 1)), int(rng.randint(y0 + 1, H + 1))))
    return out


def ramp_image(H=300, W=500):
    """linear ramp 0.3 x + 0.4 y at the pixel centres, rounded to uint8"""
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.rint(0.3 * (xx + 0.5) + 0.4 * (yy + 0.5)).astype(np.uint8)
    return np.stack([r] * 3, -1)


def arc_poly(cx=250.0, cy=400.0, r_top=300.0, r_bot=250.0, half_angle=0.6):
    """a word on a 70-degree arc: 8 points on the outer circle, 8 back along the inner one"""
    th = np.linspace(-half_angle, half_angle, 8)
    top = [(cx + r_top * math.sin(a), cy - r_top * math.cos(a)) for a in th]
    bot = [(cx + r_bot * math.sin(a), cy - r_bot * math.cos(a)) for a in th[::-1]]
    return top + bot


def arc_ramp_error(strip, poly):
    """worst |ramp's analytic value at the analytically mapped point - strip pixel| (grey levels)"""
    P = np.asarray(poly, dtype=np.float64)
    T, B = P[:8], P[15:7:-1]
    sh, sw = strip.shape[:2]
    u = (np.arange(sw) + 0.5) / sw * 7
    k = np.minimum(u.astype(np.int64), 6)
    f = (u - k)[:, None]
    tp = T[k] * (1 - f) + T[k + 1] * f
    bp = B[k] * (1 - f) + B[k + 1] * f
    v = ((np.arange(sh) + 0.5) / sh)[:, None, None]
    p = tp[None] + (bp - tp)[None] * v
    return float(np.abs(0.3 * p[..., 0] + 0.4 * p[..., 1] - strip[..., 0].astype(np.float64)).max())


HOSTILE_HW = (9, 13)   # the tiny image the hostile polygons are cut from


def hostile_polys():
    """name -> (16 points, expected strip shape or None).  Heights stay small: the numpy reference holds int64 temporaries
    per strip pixel."""
    zig = [(0.0 if i % 2 == 0 else 700.0, 1.0) for i in range(8)] + [(0.0 if i % 2 else 700.0, 4.0) for i in range(8)]
    far = [(x, -5.0e4) for x in np.linspace(-1.0e5, 1.0e5, 8)] + [(x, -5.0e4 + 3.0) for x in np.linspace(1.0e5, -1.0e5, 8)]
    huge = [(x, 2.0) for x in np.linspace(-1.0e9, 1.0e9, 8)] + [(x, 4.0) for x in np.linspace(1.0e9, -1.0e9, 8)]
    bow = [(float(x), 1.0) for x in np.linspace(1, 11, 8)] + [(float(x), 7.0) for x in np.linspace(1, 11, 8)]   # bottom edge NOT walked back
    twist = [(2.0, 2.0), (9.0, 6.0), (3.0, 1.0), (10.0, 8.0), (1.0, 7.0), (8.0, 0.0), (4.0, 4.0), (12.0, 3.0),
             (0.0, 5.0), (11.0, 2.0), (5.0, 8.0), (7.0, 1.0), (2.0, 6.0), (9.0, 0.0), (6.0, 5.0), (3.0, 3.0)]
    odd = [(float('nan'), 1.0), (float('inf'), 2.0)] + [(4.0, 4.0)] * 5 + [(-float('inf'), 3.0)] + [(5.0, 6.0)] * 8
    return {
        'all points equal': ([(6.25, 3.5)] * 16, (1, 1)),
        'far outside the image': (far, (3, SMAX)),
        'beyond the coordinate clamp': (huge, (2, SMAX)),
        'bow tie (self-intersecting)': (bow, None),
        'twisted ring': (twist, None),
        'zig-zag clamped to SMAX': (zig, (3, SMAX)),
        'non-finite points': (odd, None),
    }


def word_scene(angle):
    """A string in Pillow's built-in bitmap font on a light plate over a blocky textured background, rotated by `angle`.
    -> (rotated image uint8, the rotated rectangle as 16 points, the upright tight crop resized to 32 x 128 as float)"""
    rng = np.random.RandomState(1)
    H, W = 120, 260
    bg = (rng.randint(0, 256, (H // 4, W // 4, 3)).repeat(4, 0).repeat(4, 1) // 3 + 150).astype(np.uint8)
    im = Image.fromarray(bg)
    d = ImageDraw.Draw(im)
    x0, y0, x1, y1 = WORD_BOX
    d.rectangle((x0, y0, x1 - 1, y1 - 1), fill=(250, 250, 240))
    d.text((x0 + 4, y0 + 5), 'OmniParser MI355X gfx950', fill=(10, 10, 10), font=ImageFont.load_default())
    up = np.asarray(im)
    target = np.asarray(Image.fromarray(up[y0:y1, x0:x1]).resize((128, 32), Image.BICUBIC)).astype(np.float64)
    R = np.ascontiguousarray(np.asarray(im.rotate(angle, resample=Image.BICUBIC, expand=True)))
    Hr, Wr = R.shape[:2]
    a = math.radians(angle)
    c, s = math.cos(a), math.sin(a)

    def fwd(x, y):   # Image.rotate turns counter-clockwise about the centre
        dx, dy = x - W / 2, y - H / 2
        return (c * dx + s * dy + Wr / 2, -s * dx + c * dy + Hr / 2)

    xs = np.linspace(x0, x1, 8)
    poly = [fwd(x, y0) for x in xs] + [fwd(x, y1) for x in xs[::-1]]
    return R, poly, target


def pillow_crop(strip, out_h=32, out_w=128):
    """uint8 strip -> uint8 [out_h, out_w, 3]: MGP-STR's crop transform (OCR/MGP-STR/dataset.py:462), the real Pillow"""
    return np.asarray(Image.fromarray(strip).resize((out_w, out_h), Image.BICUBIC))


def reference_crop(image, poly, out_h=32, out_w=128):
    """-> float32 [3, out_h, out_w]: rectify_polygon_cpu + Pillow bicubic + ToTensor"""
    c = pillow_crop(rectify_polygon_cpu(image, poly), out_h, out_w)
    return np.ascontiguousarray((c.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))


def crop_set():
    """The crops of the GPU parity check: (images, [(tag, image index, polygon, box or None)]).  Three random images of
    different sizes carry 600 rectangles (strips smaller and larger than 32 x 128 on each axis), then vertical text, the
    arc on the ramp, the hostile polygons on a tiny image and the rotated words."""
    rng = np.random.RandomState(11)
    images = [rng.randint(0, 256, (300, 500, 3), dtype=np.uint8), rng.randint(0, 256, (64, 48, 3), dtype=np.uint8),
              rng.randint(0, 256, (173, 911, 3), dtype=np.uint8)]
    crops = []
    for bi, n in ((0, 300), (1, 100), (2, 200)):
        H, W = images[bi].shape[:2]
        for r in random_rects(rng, H, W, n):
            crops.append(('rect', bi, rect_poly(*r), r))
    for r in random_rects(rng, 300, 500, 12 + 24)[12:]:   # 24 random ones after the fixed dozen
        crops.append(('vertical', 0, vertical_poly(*r), None))
    images.append(ramp_image())
    crops.append(('arc', len(images) - 1, arc_poly(), None))
    crops.append(('arc', 0, arc_poly(240.0, 310.0, 280.0, 200.0, 0.9), None))
    images.append(rng.randint(0, 256, HOSTILE_HW + (3,), dtype=np.uint8))
    for name, (poly, _) in hostile_polys().items():
        crops.append(('hostile: ' + name, len(images) - 1, poly, None))
    for ang in WORD_ANGLES:
        R, poly, _ = word_scene(ang)
        images.append(R)
        crops.append(('word at %d degrees' % ang, len(images) - 1, poly, None))
    return images, crops


# ---------------------------------------------------------------------------------------------
# GPU checks
# ---------------------------------------------------------------------------------------------
def check_polygon_cropper():
    """PolygonCropper == rectify_polygon_cpu + Pillow bicubic + / 255 on every float, over crop_set() in ONE call whose
    scratch budget (3 MB) cuts it into several chunks; on the rectangles also == CropResizer on the matching boxes."""
    import torch
    from advancedliteratemachinery_amd.utils.preprocess import CropResizer
    from advancedliteratemachinery_amd.utils.word_crops import PolygonCropper
    from tests.gpu_checks import DEV, rec
    images, crops = crop_set()
    dev_images = [torch.from_numpy(np.array(i)).to(DEV) for i in images]
    polys =[(bi, poly) for _, bi, poly, _ in crops]
    pc = PolygonCropper(DEV, scratch_bytes=3 << 20)
    got = pc(dev_images, polys).cpu()
    out = [rec('polygon_cropper: crops in the call', 0 if len(crops) >= 600 else 1, 0, '%d crops' % len(crops)),
           rec('polygon_cropper: chunks at a 3 MB budget', 0 if pc.last_chunks > 1 else 1, 0, '%d chunks' % pc.last_chunks)]
    worst, shapes = {}, set()
    for n, (tag, bi, poly, _) in enumerate(crops):
        sh, sw = polygon_strip_size(poly)
        shapes.add((sh < 32, sh > 32, sw < 128, sw > 128))
        ref = torch.from_numpy(reference_crop(images[bi], poly))
        e = 0.0 if torch.equal(got[n], ref) else max(float((got[n] - ref).abs().max()), 1e-9)
        worst[tag] = max(worst.get(tag, 0.0), e)
    for tag, e in worst.items():
        out.append(rec('polygon_cropper[%s] == cpu rectify + Pillow' % tag, e, 0.0))
    for i, name in enumerate(('lower', 'higher', 'narrower', 'wider')):
        out.append(rec('polygon_cropper: strips %s than 32 x 128 present' % name, 0 if any(s[i] for s in shapes) else 1, 0))
    rects = [n for n, c in enumerate(crops) if c[0] == 'rect']
    box = CropResizer(DEV)(dev_images, [(crops[n][1],) + tuple(crops[n][3]) for n in rects]).cpu()
    e = 0.0 if torch.equal(box, got[rects]) else max(float((box - got[rects]).abs().max()), 1e-9)
    out.append(rec('polygon_cropper == CropResizer on %d rectangles' % len(rects), e, 0.0))
    # one chunk (the default budget) gives the same floats as several
    one = PolygonCropper(DEV)
    again = one(dev_images, polys).cpu()
    out.append(rec('polygon_cropper: one chunk == several', 0 if torch.equal(again, got) and one.last_chunks == 1 else 1, 0, '%d chunk' % one.last_chunks))
    return out


def polygon_chain(sd_omni, args, depths, sd_mgp, cfg_mgp, images_u8, min_size, max_size):
    """oracle/two_stage_ref.py: chain with the crop step replaced: rectify_polygon_cpu + Pillow bicubic + ToTensor"""
    import torch
    from oracle import mgp_str_ref as R
    from oracle import omniparser_ref as O
    from oracle import preprocess_ref as P
    from oracle import two_stage_ref as T
    tens, mask, _ = P.preprocess_batch(images_u8, min_size, max_size)
    seqs = O.default_prompts(args)
    results = []
    for b, im in enumerate(images_u8):
        with torch.no_grad():
            out = O.forward(sd_omni, args, torch.from_numpy(tens[b:b + 1]), torch.from_numpy(mask[b:b + 1]), seqs, depths=depths)
        recs = T.records_from_output(out, args, (im.shape[0], im.shape[1]))
        crops = []
        for r in recs:
            r['strip'] = polygon_strip_size(r['polys'])
            crops.append(torch.from_numpy(reference_crop(im, r['polys'], cfg_mgp['img'][0], cfg_mgp['img'][1])))
        if crops:
            with torch.no_grad():
                _, ch, bp, wp = R.forward(sd_mgp, cfg_mgp, torch.stack(crops))
            for r, d in zip(recs, R.decode(ch, bp, wp)):
                r.update(d)
        results.append(recs)
    return results


def check_two_stage_polygon():
    """The models, images and args of check_two_stage: spot_and_recognize(crop='polygon') against polygon_chain, and
    crop='box' in the same run against oracle.two_stage_ref.chain (nothing moved)."""
    import torch
    from advancedliteratemachinery_amd.engine.two_stage import spot_and_recognize
    from advancedliteratemachinery_amd.utils import synthetic as weights
    from advancedliteratemachinery_amd.utils.parser import make_args
    from oracle import mgp_str_ref as R
    from oracle import two_stage_ref as T
    from tests.gpu_checks import build_model, rec
    from tests.gpu_checks_mgp import build
    depths = (2, 2, 2, 2)
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, pt_seq_length=6, test_min_size=64, test_max_size=112)
    sd = weights.make_state_dict(args, seed=5, depths=depths)
    omni = build_model(args, sd, depths, torch.float32)
    c = R.cfg(depth=2)
    sdm = R.make_state_dict(c, seed=17)
    mgp = build(c, sdm, torch.float32)
    rng = np.random.RandomState(3)
    images = [rng.randint(0, 256, (90, 140, 3), dtype=np.uint8), rng.randint(0, 256, (70, 100, 3), dtype=np.uint8)]
    out = []
    for mode in ('polygon', 'box'):
        got, _, _ = spot_and_recognize(omni, mgp, [torch.from_numpy(i) for i in images], args, crop=mode)
        chain = polygon_chain if mode == 'polygon' else T.chain
        want = chain(sd, args, depths, sdm, c, images, args.test_min_size, args.test_max_size)
        n_words = 0
        for b, (g, w) in enumerate(zip(got, want)):
            out.append(rec('two_stage[%s] img%d: detections' % (mode, b), abs(len(g) - len(w)), 0, '%d vs %d' % (len(g), len(w))))
            for i, (rg, rw) in enumerate(zip(g, w)):
                n_words += 1
                tag = 'two_stage[%s] img%d word%d' % (mode, b, i)
                if mode == 'polygon':
                    ok = rg.get('crop') == 'polygon' and tuple(rg['strip']) == tuple(rw['strip'])
                    out.append(rec(tag + ' strip', 0 if ok else 1, 0, '%s vs %s' % (rg.get('strip'), rw['strip'])))
                else:
                    out.append(rec(tag + ' box', 0 if tuple(rg['box']) == tuple(rw['box']) and 'strip' not in rg else 1, 0))
                for k in ('char', 'bpe', 'wp'):
                    out.append(rec(tag + ' %s ids' % k, sum(int(x != y) for x, y in zip(rg['mgp_ids'][k], rw[k + '_ids'])), 0))
                out.append(rec(tag + ' choice', 0 if rg['mgp_choice'] == rw['choice'] else 1, 0))
                out.append(rec(tag + ' confidences', max(abs(x - y) for x, y in zip(rg['mgp_conf'], rw['conf'])), 1e-4))
                out.append(rec(tag + ' text', 0 if rg['mgp_text'] == rw['char_text'] else 1, 0))
        out.append(rec('two_stage[%s]: words recognised' % mode, 0 if n_words > 0 else 1, 0, '%d words' % n_words))
    return out


def check_word_crop_speed():
    """512 rectangle polygons through PolygonCropper (two launches) against the same 512 boxes through CropResizer (512
    launches), timed back to back (tools/word_crop_bench.py): the polygon median at or below the box path's p90."""
    import os
    import sys
    from tests.gpu_checks import rec
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import word_crop_bench
    r = word_crop_bench.measure()
    note = 'polygon p10 / median / p90 %.3f / %.3f / %.3f ms, box %.3f / %.3f / %.3f ms' % (
        r['polygon_ms']['p10'], r['polygon_ms']['median'], r['polygon_ms']['p90'], r['box_ms']['p10'], r['box_ms']['median'], r['box_ms']['p90'])
    print(note)
    return [rec('word crops: 512 polygons, median <= box path p90', r['polygon_ms']['median'], r['box_ms']['p90'], note),
            rec('word crops: chunks of the 512-crop call', abs(r['chunks'] - 1), 0, '%d chunks, 2 launches each' % r['chunks'])]
