"""Polygon-rectified word crops, CPU side: the integer map of utils/word_crops.py
(rectify_polygon_cpu, the specification the kernel is held to on the GPU) on rectangles, vertical text, an arc, hostile
polygons and a rendered word; the host packing of PolygonCropper; the entry points' arguments."""
import numpy as np
import pytest
from PIL import Image

from advancedliteratemachinery_amd.utils import word_crops as WC
from advancedliteratemachinery_amd.utils.word_crops import polygon_strip_size, rectify_polygon_cpu
from tests import gpu_checks_word_crops as K


@pytest.fixture(scope='module')
def image():
    return np.random.RandomState(0).randint(0, 256, (300, 500, 3), dtype=np.uint8)


def test_rectangle_is_the_slice_and_resizes_like_a_box_crop(image):
    """integer-cornered rectangles as 16 evenly spaced points (one pixel wide / high and border-touching ones included):
    the strip IS the slice, and strip -> Pillow bicubic == crop -> Pillow bicubic"""
    H, W = image.shape[:2]
    rects = K.random_rects(np.random.RandomState(1), H, W, 1200)
    assert any(x1 - x0 == 1 for x0, _, x1, _ in rects) and any(y1 - y0 == 1 for _, y0, _, y1 in rects)
    assert any(x0 == 0 for x0, _, _, _ in rects) and any(x1 == W for _, _, x1, _ in rects)
    assert any(y0 == 0 for _, y0, _, _ in rects) and any(y1 == H for _, _, _, y1 in rects)
    pil = Image.fromarray(image)
    bad = []
    for (x0, y0, x1, y1) in rects:
        poly = K.rect_poly(x0, y0, x1, y1)
        assert polygon_strip_size(poly) == (y1 - y0, x1 - x0)
        s = rectify_polygon_cpu(image, poly)
        if s.shape != (y1 - y0, x1 - x0, 3) or not np.array_equal(s, image[y0:y1, x0:x1]):
            bad.append(('strip', x0, y0, x1, y1))
        elif not np.array_equal(K.pillow_crop(s), np.asarray(pil.crop((x0, y0, x1, y1)).resize((128, 32), Image.BICUBIC))):
            bad.append(('resize', x0, y0, x1, y1))
    assert not bad, bad[:10]


def test_vertical_text_is_the_rotated_slice(image):
    H, W = image.shape[:2]
    bad = []
    for (x0, y0, x1, y1) in K.random_rects(np.random.RandomState(2), H, W, 600):
        s = rectify_polygon_cpu(image, K.vertical_poly(x0, y0, x1, y1))
        want = np.rot90(image[y0:y1, x0:x1])
        if s.shape != want.shape or not np.array_equal(s, want):
            bad.append((x0, y0, x1, y1))
    assert not bad, bad[:10]


def test_curved_text_follows_the_arc():
    """a 70-degree arc over a linear ramp: every strip pixel within 1 grey level of the ramp's analytic value at the
    analytically mapped point (0.5 from the ramp's own rounding + 0.5 from the strip's)"""
    ramp = K.ramp_image()
    poly = K.arc_poly()
    strip = rectify_polygon_cpu(ramp, poly)
    assert strip.shape[:2] == polygon_strip_size(poly)
    assert strip.shape[0] == 50 and 300 < strip.shape[1] < 340      # radii 300 / 250, 1.2 rad: chords of 330 and 275
    err = K.arc_ramp_error(strip, poly)
    print('arc strip %s worst ramp error %.3f grey levels' % (strip.shape[:2], err))
    assert err <= 1.0


@pytest.mark.parametrize('name', sorted(K.hostile_polys()))
def test_hostile_polygons_clamp(name):
    poly, shape = K.hostile_polys()[name]
    img = np.random.RandomState(3).randint(0, 256, K.HOSTILE_HW + (3,), dtype=np.uint8)
    sh, sw = polygon_strip_size(poly)
    assert 1 <= sh <= WC.SMAX and 1 <= sw <= WC.SMAX
    if shape is not None:
        assert (sh, sw) == shape
    s = rectify_polygon_cpu(img, poly)
    assert s.dtype == np.uint8 and s.shape == (sh, sw, 3)
    assert img.min() <= s.min() and s.max() <= img.max()            # an interpolation of image bytes, nothing else
    if name == 'all points equal':
        # (6.25, 3.5) is the centre of row 3, three quarters of the way from the centre of column 5 to that of column 6
        assert np.array_equal(s[0, 0], (img[3, 5].astype(np.int64) * 16384 + img[3, 6].astype(np.int64) * 49152 + 32768) >> 16)
    rectify_polygon_cpu(np.zeros((1, 1, 3), np.uint8), poly)        # a one-pixel image: every coordinate clamps to it


def test_a_polygon_is_16_points():
    with pytest.raises(ValueError):
        polygon_strip_size([(0.0, 0.0)] * 15)
    with pytest.raises(ValueError):
        rectify_polygon_cpu(np.zeros((4, 4, 3), np.float32), K.rect_poly(0, 0, 2, 2))


@pytest.mark.parametrize('angle', K.WORD_ANGLES)
def test_it_is_a_word_not_a_rectangle(angle):
    """A rendered word rotated by `angle`, handed over as its rotated rectangle: against the upright tight crop resized
    to 32 x 128, the polygon crop's mean absolute difference is at most a quarter of today's bounding-box crop's (the
    residue is the rotation's own bicubic resampling), exactly 0 at 90 degrees, and the strip is the word's 24 x 180."""
    R, poly, target = K.word_scene(angle)
    strip = rectify_polygon_cpu(R, poly)
    assert strip.shape == (24, 180, 3)
    from advancedliteratemachinery_amd.engine.two_stage import polygon_box
    x0, y0, x1, y1 = polygon_box(poly, R.shape[1], R.shape[0])
    mad_poly = float(np.abs(K.pillow_crop(strip).astype(np.float64) - target).mean())
    mad_box = float(np.abs(K.pillow_crop(R[y0:y1, x0:x1]).astype(np.float64) - target).mean())
    print('angle %d: polygon MAD %.2f, box MAD %.2f grey levels' % (angle, mad_poly, mad_box))
    assert mad_poly <= 0.25 * mad_box
    if angle == 90:
        assert mad_poly == 0.0


def test_chunks_follow_the_scratch_budget():
    pc = WC.PolygonCropper('cpu', scratch_bytes=1000, max_crops=3)
    assert list(pc._chunks([400, 400, 400, 5000, 10, 10, 10, 10, 991])) == [(0, 2), (2, 3), (3, 4), (4, 7), (7, 8), (8, 9)]
    assert list(pc._chunks([])) == []
    assert list(WC.PolygonCropper('cpu')._chunks([48 << 20] * 6)) == [(0, 5), (5, 6)]      # 256 MB of worst-case strips


def test_packed_tables_are_pillows():
    """the per-axis block PolygonCropper packs = resize_coeffs' bounds then coefficients; no block when the size stays"""
    from advancedliteratemachinery_amd.utils.preprocess import resize_coeffs
    pc = WC.PolygonCropper('cpu')
    ks, flat = pc._axis(57, 128)
    k2, b, k = resize_coeffs(57, 128, 'bicubic')
    assert ks == k2 and flat.dtype == np.int32
    assert np.array_equal(flat[:256].reshape(128, 2), b) and np.array_equal(flat[256:].reshape(128, ks), k)
    assert pc._axis(128, 128) == (0, None)
    assert pc._axis(57, 128)[1] is flat                                   # cached per (n_in, n_out)


def test_descriptor_layouts_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'omp355.h')).read()
    for name, dt in (('omp_rectify_desc', WC.RECTIFY_DESC), ('omp_resize_desc', WC.RESIZE_DESC)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                fields += [re.sub(r'\[.*', '', f.split()[-1]).lstrip('*') for f in decl.split(',')]
        assert fields == list(dt.names), (fields, dt.names)


def test_entry_points_take_crop_and_ragged():
    import inspect
    from advancedliteratemachinery_amd.engine import two_stage
    sig = inspect.signature(two_stage.spot_and_recognize).parameters
    assert sig['crop'].default == 'box' and sig['ragged'].default is False
    assert inspect.signature(two_stage.recognize_crops).parameters['polys'].default is None
    with pytest.raises(ValueError):
        two_stage.spot_and_recognize(None, None, [], None, crop='circle')
    assert two_stage.recognize_crops(None, [], [], polys=[]) == ([], None)
