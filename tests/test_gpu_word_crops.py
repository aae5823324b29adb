"""Polygon-rectified word crops on the GPU: omp_polygon_rectify + omp_resize_crops through
PolygonCropper against rectify_polygon_cpu + the real Pillow, float for float; spot_and_recognize(crop='polygon') against
the oracle chain; two launches against 512."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _assert_all(records):
    bad = [r for r in records if not r['ok']]
    assert not bad, '\n'.join('%s: err=%.3e tol=%.1e %s' % (r['name'], r['err'], r['tol'], r['note']) for r in bad)


@pytest.fixture(scope='module')
def C():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from tests import gpu_checks_word_crops
    return gpu_checks_word_crops


def test_polygon_cropper_bit_exact_with_cpu_rectify_and_pillow(C):
    """600 rectangles over three images, vertical text, arcs, hostile polygons and rotated words in one call of several
    chunks: every float equal; the rectangles also equal CropResizer on their boxes"""
    _assert_all(C.check_polygon_cropper())


def test_two_stage_polygon_matches_oracle_chain(C):
    """OmniParser detections -> device polygon crops -> MGP-STR against the chain built from the oracle's pieces with
    rectify_polygon_cpu + Pillow as the crop step; crop='box' still equals oracle.two_stage_ref.chain"""
    _assert_all(C.check_two_stage_polygon())


def test_two_launches_do_not_lose_to_512(C):
    """512 rectangle polygons through PolygonCropper, median of 30 timed calls, at or below the p90 of the same boxes
    through CropResizer timed back to back"""
    _assert_all(C.check_word_crop_speed())
