"""Tiled pages on the GPU (tests/gpu_checks_tiles.py): omp_tile_remap against its numpy specification on every output integer, tiled
engine calls against every tile alone and against the specification applied to the same ids, the identity tiling against today's
predict_images, the page stages against their specifications on the page polygons, and the two-stage reader."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _assert_all(records):
    assert records
    bad = [r for r in records if not r['ok']]
    assert not bad, '\n'.join('%s: err=%.3e tol=%.1e %s' % (r['name'], r['err'], r['tol'], r['note']) for r in bad[:40])


@pytest.fixture(scope='module')
def C():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from tests import gpu_checks_tiles
    return gpu_checks_tiles


@pytest.mark.timeout(300, method='thread')
def test_tile_remap_equals_the_specification(C):
    """1 .. 5000 words on 1 .. 5 pages of 1 .. 64 tiles, empty tiles and pages; both drop_cut values; edge 0, 2 and nb; out-of-range ids;
    the 65535-pixel and 4096-bin corners; a cap at half the total; refused descriptors: every output integer"""
    _assert_all(C.check_tile_remap_op())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.timeout(400, method='thread')
def test_tiled_call_equals_every_tile_alone_and_the_specification(C, dtype):
    """tiles=(2, 2) on a 150x220 and a 110x160 page, ragged: ids identical to every tile view alone (fp32, bf16x3; bf16 within the
    agreement bound of the ragged window checks, 0.95), the page records == tile_records(remap_cpu(ids))"""
    _assert_all(C.check_engine_tiles(dtype))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.timeout(300, method='thread')
def test_identity_tiling_is_todays_predict_images(C, dtype):
    _assert_all(C.check_identity_tiling(dtype))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.timeout(300, method='thread')
def test_page_stages_run_on_the_page_polygons(C, dtype):
    """suppress= and reading_order=True of a tiled call: merged, line, line_pos == suppress_cpu / lines_cpu on page_polys at page_bins"""
    _assert_all(C.check_page_stages(dtype))


@pytest.mark.timeout(300, method='thread')
def test_two_stage_with_tiles(C):
    """spot_and_recognize(tiles=(2, 2)): mgp_* equal to recognize_crops on the records' page polygons, for 'box' and 'polygon'"""
    _assert_all(C.check_two_stage_tiles())
