"""Overlap suppression on the GPU (tests/gpu_checks_overlap.py): omp_polygon_overlap / omp_polygon_keep against their numpy
specification on every output integer, and `suppress=` of predict / spot_and_recognize against suppress_cpu on the host."""
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
    from tests import gpu_checks_overlap
    return gpu_checks_overlap


@pytest.mark.timeout(300, method='thread')
def test_polygon_overlap_and_keep_equal_the_specification(C):
    """groups of 1, 2, 0, 63, 64, 65, 129; G = 1 and 40; word-like rectangles, random 16-gons, duplicates, whole-grid pairs at
    grid 1000 and 4096; grid 64; both measures at t = 1, 500, 1000; identity, reversed and random order; inter on and off"""
    _assert_all(C.check_overlap_op())


@pytest.mark.parametrize('call', [0, 1, 2], ids=['4097', '4032-4096-4161', '8192'])
@pytest.mark.timeout(300, method='thread')
def test_polygon_overlap_and_keep_above_4096_polygons(C, call):
    """groups of 4097 | 4032, 4096, 4161 | 8192 on grid 4096: duplicates and chains planted across position 4096, so that the keep
    kernel's second wave hands over its word, takes kept rows from wave 0 and assigns owners; (iou, 500) in identity, reversed and
    random order, (iomin, 1000) random, (iou, 1) identity; every mask word up to 4161, sampled mask rows at 8192"""
    _assert_all(C.check_overlap_large_groups(call))


@pytest.mark.timeout(120, method='thread')
def test_polygon_overlap_refuses_with_error_codes(C):
    """the entry points' error codes, and what only the device tables show: a group of 8193 and a group whose rows do not fit the mask
    come back as kept = -1 with owner = identity, beside a group that is processed"""
    _assert_all(C.check_overlap_refusals())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.timeout(400, method='thread')
def test_predict_suppress_equals_the_host_specification(C, dtype):
    """spot_windows' image and weights, windows = [default, default, 2 x 2 grid]: survivors and merged lists as suppress_cpu on the
    records of the same call; at least one record removed; suppress=None is today's predict"""
    _assert_all(C.check_engine_suppress(dtype))


@pytest.mark.timeout(300, method='thread')
def test_two_stage_recognises_the_survivors_only(C):
    _assert_all(C.check_two_stage_suppress())
