"""The reading-order stage on the GPU (tests/gpu_checks_reading.py): omp_reading_links / omp_reading_lines against their numpy
specification on every output integer, and `reading_order=` of predict / spot_and_recognize against lines_cpu on the host."""
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
    from tests import gpu_checks_reading
    return gpu_checks_reading


@pytest.mark.timeout(300, method='thread')
def test_reading_links_and_lines_equal_the_specification(C):
    """groups of 0, 1, 2, 63, 64, 65, 255, 256, 257, 513; G = 1 and 40 with empty groups; word rows, rotated rows, the ring, random
    16-gons, exact duplicates, all-degenerate groups; grids 1000, 4096 and 64; aspects (256, 256), (256, 128), (37, 256), (1, 1);
    parameters at their defaults, all 0 and all 10000; groups of 1023, 1024, 1025 and 2049 on grid 4096 at the defaults"""
    _assert_all(C.check_reading_op())


@pytest.mark.timeout(300, method='thread')
def test_reading_largest_group(C):
    """one group of exactly 8192 words, a page of 128 rows of 64, against lines_cpu (its blocked links take a few seconds on the host)"""
    _assert_all(C.check_reading_largest_group())


@pytest.mark.timeout(300, method='thread')
def test_reading_lines_resolve_planted_links(C):
    """omp_reading_lines alone on planted succ0 / cost0 against resolve_cpu: groups of 1023, 1024, 1025, 2048, 2049, 4097, 8191 and 8192
    words, and [1025, 0, 1, 8192, 1023] in one call; one chain, one cycle, many cycles and paths, stars of 2, 64 and 1025 claimants with
    equal and with distinct costs, costs 0 and 2^43 - 1, links the kernel ignores; random words, identical words, every y at 4095"""
    _assert_all(C.check_reading_resolution())


@pytest.mark.timeout(120, method='thread')
def test_reading_refuses_with_error_codes(C):
    _assert_all(C.check_reading_refusals())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.timeout(400, method='thread')
def test_predict_reading_order_equals_the_host_specification(C, dtype):
    """spot_windows' image and weights, windows = [default, 2 x 2 grid], suppress=0.5: the records are a permutation of the call
    without reading_order; order, line and line_pos as lines_cpu on the survivors' raw polygon ids; reading_order=False is today's"""
    _assert_all(C.check_engine_reading(dtype))


@pytest.mark.timeout(300, method='thread')
def test_two_stage_reads_in_reading_order(C):
    _assert_all(C.check_two_stage_reading())
