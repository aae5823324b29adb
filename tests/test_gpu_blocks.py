"""The block stage on the GPU (tests/gpu_checks_blocks.py): omp_reading_blocks against its numpy specification blocks_cpu on every
output integer, and `blocks=` of predict / spot_and_recognize against lines_cpu + blocks_cpu on the host."""
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
    from tests import gpu_checks_blocks
    return gpu_checks_blocks


@pytest.mark.timeout(300, method='thread')
def test_reading_blocks_equal_the_specification(C):
    """groups of 0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025 lines; G = 1 and 40 with empty groups; column pages, nested
    pages, random 16-gons, exact duplicates, all-degenerate groups; grids 1000, 4096 and 64; aspects (256, 256), (256, 128),
    (37, 256), (1, 1); gaps 0, the defaults and 10000; depths 1, 2, 8 and 16"""
    _assert_all(C.check_blocks_op())


@pytest.mark.timeout(300, method='thread')
def test_links_lines_and_blocks_in_one_call(C):
    """ReadingOrder.run(blocks=...) on column pages, the nested page, random 16-gons, duplicates and degenerate groups: blocks_cpu on
    lines_cpu's lines, and the lines themselves unchanged"""
    _assert_all(C.check_blocks_pipeline())


@pytest.mark.timeout(300, method='thread')
def test_reading_blocks_largest_group(C):
    """one group of exactly 8192 single-word lines, 8 columns of 1024"""
    _assert_all(C.check_blocks_largest_group())


@pytest.mark.timeout(120, method='thread')
def test_reading_blocks_refuses_with_error_codes(C):
    _assert_all(C.check_blocks_refusals())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.timeout(400, method='thread')
def test_predict_blocks_equal_the_host_specification(C, dtype):
    """spot_windows' image and weights, windows = [default, 2 x 2 grid], suppress=0.5: the records are a permutation of the call
    without blocks; order, block, line and line_pos as lines_cpu + blocks_cpu on the survivors' raw polygon ids; blocks=False is
    today's predict(reading_order=True)"""
    _assert_all(C.check_engine_blocks(dtype))


@pytest.mark.timeout(300, method='thread')
def test_two_stage_reads_block_by_block(C):
    _assert_all(C.check_two_stage_blocks())
