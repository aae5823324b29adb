"""Page text scoring on the GPU (tests/gpu_checks_page_text.py): omp_page_edit_distance against its numpy specification on every
integer, closed forms at the length limit, the chunked device stage, the refusals, score_page_text and sweep_reading on the device against
the host scorer on a real engine call, and the structural time gate."""
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
    from tests import gpu_checks_page_text
    return gpu_checks_page_text


@pytest.mark.timeout(300, method='thread')
def test_page_edit_distance_equals_the_specification_at_the_edges(C):
    """la of 0, 1, 2, 63 .. 65, 127 .. 129, 4095 .. 4097, 8193 against lb of 0, 1, 64, 65, 300, 4097 and swapped: all-equal strings, sigma 1,
    2, 26 and 254, no common character, b all 255, 5 % edits, halves swapped; every variant alone, under sigma 254, and all mixed into one
    call with shared ranges"""
    _assert_all(C.check_edges())


@pytest.mark.timeout(120, method='thread')
def test_page_edit_distance_at_the_length_limit(C):
    """65 535 random characters against themselves (0), with 7 substitutions (7), their tail from 100 (100), the empty string (65 535) and
    64 characters (the definition), each way round"""
    _assert_all(C.check_limit())


@pytest.mark.timeout(120, method='thread')
def test_a_chunked_call_equals_the_unchunked_specification(C):
    _assert_all(C.check_chunked())


@pytest.mark.timeout(120, method='thread')
def test_page_edit_distance_refuses_with_error_codes(C):
    _assert_all(C.check_refusals())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.timeout(400, method='thread')
def test_score_page_text_on_the_device_equals_the_host_scorer(C, dtype):
    """spot_windows' image and weights, windows = [default, 2 x 2 grid], suppress=0.5; ground truth = the blocks=True call's own page
    strings: score_page_text == the host scorer on every integer, the blocks=True records score 1.0, sweep_reading over 4 settings == the
    host sweep and runs one device call"""
    _assert_all(C.check_engine_page_text(dtype))


@pytest.mark.timeout(120, method='thread')
def test_device_page_scoring_is_not_slower_than_the_host_definition(C):
    _assert_all(C.check_timing())
