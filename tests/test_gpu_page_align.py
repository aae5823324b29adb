"""Page text alignment on the GPU (tests/gpu_checks_page_align.py): omp_page_align against its numpy specification on every integer of
the counts and both maps -- at the edges of blocks and stripes, through three stripes, at the length limit, chunked --, the guards around
the owned slices, the refusals, and align_page_text on the device against the host aligner on a real engine call."""
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
    from tests import gpu_checks_page_align
    return gpu_checks_page_align


@pytest.mark.timeout(300, method='thread')
def test_page_align_equals_the_specification_at_the_edges(C):
    """la of 0, 1, 2, 63 .. 65, 127 .. 129, 4095 .. 4097 against lb of 0, 1, 63 .. 65, 300, 4097 and swapped: equal strings, sigma 1 with
    la != lb (every cell a tie: the canonical rule), sigma 2, 26 and 254, no common character, b all 255, 5 % edits, halves swapped; every
    variant alone and all mixed into one call with shared ranges.  Pairs with both sides at or above 4095 run under 5 % edits and sigma 1"""
    _assert_all(C.check_edges())


@pytest.mark.timeout(120, method='thread')
def test_page_align_through_three_stripes(C):
    _assert_all(C.check_stripes())


@pytest.mark.timeout(120, method='thread')
def test_page_align_of_thin_pairs_at_the_length_limit(C):
    _assert_all(C.check_limit())


@pytest.mark.timeout(120, method='thread')
def test_a_chunked_call_equals_the_unchunked_specification(C):
    _assert_all(C.check_chunked())


@pytest.mark.timeout(120, method='thread')
def test_page_align_writes_only_the_slices_it_owns(C):
    _assert_all(C.check_guards())


@pytest.mark.timeout(120, method='thread')
def test_page_align_refuses_with_error_codes(C):
    _assert_all(C.check_refusals())


@pytest.mark.timeout(400, method='thread')
def test_align_page_text_on_the_device_equals_the_host_aligner(C):
    """spot_windows' image and weights, windows = [default, 2 x 2 grid], suppress=0.5, fp32: align_page_text == the host aligner on
    every integer and status; a call against its own words is all MATCH with every word CORRECT and cer 0; against the blocks=True
    ordering the distance is score_page_text's"""
    _assert_all(C.check_engine_page_align('fp32'))
