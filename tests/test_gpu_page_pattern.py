"""Page patterns on the GPU (tests/gpu_checks_page_pattern.py): omp_page_pattern_search against its numpy specification on every integer
at the edges of chunks, warm-up, pattern length and optional runs, at the page length limit, the chunked device stage, the order of the
hits, the refusals, find_pattern on the device against the host searcher on a real engine call, and the structural time gate."""
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
    from tests import gpu_checks_page_pattern
    return gpu_checks_page_pattern


@pytest.mark.timeout(300, method='thread')
def test_page_pattern_equals_the_specification_at_the_edges(C):
    """P of 1, 2, 31 .. 33, 63, 64 against texts of 0, 1, P + k - 1 .. P + k + 1, 127 .. 129, 255 .. 257 and 643 characters under k = 0,
    the largest k and one between; no optional position, a leading and a trailing optional run, a run across bit 31 / 32, all but one
    position optional; sigma 1, 2, 26 and 254, a text of codes at or above sigma, a class that holds every code; an instance planted so
    that a hit ends at 127, 128, 129 and n, across 256 and inside the first P + k columns, exact, with one substitution, one lost and
    one extra character; every variant alone and all mixed into one call, at max_hits 64 and 1, into buffers prefilled with garbage"""
    _assert_all(C.check_edges())


@pytest.mark.timeout(120, method='thread')
def test_page_pattern_at_the_length_limit(C):
    """one page of 65 535 characters (all 8 rounds): a 64-position pattern planted at the start, in the middle and as the last 64
    characters, exact and with 3 errors, and a pattern that occurs nowhere"""
    _assert_all(C.check_limit())


@pytest.mark.timeout(120, method='thread')
def test_a_chunked_pattern_call_equals_the_unchunked_specification(C):
    _assert_all(C.check_chunked())


@pytest.mark.timeout(120, method='thread')
def test_pattern_hits_come_out_in_ascending_order_and_repeatably(C):
    """64 jobs on one page of 20 000 characters whose hits fall in many chunks and rounds"""
    _assert_all(C.check_ordering())


@pytest.mark.timeout(120, method='thread')
def test_page_pattern_refuses_with_error_codes(C):
    _assert_all(C.check_refusals())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.timeout(400, method='thread')
def test_find_pattern_on_the_device_equals_the_host_searcher(C, dtype):
    """the image, weights and call of the page-search engine test; patterns from the call's own records: a word as a literal, a word with
    a class for one of its characters, and a two-word shape with an optional separator"""
    _assert_all(C.check_engine_search(dtype))


@pytest.mark.timeout(120, method='thread')
def test_device_page_pattern_is_not_slower_than_the_host_definition(C):
    _assert_all(C.check_timing())
