"""Page search on the GPU (tests/gpu_checks_page_search.py): omp_page_search against its numpy specification on every integer at the
edges of chunks, warm-up and query length, at the page length limit, the chunked device stage, the order of the hits, the refusals,
find_text on the device against the host searcher on a real engine call, and the structural time gate."""
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
    from tests import gpu_checks_page_search
    return gpu_checks_page_search


@pytest.mark.timeout(300, method='thread')
def test_page_search_equals_the_specification_at_the_edges(C):
    """m of 1, 2, 31 .. 33, 63, 64 against texts of 0, 1, m - 1 .. m + 1, 2m - 1 .. 2m + 1, C - 1 .. C + 1, 2C - 1 .. 2C + 1 and 5C + 3
    characters: all-equal strings, sigma 1, 2, 26 and 254, no common character, a text of 255s; the query planted so that a hit ends at
    C - 1, C, C + 1 and n, across a chunk boundary and inside the first 2m columns, under k = 0 and k = m - 1; every variant alone and
    all mixed into one call with shared ranges, at max_hits 64 and 1, into buffers prefilled with garbage"""
    _assert_all(C.check_edges())


@pytest.mark.timeout(120, method='thread')
def test_page_search_at_the_length_limit(C):
    """one page of 65 535 characters: a 64-character query planted at the start, in the middle and as the last 64 characters, exact and
    with 3 substitutions, and a query that occurs nowhere"""
    _assert_all(C.check_limit())


@pytest.mark.timeout(120, method='thread')
def test_a_chunked_call_equals_the_unchunked_specification(C):
    _assert_all(C.check_chunked())


@pytest.mark.timeout(120, method='thread')
def test_hits_come_out_in_ascending_order_and_repeatably(C):
    """64 jobs on one page of 20 000 characters whose hits fall in many chunks and rounds"""
    _assert_all(C.check_ordering())


@pytest.mark.timeout(120, method='thread')
def test_page_search_refuses_with_error_codes(C):
    _assert_all(C.check_refusals())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.timeout(400, method='thread')
def test_find_text_on_the_device_equals_the_host_searcher(C, dtype):
    """the image, weights and call of the page-text engine test; queries from the call's own records: three single words, two two-word
    phrases and one phrase with a character substituted"""
    _assert_all(C.check_engine_search(dtype))


@pytest.mark.timeout(120, method='thread')
def test_device_page_search_is_not_slower_than_the_host_definition(C):
    _assert_all(C.check_timing())
