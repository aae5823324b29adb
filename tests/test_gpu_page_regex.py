"""Page expressions on the GPU (tests/gpu_checks_page_regex.py): omp_page_regex_search against its numpy specification on every integer at
the edges of chunks, rounds and byte tables, with carries across lanes and rounds, hit decisions across owners, starts in other chunks
and rounds, at the page length limit, the order of the hits, the refusals, find_regex on the device against the host searcher on a real
engine call, and the structural time gate."""
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
    from tests import gpu_checks_page_regex
    return gpu_checks_page_regex


@pytest.mark.timeout(300, method='thread')
def test_page_regex_equals_the_specification_at_the_edges(C):
    """random automata of P = 1, 8, 9, 16, 17, 63 and 64 positions (the byte-table edges) against texts of 0, 1, 127 .. 129, 255 .. 257 and
    8191 .. 8193 characters; sigma 1, 2, 26 and 254, a text of codes at or above sigma, a class that holds every code; every variant alone
    and all mixed into one call, at max_hits 64 and 1, into buffers prefilled with garbage"""
    _assert_all(C.check_edges())


@pytest.mark.timeout(120, method='thread')
def test_carries_hit_decisions_and_starts_across_lanes_and_rounds(C):
    """real expressions on planted texts.  Carry: a bounded expression across a 128-column edge and across the 8192 edge, a digit run of
    300 (three lanes) and of 9000 characters (across a round), a.*b with a at column 1 and b at column 129, 8193 and 20 000, a carried
    state that is a subset of the speculative one.  Hits: runs of ends across 64 / 65, 128 / 129 and 8192 / 8193, a run that stops
    exactly at 128, at 8192, at 16 384 = n and at n, a pending end at 8192 followed by a non-end and by an end.  Starts: in the same
    chunk, the previous chunk, the previous round, at 0, and the longest of several."""
    _assert_all(C.check_carry())


@pytest.mark.timeout(120, method='thread')
def test_page_regex_at_the_length_limit(C):
    """one page of 65 535 characters (all 8 rounds): a 64-position expression planted at the start, in the middle and as the last 64
    characters, a loop over the whole page, and an expression that occurs nowhere"""
    _assert_all(C.check_limit())


@pytest.mark.timeout(120, method='thread')
def test_regex_hits_come_out_in_ascending_order_and_repeatably(C):
    """64 jobs on one page of 20 000 characters whose hits fall in many chunks and rounds"""
    _assert_all(C.check_ordering())


@pytest.mark.timeout(120, method='thread')
def test_page_regex_refuses_with_error_codes(C):
    _assert_all(C.check_refusals())


@pytest.mark.timeout(400, method='thread')
def test_find_regex_on_the_device_equals_the_host_searcher(C):
    """the image, weights and call of the page-pattern engine test at fp32; expressions from the call's own records: an alternation of two
    of its words and a `+` loop over a class"""
    _assert_all(C.check_engine_search('fp32'))


@pytest.mark.timeout(120, method='thread')
def test_device_page_regex_is_not_slower_than_the_host_definition(C):
    _assert_all(C.check_timing())
