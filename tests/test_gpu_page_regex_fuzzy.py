"""Page expressions with errors on the GPU (tests/gpu_checks_page_regex_fuzzy.py): omp_page_regex_fuzzy_search against its numpy
specification on every integer: random automata at the byte-table edges crossed with every tolerance, carries of the rows above 0 across
lanes and rounds, valley and plateau decisions across words, lanes and rounds, starts in other chunks and rounds, the page length limit
at k = 4, k = 0 against the exact kernel, the order of the hits, the refusals, find_regex(max_dist=1) on the device against the host
searcher on a real engine call, and the structural time gate."""
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
    from tests import gpu_checks_page_regex_fuzzy
    return gpu_checks_page_regex_fuzzy


@pytest.mark.timeout(300, method='thread')
def test_page_regex_fuzzy_equals_the_specification_at_the_edges(C):
    """chain automata with loops and backward edges of P = 1, 8, 9, 16, 17, 63 and 64 positions crossed with k = 0 .. 4 (bounded by the
    shortest word) against texts of 0, 1, 127 .. 129, 255 .. 257 and 8191 .. 8193 characters that hold noisy words of their languages;
    sigma 1 and 254, a text with codes at or above sigma; every variant alone and all mixed into one call with differing k, at max_hits
    64 and 1, into buffers prefilled with garbage"""
    _assert_all(C.check_edges())


@pytest.mark.timeout(120, method='thread')
def test_carries_valleys_plateaus_and_starts_across_lanes_and_rounds(C):
    """real expressions on planted texts at k = 1.  Carry: a misread bounded expression across column 128 and column 8192 with the error
    on either side, a digit run of 300 and of 9000 characters with one letter inside, a.*b with a substituted a.  Hits: valleys and
    plateaus whose three columns fall on bits 63 / 64 of a lane's words, on lanes and on rounds; a pending end of distance 1 at 8192
    followed by a distance 0, an equal and a greater one; a plateau that ends at n = 8192.  Starts: in the same chunk, the previous chunk,
    the previous round, at 0, and one that a walk which went on injecting last would put too early."""
    _assert_all(C.check_carry())


@pytest.mark.timeout(120, method='thread')
def test_page_regex_fuzzy_at_the_length_limit(C):
    """one page of 65 535 characters (all 8 rounds), a 64-position expression at k = 4, planted with errors at the start, in the middle,
    across a round's edge and at the end"""
    _assert_all(C.check_limit())


@pytest.mark.timeout(120, method='thread')
def test_k_0_gives_the_ends_and_starts_of_the_exact_kernel(C):
    """the exact entry point launches the instance of the expression kernel that holds one row, the entry point with errors the one that
    dispatches over k: both at k = 0 against each other and against search_cpu, on the edge jobs (every P, so every byte-table count; texts
    of 0, 1, 127 .. 129, 255 .. 257 and 8191 .. 8193 characters), on a pending end at column 8192 that is a hit and one that is none, and on
    one refused job"""
    _assert_all(C.check_exact())


@pytest.mark.timeout(120, method='thread')
def test_fuzzy_hits_come_out_in_ascending_order_and_repeatably(C):
    """32 jobs on one page of 20 000 characters whose hits fall in many chunks and all rounds, at max_hits 64 and 1"""
    _assert_all(C.check_ordering())


@pytest.mark.timeout(120, method='thread')
def test_page_regex_fuzzy_refuses_with_error_codes(C):
    _assert_all(C.check_refusals())


@pytest.mark.timeout(400, method='thread')
def test_find_regex_with_errors_on_the_device_equals_the_host_searcher(C):
    """the image, weights and call of the page-expression engine test at fp32; expressions from the call's own words with one character
    changed, so that the exact search misses them and max_dist=1 finds them; one FuzzyRegexSearcher.run for the call"""
    _assert_all(C.check_engine_search('fp32'))


@pytest.mark.timeout(120, method='thread')
def test_device_page_regex_fuzzy_is_not_slower_than_the_host_definition(C):
    _assert_all(C.check_timing())
