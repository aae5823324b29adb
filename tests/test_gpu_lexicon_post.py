"""Posterior lexicon decoding on the GPU: omp_logprob_costs against costs_cpu (within one unit) and
greedy_cpu, omp_lexicon_posterior against score_cpu key for key, descriptors the kernels must refuse or clamp, PosteriorMatcher,
MGPSTR.recognize(lexicon=...) and spot_and_recognize(lexicon_mode='posterior') end to end, one call against the host computation."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _assert_all(records):
    for r in records:
        print('%s: err=%g tol=%g %s' % (r['name'], r['err'], r['tol'], r['note']))
    bad = [r for r in records if not r['ok']]
    assert not bad, '\n'.join('%s: err=%.3e tol=%.1e %s' % (r['name'], r['err'], r['tol'], r['note']) for r in bad)


@pytest.fixture(scope='module')
def C():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from tests import gpu_checks_lexicon_post
    return gpu_checks_lexicon_post


def test_costs_equal_costs_cpu_within_one_unit(C):
    """N in (1, 2, 63, 65, 513), random normal logits times 1, 8 and 50 with planted equal rows and ties and the worked rows: every
    cost within one unit of costs_cpu (the fp32 log-softmax is good to about 1e-5 nat = 0.01 unit, so only a rounding boundary can
    move a value, and by one), the worked rows exact, greedy == greedy_cpu of the device's own costs"""
    _assert_all(C.check_costs())


def test_search_equals_score_cpu(C):
    """N in (1, 2, 63, 65) x L in (1, 2, 255, 256, 257, 1025, 20000), word lengths 0, 1, 7, 8, 9, 25, 26, 255, a last word ending
    exactly at an odd pool_bytes, duplicates, unscorable words; whole, random (empty, single-word, inverted among them) and
    per-image ranges; range_hint 0 and the largest range -- both keys of every query identical"""
    _assert_all(C.check_search())


def test_search_edges(C):
    """duplicates across a slice boundary, an all-unscorable lexicon, every cost at COST_CAP, single-word and empty ranges"""
    _assert_all(C.check_search_edges())


def test_hostile_descriptors_are_refused_or_clamped(C):
    """falling and overlong offsets, pool_bytes 0, ranges outside [0, L], null pointers, negative counts, straight through ops: an
    error code or the specification's answer under its clamping rules; canaries round best and work intact"""
    _assert_all(C.check_hostile_descriptors())


def test_posterior_matcher(C):
    """one chunk and chunks of 100, per-image ranges, a side stream, the acceptance rule"""
    _assert_all(C.check_matcher())


@pytest.mark.parametrize('dtype_name', ['fp32', 'bf16x3'])
def test_engine_posterior_end_to_end(C, dtype_name):
    """MGPSTR.recognize(lexicon=...) and spot_and_recognize(crop='polygon', lexicon=..., lexicon_mode='posterior') with a shared list
    and per-image lists: records minus the new keys equal the call without them, the new keys equal score_cpu / greedy_cpu /
    accept_post on the costs the device produced for those crops, lex* equals the 'edit' call's, the default call is unchanged"""
    _assert_all(C.check_end_to_end(dtype_name))


def test_one_call_does_not_lose_to_the_host(C):
    """512 queries against 90 000 words (tools/lexicon_post_bench.py): the median of 30 device calls after 5 at or below score_cpu's
    time for the same 512 queries, timed on 32 of them in the same session and scaled linearly.  No margin: the gate catches a launch
    or a synchronisation per query, not a tuning"""
    _assert_all(C.check_timing())
