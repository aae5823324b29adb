"""Lexicon correction on the GPU: omp_lexicon_nearest through LexiconMatcher against
utils/lexicon.py: nearest_cpu, index for index and distance for distance; descriptors the kernel must refuse or clamp; the
engine's `lexicon=` end to end; one launch against the host computation."""
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
    from tests import gpu_checks_lexicon
    return gpu_checks_lexicon


def test_kernel_equals_nearest_cpu(C):
    """20 000 synthetic words of length 1 to 40 (duplicates and near-duplicates among them), 1 024 queries (edited lexicon
    words, random strings, the empty string, length-64 strings, repeated characters): the whole lexicon, random ranges
    including empty and single-word ones, 64 per-image ranges -- idx and dist identical for every query"""
    _assert_all(C.check_kernel_against_nearest_cpu())


def test_edges(C):
    """a lexicon of one word, L and N off every tile, query chunks of 100, consecutive calls with different ranges on
    one matcher, a side stream, the acceptance rule"""
    _assert_all(C.check_edges())


def test_hostile_descriptors_are_refused_or_clamped(C):
    """q_len of -1 and 200, hi > L, lo < 0 and an inverted range, straight through ops: the documented outputs"""
    _assert_all(C.check_hostile_descriptors())


def test_engine_lexicon_end_to_end(C):
    """predict_images(lexicon=...) and spot_and_recognize(crop='polygon', lexicon=...): the records minus the new keys are
    those of the call without a lexicon, the new keys are nearest_cpu of the records' own strings"""
    _assert_all(C.check_end_to_end())


def test_one_launch_does_not_lose_to_the_host(C):
    """512 queries against 90 000 words (tools/lexicon_bench.py): the median of 30 device calls after 5 at or below
    nearest_cpu's time for the same 512 queries, timed on 32 of them in the same session and scaled linearly"""
    _assert_all(C.check_timing())
