"""Lexicon correction on the GPU: omp_lexicon_nearest through LexiconMatcher against
utils/lexicon.py: nearest_cpu, index for index and distance for distance; descriptors the kernel must refuse or clamp; the
engine's `lexicon=` end to end; one launch against the host computation.  Straight through ops.lexicon_nearest: every
(query length, word length) pair against the definition, slice boundaries, the pool's last bytes, damaged tables between
canaries, the fill kernel off its tile."""
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


def test_length_grid(C):
    """query lengths 0 to 64 x word lengths 0 to 255 x six variants (carry chains, two symbols, the whole alphabet, near
    matches, disjoint alphabets, unknowns), one word per pair: every distance equals the definition under any range_hint,
    unknown codes match nothing (themselves included), and the distinct queries against the whole grid equal nearest_cpu"""
    _assert_all(C.check_length_grid())


def test_slices(C):
    """2 queries x 2049 words in 9 slices: equal spellings across a slice boundary and at both ends, the nearest word at the
    last index, a tie between the last index and index 5, ranges that re-cut the slices"""
    _assert_all(C.check_slices())


def test_pool_tail(C):
    """pool_bytes = P - 16 .. P with live bytes behind: the cut word answers, nothing at or beyond pool_bytes is used"""
    _assert_all(C.check_pool_tail())


def test_damaged_tables_are_clamped(C):
    """falling, negative, overlong and 2^31 - 1 offsets, pool_bytes 0 and lowered, a word of 300 characters: answered as
    the materialised table, canaries round best intact; argument errors leave best untouched"""
    _assert_all(C.check_damaged_tables())


def test_fill_edges(C):
    """N = 1, 255, 256, 257, 513 into a best full of canary words: empty ranges for all queries, then for the even ones only (the odd ones are answered)"""
    _assert_all(C.check_fill_edges())


def test_engine_lexicon_end_to_end(C):
    """predict_images(lexicon=...) and spot_and_recognize(crop='polygon', lexicon=...): the records minus the new keys are
    those of the call without a lexicon, the new keys are nearest_cpu of the records' own strings"""
    _assert_all(C.check_end_to_end())


def test_one_launch_does_not_lose_to_the_host(C):
    """512 queries against 90 000 words (tools/lexicon_bench.py): the median of 30 device calls after 5 at or below
    nearest_cpu's time for the same 512 queries, timed on 32 of them in the same session and scaled linearly"""
    _assert_all(C.check_timing())
