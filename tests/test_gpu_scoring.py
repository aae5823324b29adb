"""Scoring on the GPU (tests/gpu_checks_scoring.py): omp_spotting_match against its numpy specification on every output integer,
the chunked device stage, the refusals, score_records on the device against the host scorer on a real engine call, and the
structural time gate."""
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
    from tests import gpu_checks_scoring
    return gpu_checks_scoring


@pytest.mark.timeout(300, method='thread')
def test_spotting_match_equals_the_specification(C):
    """(ground truth, detections) of (0,0), (0,3), (3,0), (1,1), (63,65), (64,64), (130,257) alone and mixed into 40 images; n_thr 1, 2
    and 64; grids 64 and 1000; word-like rectangles with jitter, exact duplicates, detections of area 0, all ground truth don't-care;
    t_iou and t_dc at 1, 500 and 1000; report at the first threshold, the last and -1"""
    _assert_all(C.check_match_op())


@pytest.mark.timeout(300, method='thread')
def test_spotting_match_beyond_one_stride_of_the_free_set(C):
    """pages of (40, 1100), (1100, 40) and (300, 700): up to 18 words of the free set, so that a wave matches out of its second and later
    words; one call of the three at n_thr = 2 against match_pages_cpu and the naive matcher, each alone at n_thr = 64"""
    _assert_all(C.check_match_large())


@pytest.mark.timeout(120, method='thread')
def test_a_chunked_call_equals_the_unchunked_specification(C):
    _assert_all(C.check_chunked())


@pytest.mark.timeout(120, method='thread')
def test_spotting_match_refuses_with_error_codes(C):
    _assert_all(C.check_refusals())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.timeout(400, method='thread')
def test_score_records_on_the_device_equals_the_host_scorer(C, dtype):
    """spot_windows' image and weights, windows = [default, default, 2 x 2 grid]; ground truth = the suppress=0.5 call's own records (the
    plain call's hold every word of the doubled window twice, and so would their ground truth) with every third dropped, every fifth
    don't-care and every seventh with another text: counts, best and `gt` on every record, for the plain and the suppressed records;
    with suppress=0.5 the care detections fall and the matches do not"""
    _assert_all(C.check_engine_score(dtype))


@pytest.mark.timeout(120, method='thread')
def test_device_scoring_is_not_slower_than_the_host_matcher(C):
    _assert_all(C.check_timing())
