"""Window prompts on the GPU (tests/gpu_checks_windows.py): omp_window_points against its numpy specification, windowed engine calls
against the reference run once per window, against every window alone, against today's predict, ragged, graphed and two-stage."""
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
    from tests import gpu_checks_windows
    return gpu_checks_windows


@pytest.mark.timeout(300, method='thread')
def test_window_points_equals_the_specification(C):
    """1 .. 4096 rows; all / none / some rows finished; empty rows; clip on and off; a cap below the total: every output integer"""
    _assert_all(C.check_window_points_op())


@pytest.mark.parametrize('variant', ['forced', 'eos'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.timeout(400, method='thread')
def test_fixture_windows_in_one_call(C, dtype, variant):
    """spot_windows: the reference's forward once per prompt; the engine on all eight prompts in ONE call: ids identical, probabilities
    within 1e-3 (the fp32 gates of the end-to-end tests)"""
    _assert_all(C.check_fixture(dtype, variant))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.timeout(400, method='thread')
def test_windows_equal_each_window_alone(C, dtype):
    """4, 9 and 3 (with character windows) windows in one call == each window through forward(samples, seqs) on the same engine"""
    _assert_all(C.check_windows_equal_alone(dtype))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.timeout(300, method='thread')
def test_no_windows_and_the_default_window_are_todays_predict(C, dtype):
    _assert_all(C.check_default_equals_today(dtype))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.timeout(400, method='thread')
def test_ragged_windows_equal_alone(C, dtype):
    _assert_all(C.check_ragged_windows(dtype))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.timeout(300, method='thread')
def test_windows_graph_replay_equals_eager(C, dtype):
    _assert_all(C.check_graph_windows(dtype))


@pytest.mark.timeout(300, method='thread')
def test_two_stage_with_a_grid(C):
    """spot_and_recognize(grid=(2, 2)): records with window / window_bins and the mgp_* fields, equal to recognize_crops on the same crops"""
    _assert_all(C.check_two_stage_windows())
