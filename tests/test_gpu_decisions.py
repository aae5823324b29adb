"""GPU tests of the kernels that turn numbers into decisions (sampling, arg-max, packing, masks, embedding) at their edges, against the
oracle's filter + topk and fp64 restatements (tests/gpu_checks_decide.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _assert_all(records):
    bad = [r for r in records if not r['ok']]
    assert not bad, '\n'.join('%s: err=%.3e tol=%.1e %s' % (r['name'], r['err'], r['tol'], r['note']) for r in bad)


@pytest.fixture(scope='module')
def C():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from tests import gpu_checks_decide
    return gpu_checks_decide


@pytest.mark.parametrize('name', ['check_sample_edges', 'check_row_argmax_prob_edges', 'check_pack_spotting', 'check_dec_embed_ln',
                                  'check_mask_nearest', 'check_posembed_edges'])
def test_decision(C, name):
    _assert_all(getattr(C, name)())
