"""Ragged batches on the GPU: per-image key counts in the cross-attention kernels, and mixed-size engine calls decoded exactly as
each image alone (tests/gpu_checks_ragged.py)."""
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
    from tests import gpu_checks_ragged
    return gpu_checks_ragged


@pytest.mark.timeout(600, method='thread')
def test_cross_attn_key_len(C):
    """omp_dec_cross_attn_step with key_len: bf16 / fp32 / split-plane slabs, n_split 1-16, q_tiles 1/2/4, every ring variant, NT
    on and off, against fp64 attention over each image's own keys; NaN beyond key_len is never used; key_len = [M] * B == NULL bit
    for bit."""
    _assert_all(C.check_cross_attn_key_len())


@pytest.mark.parametrize('graph', [False, True])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.timeout(400, method='thread')
def test_ragged_equals_alone(C, dtype, graph):
    """three sizes in one ragged call == one call per image, then two more ragged calls with other length mixes on the same model
    (graph=True: the second call replays the graphs captured by the first)"""
    _assert_all(C.check_ragged_equals_alone(dtype, graph))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.timeout(400, method='thread')
def test_ragged_against_reference_alone(C, dtype):
    """spot_alone: the reference on every image alone, unpadded; the engine on all of them in ONE ragged call"""
    _assert_all(C.check_ragged_golden(dtype))


@pytest.mark.parametrize('dtype', ['bf16x3', 'bf16'])
@pytest.mark.timeout(400, method='thread')
def test_ragged_on_the_chains(C, dtype):
    """the same ragged call with every phase on the row-owner chains (the rows-fused step's cross-attention)"""
    _assert_all(C.check_ragged_golden(dtype, chains=True))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.timeout(400, method='thread')
def test_ragged_kie(C, dtype):
    _assert_all(C.check_ragged_kie(dtype))
