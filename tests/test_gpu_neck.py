"""GPU tests of the kernels between the encoder and the decoders at their edges -- the FPN fuse, the split-bf16 producer with row pitches,
the row-owner K / V^T memory projection, the cached memory slabs' padded tail and the device pre-processing -- against float64
restatements, element by element (tests/gpu_checks_neck.py)."""
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
    from tests import gpu_checks_neck
    return gpu_checks_neck


@pytest.mark.parametrize('name', ['check_fpn_geometry_fp32', 'check_fpn_geometry_bf16', 'check_split_bf16_pitch', 'check_kv_rows_edges',
                                  'check_memory_slab_tail_fp32', 'check_memory_slab_tail_bf16', 'check_memory_slab_tail_bf16x3',
                                  'check_preprocess_edges'])
def test_neck(C, name):
    _assert_all(getattr(C, name)())
