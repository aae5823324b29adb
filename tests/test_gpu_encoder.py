"""GPU tests of the Swin encoder kernels at every window count, padding, shift and head count: float64 per window / row on distinct base
images (edge windows and rows included), every image of every larger launch bit-identical to its source image, guard rows, determinism,
in place == out of place, the benchmark's own launches (tests/gpu_checks_encoder.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ATTN_IMPLS = ['mfma_expb_bf16', 'mfma_table_bf16', 'scalar_bf16', 'mfma_expb_f32', 'mfma_table_f32', 'scalar_f32', 'x3_split', 'x3_f32',
              'mfma_f32_split']


def _assert_all(records):
    bad = [r for r in records if not r['ok']]
    assert not bad, '\n'.join('%s: err=%.3e tol=%.1e %s' % (r['name'], r['err'], r['tol'], r['note']) for r in bad)


@pytest.fixture(scope='module')
def E():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from tests import gpu_checks_encoder
    return gpu_checks_encoder


@pytest.mark.parametrize('impl', ATTN_IMPLS)
def test_window_attn_geometry(E, impl):
    _assert_all(E.check_attn_geometry(impl))


@pytest.mark.parametrize('impl', ['mfma_expb_bf16', 'mfma_table_bf16', 'scalar_bf16', 'x3_split', 'mfma_expb_f32'])
def test_window_attn_heads(E, impl):
    _assert_all(E.check_attn_heads(impl))


@pytest.mark.parametrize('impl,nH', [('mfma_expb_bf16', 4), ('mfma_expb_bf16', 6), ('mfma_expb_bf16', 32), ('x3_split', 4), ('x3_split', 16),
                                     ('mfma_expb_f32', 4), ('mfma_table_bf16', 4)])
def test_window_attn_walks(E, impl, nH):
    _assert_all(E.check_attn_walks(impl, nH))


@pytest.mark.parametrize('stage', [0, 1, 2, 3])
def test_window_attn_stage_bf16(E, stage):
    _assert_all(E.check_attn_stage(stage, 'mfma_expb_bf16'))


@pytest.mark.parametrize('stage', [0, 1, 2, 3])
def test_window_attn_stage_x3(E, stage):
    _assert_all(E.check_attn_stage(stage, 'x3_split'))


@pytest.mark.parametrize('C', [128, 256])
def test_attn_block_geometry(E, C):
    _assert_all(E.check_block_geometry(C))


@pytest.mark.parametrize('C', [128, 256])
def test_attn_block_walks(E, C):
    _assert_all(E.check_block_walks(C))


@pytest.mark.parametrize('C', [128, 256])
def test_attn_block_stage(E, C):
    _assert_all(E.check_block_stage(C))


@pytest.mark.parametrize('stream', ['bf16', 'f32'])
@pytest.mark.parametrize('C', [128, 256, 512])
def test_mlp_fused(E, C, stream):
    _assert_all(E.check_mlp(C, stream))


def test_mlp_fused_stage(E):
    _assert_all(E.check_mlp_stage())


@pytest.mark.parametrize('path', ['mfma8', 'mfma6', 'tok_f32_128', 'tok_f32_96', 'tok_bf16_128', 'generic_f32_192', 'generic_bf16_192'])
def test_patch_embed(E, path):
    _assert_all(E.check_patch_embed(path))


def test_patch_embed_stage(E):
    _assert_all(E.check_patch_embed_stage())


@pytest.mark.parametrize('mode', ['f32_f32', 'f32_bf16', 'f32_split', 'bf16_bf16'])
def test_patch_merge(E, mode):
    _assert_all(E.check_patch_merge(mode))


def test_patch_merge_stage(E):
    _assert_all(E.check_patch_merge_stage())


def test_stage_layernorm(E):
    _assert_all(E.check_stage_layernorm())
