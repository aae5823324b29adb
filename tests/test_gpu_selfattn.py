"""GPU tests of the causal self-attention step kernels of csrc/decoder.hip (one wave per (row, head), one wave per row, the fused LN1 +
projection + attention kernel of the point decoder through omp_debug_fused_self_attn) at every cache position where their loops change
shape: planted uniform and peaked key walks with exact outputs, score ramps, random bases and the fused projection against float64, NaN
guards around everything a launch may not touch, refusals (tests/gpu_checks_selfattn.py; tests/test_selfattn_reference.py proves the plants)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

VARIANTS = [('head', 'fp32'), ('head', 'bf16'), ('row', 'fp32'), ('row', 'bf16'), ('fused', 'bf16'), ('fused_embed', 'bf16')]


def _assert_all(records):
    bad = [r for r in records if not r['ok']]
    assert not bad, '\n'.join('%s: err=%.3e tol=%.1e %s' % (r['name'], r['err'], r['tol'], r['note']) for r in bad)


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from tests import gpu_checks_selfattn
    return gpu_checks_selfattn


@pytest.mark.parametrize('lo,hi', [(0, 129), (191, 321), (383, 449)])
@pytest.mark.parametrize('kern,dtype', VARIANTS)
def test_key_walks_every_position(S, kern, dtype, lo, hi):
    _assert_all(S.check_walks(kern, dtype, [p for p in S.POSITIONS if lo <= p <= hi]))


@pytest.mark.parametrize('kern', ['fused', 'fused_embed'])
def test_key_walks_position_1023(S, kern):
    _assert_all(S.check_walk_long(kern))


@pytest.mark.parametrize('kern,dtype', VARIANTS)
def test_score_ramps(S, kern, dtype):
    _assert_all(S.check_ramps(kern, dtype))


@pytest.mark.parametrize('kern,dtype', VARIANTS)
def test_random_vs_float64(S, kern, dtype):
    _assert_all(S.check_random(kern, dtype))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_random_six_three_one_heads(S, dtype):
    _assert_all(S.check_random_heads(dtype))


@pytest.mark.parametrize('embed', [False, True])
def test_fused_projection(S, embed):
    _assert_all(S.check_fused_projection(embed))


def test_refusals(S):
    _assert_all(S.check_refusals())
