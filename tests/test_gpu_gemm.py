"""GPU tests of omp_gemm_bias_act (csrc/gemm.hip, gemm256.hip, gemm4w.hip, gemm4wr.hip, gemm4wp.hip) at every ragged edge, pitch and few-row count: sentinel-guarded destinations,
NaN-guarded operands, every K-tile count around each ring depth, every epilogue on vector and scalar pitches, bit equality of the 256x256
kernels with the 128x128 kernel, every M from 1 to 64 through gemm_rows and gemm_small, the fused LayerNorm prologue with planted rows and
two eps values, in place against out of place, clean refusals; the bias table's per-row form (bias_row_mod / bias_row_off) through selectors
4, 5 and 6 against float64 and, bit for bit, against the one-row form of each table row (tests/gpu_checks_gemm.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE_SELS = [(5, 'bf16'), (5, 'fp32'), (6, 'bf16'), (6, 'fp32'), (9, 'bf16'), (10, 'bf16'), (16, 'bf16'), (20, 'bf16')]
FEW = [(3, 'bf16'), (3, 'fp32'), (4, 'bf16'), (4, 'fp32')]


def _assert_all(records):
    assert records
    bad = [r for r in records if not r['ok']]
    assert not bad, '\n'.join('%s: err=%.3e tol=%.1e %s' % (r['name'], r['err'], r['tol'], r['note']) for r in bad)


@pytest.fixture(scope='module')
def G():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from tests import gpu_checks_gemm
    return gpu_checks_gemm


@pytest.mark.parametrize('sel,dtn', TILE_SELS)
def test_tile_m_n_edges(G, sel, dtn):
    _assert_all(G.check_tile_mn(sel, dtn))


@pytest.mark.parametrize('sel,dtn', TILE_SELS)
def test_tile_k_against_ring_depth(G, sel, dtn):
    _assert_all(G.check_tile_k(sel, dtn))


@pytest.mark.parametrize('dtn', ['bf16', 'fp32'])
def test_tile_64_four_stage_ring(G, dtn):
    _assert_all(G.check_ring4(dtn))


@pytest.mark.parametrize('sel,dtn', TILE_SELS)
def test_tile_epilogues(G, sel, dtn):
    _assert_all(G.check_tile_epilogues(sel, dtn))


@pytest.mark.parametrize('sel,dtn', TILE_SELS)
def test_tile_pitch_classes(G, sel, dtn):
    _assert_all(G.check_tile_pitches(sel, dtn))


@pytest.mark.parametrize('sel', [9, 10, 16, 20])
def test_tile_refusals(G, sel):
    _assert_all(G.check_tile_refusals(sel))


@pytest.mark.parametrize('sel,dtn', FEW + [(6, 'bf16'), (6, 'fp32')])
def test_in_place_equals_out_of_place(G, sel, dtn):
    _assert_all(G.check_inplace(sel, dtn))


@pytest.mark.parametrize('sel,dtn,K', [(s, d, K) for (s, d) in FEW for K in (64, 128, 512, 1152, 2048) if not (d == 'bf16' and K == 64)])
def test_few_rows_every_m(G, sel, dtn, K):
    assert K in G.FEW_K[dtn]
    _assert_all(G.check_few_rows(sel, dtn, K))


@pytest.mark.parametrize('sel,dtn', FEW)
def test_few_rows_epilogues(G, sel, dtn):
    _assert_all(G.check_few_epilogues(sel, dtn))


@pytest.mark.parametrize('dtn,K', [('bf16', 128), ('bf16', 384), ('bf16', 512), ('bf16', 1024),
                                   ('fp32', 64), ('fp32', 128), ('fp32', 384), ('fp32', 512), ('fp32', 1024)])
def test_layernorm_prologue(G, dtn, K):
    assert K in G.LN_K[dtn]
    _assert_all(G.check_ln(dtn, K))


# the bias table's per-row form (bias_row_mod / bias_row_off): float64 and bit equality with the one-row form
@pytest.mark.parametrize('ln', [False, True], ids=['plain', 'ln'])
@pytest.mark.parametrize('dtn,out', [('bf16', 'bf16'), ('bf16', 'fp32'), ('fp32', 'fp32')])
def test_table_bias_small(G, dtn, out, ln):
    _assert_all(G.check_table_small(dtn, out, ln))


@pytest.mark.parametrize('sel,N', [(6, 64), (6, 72), (6, 67), (5, 128), (5, 136), (5, 131)])
def test_table_bias_tile(G, sel, N):
    assert N in G.TABLE_TILE_SHAPES[sel][1]
    _assert_all(G.check_table_tile(sel, N))


def test_table_bias_four_stage_ring(G):
    _assert_all(G.check_table_ring4())


def test_table_bias_refusals(G):
    _assert_all(G.check_table_refusals())
