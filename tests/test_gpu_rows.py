"""GPU tests of the row-owner chains at every row count, tile and grid the engine launches: float64 on 256 distinct base rows (edge rows
included), every row of every larger launch bit-identical to its source row, guard rows, determinism, XCD masks, the memory projection in
full, the mid chain with a position per row (pos_mod) against the one-position launches (tests/gpu_checks_rows.py)."""
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
    from tests import gpu_checks_rows
    return gpu_checks_rows


def test_rows_tile_rule(C):
    _assert_all(C.check_rows_tile_rule())


@pytest.mark.parametrize('kind', ['mid', 'ffn_qkv', 'ffn_head', 'embed'])
def test_dec_rows_bf16(C, kind):
    _assert_all(C.check_dec_chain(kind, x3=False))


@pytest.mark.parametrize('kind', ['mid', 'ffn_qkv', 'ffn_head', 'embed'])
def test_dec_rows_x3(C, kind):
    _assert_all(C.check_dec_chain(kind, x3=True))


def test_dec_rows_xcd_branches(C):
    _assert_all(C.check_dec_rows_xcd_branches())


@pytest.mark.parametrize('x3', [False, True], ids=['bf16', 'x3'])
@pytest.mark.parametrize('mode', [0, 1, '1q'], ids=['mode0', 'mode1', 'mode1_qkv'])
def test_swin_rows(C, mode, x3):
    _assert_all(C.check_swin_chain(mode, x3=x3))


def test_kv_rows_full(C):
    _assert_all(C.check_kv_rows_full())


def test_kv_rows_batch(C):
    _assert_all(C.check_kv_rows_batch())


@pytest.mark.parametrize('pos_mod', [1, 2, 6, 7, 1024])
def test_dec_rows_mid_pos_mod(C, pos_mod):
    assert pos_mod in C.MID_POS_MODS and C.P == 1024
    _assert_all(C.check_dec_mid_pos_mod(pos_mod))


def test_dec_rows_mid_pos_mod_refusals(C):
    _assert_all(C.check_dec_mid_pos_mod_refusals())
