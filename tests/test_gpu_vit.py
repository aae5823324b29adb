"""GPU tests of the MGP-STR recogniser kernels (csrc/vit.hip) at every token count and key slot, and of the row statistics of the head
products: exact planted inputs (key-slot walk, dead keys, ties across the softmax chunks, one-hot pooling, planted winners), float64 per
row on random bases, both attention entry points bit-identical, guard rows and gap columns, refusals (tests/gpu_checks_vit.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _assert_all(records):
    bad = [r for r in records if not r['ok']]
    assert not bad, '\n'.join('%s: err=%.3e tol=%.1e %s' % (r['name'], r['err'], r['tol'], r['note']) for r in bad)


@pytest.fixture(scope='module')
def V():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from tests import gpu_checks_vit
    return gpu_checks_vit


@pytest.mark.parametrize('B,nH', [(1, 12), (3, 12)])
def test_attn_key_slot_walk(V, B, nH):
    _assert_all(V.check_attn_walk(B, nH))


def test_attn_key_slot_walk_three_heads(V):
    _assert_all(V.check_attn_walk(3, 3, tokens=(17, 257)))


@pytest.mark.parametrize('lo,hi', [(1, 96), (97, 192), (193, 287)])
def test_attn_dead_keys_every_token_count(V, lo, hi):
    _assert_all(V.check_attn_dead(1, 3, range(lo, hi + 1)))


def test_attn_dead_keys_all_heads(V):
    _assert_all(V.check_attn_dead(3, 12, [T for T in V.TOKENS if T < 288]))


def test_attn_ties_across_chunks(V):
    _assert_all(V.check_attn_ties())


@pytest.mark.parametrize('T', [17, 97, 257, 288])
def test_attn_random_vs_float64(V, T):
    _assert_all(V.check_attn_random(T))


def test_attn_refusals(V):
    _assert_all(V.check_attn_refusals())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('E', [768, 192, 100])
def test_patch_embed(V, E, dtype):
    _assert_all(V.check_patch_embed(E, dtype))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('axis', ['T', 'S', 'C', 'corner'])
def test_a3_pool(V, axis, dtype):
    _assert_all(V.check_a3_pool(axis, dtype))


def test_a3_pool_one_hot(V):
    _assert_all(V.check_a3_onehot())


def test_a3_pool_refusals(V):
    _assert_all(V.check_a3_refusals())


@pytest.mark.parametrize('kind', ['bf16', 'fp32', 'bf16x3'])
def test_row_statistics(V, kind):
    _assert_all(V.check_row_stats(kind))
