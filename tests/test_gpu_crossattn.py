"""GPU tests of the decoder cross-attention kernels of csrc/decoder.hip (dec_cross_attn_kernel, dec_cross_attn_q4_kernel,
dec_cross_merge_kernel through ops.dec_cross_attn_step; the split-pair output rows through omp_debug_cross_attn_pairs) with planted keys at
every key count where a key block, a wave slice, a workgroup split, the register ring or the LDS ring changes shape: peaked and uniform key
walks with exact outputs and loud dead keys, score ramps, plane ramps, random bases against float64, several groups per image, NaN guards
around everything a launch may not touch, refusals (tests/gpu_checks_crossattn.py; tests/test_crossattn_reference.py proves the plants)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# kind, q_tiles, rings of omp_debug_cross_q4 (q_tiles 4 only; 0 = the register-streaming kernel)
CASES = [(kind, qt, None) for kind in ('bf16', 'fp32', 'split') for qt in (1, 2)] + \
        [(kind, 4, rings) for kind in ('bf16', 'fp32') for rings in ((1,), (2, 4), (5, 6), (0,))] + \
        [('split', 4, rings) for rings in ((1,), (4, 5), (6, 0))]
SPLIT_CASES = [(qt, rings) for kind, qt, rings in CASES if kind == 'split']
IDS = lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def _assert_all(records):
    bad = [r for r in records if not r['ok']]
    assert not bad, '\n'.join('%s: err=%.3e tol=%.1e %s' % (r['name'], r['err'], r['tol'], r['note']) for r in bad[:40]) + '\n(%d records failed)' % len(bad)


@pytest.fixture(scope='module')
def C():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from tests import gpu_checks_crossattn
    return gpu_checks_crossattn


@pytest.mark.parametrize('kind,qt,rings', CASES, ids=IDS)
def test_key_walks_every_length(C, kind, qt, rings):
    _assert_all(C.check_walks(kind, qt, rings))


@pytest.mark.parametrize('kind,qt,rings', CASES, ids=IDS)
def test_key_walks_ragged_m_and_2081_keys(C, kind, qt, rings):
    _assert_all(C.check_walks_ragged_m(kind, qt, rings))


@pytest.mark.parametrize('kind,qt,rings', CASES, ids=IDS)
def test_score_ramps(C, kind, qt, rings):
    _assert_all(C.check_ramps(kind, qt, rings))


@pytest.mark.parametrize('qt,rings', SPLIT_CASES, ids=IDS)
def test_plane_ramps(C, qt, rings):
    _assert_all(C.check_plane_ramps(qt, rings))


@pytest.mark.parametrize('kind,qt,rings', CASES, ids=IDS)
def test_random_vs_float64(C, kind, qt, rings):
    """randn x 1.5 against float64 at the project's gates.  The split cases found the two-plane truncation of q and P (7.7e-5 against the gate
    of 5e-5 with three products per block; 6.1e-6 with the five the kernels form now), see tests/gpu_checks_crossattn.py."""
    _assert_all(C.check_random(kind, qt, rings))


@pytest.mark.parametrize('kind,qt,rings', CASES, ids=IDS)
def test_groups_per_image(C, kind, qt, rings):
    _assert_all(C.check_groups(kind, qt, rings))


@pytest.mark.parametrize('qt,rings', SPLIT_CASES, ids=IDS)
def test_split_pair_rows(C, qt, rings):
    _assert_all(C.check_pairs(qt, rings))


def test_refusals(C):
    _assert_all(C.check_refusals())
