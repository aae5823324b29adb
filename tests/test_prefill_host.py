"""Batched prompt prefill, host side: the prefill tiles table (model/transformer.py::Decoder.make_prefill_tiles) against a brute-force
statement of its rule, the eligibility the plan binding applies, and the strict OMP355_PREFILL knob.  No GPU."""
import random

import pytest
import torch

from advancedliteratemachinery_amd.model.transformer import Decoder
from advancedliteratemachinery_amd.utils.env import env_flag

COUNTS = ([1] * 64, [1] * 70, [3, 1, 20, 17, 9, 16, 2], [64, 33, 40, 1, 50, 64], [16], [17], [32], [33], [5, 0, 7], [1])


def _cases():
    rng = random.Random(7)
    out = [(c, L) for c in COUNTS for L in (1, 2, 6, 9)]
    for _ in range(40):
        out.append(([rng.randint(1, 64) for _ in range(rng.randint(1, 9))], rng.randint(1, 12)))
    return out


@pytest.mark.parametrize('counts,L', _cases())
def test_prefill_tiles_rule(counts, L):
    groups, qt = Decoder.make_tiles(counts)
    cap = 16 * qt
    tiles = Decoder.make_prefill_tiles(groups, qt, L)
    # prefill row r * L + j is plan row r at position j: the image of every prefill row, by brute force
    image_of = [img for img, n in enumerate(counts) for _ in range(n * L)]
    seen = [0] * len(image_of)
    for row0, nrows, img in tiles:
        assert 1 <= nrows <= cap                                   # no group exceeds 16 * q_tiles rows
        for r in range(row0, row0 + nrows):
            seen[r] += 1
            assert image_of[r] == img                              # groups never span images
    assert seen == [1] * len(image_of)                             # every prefill row is in exactly one group
    assert len(tiles) == sum((n * L + cap - 1) // cap for n in counts)   # ceil(R_img * L / (16 * q_tiles)) slab passes per image
    if L > 1 and max(counts) <= cap:
        assert len(tiles) <= L * len(groups)                       # never more passes than the stepwise prefill's


def test_prefill_tiles_follow_the_step_tiles():
    """L = 1 is the step's own table (one position: the rows are the plan's rows)"""
    for counts in COUNTS:
        groups, qt = Decoder.make_tiles(counts)
        assert Decoder.make_prefill_tiles(groups, qt, 1) == groups


class _Ph(object):
    def __init__(self, kind, R):
        self.kind, self.R = kind, R


def _dec(dtype=torch.bfloat16, pre_norm=True, kv_split=False, prefill=True):
    d = Decoder.__new__(Decoder)
    d.dtype, d.kv_split, d.prefill = dtype, kv_split, prefill
    d.args = type('A', (), {'tfm_pre_norm': pre_norm})()
    return d


def test_prefill_switch_eligibility():
    ok = _dec()
    assert ok._prefill_ok(_Ph('pt', 160), 7, False, False)
    assert ok._prefill_ok(_Ph('pt', 64), 3, False, False)
    assert not ok._prefill_ok(_Ph('pt', 63), 7, False, False)      # the fused few-row step
    assert not ok._prefill_ok(_Ph('pt', 160), 2, False, False)     # one prompt position: nothing to batch
    assert not ok._prefill_ok(_Ph('pt', 1000), 7, False, False)    # more prefill rows than the tile-kernel family is pinned for
    assert not ok._prefill_ok(_Ph('poly', 160), 3, False, False)   # point phases only
    assert not ok._prefill_ok(_Ph('pt', 160), 7, True, False)      # rows_fused
    assert not ok._prefill_ok(_Ph('pt', 160), 7, False, True)      # bf16x3
    assert not _dec(dtype=torch.float32)._prefill_ok(_Ph('pt', 160), 7, False, False)
    assert not _dec(pre_norm=False)._prefill_ok(_Ph('pt', 160), 7, False, False)
    assert not _dec(prefill=False)._prefill_ok(_Ph('pt', 160), 7, False, False)


def test_prefill_knob_is_strict(monkeypatch):
    monkeypatch.setenv('OMP355_PREFILL', '0')
    assert env_flag('OMP355_PREFILL', True) is False
    monkeypatch.setenv('OMP355_PREFILL', 'off')
    with pytest.raises(ValueError):
        env_flag('OMP355_PREFILL', True)
