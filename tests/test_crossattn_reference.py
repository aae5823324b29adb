"""The float64 restatement of the decoder cross-attention checks (tests/gpu_checks_crossattn.py ref_cross) against plain torch softmax
attention, the slab builders against their inverse, the planted inputs against the outputs stated for them, the teeth of the walks and ramps
-- a restatement that drops the target, reads K one key off, reads V^T without the slot permutation, swaps two slots, reuses a stale ring
stage, counts one dead key, ignores a lo plane or drops a split cross term must miss the gates by a wide margin -- and the coverage of
LENGTHS: every built configuration gets an empty slice and slices of 1, depth - 1, depth, depth + 1 and 2 depth + 1 blocks.  One mutant
has no teeth to find: a merge that gives a -inf partial the weight 1 adds l = 0 and o = 0, the sum is bit-identical
(test_restatement_is_plain_softmax_attention shows it); what such a slice can get wrong is not writing its zeros, which the NaN-filled
partial buffer of the GPU checks catches.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

from tests import gpu_checks_crossattn as C
from tests.gpu_checks_ragged import RINGS, TOL, _slot_of_key

TOL64 = 1e-12
WIDE = 0.2           # 51 times the bf16 walk gate (2^-8), 2e5 times the fp32 one
NH, HD, D = C.NH, C.HD, C.D


def _values(p):
    """the float64 values of a plant's slabs in natural order, its float64 q and live keys"""
    K, Vt = C.slabs(p.lay.kind, p.Kn, p.Vn)
    Kv, Vv = C.natural(p.lay.kind, K, Vt)
    return p.q, Kv, Vv, p.lay.counts, p.lay.live


def _per_image(p, got):
    """max head_rel against the stated output per image -> [B]"""
    e = C.head_rel(got, p.want, NH).amax(-1)
    return torch.stack([e[p.lay.row_img == b].max() for b in range(p.lay.B)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# restatement and slab builders
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mask', C.MASKS)
@pytest.mark.parametrize('key_len', [True, False])
def test_restatement_is_plain_softmax_attention(mask, key_len):
    lay = C.Layout('fp32', [5, 40, 33, 1], [3, 17, 1, 2], 48, 2, mask, key_len)
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 1.5
    q, Kv, Vv = r(lay.R, D), r(lay.B, NH, lay.Mpad, HD), r(lay.B, NH, lay.Mpad, HD)
    Kv[~lay.live[:, None, :, None].expand_as(Kv)] = float('nan')              # the restatement reads no dead key
    Vv[~lay.live[:, None, :, None].expand_as(Vv)] = float('nan')
    got = C.ref_cross(q, Kv, Vv, lay.counts, lay.live)
    for b, n in enumerate(lay.counts):
        keys = torch.nonzero(lay.live[b])[:, 0]
        if lay.mask is None:
            assert keys.tolist() == list(range(lay.lens[b]))
        else:
            assert keys.tolist() == [j for j in range(lay.lens[b]) if not lay.mask[b, j]]
        qh = q[lay.row0[b]:lay.row0[b] + n].reshape(n, NH, HD).transpose(0, 1)
        plain = (F.softmax(qh @ Kv[b][:, keys].transpose(-1, -2) / 8.0, dim=-1) @ Vv[b][:, keys]).transpose(0, 1).reshape(n, D)
        assert (got[lay.row0[b]:lay.row0[b] + n] - plain).abs().max().item() < TOL64
    # the identity maps and unit weights of the mutants change nothing
    idx = torch.arange(lay.Mpad).expand(lay.B, lay.Mpad)
    assert torch.equal(C.ref_cross(q, Kv, Vv, lay.counts, lay.live, ksrc=idx, vsrc=idx, weight=torch.ones(lay.R, NH, lay.Mpad, dtype=torch.float64)), got)
    # the same sum formed slice by slice and merged, as a launch with n_split S forms it
    for cfg, S in ((C.config('fp32', 2, 1, 1), 1), (C.config('fp32', 2, 1, 1), 4), (C.config('fp32', 4, 6, 1), 2)):
        merged = C.ref_cross_merged(q, Kv, Vv, lay.counts, lay.live, lay.lens, S, cfg)
        assert (merged - got).abs().max().item() < TOL64
        assert any(n == 0 for L in lay.lens for n in C.slice_blocks(L, S, cfg)) or S == 1 or not key_len        # there are -inf partials
        # a slice without a live key is (m, l, o) = (-inf, 0, 0): whatever weight the merge gives it, the sum is the same.  What guards the
        # merge is that such a slice WRITES those zeros: the GPU checks fill `partial` with NaN
        assert torch.equal(C.ref_cross_merged(q, Kv, Vv, lay.counts, lay.live, lay.lens, S, cfg, inf_weight=1.0), merged)


@pytest.mark.parametrize('kind', C.KINDS)
def test_slab_builders_invert(kind):
    g = torch.Generator().manual_seed(5)
    B, M = 2, 96
    Kn = C.to_kind(kind, torch.randn(B, NH, M, HD, generator=g) * 1.5)
    Vn = C.to_kind(kind, torch.randn(B, NH, M, HD, generator=g) * 1.5)
    K, Vt = C.slabs(kind, Kn, Vn)
    Kv, Vv = C.natural(kind, K, Vt)
    assert torch.equal(Kv, Kn.double()) and torch.equal(Vv, Vn.double())
    KB = C.key_block(kind)
    assert torch.equal(C._unblock(C._vblocks(Vn, KB, kind != 'fp32'), kind != 'fp32'), Vn)
    slot = _slot_of_key() if kind != 'fp32' else torch.arange(16)
    assert sorted(slot.tolist()) == list(range(KB))
    hi = lambda x: x.to(torch.bfloat16)
    for key in (0, 4, 17, 37, 95):
        blk, kl = key // KB, key % KB
        if kind == 'split':
            # plane order: hi then lo, in K and in V^T
            assert K.shape == (B, NH, M // 32, 2, 32, HD) and Vt.shape == (B, NH, M // 32, 2, HD, 32)
            assert torch.equal(K[:, :, blk, 0, kl], hi(Kn[:, :, key])) and torch.equal(K[:, :, blk, 1, kl], hi(Kn[:, :, key] - hi(Kn[:, :, key]).float()))
            assert torch.equal(Vt[:, :, blk, 0, :, slot[kl]], hi(Vn[:, :, key])) and torch.equal(Vt[:, :, blk, 1, :, slot[kl]], hi(Vn[:, :, key] - hi(Vn[:, :, key]).float()))
        else:
            assert torch.equal(K[:, :, key], Kn[:, :, key].to(K.dtype)) and torch.equal(Vt[:, :, blk, :, slot[kl]], Vn[:, :, key].to(Vt.dtype))
    if kind == 'split':
        (kh, kl_), (vh, vl) = C.natural(kind, K, Vt, planes=True)
        assert torch.equal(kh + kl_, Kv) and torch.equal(vh + vl, Vv) and bool((kl_ != 0).any()) and bool((vl != 0).any())


def test_hadamard_codes():
    H = C.hadamard()
    assert torch.equal(H @ H.T, 64.0 * torch.eye(64, dtype=torch.float64)) and bool((H[:, 0] == 1).all()) and bool((H.abs() == 1).all())


def test_gates_are_the_stated_ones():
    assert C.walk_gate('bf16') == 2.0 ** -8 and C.walk_gate('fp32') == 1e-6 and C.walk_gate('split') == 1e-6
    assert TOL == {'bf16': 2e-2, 'fp32': 2e-5, 'split': 5e-5}
    assert C.ROWS == {1: (1, 2, 15, 16), 2: (1, 17, 31, 32), 4: (1, 16, 17, 33, 47, 48, 49, 63, 64)}
    assert C.S_ALL == (1, 2, 4, 8, 16) and C.RAGGED_M == (77, 129, 640) and C.LONG_M == 2081 and C.M_SLAB == 640


# ---------------------------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_lengths_are_the_listed_ones():
    L = set(C.LENGTHS)
    assert {1, 2, 639, 640} <= L and max(L) == 640
    for m in (16, 32, 48, 64, 96, 128, 192, 256, 320, 384, 512):
        assert {m - 1, m, m + 1} <= L


def _configs():
    for kind in C.KINDS:
        for qt in (1, 2, 4):
            for ring, nt in C.variants(kind, qt):
                yield kind, qt, ring, nt, C.config(kind, qt, ring, nt)


def test_configurations_are_launch_cross():
    """the table of csrc/decoder.hip launch_cross: kind, q_tiles, ring -> KB, slices per n_split, PD or NS / CH"""
    assert RINGS == {'bf16': (1, 2, 4, 5, 6, 0), 'fp32': (1, 2, 4, 5, 6, 0), 'split': (1, 4, 5, 6, 0)}
    ring = {(k, r, nt): (c['NS'], c['CH']) for k, qt, r, nt, c in _configs() if c['ring']}
    assert {ring['split', r, 1] for r in (1, 4, 5, 6)} == {(2, 1), (8, 2), (4, 1), (3, 1)}
    assert [ring['fp32', r, 1] for r in (1, 2, 4, 5, 6)] == [(8, 2), (8, 1), (8, 2), (6, 2), (4, 1)]
    assert [ring['bf16', r, 1] for r in (1, 2, 4, 5, 6)] == [(6, 2), (8, 1), (8, 2), (8, 2), (4, 1)] and ring['bf16', 1, 0] == (8, 2)
    assert {ns for ns, _ in ring.values()} == {2, 3, 4, 6, 8}
    for kind, qt, r, nt, c in _configs():
        assert c['KB'] == (16 if kind == 'fp32' else 32) and c['mult'] == (1 if c['ring'] else 4) and c['ring'] == (qt == 4 and r != 0)
    pd = {(k, qt): c['PD'] for k, qt, r, nt, c in _configs() if not c['ring']}
    assert pd == {('fp32', 1): 4, ('fp32', 2): 2, ('fp32', 4): 2, ('bf16', 1): 4, ('bf16', 2): 2, ('bf16', 4): 2, ('split', 1): 2, ('split', 2): 2, ('split', 4): 1}


def test_lengths_reach_every_loop_edge_of_every_configuration():
    for kind, qt, ring, nt, cfg in _configs():
        CH, depth = cfg['CH'], cfg['depth']
        blocks = {n for L in C.LENGTHS for S in C.S_ALL for n in C.slice_blocks(L, S, cfg)}
        units = {(n + CH - 1) // CH for n in blocks}                       # blocks in flight (PD), or chunks against the ring's chunk slots
        reach = max((n + CH - 1) // CH for n in C.slice_blocks(C.M_SLAB, 1, cfg))
        need = {0, 1} | {u for u in (depth - 1, depth, depth + 1, 2 * depth + 1) if u <= reach}
        assert need <= units, (kind, qt, ring, nt, sorted(need - units))
        if CH == 2:
            assert any(n % 2 == 1 and n > 2 for n in blocks) and 1 in blocks, (kind, qt, ring, nt)      # a ragged last chunk
        # a split that is empty while its neighbour holds one block
        assert any(a == 1 and b == 0 for L in C.LENGTHS for S in C.S_ALL[1:] for a, b in zip(C.slice_blocks(L, S, cfg), C.slice_blocks(L, S, cfg)[1:]))
        long_blocks = C.slice_blocks(C.LONG_M, 1, cfg)[0]
        if cfg['ring'] and cfg['NS'] == 8:
            assert long_blocks >= 8 * 8                                   # eight wraps of the eight-stage ring (two at the least)
        assert long_blocks // CH >= 2 * depth + 1
    # every row count of the issue, and with them inactive waves (nrows <= 48) and clamped queries of the ring kernel
    for qt, rows in C.ROWS.items():
        assert max(rows) == 16 * qt and 1 in rows
        assert set(rows) <= {c for p in range(len(rows)) for c in C.rows_of_phase(qt, p, len(C.LENGTHS))}


@pytest.mark.parametrize('mask', C.MASKS)
@pytest.mark.parametrize('qt', [1, 2, 4])
def test_sweep_aims_at_every_live_key(qt, mask):
    phases = C.sweep('bf16', qt, mask)
    lay0 = phases[0][0]
    seen = torch.zeros(lay0.B, lay0.Mpad, dtype=torch.bool)
    for lay, bases in phases:
        tg = lay.targets(bases)
        assert bool(lay.live[lay.pair_img[:, None].expand_as(tg), tg].all())                 # targets are live keys
        seen[lay.pair_img[:, None].expand_as(tg), tg] = True
        first = torch.stack([torch.nonzero(lay.live[b])[0, 0] for b in range(lay.B)])
        last = torch.stack([torch.nonzero(lay.live[b])[-1, 0] for b in range(lay.B)])
        for b in range(lay.B):
            own = tg[lay.pair0[b]:lay.pair0[b] + lay.ncode[b]]
            assert first[b] in own and last[b] in own
            if lay.ncode[b] > 1 and int(lay.n_live[b]) >= 16:
                assert len(set(own[1, :NH - 1].tolist())) == NH - 1                     # the heads aim at different keys
    assert torch.equal(seen, lay0.live)
    if mask != 'none':
        # whole blocks, wave slices and trailing splits are dead / m stays -inf through the first blocks
        b = C.LENGTHS.index(640)
        dead_blocks = [k for k in range(20) if not lay0.live[b, 32 * k:32 * k + 32].any()]
        assert dead_blocks and (mask == 'pad2d' and dead_blocks[-1] == 19 and len(dead_blocks) >= 5 or mask == 'lead' and dead_blocks[:2] == [0, 1])
        assert bool((lay0.n_live > 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# planted inputs and stated outputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _exact(kind, x):
    ok = torch.isfinite(x)
    return torch.equal(C.to_kind(kind, x)[ok], x.float()[ok])


@pytest.mark.parametrize('mask', C.MASKS)
@pytest.mark.parametrize('kind,qt', [('bf16', 4), ('fp32', 1), ('split', 2)])
def test_walks_give_the_stated_outputs(kind, qt, mask):
    phases = C.sweep(kind, qt, mask)
    for pi in sorted({len(phases) // 2, len(phases) - 1}):
        lay, bases = phases[pi]
        for p in (C.plant_peaked(lay, bases), C.plant_uniform(lay, bases, pi)):
            assert _exact(kind, p.Kn) and _exact(kind, p.Vn) and _exact('bf16', p.q)
            assert _exact('bf16', p.Kn) and (kind == 'split' or _exact('bf16', p.Vn))
            if kind == 'split':
                live = lay.live[:, None, :, None].expand_as(p.Vn)
                assert not _exact('bf16', p.Vn[live & (p.Vn != 0)])                     # a lo plane that matters
            # loud dead keys in every loaded block, NaN in every block that is never loaded
            loud, never = lay.loud[:, None, :, None].expand_as(p.Kn), lay.never[:, None, :, None].expand_as(p.Kn)
            assert bool(torch.isnan(p.Kn[never]).all()) and bool(torch.isnan(p.Vn[never]).all())
            assert bool((p.Vn[loud] == C.LOUD_V).all()) and bool((p.Kn[loud].reshape(-1, HD)[:, 0] == C.LOUD_K).all())
            assert bool((p.Kn[loud].reshape(-1, HD)[:, 1:] == 0).all()) and bool(torch.isfinite(p.Kn[~never]).all())
            assert lay.loud.any() and (lay.never.any() or not lay.key_len)
            got = C.ref_cross(*_values(p))
            assert C.head_rel(got, p.want, NH).max().item() < 1e-10
            if kind == 'bf16':
                assert torch.equal(got.to(torch.bfloat16), p.want.to(torch.bfloat16)) or p.name == 'uniform'
            # every score of a dead key is 64, of a target 32, of every other live key 0
            if p.name == 'peaked':
                assert p.Kn[torch.isfinite(p.Kn)].abs().max().item() <= C.LOUD_K
                b = lay.B - 1
                rows = slice(lay.row0[b], lay.row0[b] + lay.counts[b])
                s = torch.einsum('rhd,hkd->rhk', p.q[rows].reshape(-1, NH, HD) / 8.0, p.Kn[b, :, :lay.lens[b]].double())
                hit = torch.zeros_like(s, dtype=torch.bool).scatter_(2, p.tgt[rows][..., None], True)
                lv = lay.live[b, :lay.lens[b]][None, None, :].expand_as(s)
                assert bool((s[hit] == 32).all()) and bool((s[~hit & lv] == 0).all()) and bool((s[~lv] == 64).all())


def test_ragged_m_long_case_and_groups_give_the_stated_outputs():
    cases = [C.Layout(kind, [M] * 2, [16, 15], M, 1, mask, key_len=False) for kind in C.KINDS for M in C.RAGGED_M[:2] for mask in ('none', 'lead')]
    cases += [C.Layout('split', [C.LONG_M] * 2, [64, 63], C.LONG_M, 4, 'none', key_len=False), C.groups_layout('fp32', 2), C.groups_layout('bf16', 4, 'pad2d')]
    for lay in cases:
        assert lay.Mpad % lay.KB == 0 and lay.Mpad - lay.M < lay.KB
        if lay.Mpad > lay.M:
            assert bool(lay.loud[:, lay.M:].all())                                    # padded keys M .. Mpad are loud
        for pi, (_, bases) in enumerate(C.edge_phases(lay)):
            for p in (C.plant_peaked(lay, bases), C.plant_uniform(lay, bases, pi)):
                assert C.head_rel(C.ref_cross(*_values(p)), p.want, NH).max().item() < 1e-10
    g = C.groups_layout('bf16', 4)
    assert [n for _, n, b in g.groups if b == 1] == [64, 64, 64, 1] and g.groups[3][0] % 16 == 5


def test_stated_outputs_hold_at_4096_keys_and_a_leaked_key_is_loud():
    lay = C.Layout('bf16', [4096], [64], 4096, 4)
    p = C.plant_peaked(lay, C.edge_phases(lay)[1][1])
    # 4095 keys of score 0 beside the target's 32: the output is V[target] to 4095 e^-32 = 5.19e-11 of its largest value
    assert C.head_rel(C.ref_cross(*_values(p)), p.want, NH).max().item() < 4095 * 2.718281828459045 ** -32 * 1.001 < 5.2e-11
    u = C.plant_uniform(lay, [0], 0)
    assert C.head_rel(C.ref_cross(*_values(u)), u.want, NH).max().item() < 5e-11
    assert (abs(C.LOUD_V) - 17) / 17 > 13 and C.LOUD_K / 8 == 64 and C.LOUD_V == float(torch.tensor(C.LOUD_V).to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------------------------------------------
# teeth
# ---------------------------------------------------------------------------------------------------------------------------------------
def _walk_plants(kind, qt, mask='none', key_len=True, lens=None, M=C.M_SLAB):
    phases = C.sweep(kind, qt, mask, lens, M, key_len)
    for pi in sorted({0, len(phases) - 1}):
        lay, bases = phases[pi]
        yield C.plant_peaked(lay, bases), C.plant_uniform(lay, bases, pi)


def _hit(p):
    """[R][nH][Mpad]: 1 at the target of (row, head)"""
    return torch.zeros(p.lay.R, NH, p.lay.Mpad, dtype=torch.float64).scatter_(2, p.tgt[..., None], 1.0)


def _assert_broken(name, lay, plants, applies, **kw):
    """the mutant misses the walk gates by WIDE in every image it applies to (the worse of the two walks)"""
    e = torch.stack([_per_image(p, C.ref_cross(*_values(p), **{k: (v(p) if callable(v) else v) for k, v in kw.items()})) for p in plants]).amax(0)
    for b in range(lay.B):
        if applies(lay.lens[b]):
            assert e[b].item() >= WIDE and e[b].item() >= 50 * C.walk_gate('bf16'), (name, lay.kind, lay.lens[b], e[b].item())


@pytest.mark.parametrize('kind', C.KINDS)
def test_mutants_break_the_walk_gates(kind):
    KB = C.key_block(kind)
    for plants in _walk_plants(kind, 4):
        lay = plants[0].lay
        j = torch.arange(lay.Mpad).expand(lay.B, lay.Mpad)
        L = torch.tensor(lay.lens)[:, None]
        for p in plants:
            assert C.head_rel(C.ref_cross(*_values(p)), p.want, NH).max().item() < 1e-10          # unharmed: far inside both gates
        _assert_broken('drops the target', lay, plants, lambda n: True, weight=lambda p: 1.0 - _hit(p))
        _assert_broken('takes the target twice', lay, plants, lambda n: n >= 2, weight=lambda p: 1.0 + _hit(p))
        _assert_broken('K one key off', lay, plants, lambda n: n >= 2, ksrc=torch.where(j < L, (j + 1) % L, j))
        sw = j.clone()
        sw[:, 0], sw[:, 1] = 1, 0
        _assert_broken('swaps slots 0 and 1 of block 0', lay, plants, lambda n: n >= 2, vsrc=sw)
        sw = torch.where(j == L - 1, L - 2, torch.where(j == L - 2, L - 1, j))
        _assert_broken('swaps the last two keys', lay, plants, lambda n: n >= 2, vsrc=sw)
        if kind != 'fp32':
            inv = torch.empty(32, dtype=torch.int64)
            inv[_slot_of_key()] = torch.arange(32)
            _assert_broken('reads V^T without the slot permutation', lay, plants, lambda n: n >= 5, vsrc=j // 32 * 32 + inv[j % 32])
        for NS in sorted({c['NS'] for k, qt, r, nt, c in _configs() if k == kind and c['ring']}):
            stale = torch.where(j >= NS * KB, j - NS * KB, j)
            _assert_broken('block c reads ring stage c - %d' % NS, lay, plants, lambda n: n > NS * KB, ksrc=stale, vsrc=stale)
        if kind == 'split':
            # the V^T lo plane ignored: 2^-10 (1 .. 7) of values up to 7 (17 / n_live): 140 times the gate at the least
            for p in plants:
                q, Kv, Vv, counts, live = _values(p)
                e = _per_image(p, C.ref_cross(q, Kv, Vv.to(torch.bfloat16).double(), counts, live))
                assert e.min().item() >= 100 * C.walk_gate('split'), (p.name, e.min().item())


@pytest.mark.parametrize('kind', C.KINDS)
@pytest.mark.parametrize('case', ['pad', 'masked', 'beyond key_len'])
def test_one_counted_dead_key_breaks_the_walk_gates(kind, case):
    KB = C.key_block(kind)
    if case == 'pad':
        gen = _walk_plants(kind, 1, 'none', False, [77] * 4, 77)
    else:
        gen = _walk_plants(kind, 2, 'lead' if case == 'masked' else 'none')
    for plants in gen:
        lay = plants[0].lay
        live = lay.live.clone()
        applies = []
        for b, n in enumerate(lay.lens):
            dead = {'pad': lay.M, 'masked': 0, 'beyond key_len': n}[case]
            ok = dead < lay.Mpad and bool(lay.loud[b, dead])
            applies.append(ok)
            if ok:
                live[b, dead] = True
        assert sum(applies) >= (lay.B if case == 'pad' else 20)
        for p in plants:
            q, Kv, Vv, counts, _ = _values(p)
            e = C.head_rel(C.ref_cross(q, Kv, Vv, counts, live), p.want, NH)
            for b in range(lay.B):
                if applies[b]:          # EVERY row of the image moves by more than 13 times its largest stated value
                    assert e[lay.row_img == b].min().item() > 13, (case, kind, lay.lens[b], p.name)


def test_mutants_break_the_plane_ramp_gates():
    """the walks cannot see K's lo plane or the split cross terms (their K is exact in one bf16, their q too): the plane ramps do"""
    lay = C.Layout('split', C.LENGTHS, C.rows_of_phase(1, 0, len(C.LENGTHS)), C.M_SLAB, 1)
    gate = TOL['split']
    for which, drop in (('klo', 'klo_qhi'), ('qlo', 'khi_qlo')):
        p = C.plant_plane_ramp(lay, which)
        K, Vt = C.slabs('split', p.Kn, p.Vn)
        Kv, Vv = C.natural('split', K, Vt)
        (kh, kl), _ = C.natural('split', K, Vt, planes=True)
        assert torch.equal(Kv[torch.isfinite(Kv)], p.Kn.double()[torch.isfinite(Kv)]) and torch.equal(Vv[torch.isfinite(Vv)], p.Vn.double()[torch.isfinite(Vv)])
        ref = C.ref_cross(p.q, Kv, Vv, lay.counts, lay.live)
        # the three leading products give exactly the scores of the plant: nothing of it lives in K_lo q_lo or in a third plane of q
        three = C.ref_cross(p.q, Kv, Vv, lay.counts, lay.live, kplanes=(kh, kl))
        assert (three - ref).abs().max().item() < TOL64
        other = 'khi_qlo' if drop == 'klo_qhi' else 'klo_qhi'
        assert (C.ref_cross(p.q, Kv, Vv, lay.counts, lay.live, kplanes=(kh, kl), drop=other) - ref).abs().max().item() < TOL64
        live = lay.live[:, None, :, None]
        if which == 'klo':
            assert bool((kh[live.expand_as(kh)].reshape(-1, HD)[:, 0] == 256).all()) and bool((kl[..., 1:][live.expand_as(kl[..., 1:])] == 0).all())
            mutants = {'drops K_lo q_hi': dict(kplanes=(kh, kl), drop=drop), 'ignores the K lo plane': dict(kplanes=(kh, torch.zeros_like(kl)))}
        else:
            assert bool((kl[live.expand_as(kl)] == 0).all())
            qh, ql = C.split_q(p.q)
            assert bool((ql.reshape(-1, HD)[:, 0] == 2.0 ** -13).all()) and bool((ql.reshape(-1, HD)[:, 1:] == 0).all()) and torch.equal(qh + ql, p.q / 8)
            mutants = {'drops K_hi q_lo': dict(kplanes=(kh, kl), drop=drop)}
        for name, kw in mutants.items():
            e = (C.ref_cross(p.q, Kv, Vv, lay.counts, lay.live, **kw) - ref).abs()
            for b, n in enumerate(lay.lens):
                if n >= 16:      # below, the ramp has too few steps to move the weights of every image by ten gates
                    rows = slice(lay.row0[b], lay.row0[b] + lay.counts[b])
                    assert e[rows].max().item() >= 10 * gate, (name, n, e[rows].max().item())


@pytest.mark.parametrize('kind', C.KINDS)
def test_ramps_move_the_maximum_at_every_block_or_never(kind):
    lay = C.Layout(kind, C.LENGTHS, C.rows_of_phase(1, 0, len(C.LENGTHS)), C.M_SLAB, 1)
    for rising in (True, False):
        p = C.plant_ramp(lay, rising)
        assert _exact(kind, p.Kn) and _exact(kind, p.Vn)
        for b, n in enumerate(lay.lens):
            s = p.Kn[b, 0, :n, 0].double() / 8.0
            step = s[1:] - s[:-1]
            assert bool((step >= 0).all() if rising else (step <= 0).all())
            if n > 1:
                assert abs(s.max().item() - C.RAMP_TOP[kind]) < 0.5 and s.min().item() == 0
            blocks = s[:n // lay.KB * lay.KB].reshape(-1, lay.KB).amax(1)
            if n >= 2 * lay.KB and (kind != 'bf16' or n <= 192):
                assert bool((blocks[1:] > blocks[:-1]).all() if rising else (blocks[1:] < blocks[:-1]).all())
        assert p.Vn[lay.live[:, None, :, None].expand_as(p.Vn)].abs().max().item() < (2.0 if kind == 'bf16' else 9.0)
