"""Batched prompt prefill on the GPU (csrc/decoder.hip: prefill_launch; include/omp355.h omp_decoder_plan.prefill): the same plan runs
twice in one process, once with the pass and once with the stepwise prefill forced (omp_debug_prefill), and everything later steps
read must be the SAME BITS -- the self-attention caches of every layer at the prompt positions and, after a handful of sampling steps,
seq / probs / finished / lengths.  The memory is synthetic (random rows through project_memory; no encoder), about 40 keys: a key
range per wave plus a ragged last block.  The pass must write nothing it does not own: cache positions behind the prompt and scratch
rows behind R * L are planted with NaN and must still be NaN.  Ineligible plans get the table and the scratch bound and must run --
and are asserted to run -- the stepwise prefill.  The pass's own kernel forms are also gated one by one through what the last layer leaves in
the scratch (embedding, q|k|v rows, self-attention output), and the engine's call form (Decoder.decode_point_rows: the table bound by
Decoder._bind, the pass and sampling steps in one omp_decoder_run) runs counts A, B, A on one decoder."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
M_KEYS = 40
STEPS = 4   # sampling steps behind the prompt


@pytest.fixture(scope='module')
def E():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advancedliteratemachinery_amd import _lib
    from advancedliteratemachinery_amd.model.transformer import Decoder
    from advancedliteratemachinery_amd.utils.parser import make_args
    from advancedliteratemachinery_amd.utils import synthetic as weights

    class Env(object):
        lib = _lib.lib()
        decoders = {}

        @classmethod
        def decoder(cls, dtype=torch.bfloat16, pre_norm=True, x3=False, layers=4):
            key = (dtype, pre_norm, x3, layers)
            if key not in cls.decoders:
                args = make_args(tfm_pre_norm=pre_norm, use_fpn=True, use_char_window_prompt=True, tfm_dec_layers=layers)
                sd = weights.make_state_dict(args, seed=11, depths=(1, 1, 1, 1))
                sd = {k: v.to(DEV) for k, v in sd.items() if k.startswith('transformer.')}
                cls.decoders[key] = Decoder(sd, args, dtype, DEV, x3=x3)
            return cls.decoders[key]

    yield Env
    Env.lib.omp_debug_prefill(0)
    for d in Env.decoders.values():
        d.release()


def _memory(dec, B, key_len, masked):
    """synthetic memory of B images x M_KEYS keys -> the decoder's K / V^T slabs"""
    g = torch.Generator().manual_seed(5)
    dt = dec.dtype
    mem = torch.randn(B * M_KEYS, dec.d, generator=g).to(DEV, dt)
    mem_pos = (mem.float() + torch.randn(B * M_KEYS, dec.d, generator=g).to(DEV)).to(dt)
    mask = None
    if masked:
        mask = (torch.rand(B, M_KEYS, generator=g) > 0.8)
        mask[:, 0] = False
        mask = mask.to(torch.uint8).to(DEV)
    return dec.project_memory(mem, mem_pos, B, M_KEYS, mask, key_len=key_len)


def _bind_prefill(dec, ph, tiles, n_prompt):
    """the table and the scratch on a plan whatever its eligibility (the library decides); 8 scratch rows more than the pass owns"""
    groups, qt = tiles
    L = n_prompt - 1
    rows = ph.R * L
    pf = ph.prefill_scratch(dec, rows + 8)
    pt = torch.tensor(dec.make_prefill_tiles(groups, qt, L), dtype=torch.int32).reshape(-1, 3)
    pf['tiles'][:pt.shape[0]].copy_(pt.to(DEV))
    P = ph.plan
    P.prefill, P.n_prefill_tiles, P.prefill_tiles, P.pf_rows = 1, pt.shape[0], pf['tiles'].data_ptr(), pf['rows']
    for n in ('x', 'qkv', 'att', 'q', 'ffh', 'partial'):
        setattr(P, 'pf_' + n, pf[n].data_ptr())
    return pf


def _run(E, dec, counts, n_prompt, stepwise, key_len=None, masked=False):
    """one point phase: prompt prefill, then STEPS sampling steps -> (batched passes run, dict of everything later steps read)"""
    B, R, L = len(counts), sum(counts), n_prompt - 1
    kv = _memory(dec, B, key_len, masked)
    tiles = dec.make_tiles(counts)
    ph = dec._phase('pt', R, L + STEPS, n_prompt + STEPS + 1, dec._n_split(tiles, M_KEYS))
    dec._bind(ph, kv, tiles, n_prompt, True, False)
    pf = _bind_prefill(dec, ph, tiles, n_prompt) if L >= 1 else None
    for t in ph.kc + ph.vc + ([pf[n] for n in ('x', 'qkv', 'att', 'q', 'ffh', 'partial')] if pf else []):
        t.fill_(float('nan'))
    ph.seq.zero_(); ph.probs.zero_(); ph.finished.zero_(); ph.lengths.zero_(); ph.d_pos.zero_()
    g = torch.Generator().manual_seed(R * 31 + n_prompt)
    ph.seq[:, :n_prompt] = torch.randint(0, dec.args.num_bins, (R, n_prompt), generator=g).to(DEV, torch.int32)
    E.lib.omp_debug_prefill(1 if stepwise else 0)
    try:
        before = E.lib.omp_debug_prefill_passes()
        dec._run(ph, 0, L)
        torch.cuda.synchronize()
        passes = E.lib.omp_debug_prefill_passes() - before
        out = dict(d_pos=ph.d_pos.tolist())
        for l in range(dec.L):
            out['kcache%d' % l], out['vcache%d' % l] = ph.kc[l][:, :L].clone(), ph.vc[l][:, :L].clone()
        out['behind'] = all(bool(torch.isnan(t[:, L:].float()).all()) for t in ph.kc + ph.vc)
        if pf and passes:
            out['scratch'] = all(bool(torch.isnan(pf[n][R * L:].float()).all()) for n in ('x', 'qkv', 'att', 'q', 'ffh', 'partial'))
        dec._run(ph, L, STEPS)
        torch.cuda.synchronize()
    finally:
        E.lib.omp_debug_prefill(0)
    for n in ('seq', 'probs', 'finished', 'lengths'):
        out[n] = getattr(ph, n).clone()
    return passes, out


def _same_bits(a, b):
    assert a['d_pos'] == b['d_pos']
    for k in a:
        if torch.is_tensor(a[k]):
            assert not torch.isnan(a[k].float()).any(), k
            assert torch.equal(a[k], b[k]), '%s differs between the batched pass and the stepwise prefill' % k


def _both(E, dec, counts, n_prompt, takes_pass, **kw):
    p0, a = _run(E, dec, counts, n_prompt, False, **kw)
    p1, b = _run(E, dec, counts, n_prompt, True, **kw)
    assert p1 == 0                                   # forced: never the pass
    assert p0 == (1 if takes_pass else 0), 'the %s prefill ran' % ('stepwise' if takes_pass else 'batched')
    assert a['d_pos'][0] == n_prompt - 1 and a['d_pos'][1] == 0   # the ticket word is untouched
    assert a['behind'] and b['behind']               # cache positions behind the prompt: still NaN
    if takes_pass:
        assert a['scratch']                          # scratch rows behind R * L: still NaN
    _same_bits(a, b)


WINDOWS = [3, 1, 20, 17, 9, 16, 2]   # 68 rows, q_tiles 2: 120 and 102 prefill rows of an image are cut inside the image
WINDOWS4 = [64, 33, 1, 48]           # 146 rows, q_tiles 4: 384, 198 and 288 prefill rows of an image cut into groups of 64


def _few_images(R):
    """R rows on few images (64 rows each and the rest): big R with a small memory; q_tiles 4"""
    return [64] * (R // 64) + ([R % 64] if R % 64 else [])


# behind the first seven (R = 64 / 70 / windows at n_prompt 7 / 3 / 2), the pass at its limits -- tests/test_host_logic.py
# (test_prefill_limits_reach_the_other_tile_kernels) pins which kernels each of them runs, pass and step:
#   n_prompt 7: R = 128, 129; 200 (linear1 on the 4-deep ring of the 64x64 kernel); 321 (linear1 on 128x128, the step on 64x64); 682 (4092
#   prefill rows: q|k|v with its per-row bias and linear1 on 128x128, the mid chain's 32-row tile, q_tiles 4); 683 (4098 rows: stepwise)
#   n_prompt 3: R = 1023 (the last row count the pass takes);  n_prompt 34 / 42 at R = 64 / 70: the second key block of the prefill
#   self-attention (p >= 32), 32-row mid tile;  WINDOWS4: groups cut inside images at q_tiles 4
@pytest.mark.parametrize('mid', [True, False])
@pytest.mark.parametrize('counts,n_prompt,takes', [([1] * 64, 7, True), ([1] * 70, 7, True), ([1] * 64, 3, True), ([1] * 70, 3, True),
                                                   ([1] * 70, 2, False), (WINDOWS, 7, True), (WINDOWS, 3, True),
                                                   (_few_images(128), 7, True), (_few_images(129), 7, True), (_few_images(200), 7, True),
                                                   (_few_images(321), 7, True), (_few_images(682), 7, True), (_few_images(683), 7, False),
                                                   (_few_images(1023), 3, True), ([1] * 64, 34, True), ([1] * 70, 34, True),
                                                   ([1] * 64, 42, True), ([1] * 70, 42, True), (WINDOWS4, 7, True)])
def test_pass_equals_stepwise(E, counts, n_prompt, takes, mid):
    """R = 64 (the split-K small-M kernel on both sides) and 70 (the tile kernels; 70 * 6 rows cross the mid chain's 16-row workgroups
    mid-image), window prompts, with layers[].rows_mid bound and without; n_prompt 2 has nothing to batch and must stay stepwise; then
    the row counts at which the pass and the step run DIFFERENT tile kernels, up to the limits R < 1024 and R * L <= 4096"""
    dec = E.decoder()
    keep = dec.MID_MIN_ROWS
    try:
        dec.MID_MIN_ROWS = keep if mid else 1 << 30
        _both(E, dec, counts, n_prompt, takes)
    finally:
        dec.MID_MIN_ROWS = keep


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('n_split', [0, 2])
def test_pass_equals_stepwise_ragged(E, masked, n_split):
    """ragged key_len 1, 33 and M (one key; one key behind a block; every key), with a key_mask and without; n_split 2: partials + merge"""
    dec = E.decoder()
    keep = dec.n_split_override
    try:
        dec.n_split_override = n_split
        _both(E, dec, [1] * 66, 7, True, key_len=[(1, 33, M_KEYS)[b % 3] for b in range(66)], masked=masked)
    finally:
        dec.n_split_override = keep


def test_ineligible_plans_stay_stepwise(E):
    """the table and the scratch are bound, the library must decline: <= 63 rows, rows_fused, fp32, bf16x3, post-norm"""
    dec = E.decoder()
    _both(E, dec, [1] * 40, 7, False)
    keep = dec.rows_min
    try:
        dec.rows_min = 1
        _both(E, dec, [1] * 70, 7, False)
    finally:
        dec.rows_min = keep
    _both(E, E.decoder(dtype=torch.float32), [1] * 70, 7, False)
    _both(E, E.decoder(dtype=torch.float32, x3=True), [1] * 70, 7, False)
    _both(E, E.decoder(pre_norm=False), [1] * 70, 7, False)


def test_short_table_or_scratch_is_refused(E):
    dec = E.decoder()
    counts, n_prompt = [1] * 70, 7
    kv = _memory(dec, len(counts), None, False)
    tiles = dec.make_tiles(counts)
    ph = dec._phase('pt', 70, 6 + STEPS, n_prompt + STEPS + 1, dec._n_split(tiles, M_KEYS))
    dec._bind(ph, kv, tiles, n_prompt, True, False)
    _bind_prefill(dec, ph, tiles, n_prompt)
    for field, value in (('pf_rows', 70 * 6 - 1), ('n_prefill_tiles', 70 * 6 // 16 - 1)):
        good = getattr(ph.plan, field)
        setattr(ph.plan, field, value)
        ph.d_pos.zero_()
        assert E.lib.omp_decoder_run(ctypes.byref(ph.plan), 0, 6, -1, None) == -22
        setattr(ph.plan, field, good)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the pass's own kernels, through what the pass leaves behind: the last layer stops behind its cache append, so its q|k|v rows (pf_qkv) and
# its self-attention output (pf_att) are still in the scratch, and with ONE layer pf_x is still the embedding
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pass_only(E, dec, counts, n_prompt):
    """bind, plant NaN, run the prompt positions as the pass (asserted) -> (phase, scratch)"""
    B, R, L = len(counts), sum(counts), n_prompt - 1
    kv = _memory(dec, B, None, False)
    tiles = dec.make_tiles(counts)
    ph = dec._phase('pt', R, L + STEPS, n_prompt + STEPS + 1, dec._n_split(tiles, M_KEYS))
    dec._bind(ph, kv, tiles, n_prompt, True, False)
    pf = _bind_prefill(dec, ph, tiles, n_prompt)
    for t in ph.kc + ph.vc + [pf[n] for n in ('x', 'qkv', 'att', 'q', 'ffh', 'partial')]:
        t.fill_(float('nan'))
    ph.seq.zero_(); ph.probs.zero_(); ph.finished.zero_(); ph.lengths.zero_(); ph.d_pos.zero_()
    g = torch.Generator().manual_seed(R * 31 + n_prompt)
    ph.seq[:, :n_prompt] = torch.randint(0, dec.args.num_bins, (R, n_prompt), generator=g).to(DEV, torch.int32)
    E.lib.omp_debug_prefill(0)
    before = E.lib.omp_debug_prefill_passes()
    dec._run(ph, 0, L)
    torch.cuda.synchronize()
    assert E.lib.omp_debug_prefill_passes() - before == 1
    return ph, pf


@pytest.mark.parametrize('R', [64, 70])
@pytest.mark.parametrize('layers,n_prompt', [(1, 7), (1, 34), (1, 42), (4, 7)])
def test_pass_kernels_through_its_scratch(E, layers, n_prompt, R):
    """dec_embed_ln_kernel<float, ROWPOS> against float64 and the one-position launch (one layer: pf_x is still the embedding), and
    dec_self_attn_kernel<bf16, PREFILL> of the last layer against the stepwise kernel fed the pass's own q|k|v rows position by position
    (outputs and caches bit for bit) and against float64 causal attention.  At n_prompt 34 position 32 opens the second 32-key block with
    the wave's own key alone; at 42 position 40 reads eight keys of the pass's rows at pitch 3 d there, plus its own."""
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks_selfattn import GATE, LN_GATE, ref_attn, ref_embed
    dec = E.decoder(layers=layers)
    assert dec.L == layers
    ph, pf = _pass_only(E, dec, [1] * R, n_prompt)
    L, d, nH = n_prompt - 1, dec.d, dec.nH
    qkv, att, x = pf['qkv'][:R * L].view(R, L, 3, d), pf['att'][:R * L].view(R, L, d), pf['x'][:R * L].view(R, L, d)
    assert bool(torch.isfinite(qkv.float()).all())
    dpos = torch.zeros(2, dtype=torch.int32, device=DEV)
    if layers == 1:
        tok = ph.seq[:, :L].cpu()
        word, ptab = dec.word.double().cpu(), dec.pos_tab['pt'].double().cpu()
        ref = torch.stack([ref_embed(word, ptab[j], tok[:, j], dec.emb_g.double().cpu(), dec.emb_b.double().cpu()) for j in range(L)], 1)
        err = (x.double().cpu() - ref).abs().max().item()
        print('prefill embedding R=%d L=%d: max |x - float64| %.3e (gate %.1e)' % (R, L, err, LN_GATE))
        assert err <= LN_GATE
        for j in range(L):
            dpos[0] = j
            xj = torch.full((R, d), float('nan'), device=DEV)
            ops.dec_embed_ln(ph.seq, dpos, dec.word, dec.pos_tab['pt'], dec.emb_g, dec.emb_b, x=xj)
            assert torch.equal(xj, x[:, j]), 'embedding of position %d differs from the one-position launch' % j
    # the stepwise kernel (a wave per (row, head)) on fresh caches, fed the pass's rows
    kc = torch.full((R, ph.Lmax, d), float('nan'), dtype=torch.bfloat16, device=DEV)
    vc = torch.full_like(kc, float('nan'))
    ops.self_attn_impl(1)
    try:
        for j in range(L):
            dpos[0] = j
            out = torch.full((R, d), float('nan'), dtype=torch.bfloat16, device=DEV)
            ops.dec_self_attn_step(qkv[:, j].reshape(R, 3 * d).contiguous(), kc, vc, out, dpos, nH)
            assert torch.equal(out, att[:, j]), 'self-attention at position %d differs from the stepwise kernel' % j
    finally:
        ops.self_attn_impl(0)
    assert torch.equal(kc[:, :L], ph.kc[-1][:, :L]) and torch.equal(vc[:, :L], ph.vc[-1][:, :L])
    assert torch.equal(kc[:, :L], qkv[:, :, 1]) and torch.equal(vc[:, :L], qkv[:, :, 2])       # the caches hold the k / v thirds exactly
    assert bool(torch.isnan(kc[:, L:].float()).all()) and bool(torch.isnan(ph.kc[-1][:, L:].float()).all())
    q64, k64, v64 = qkv[:, :, 0].double(), qkv[:, :, 1].double(), qkv[:, :, 2].double()
    err = max((att[:, j].double() - ref_attn(q64[:, j], k64[:, :j + 1], v64[:, :j + 1], nH)).abs().max().item() for j in range(L))
    print('prefill self-attention R=%d L=%d layers=%d: max |att - float64| %.3e (gate %.1e)' % (R, L, layers, err, GATE[torch.bfloat16]))
    assert err <= GATE[torch.bfloat16]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the engine's own call form: Decoder.decode_point_rows, nothing bound by the test -- Decoder._bind keeps the prefill tiles table across
# calls (pf['tiles_key']), and the first omp_decoder_run holds the pass AND sampling steps
# ---------------------------------------------------------------------------------------------------------------------------------------
def _engine_call(E, dec, kv, prompts, counts, stepwise, forced):
    E.lib.omp_debug_prefill(1 if stepwise else 0)
    try:
        before = E.lib.omp_debug_prefill_passes()
        r = dec.decode_point_rows(kv, prompts, counts, max_new=6, forced_instances=3 if forced else None, poll=2)
        torch.cuda.synchronize()
        passes = E.lib.omp_debug_prefill_passes() - before
    finally:
        E.lib.omp_debug_prefill(0)
    out = {n: getattr(r['ph'], n).clone() for n in ('seq', 'probs', 'finished', 'lengths')}
    return passes, r['sampled'], out, r['ph']


ENGINE_COUNTS = {   # A, B: 70 rows on six images; the same q_tiles class (max 20: q_tiles 2) / another one (17 -> 40: q_tiles 2 -> 4)
    'same q_tiles': ([17, 3, 20, 9, 16, 5], [10, 20, 4, 17, 12, 7]),
    'other q_tiles': ([17, 3, 16, 9, 16, 9], [40, 3, 2, 9, 8, 8]),
}


@pytest.mark.parametrize('forced', [True, False], ids=['one run', 'poll loop'])
@pytest.mark.parametrize('which', sorted(ENGINE_COUNTS))
def test_engine_calls_rebind_the_tiles_table(E, which, forced):
    """counts A, counts B (the same rows, split otherwise over the images), counts A again on one decoder and one memory: every call takes
    the pass exactly once and gives what the same call gives under the stepwise prefill"""
    dec = E.decoder()
    A, B = ENGINE_COUNTS[which]
    assert sum(A) == sum(B) and len(A) == len(B) and A != B
    qa, qb = dec.make_tiles(A)[1], dec.make_tiles(B)[1]
    assert (qa == qb) == (which == 'same q_tiles')
    assert dec._n_split(dec.make_tiles(A), M_KEYS) == dec._n_split(dec.make_tiles(B), M_KEYS)      # one phase, one scratch for all calls
    kv = _memory(dec, len(A), None, False)
    n_prompt = 7
    g = torch.Generator().manual_seed(77)
    prompts = torch.randint(0, dec.args.num_bins, (sum(A), n_prompt), generator=g).to(DEV, torch.int32)
    phases = set()
    for counts in (A, B, A):
        p0, s0, a, ph = _engine_call(E, dec, kv, prompts, counts, False, forced)
        p1, s1, b, ph1 = _engine_call(E, dec, kv, prompts, counts, True, forced)
        phases |= {id(ph), id(ph1)}
        assert (p0, p1) == (1, 0), 'counts %s: %d batched passes (1 expected), %d under the forced stepwise prefill' % (counts, p0, p1)
        assert s0 == s1 and s0 >= 2
        for n in a:
            assert not torch.isnan(a[n].float()).any(), n
            assert torch.equal(a[n], b[n]), '%s differs between the pass and the stepwise prefill at counts %s' % (n, counts)
        assert ph.pf is not None and ph.pf['tiles_key'][0] == tuple(dec.make_tiles(counts)[0])
    assert len(phases) == 1
