"""The float64 restatements of the MGP-STR recogniser kernels (tests/gpu_checks_vit.py ref_*, rounding off) against the oracle
(oracle/mgp_str_ref.py) in float64 and against plain torch softmax attention, and the planted inputs of the GPU tests against the
properties claimed for them: with bf16 rounding on, the key-slot walk, the dead-key and the tie inputs give EXACTLY the stated outputs.
Without this a wrong restatement could pass against an equally wrong kernel.  CPU only."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import mgp_str_ref as R
from tests import gpu_checks_vit as V

TOL = 1e-12   # float64 against float64: only the summation order differs


def _r(*shape, seed, s=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * s


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _sd(c, seed):
    return {k: v.double() for k, v in R.make_state_dict(c, seed=seed).items()}


def _cfg(E, nH, T):
    return R.cfg(embed=E, heads=nH, depth=1, img=(4, 4 * (T - 1)) if T > 1 else (4, 4), bpe_vocab=64, wp_vocab=64)


@pytest.mark.parametrize('T', [1, 17, 97, 257])
@pytest.mark.parametrize('E,nH', [(192, 3), (768, 12)])
def test_attention_restatement(E, nH, T):
    """ref_vit_attn == the attention of R.block (proj = identity, MLP switched off), and == torch softmax attention"""
    c = _cfg(E, nH, T)
    sd = _sd(c, 3)
    b = 'mgp_str.blocks.0.'
    sd[b + 'attn.proj.weight'], sd[b + 'attn.proj.bias'] = torch.eye(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    sd[b + 'mlp.fc2.weight'], sd[b + 'mlp.fc2.bias'] = torch.zeros(E, 4 * E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    sd[b + 'attn.qkv.weight'] = sd[b + 'attn.qkv.weight'] * 3.0          # a peaked softmax
    B = 2
    x = _r(B, T, E, seed=T, s=1.5)
    want = R.block(sd, c, x, 0) - x
    y = F.layer_norm(x, (E,), sd[b + 'norm1.weight'], sd[b + 'norm1.bias'], 1e-6)
    qkv = F.linear(y, sd[b + 'attn.qkv.weight'], sd[b + 'attn.qkv.bias']).reshape(B, T, 3, nH, 64).permute(2, 0, 3, 1, 4)
    got = V.ref_vit_attn(qkv[0], qkv[1], qkv[2], False)
    assert _rel(got.transpose(1, 2).reshape(B, T, E), want) < 1e-10   # (x + att) - x: att's bits below x's ulp are gone
    plain = F.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * 0.125, dim=-1) @ qkv[2]
    assert _rel(got, plain) < TOL


@pytest.mark.parametrize('E', [768, 192, 100])
@pytest.mark.parametrize('Hp,Wp', [(1, 1), (2, 17), (8, 32), (8, 33), (1, 15)])
def test_patch_embed_restatement(E, Hp, Wp):
    c = R.cfg(embed=E, heads=1, depth=0, img=(4 * Hp, 4 * Wp), bpe_vocab=64, wp_vocab=64)
    sd = _sd(c, 5)
    img = _r(3, 3, 4 * Hp, 4 * Wp, seed=Hp + Wp)
    T = Hp * Wp + 1
    got = V.ref_patch_embed(img, sd['mgp_str.patch_embed.proj.weight'].reshape(E, 48), sd['mgp_str.patch_embed.proj.bias'],
                            sd['mgp_str.cls_token'].reshape(E), sd['mgp_str.pos_embed'].reshape(T, E), False)
    assert _rel(got, R.embed(sd, c, img)) < TOL


@pytest.mark.parametrize('T', [1, 65, 257])
def test_a3_pool_restatement(T):
    """ref_a3_pool on the selector logits and features of R.token_learner (its own lines up to the softmax) == the maps it returns, and
    its output through the final LayerNorm"""
    E = 192
    c = _cfg(E, 3, T)
    sd = _sd(c, 7)
    x = _r(2, T, E, seed=T + 1)
    maps, want = R.token_learner(sd, c, x, 'char')
    t = 'mgp_str.char_tokenLearner.'
    y4 = F.layer_norm(x, (E,), sd[t + 'token_norm.weight'], sd[t + 'token_norm.bias'], 1e-5).transpose(1, 2).unsqueeze(-1)
    sel = F.conv2d(F.conv2d(y4, sd[t + 'tokenLearner.0.weight'], groups=8), sd[t + 'tokenLearner.1.weight']).flatten(2)   # [B, L, T]
    feat = F.conv2d(y4, sd[t + 'feat.weight'], groups=8).flatten(2).transpose(1, 2)
    pooled, gm = V.ref_a3_pool(sel.transpose(1, 2), feat)
    assert _rel(gm, maps) < TOL
    assert _rel(F.layer_norm(pooled, (E,), sd[t + 'norm.weight'], sd[t + 'norm.bias'], 1e-5), want) < 1e-10


def test_row_stats_restatement():
    """ref_row_stats == the greedy ids and max-softmax probabilities of R.decode's lines (test_final.py:145-170); ties go to the lowest index"""
    lgs = [_r(3, 28, n, seed=n, s=3.0) for n in (38, 64, 65)]
    res = R.decode(*lgs)
    for k, lg in zip(('char_ids', 'bpe_ids', 'wp_ids'), lgs):
        ids, prob = V.ref_row_stats(lg.reshape(-1, lg.shape[-1]))
        assert ids.reshape(3, 28)[:, 1:].tolist() == [r[k] for r in res]
        assert _rel(prob.reshape(3, 28), F.softmax(lg, dim=2).max(dim=2)[0]) < TOL
    tie = torch.tensor([[1.0, 5.0, 5.0, -2.0], [7.0, 7.0, 7.0, 7.0]], dtype=torch.float64)
    ids, prob = V.ref_row_stats(tie)
    assert ids.tolist() == [1, 0] and abs(prob[1].item() - 0.25) < 1e-15


# ---------------------------------------------------------------------------------------------------------------------------------------
# the planted inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _is_bf16(t):
    return torch.equal(t, t.to(torch.bfloat16).double())


def test_key_codes_differ_in_seven_dimensions():
    k = V.key_codes(V.MPAD)
    assert (k.abs() == 1).all()
    dot = k @ k.T
    assert (dot.diagonal() == 64).all()
    off = dot - 128.0 * torch.eye(V.MPAD, dtype=torch.float64)
    assert off.max().item() <= 64 - 2 * 7


@pytest.mark.parametrize('T', V.TOKENS)
def test_walk_inputs_are_exact(T):
    """pi is a permutation and not the identity, the hit is 28 ahead of every other score, V rows are distinct non-zero integers, and
    ref_vit_attn(bf=True) returns V[pi(i)] exactly"""
    B, nH = 3, 12
    pi = V.walk_perm(B, nH, T)
    assert (pi.sort(-1).values == torch.arange(T)).all()
    if T > 1:
        assert (pi != torch.arange(T)).any(-1).all()
        assert len({tuple(p.tolist()) for p in pi.reshape(-1, T)}) > 1      # another permutation per image / head
    q, k, v, want = V.walk_inputs(B, nH, T)
    assert _is_bf16(q) and _is_bf16(k) and _is_bf16(v)
    assert (v != 0).all() and (v.abs() <= 8).all() and (v == v.round()).all()
    assert len({tuple(r.tolist()) for r in v[0, 0]}) == T
    s = (q * 0.125) @ k.transpose(-1, -2)
    hit = s.gather(-1, pi[..., None])
    assert (hit == 128).all()
    if T > 1:
        rest = s.scatter(-1, pi[..., None], -math.inf)
        assert rest.max().item() <= 100
    assert torch.equal(want, v.gather(2, pi[..., None].expand_as(v)))
    assert torch.equal(V.ref_vit_attn(q, k, v, True), want)


def test_dead_key_inputs_are_exact():
    """every output is bf16(256 / T) under ref_vit_attn(bf=True) -- and under the kernel's own fp32 arithmetic (256 * (1.0f / T) rounded
    to fp32, then to bf16), so the stated output does not hang on a double rounding; a padding key with weight would give another value"""
    for T in range(1, V.MPAD):
        q, k, v, want = V.dead_inputs(1, 3, T)
        assert torch.equal(V.ref_vit_attn(q, k, v, True), want)
        inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(T), dtype=torch.float32)
        assert (torch.tensor(256.0, dtype=torch.float32) * inv).to(torch.bfloat16).double().item() == want[0, 0, 0, 0].item()
        # one padding key with weight shows wherever bf16 resolves 256 / T from 256 / (T + 1) (everywhere up to T = 100; beyond, not at
        # every T); all of them with weight (the mask dropped: 256 / 288) show at every T below 280
        if T <= 100:
            assert torch.tensor(256.0 / (T + 1)).to(torch.bfloat16).double().item() != want[0, 0, 0, 0].item()
        if T < 280:
            assert torch.tensor(256.0 / V.MPAD).to(torch.bfloat16).double().item() != want[0, 0, 0, 0].item()


@pytest.mark.parametrize('T', [17, 33, 97, 193, 257, 273, 288])
def test_tie_inputs_are_exact(T):
    pairs = V.tie_pairs(T)
    assert (0, T - 1) in pairs
    if T > 200:
        assert {(3, 200), (200, 3)} <= set(pairs)       # chunk 0 and chunk 2 (keys 192 ..), both orders
        assert 3 // 96 == 0 and 200 // 96 == 2
    for (a, b) in pairs:
        q, k, v, want = V.tie_inputs(1, 3, T, a, b)
        assert torch.equal(k[:, :, a], k[:, :, b]) and not torch.equal(v[:, :, a], v[:, :, b])
        pi = V.walk_perm(1, 3, T)
        both = (pi == a) | (pi == b)
        assert both.sum().item() == 2 * 3
        mean = (v[:, :, a] + v[:, :, b]) / 2
        assert (mean > 0).all() and _is_bf16(mean)
        assert torch.equal(want[both], mean[:, :, None].expand(1, 3, 2, 64).reshape(-1, 64))
        assert torch.equal(V.ref_vit_attn(q, k, v, True), want)
    # rows of the walk whose best key sits in chunk 0 (alpha = 1 afterwards) and in the last live chunk (alpha ~ exp(-28))
    pi = V.walk_perm(1, 3, T)[0, 0]
    assert (pi < 96).any() and (pi // 96 == (T - 1) // 96).any()


def test_random_inputs_have_a_peaked_softmax():
    q, k, v = V.random_inputs(1, 3, 257)
    assert _is_bf16(q) and _is_bf16(k) and _is_bf16(v)
    s = (q * 0.125) @ k.transpose(-1, -2)
    assert 2.5 < s.std().item() < 3.5
    assert torch.softmax(s, -1).amax(-1).median().item() > 0.2


def test_onehot_selector_is_one_hot():
    sel, tok = V.onehot_sel(3, 257, 27)
    assert torch.equal(sel, sel.float().double())
    feat = _r(3, 257, 64, seed=1).to(torch.bfloat16).double()
    pooled, maps = V.ref_a3_pool(sel, feat)
    assert torch.equal(pooled, feat.gather(1, tok[..., None].expand(3, 27, 64)))
    assert torch.equal(maps.float().sum(-1), torch.ones(3, 27)) and (maps.amax(-1) == 1).all()
    assert math.exp(-2e4) == 0.0


def test_winner_bias_lifts_the_column_by_five():
    lg = _r(1, 200, seed=2)
    for c in (0, 63, 64, 127, 128, 199):
        s = lg + V.winner_bias(lg, c)
        top = s.sort(-1, descending=True)
        assert top.indices[0, 0].item() == c and abs((top.values[0, 0] - top.values[0, 1]).item() - 5.0) < 1e-5
    assert V.winner_bias(_r(1, 1, seed=3), 0).shape == (1,)


def test_tol_table_follows_the_three_times_rule():
    """every non-zero gate carries its measured value and is at most 4 times it"""
    assert V.TOL
    for key, (gate, meas) in V.TOL.items():
        assert meas is not None and gate <= 4.0 * meas and gate >= meas, key
