"""The float64 restatements of the decoder self-attention checks (tests/gpu_checks_selfattn.py ref_*) against plain torch softmax attention and
F.layer_norm + F.linear, the planted inputs against the outputs stated for them, and the teeth of the walks: a reference that drops the
target key, reads K one key off, reuses the keys of chunk c - 3 for chunk c (a stale stage of the fused kernel's ring of three 64-key
chunks) or skips the new key must miss the walk gates by a wide margin at every listed position.  Without this the GPU cases could pass
against an equally wrong kernel -- or prove nothing.  CPU only; one head (d = 64) where the head count does not matter."""
import pytest
import torch
import torch.nn.functional as F

from tests import gpu_checks_selfattn as S

TOL = 1e-12
WIDE = 0.2      # 51 times the bf16 walk gate (2^-8), 2e5 times the fp32 one


def _r(*shape, seed, s=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * s


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _is_bf16(t):
    return torch.equal(t, t.to(torch.bfloat16).double())


def _targets(pos):
    """every key at short positions; beyond, the keys at the kernels' loop edges, both ends and the new key"""
    if pos <= 40:
        return list(range(pos + 1))
    edges = {0, 1, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 191, 192, 193, 255, 256, 383, 384, 385, pos - 192, pos - 2, pos - 1, pos}
    return sorted(t for t in edges if 0 <= t <= pos)


CASES = [(pos, _targets(pos)) for pos in S.POSITIONS] + [(S.LONG_POS, S.LONG_TARGETS)]


def test_positions_cover_every_loop_edge():
    P = set(S.POSITIONS)
    assert set(range(10)) <= P and S.LMAX - 1 in P and max(P) < S.LMAX
    for m in list(range(32, 129, 32)) + list(range(64, 449, 64)):
        assert {m - 1, m, m + 1} <= P
    assert {191, 192, 193, 383, 384, 385} <= P                     # the ring of three 64-key chunks wraps at 192 and at 384
    assert S.LONG_POS < S.LONG_LMAX and {0, 1022, 1023} <= set(S.LONG_TARGETS) and set(range(0, 1024, 16)) <= set(S.LONG_TARGETS)


@pytest.mark.parametrize('nH', [1, 3, 8])
@pytest.mark.parametrize('L', [1, 5, 70])
def test_attention_restatement(nH, L):
    R, d = 6, 64 * nH
    q, K, V = _r(R, d, seed=L, s=1.5), _r(R, L, d, seed=L + 1, s=1.5), _r(R, L, d, seed=L + 2)
    heads = lambda t: t.reshape(R, -1, nH, 64).transpose(1, 2)
    plain = (F.softmax(heads(q[:, None]) @ heads(K).transpose(-1, -2) * 0.125, dim=-1) @ heads(V)).transpose(1, 2).reshape(R, d)
    assert _rel(S.ref_attn(q, K, V, nH), plain) < TOL
    assert _rel(S.ref_attn(q, K, V, nH, chunk=4), plain) < TOL
    # the identity maps and unit weights of the mutants change nothing
    idx = torch.arange(L)
    assert torch.equal(S.ref_attn(q, K, V, nH, ksrc=idx, vsrc=idx, weight=torch.ones(R, L, dtype=torch.float64)), S.ref_attn(q, K, V, nH))


def test_projection_restatement():
    x, g, b = _r(7, 512, seed=1, s=2.0), 1 + 0.1 * _r(512, seed=2), 0.1 * _r(512, seed=3)
    W, bias = _r(1536, 512, seed=4, s=0.07), _r(1536, seed=5)
    assert _rel(S.ref_fused_qkv(x, g, b, W, bias, False), F.linear(F.layer_norm(x, (512,), g, b, 1e-5), W, bias)) < TOL
    word, pos = _r(9, 512, seed=6), _r(512, seed=7, s=0.5)
    tok = torch.tensor([3, 0, 8], dtype=torch.int32)
    assert _rel(S.ref_embed(word, pos, tok, g, b), F.layer_norm(word[[3, 0, 8]] + pos, (512,), g, b, 1e-5)) < TOL
    # with rounding on: bf16 values, one rounding of LN1 and one of the sum
    y = S.ref_fused_qkv(x, g, b, W, bias, True)
    assert _is_bf16(y)
    ln = F.layer_norm(x, (512,), g, b, 1e-5).to(torch.bfloat16).double()
    assert torch.equal(y, (ln @ W.T + bias).to(torch.bfloat16).double())


def test_patterns():
    q = S.q_dir(512)
    assert (q.abs() == 1).all() and all(0 < (q[h * 64:(h + 1) * 64] > 0).sum() < 64 for h in range(8))
    u = S.u_pat(list(range(1100)), 512)
    assert (u != 0).all() and (u.abs() <= 17).all() and (u == u.round()).all() and _is_bf16(u)
    v = S.v_pat(list(range(1024)), 512)
    assert (v != 0).all() and (v.abs() <= 7).all() and _is_bf16(v)
    for h in (0, 7):                         # two keys differ in sign in at least 6 dimensions of a head: by 2 / 7 of the largest value
        s = torch.sign(v[:, h * 64:(h + 1) * 64])
        same = s @ s.T
        assert (same - 64 * torch.eye(1024, dtype=torch.float64)).max().item() <= 64 - 2 * 6


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('pos,targets', CASES)
def test_walks_give_the_stated_outputs(pos, targets, shared):
    """bf16 rounding on: the uniform walk returns bf16(u / (pos + 1)) (shared: (u + w) / (pos + 1), the last row w / (pos + 1)), the peaked
    walk V[target]; the peaked target leads every other key by at least 30; all planted values are exact in bf16"""
    d = 64
    pu, pp = S.plant_uniform(pos, targets, d, shared), S.plant_peaked(pos, targets, d, shared)
    for p in (pu, pp):
        assert all(_is_bf16(t) for t in (p.q, p.kn, p.vn, p.Kc, p.Vc))
        if shared:
            assert all(bool((t == t[:1]).all()) for t in (p.q, p.kn, p.vn))
    K, V = pu.all_keys()
    assert (K == 0).all()
    hit = torch.zeros(len(targets), pos + 1, dtype=torch.bool)
    hit[torch.arange(len(targets)), torch.tensor(targets)] = True
    if not shared:
        assert (V[~hit] == 0).all() and torch.equal(V[hit], S.u_pat(list(range(len(targets))), d))
        assert torch.equal(S.want_uniform(pu, False), S.u_pat(list(range(len(targets))), d) / (pos + 1))
    got = S.ref_attn(pu.q, K, V, 1, bf=True)
    assert torch.equal(got, S.want_uniform(pu, shared).to(torch.bfloat16).double())
    # the kernels' own fp32 arithmetic (u * (1.0f / n) and u / n) lands within the fp32 gate of the stated value
    w32 = S.want_uniform(pu, shared)
    n = torch.tensor(float(pos + 1), dtype=torch.float32)
    u32 = (w32 * (pos + 1)).float()
    assert _rel((u32 * (1.0 / n)).double(), w32) < 2e-7 and _rel((u32 / n).double(), w32) < 1e-7
    K, V = pp.all_keys()
    s = torch.einsum('rd,rld->rl', pp.q * 0.125, K)
    lead = s[hit] - s.masked_fill(hit, -1e9).amax(-1) if pos > 0 else torch.full((1,), 64.0)
    assert lead.min().item() >= 30
    assert torch.equal(S.ref_attn(pp.q, K, V, 1, bf=True), S.want_peaked(pp))
    assert S.head_rel(S.ref_attn(pp.q, K, V, 1), S.want_peaked(pp), 1).max().item() < 1e-10
    assert torch.equal(S.want_peaked(pp), S.v_pat(targets, d))


def test_walks_with_eight_heads():
    for shared in (False, True):
        pu, pp = S.plant_uniform(65, list(range(66)), 512, shared), S.plant_peaked(65, list(range(66)), 512, shared)
        assert torch.equal(S.ref_attn(pu.q, *pu.all_keys(), 8, bf=True), S.want_uniform(pu, shared).to(torch.bfloat16).double())
        assert torch.equal(S.ref_attn(pp.q, *pp.all_keys(), 8, bf=True), S.want_peaked(pp))
        if shared:
            row = S.fused_bias_row(pp)
            assert row.shape == (1536,) and _is_bf16(row)


def _mutants(pos, targets):
    """name -> (kwargs of ref_attn, applies at this position)"""
    R, L = len(targets), pos + 1
    hit = torch.zeros(R, L, dtype=torch.float64)
    hit[torch.arange(R), torch.tensor(targets)] = 1.0
    j = torch.arange(L)
    new = torch.ones(R, L, dtype=torch.float64)
    new[:, pos] = 0.0
    stale = torch.where(j >= 192, j - 192, j)
    return {
        'drop the target key': (dict(weight=1.0 - hit), True),
        'take the target key twice': (dict(weight=1.0 + hit), pos >= 1),       # at pos 0 the only key has weight 1 whatever it counts
        'K one key off': (dict(ksrc=(j + 1) % L), pos >= 1),
        'chunk c reads the keys of chunk c - 3': (dict(ksrc=stale, vsrc=stale), pos >= 192),   # there is no chunk 3 below position 192
        'skip the new key': (dict(weight=new), True),
    }


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('pos,targets', CASES)
def test_mutants_break_the_walk_gates(pos, targets, shared):
    d = 64
    pu, pp = S.plant_uniform(pos, targets, d, shared), S.plant_peaked(pos, targets, d, shared)
    wu, wp = S.want_uniform(pu, shared), S.want_peaked(pp)
    for p, w in ((pu, wu), (pp, wp)):
        assert S.head_rel(S.ref_attn(p.q, *p.all_keys(), 1), w, 1).max().item() < 1e-10       # unharmed: far inside both gates
    for name, (kw, applies) in _mutants(pos, targets).items():
        if not applies:
            continue
        e = max(S.head_rel(S.ref_attn(p.q, *p.all_keys(), 1, **kw), w, 1).max().item() for p, w in ((pu, wu), (pp, wp)))
        assert e >= WIDE, (name, e)
        assert e >= 50 * max(S.WALK_GATE.values())


def test_gates_are_the_stated_ones():
    assert S.WALK_GATE == {torch.bfloat16: 2.0 ** -8, torch.float32: 1e-6}
    assert S.GATE == {torch.float32: 2e-5, torch.bfloat16: 3e-2} and S.LN_GATE == 2e-5
    assert S.PROJ_R == (1, 2, 3, 4, 5, 8, 13, 63) and S.PROJ_POS == (0, 63, 64, 200) and S.RANDOM_R == (1, 3, 4, 5, 70)


def test_ramps_reach_eighty_and_move_the_maximum():
    for dt in (torch.float32, torch.bfloat16):
        for pos in S.RAMP_POS:
            for rising in (True, False):
                p = S.plant_ramp(pos, 2, rising, dt, d=64)
                K, _ = p.all_keys()
                s = torch.einsum('d,ld->l', p.q[0] * 0.125, K[0])
                assert abs(s.max().item() - 80) < 1 and s.min().item() == 0
                step = s[1:] - s[:-1]
                assert (step >= 0).all() if rising else (step <= 0).all()
                if dt == torch.float32:
                    assert (step > 0).all() if rising else (step < 0).all()         # the running maximum changes at every key / never
                assert torch.equal(p.Kc, p.Kc.to(dt).double()) and torch.equal(p.Vc, p.Vc.to(dt).double())


def test_bf16_steps_and_settle():
    one = torch.tensor([1.0, 1.0 + 2.0 ** -7, 1.0 - 2.0 ** -8, 3.0, 1e-6], dtype=torch.float64)
    assert S.bf16_steps(one.to(torch.bfloat16), one) == 0
    assert S.bf16_steps(torch.tensor([1.0 + 2.0 ** -7]).to(torch.bfloat16), torch.tensor([1.0], dtype=torch.float64)) == 1.0
    assert S.bf16_steps(torch.tensor([1.0 + 2.0 ** -6]).to(torch.bfloat16), torch.tensor([1.0], dtype=torch.float64)) == 2.0
    assert S.bf16_steps(torch.tensor([3e-5]).to(torch.bfloat16), torch.tensor([0.0], dtype=torch.float64)) > 1.0      # the floor is 2e-5
    tie = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 1e-4, 2.0 ** -12 * (1 + 2.0 ** -8)], dtype=torch.float64)
    assert S.near_tie(tie).tolist() == [True, False, False]
    g, b = 1 + 0.1 * _r(512, seed=2), 0.1 * _r(512, seed=3)
    x0 = _r(63, 512, seed=9).float().double()
    fn = lambda v: S.ref_ln(v, g, b)
    assert S.near_tie(fn(x0)).any()                       # unsettled random rows do hold such elements
    x = S.settle(x0, fn)
    assert not S.near_tie(fn(x)).any() and torch.equal(x, x.float().double()) and (x - x0).abs().max().item() <= 0.1
