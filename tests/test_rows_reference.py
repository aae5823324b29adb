"""The float64 restatements of the row-owner chains (tests/gpu_checks_rows.py ref_*, rounding off) against the oracle
(oracle/omniparser_ref.py) in float64: the prediction head, one pre-norm decoder layer (its attention cores from the oracle's mha) and one
shifted-window Swin block (its window attention from the oracle).  Without this a wrong restatement could pass against an equally wrong
kernel.  CPU only."""
import torch

from oracle import omniparser_ref as O
from tests import gpu_checks_rows as R

d, ff, nH = 512, 2048, 8
TOL = 1e-12   # float64 against float64: only the summation order differs


def _r(*shape, seed, s=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * s


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _layer_sd(p, seed):
    sd = {}
    for i, n in enumerate(('norm1', 'norm2', 'norm3')):
        sd[p + n + '.weight'] = 1 + _r(d, seed=seed + i, s=0.1)
        sd[p + n + '.bias'] = _r(d, seed=seed + 10 + i, s=0.1)
    for i, a in enumerate(('self_attn.', 'multihead_attn.')):
        sd[p + a + 'in_proj_weight'] = _r(3 * d, d, seed=seed + 20 + i) / d ** 0.5
        sd[p + a + 'in_proj_bias'] = _r(3 * d, seed=seed + 30 + i, s=0.1)
        sd[p + a + 'out_proj.weight'] = _r(d, d, seed=seed + 40 + i) / d ** 0.5
        sd[p + a + 'out_proj.bias'] = _r(d, seed=seed + 50 + i, s=0.1)
    sd[p + 'linear1.weight'], sd[p + 'linear1.bias'] = _r(ff, d, seed=seed + 60) / d ** 0.5, _r(ff, seed=seed + 61, s=0.1)
    sd[p + 'linear2.weight'], sd[p + 'linear2.bias'] = _r(d, ff, seed=seed + 62) / ff ** 0.5, _r(d, seed=seed + 63, s=0.1)
    return sd


def _core(q, k, v, **kw):
    """the attention core of the oracle's mha (in_proj and out_proj set to identity): softmax(q k^T / sqrt(hd) + masks) v"""
    E = q.shape[-1]
    eye = torch.eye(E, dtype=torch.float64)
    sd = {'in_proj_weight': torch.cat([eye, eye, eye]), 'in_proj_bias': torch.zeros(3 * E, dtype=torch.float64),
          'out_proj.weight': eye, 'out_proj.bias': torch.zeros(E, dtype=torch.float64)}
    return O.mha(sd, '', q, k, v, nH, **kw)


def test_head_restatement():
    kind, V = 'pt', 1108
    p = 'transformer.%s_pred_layer.layers.' % kind
    sd = {'transformer.%s_decoder.norm.weight' % kind: 1 + _r(d, seed=1, s=0.1), 'transformer.%s_decoder.norm.bias' % kind: _r(d, seed=2, s=0.1)}
    for i, n in enumerate((d, d, V)):
        sd[p + '%d.weight' % i] = _r(n, d, seed=10 + i) / d ** 0.5
        sd[p + '%d.bias' % i] = _r(n, seed=20 + i, s=0.1)
    x = _r(37, d, seed=3, s=2.0)
    ref = O.head(sd, kind, O._ln(x, sd, 'transformer.%s_decoder.norm' % kind))
    got = R.ref_head_tail(x, sd['transformer.%s_decoder.norm.weight' % kind], sd['transformer.%s_decoder.norm.bias' % kind],
                          [sd[p + '%d.weight' % i] for i in range(3)], [sd[p + '%d.bias' % i] for i in range(3)], False)
    assert _rel(got, ref) < TOL


def test_decoder_layer_restatement():
    """embedding -> qkv tail -> self-attention core -> mid chain -> cross-attention core on the memory projection -> ffn chain, position by
    position, against O.embed and O.decoder_layer (pre-norm); and the next layer's qkv tail against the oracle's own in_proj of norm1"""
    kind, V, L, N, M = 'pt', 1104, 5, 6, 23
    p, pn = 'transformer.pt_decoder.layers.0.', 'transformer.pt_decoder.layers.1.'
    sd = _layer_sd(p, 100)
    sd.update(_layer_sd(pn, 200))
    sd['transformer.embedding.word_embeddings.weight'] = _r(V, d, seed=1)
    sd['transformer.embedding.pt_position_embeddings.weight'] = _r(R.P, d, seed=2, s=0.5)
    sd['transformer.embedding.LayerNorm.weight'] = 1 + _r(d, seed=3, s=0.1)
    sd['transformer.embedding.LayerNorm.bias'] = _r(d, seed=4, s=0.1)
    seq = torch.randint(0, V, (N, L), generator=torch.Generator().manual_seed(5))
    seq[0, 0], seq[1, 0] = 0, V - 1
    x_or, qpos = O.embed(sd, seq, kind)                                    # (N, L, d)
    ptab = sd['transformer.embedding.pt_position_embeddings.weight']
    xs = torch.stack([R.ref_embed(seq[:, t], sd['transformer.embedding.word_embeddings.weight'], ptab, t, sd['transformer.embedding.LayerNorm.weight'],
                                  sd['transformer.embedding.LayerNorm.bias']) for t in range(L)])          # (L, N, d)
    assert _rel(xs, x_or.transpose(0, 1)) < TOL
    memory, mpos = _r(M, N, d, seed=6), _r(M, N, d, seed=7, s=0.5)
    kpm = torch.zeros(N, M, dtype=torch.bool)
    kpm[-1, -4:] = True
    tmask = O.causal_mask(L)
    x_ref = O.decoder_layer(sd, p, xs, memory, kpm, mpos, qpos.transpose(0, 1), tmask, nH, True)

    def tab(pp, t):   # bias_tab[t] of a layer: in_proj bias + the position term of q and k
        W, b = sd[pp + 'self_attn.in_proj_weight'], sd[pp + 'self_attn.in_proj_bias']
        return b + torch.cat([ptab[t] @ W[:d].T, ptab[t] @ W[d:2 * d].T, torch.zeros(d, dtype=torch.float64)])
    qkv = torch.stack([R.ref_qkv_tail(xs[t], sd[p + 'norm1.weight'], sd[p + 'norm1.bias'], sd[p + 'self_attn.in_proj_weight'], tab(p, t), False)
                       for t in range(L)])
    sa = _core(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], attn_mask=tmask)
    Wca = sd[p + 'multihead_attn.in_proj_weight']
    qtab = sd[p + 'multihead_attn.in_proj_bias'][:d] + ptab @ Wca[:d].T
    mid = [R.ref_mid(xs[t], sa[t], sd[p + 'self_attn.out_proj.weight'], sd[p + 'self_attn.out_proj.bias'], sd[p + 'norm2.weight'],
                     sd[p + 'norm2.bias'], Wca[:d], qtab, t, False) for t in range(L)]
    x1, qca = torch.stack([m[0] for m in mid]), torch.stack([m[1] for m in mid])
    K, Vv = R.ref_kv((memory + mpos).reshape(M * N, d), memory.reshape(M * N, d), Wca[d:2 * d], sd[p + 'multihead_attn.in_proj_bias'][d:2 * d],
                     Wca[2 * d:], sd[p + 'multihead_attn.in_proj_bias'][2 * d:], False)
    ca = _core(qca, K.reshape(M, N, d), Vv.reshape(M, N, d), key_padding_mask=kpm)
    x2 = torch.stack([R.ref_ffn_body(x1[t], ca[t], sd[p + 'multihead_attn.out_proj.weight'], sd[p + 'multihead_attn.out_proj.bias'],
                                     sd[p + 'norm3.weight'], sd[p + 'norm3.bias'], sd[p + 'linear1.weight'], sd[p + 'linear1.bias'],
                                     sd[p + 'linear2.weight'], sd[p + 'linear2.bias'], False) for t in range(L)])
    assert _rel(x2, x_ref) < TOL
    # the ffn chain's q | k | v tail = the next layer's in_proj of (norm1(x) + qpos) for q, k and of norm1(x) for v
    y = O._ln(x_ref, sd, pn + 'norm1')
    Wn, bn = sd[pn + 'self_attn.in_proj_weight'], sd[pn + 'self_attn.in_proj_bias']
    qp = qpos.transpose(0, 1)
    want = torch.cat([(y + qp) @ Wn[:d].T + bn[:d], (y + qp) @ Wn[d:2 * d].T + bn[d:2 * d], y @ Wn[2 * d:].T + bn[2 * d:]], -1)
    got = torch.stack([R.ref_qkv_tail(x2[t], sd[pn + 'norm1.weight'], sd[pn + 'norm1.bias'], Wn, tab(pn, t), False) for t in range(L)])
    assert _rel(got, want) < TOL


def _rel_index(ws):
    c = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing='ij')).flatten(1)
    r = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (ws - 1)
    return r[..., 0] * (2 * ws - 1) + r[..., 1]


def test_swin_block_restatement():
    """mode 0 (norm1 + qkv), then mode 1 (+ next block's qkv) on the oracle's window attention, against O.swin_block (shifted windows)"""
    C, nHs, ws, shift, H, W, B = 512, 16, 7, 3, 14, 14, 2
    p, pn = 'b.0.', 'b.1.'
    sd = {}
    for j, pp in enumerate((p, pn)):
        s = 1000 * (j + 1)
        sd[pp + 'norm1.weight'], sd[pp + 'norm1.bias'] = 1 + _r(C, seed=s + 1, s=0.1), _r(C, seed=s + 2, s=0.1)
        sd[pp + 'norm2.weight'], sd[pp + 'norm2.bias'] = 1 + _r(C, seed=s + 3, s=0.1), _r(C, seed=s + 4, s=0.1)
        sd[pp + 'attn.qkv.weight'], sd[pp + 'attn.qkv.bias'] = _r(3 * C, C, seed=s + 5) / C ** 0.5, _r(3 * C, seed=s + 6, s=0.1)
        sd[pp + 'attn.proj.weight'], sd[pp + 'attn.proj.bias'] = _r(C, C, seed=s + 7) / C ** 0.5, _r(C, seed=s + 8, s=0.1)
        sd[pp + 'attn.relative_position_bias_table'] = _r((2 * ws - 1) ** 2, nHs, seed=s + 9, s=0.5)
        sd[pp + 'attn.relative_position_index'] = _rel_index(ws)
        sd[pp + 'mlp.fc1.weight'], sd[pp + 'mlp.fc1.bias'] = _r(4 * C, C, seed=s + 10) / C ** 0.5, _r(4 * C, seed=s + 11, s=0.1)
        sd[pp + 'mlp.fc2.weight'], sd[pp + 'mlp.fc2.bias'] = _r(C, 4 * C, seed=s + 12) / (4 * C) ** 0.5, _r(C, seed=s + 13, s=0.1)
    x = _r(B, H * W, C, seed=7, s=2.0)
    mask = O.shift_mask(H, W, ws, shift).double()
    ref = O.swin_block(sd, p, x, H, W, nHs, ws, shift, mask)
    # mode 0 = the oracle's first step of the window attention
    qkv = R.ref_qkv_tail(x, sd[p + 'norm1.weight'], sd[p + 'norm1.bias'], sd[p + 'attn.qkv.weight'], sd[p + 'attn.qkv.bias'], False)
    want = O._ln(x, sd, p + 'norm1') @ sd[p + 'attn.qkv.weight'].T + sd[p + 'attn.qkv.bias']
    assert _rel(qkv, want) < TOL
    # the attention core with its output projection set to identity (and the MLP to zero): what the chain's att input is
    core_sd = dict(sd)
    core_sd[p + 'attn.proj.weight'] = torch.eye(C, dtype=torch.float64)
    core_sd[p + 'attn.proj.bias'] = torch.zeros(C, dtype=torch.float64)
    core_sd[p + 'mlp.fc2.weight'] = torch.zeros(C, 4 * C, dtype=torch.float64)
    core_sd[p + 'mlp.fc2.bias'] = torch.zeros(C, dtype=torch.float64)
    att = O.swin_block(core_sd, p, x, H, W, nHs, ws, shift, mask) - x
    x2 = R.ref_ffn_body(x, att, sd[p + 'attn.proj.weight'], sd[p + 'attn.proj.bias'], sd[p + 'norm2.weight'], sd[p + 'norm2.bias'],
                        sd[p + 'mlp.fc1.weight'], sd[p + 'mlp.fc1.bias'], sd[p + 'mlp.fc2.weight'], sd[p + 'mlp.fc2.bias'], False, act='gelu')
    assert _rel(x2, ref) < 1e-10   # (x + core) - x: the core's bits below x's ulp are gone
    nq = R.ref_qkv_tail(x2, sd[pn + 'norm1.weight'], sd[pn + 'norm1.bias'], sd[pn + 'attn.qkv.weight'], sd[pn + 'attn.qkv.bias'], False)
    want = O._ln(ref, sd, pn + 'norm1') @ sd[pn + 'attn.qkv.weight'].T + sd[pn + 'attn.qkv.bias']
    assert _rel(nq, want) < 1e-10


def test_rounding_switch():
    """bf=True rounds where the bf16 chains round, bf=False is exact; the V^T slot map is a permutation of the 32 keys"""
    x = R._randn(8, d, seed=1)
    assert torch.equal(R.rb(x, False), x)
    assert torch.equal(R.rb(x, True), x.to(torch.bfloat16).double())
    assert sorted(R.vt_slot(torch.arange(32)).tolist()) == list(range(32))
    xs, att = R.edge_rows(3, R._vec(4, d))
    assert torch.isfinite(xs).all() and torch.isfinite(att).all()
    y = xs[1] + R._vec(4, d)                         # the planted constant LayerNorm input
    assert y.var(unbiased=False).item() < 1e-12
    y2 = xs[2] + R._vec(4, d)
    assert y2.var(unbiased=False).item() < R.EPS


def test_pos_mod_comparison_notices_a_launch_at_one_position():
    """compare_pos_mod (the mid chain with a position per row, tests/gpu_checks_rows.py): exact on a fake launch that gives row r its row of
    the one-position result at r % L; failing when every row got *d_pos, whatever L -- the check parks d_pos at a position no row sits at --
    and when the position is taken from the source row instead of the launch's row.  ref_mid_rows is ref_mid row by row."""
    NB, Pn = R.NB, 9
    W = {k: _r(d, d, seed=i, s=d ** -0.5) for i, k in enumerate(('Wo', 'Wq'))}
    W.update(bo=_r(d, seed=3, s=0.1), g2=1 + _r(d, seed=4, s=0.1), b2=_r(d, seed=5, s=0.1), qtab=_r(Pn, d, seed=6, s=0.3))
    x, att = _r(NB, d, seed=7), _r(NB, d, seed=8).to(torch.bfloat16).double()
    per_pos = [R.ref_mid(x, att, W['Wo'], W['bo'], W['g2'], W['b2'], W['Wq'], W['qtab'], p, True) for p in range(Pn)]
    x0 = per_pos[0][0].float()
    qpos = torch.stack([q.to(torch.bfloat16) for _, q in per_pos])
    rx, rq = R.ref_mid_rows(W, x[:20], att[:20], [r % 7 for r in range(20)])
    assert _rel(rx, per_pos[0][0][:20]) < TOL
    assert all(torch.equal(rq[r], per_pos[r % 7][1][r]) for r in range(20))
    assert not torch.equal(rq[1], per_pos[0][1][1])
    for L in (1, 2, 6, 7):
        for Rn in (1, 17, 200, 300):
            src = (torch.arange(Rn) * 101 + 13) % NB
            pos = torch.arange(Rn) % L
            ok = lambda got: all(r['ok'] for r in _cmp(got, src, L, x0, qpos))      # noqa: E731
            assert ok(dict(x=x0[src], q=qpos[pos, src]))
            assert not ok(dict(x=x0[src], q=qpos[torch.full((Rn,), Pn - 1), src]))                 # *d_pos for every row
            if L > 1 and Rn > 1:
                assert not ok(dict(x=x0[src], q=qpos[torch.zeros(Rn, dtype=torch.int64), src]))    # ... at d_pos = 0
            if L > 1 and Rn > L:
                assert not ok(dict(x=x0[src], q=qpos[src % L, src]))                               # the source row's index, not the launch's
            assert not ok(dict(x=x0[src] + 1e-3, q=qpos[pos, src]))


def _cmp(got, src, L, x0, qpos):
    out = []
    R.compare_pos_mod(out, 'fake', got, [], src, L, x0, qpos)
    return out
