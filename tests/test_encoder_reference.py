"""The float64 restatements of the Swin encoder kernels (tests/gpu_checks_encoder.py ref_*, rounding off) against the oracle
(oracle/omniparser_ref.py) in float64, at padded, shifted and odd shapes: the attention half and the MLP half of a Swin block (O.swin_block
with the other half switched off, the oracle's own shift_mask), patch embedding, patch merging and the LayerNorm.  Without this a wrong
restatement could pass against an equally wrong kernel.  CPU only."""
import pytest
import torch

from oracle import omniparser_ref as O
from tests import gpu_checks_encoder as E

TOL = 1e-12   # float64 against float64: only the summation order differs
WS = 7


def _r(*shape, seed, s=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * s


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _block_sd(C, nH, seed):
    p = 'b.'
    sd = {p + 'norm1.weight': 1 + _r(C, seed=seed + 1, s=0.1), p + 'norm1.bias': _r(C, seed=seed + 2, s=0.1),
          p + 'norm2.weight': 1 + _r(C, seed=seed + 3, s=0.1), p + 'norm2.bias': _r(C, seed=seed + 4, s=0.1),
          p + 'attn.qkv.weight': _r(3 * C, C, seed=seed + 5) / C ** 0.5, p + 'attn.qkv.bias': _r(3 * C, seed=seed + 6, s=0.3),
          p + 'attn.proj.weight': _r(C, C, seed=seed + 7) / C ** 0.5, p + 'attn.proj.bias': _r(C, seed=seed + 8, s=0.1),
          p + 'attn.relative_position_bias_table': _r(169, nH, seed=seed + 9, s=0.5),
          p + 'attn.relative_position_index': E.rel_index(),
          p + 'mlp.fc1.weight': _r(4 * C, C, seed=seed + 10) / C ** 0.5, p + 'mlp.fc1.bias': _r(4 * C, seed=seed + 11, s=0.1),
          p + 'mlp.fc2.weight': _r(C, 4 * C, seed=seed + 12) / (4 * C) ** 0.5, p + 'mlp.fc2.bias': _r(C, seed=seed + 13, s=0.1)}
    return p, sd


SHAPES = [(1, 1), (2, 12), (6, 11), (8, 8), (10, 7), (7, 7), (13, 1), (17, 20)]


@pytest.mark.parametrize('shift', [0, 3])
@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('C,nH', [(128, 4), (96, 3), (192, 6)])
def test_attn_block_restatement(C, nH, H, W, shift):
    """ref_attn_block (LN, qkv, ref_window_attn with padding tokens = the bias, SW-MSA regions, proj, residual) == O.swin_block with its
    MLP switched off"""
    p, sd = _block_sd(C, nH, 10 * H + W + C)
    sd[p + 'mlp.fc2.weight'] = torch.zeros(C, 4 * C, dtype=torch.float64)
    sd[p + 'mlp.fc2.bias'] = torch.zeros(C, dtype=torch.float64)
    B = 2
    x = _r(B, H * W, C, seed=7, s=1.5)
    E.plant_edge_tokens(x.view(B, H, W, C), shift, 5)
    mask = O.shift_mask(H, W, WS, shift).double() if shift else None
    ref = O.swin_block(sd, p, x, H, W, nH, WS, shift, mask)
    got = E.ref_attn_block(x.reshape(B, H, W, C), sd[p + 'norm1.weight'], sd[p + 'norm1.bias'], sd[p + 'attn.qkv.weight'], sd[p + 'attn.qkv.bias'],
                           sd[p + 'attn.relative_position_bias_table'], sd[p + 'attn.proj.weight'], sd[p + 'attn.proj.bias'], nH, shift, False)
    assert _rel(got.reshape(B, H * W, C) - x, ref - x) < 1e-10   # (x + att) - x: att's bits below x's ulp are gone
    assert _rel(got.reshape(B, H * W, C), ref) < TOL


@pytest.mark.parametrize('shift', [0, 3])
@pytest.mark.parametrize('H,W', [(2, 12), (8, 8), (13, 1), (17, 20)])
def test_window_attn_restatement(H, W, shift):
    """ref_window_attn from a qkv map (attention edges planted: uniform, +80 key, mask-decided window) == the oracle's partition /
    shift_mask / unpartition path around _oracle_core, a copy of O.window_attention's lines between the qkv and proj Linears (the oracle
    function itself starts from C-channel tokens, not from a qkv map).  The copy is not the pin: test_attn_block_restatement pins the same
    restatement through O.swin_block, which calls O.window_attention itself; this test adds the planted attention edges."""
    nH, C = 4, 128
    qkv, bqkv, table = E.attn_inputs(2, H, W, nH, shift, torch.float32, 3)
    got = E.ref_window_attn(qkv, bqkv, table, nH, shift, False)
    Hp, Wp = E.padded(H, W)
    full = bqkv.reshape(1, 1, 1, 3 * C).expand(2, Hp, Wp, 3 * C).clone()
    full[:, :H, :W] = qkv
    if shift:
        full = torch.roll(full, (-shift, -shift), (1, 2))
    win = O.partition(full, WS).reshape(-1, WS * WS, 3 * C)
    sd = {'a.relative_position_bias_table': table, 'a.relative_position_index': E.rel_index()}
    mask = O.shift_mask(H, W, WS, shift).double() if shift else None
    o = _oracle_core(sd, win, nH, C, mask)
    y = O.unpartition(o.reshape(-1, WS, WS, C), WS, Hp, Wp)
    if shift:
        y = torch.roll(y, (shift, shift), (1, 2))
    assert _rel(got, y[:, :H, :W]) < TOL


def _oracle_core(sd, win, nH, C, mask):
    """O.window_attention on a [nW*B, 49, 3C] map whose q | k | v are given (identity qkv), proj = identity on C"""
    Bw, N, C3 = win.shape
    qkv = win.reshape(Bw, N, 3, nH, C // nH).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * (C // nH) ** -0.5, qkv[1], qkv[2]
    att = q @ k.transpose(-2, -1)
    bias = sd['a.relative_position_bias_table'][sd['a.relative_position_index'].reshape(-1)].reshape(N, N, nH).permute(2, 0, 1)
    att = att + bias[None]
    if mask is not None:
        nW = mask.shape[0]
        att = (att.reshape(Bw // nW, nW, nH, N, N) + mask[None, :, None]).reshape(-1, nH, N, N)
    return (att.softmax(-1) @ v).transpose(1, 2).reshape(Bw, N, C)


@pytest.mark.parametrize('C', [128, 256, 512])
def test_mlp_restatement(C):
    """ref_mlp == O.swin_block with its attention half switched off (proj = 0), edge rows included"""
    p, sd = _block_sd(C, C // 32, C)
    sd[p + 'attn.proj.weight'] = torch.zeros(C, C, dtype=torch.float64)
    sd[p + 'attn.proj.bias'] = torch.zeros(C, dtype=torch.float64)
    x = E.edge_rows(C, 3)[:49].reshape(1, 49, C)
    ref = O.swin_block(sd, p, x, 7, 7, C // 32, WS, 0, None)
    got = E.ref_mlp(x, sd[p + 'norm2.weight'], sd[p + 'norm2.bias'], sd[p + 'mlp.fc1.weight'], sd[p + 'mlp.fc1.bias'], sd[p + 'mlp.fc2.weight'],
                    sd[p + 'mlp.fc2.bias'], False)
    assert _rel(got, ref) < TOL


@pytest.mark.parametrize('E_', [96, 128, 192])
@pytest.mark.parametrize('H,W', [(16, 18), (13, 15), (14, 16), (15, 17), (1, 1), (3, 2)])
def test_patch_embed_restatement(E_, H, W):
    pfx = 'backbone.0.patch_embed.'
    sd = {pfx + 'proj.weight': _r(E_, 3, 4, 4, seed=1, s=0.2), pfx + 'proj.bias': _r(E_, seed=2, s=0.1),
          pfx + 'norm.weight': 1 + _r(E_, seed=3, s=0.1), pfx + 'norm.bias': _r(E_, seed=4, s=0.1)}
    img = _r(3, 3, H, W, seed=5)
    img[1] = 0.0
    ref, Hp, Wp = O.patch_embed(sd, img)
    got = E.ref_patch_embed(img, sd[pfx + 'proj.weight'].reshape(E_, 48), sd[pfx + 'proj.bias'], sd[pfx + 'norm.weight'], sd[pfx + 'norm.bias'])
    assert (Hp, Wp) == (-(-H // 4), -(-W // 4))
    assert _rel(got, ref) < TOL


@pytest.mark.parametrize('C', [96, 128])
@pytest.mark.parametrize('H,W', [(9, 13), (1, 5), (6, 1), (7, 7), (10, 12), (1, 1)])
def test_patch_merge_restatement(C, H, W):
    sd = {'d.norm.weight': 1 + _r(4 * C, seed=1, s=0.1), 'd.norm.bias': _r(4 * C, seed=2, s=0.1), 'd.reduction.weight': torch.eye(4 * C, dtype=torch.float64)}
    x = _r(2, H * W, C, seed=3)
    ref = O.patch_merging(sd, 'd.', x, H, W)
    got = E.ref_patch_merge(x.reshape(2, H, W, C), sd['d.norm.weight'], sd['d.norm.bias'])
    assert _rel(got.reshape(ref.shape), ref) < TOL


@pytest.mark.parametrize('C', [96, 128, 768, 1024])
def test_layernorm_restatement(C):
    x = E.edge_rows(C, 9)
    sd = {'n.weight': 1 + _r(C, seed=1, s=0.1), 'n.bias': _r(C, seed=2, s=0.1)}
    assert (E.row_rel(E.ln64(x, sd['n.weight'], sd['n.bias']), O._ln(x, sd, 'n')).max() < TOL).item()


def test_inputs_reach_the_edges():
    """the planted attention edges and LayerNorm edges are what the docstrings say"""
    H, W, nH, shift = 8, 13, 4, 3
    qkv, bqkv, table = E.attn_inputs(2, H, W, nH, shift, torch.bfloat16, 3)
    assert torch.equal(qkv, qkv.to(torch.bfloat16).double())
    assert (table[:, nH - 1] == 0).all()
    # uniform window: head nH - 1 of shifted window (0, 0) has zero q, hence equal scores
    Hp, Wp = E.padded(H, W)
    y, x = shift % Hp, shift % Wp
    assert (qkv[0, y, x, (nH - 1) * 32:nH * 32] == 0).all()
    # the +80 key: the softmax of head 0 in the last window is dominated by one key
    C = nH * 32
    q0 = qkv[0, :, :, :32].reshape(-1, 32)
    k0 = qkv[0, :, :, C:C + 32].reshape(-1, 32)
    s = (q0 @ k0.T) * E.SCALE
    assert s.max().item() > 70.0
    x = E.edge_rows(128, 1)
    v = x.var(-1, unbiased=False)
    assert v[1].item() == 0.0 and 0 < v[2].item() < E.EPS and (x[0] == 0).all()
    assert all(0 <= a < H and 0 <= b < W for a, b in E.edge_coords(H, W, shift))
    # both sides of every region boundary of the shifted grid are planted
    sy = {(a - shift) % Hp for a, _ in E.edge_coords(H, W, shift)}
    pad = {(a - shift) % Hp for a in range(H, Hp)}   # padding rows (no token to plant)
    assert {Hp - 8, Hp - 7, Hp - 4, Hp - 3} <= sy | pad


def test_region_ids_match_the_oracle_mask():
    for H, W in SHAPES:
        for shift in (1, 3):
            Hp, Wp = E.padded(H, W)
            ry, rx = E.region_ids(Hp, shift), E.region_ids(Wp, shift)
            rid = (ry[:, None] * 3 + rx[None, :]).double()
            w = O.partition(rid.reshape(1, Hp, Wp, 1), WS).reshape(-1, 49)
            mine = torch.where(w[:, :, None] != w[:, None, :], -100.0, 0.0)
            assert torch.equal(mine.float(), O.shift_mask(H, W, WS, shift).float())
