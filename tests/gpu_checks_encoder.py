"""The Swin encoder kernels at every window count, padding, shift and head count (csrc/swin_attn.hip, csrc/swin_block.hip, csrc/mlp.hip,
csrc/norm.hip).

Windows are image-local and rows are row-local, so every kernel is checked in two steps, as tests/gpu_checks_rows.py does for the row-owner
chains:
  * a BASE launch of a few distinct images (or 256 distinct rows) against a float64 restatement on the CPU, every element gated relative to
    its own window's (head's) max |ref| -- or its own row's -- not the tensor's; edge windows (the last window row / column of the padded
    grid: padding tokens and SW-MSA regions) and edge rows (the planted LayerNorm edges) are gated apart from the ordinary ones;
  * every larger launch builds its input on the device by gathering base images (rows) by a fixed index map src[b], and output image b must
    then be image src[b] of the base launch BIT FOR BIT (torch.equal on the device).  The window counts cross every persistent step of the
    walks (k * 64 - 1, k * 64, k * 64 + 1 windows up to past 4 * 512), so waves take 1 .. 65 windows, odd and even.  Each of those launches
    runs twice (identical bits), its inputs and outputs are buf[:R] views of buffers with 64 guard rows more: the output guard rows hold a
    sentinel that must survive, the input guard rows hold NaN that must not reach a valid token (padding tokens read row 0 of the input and
    then take the bias, so an out-of-range read shows up as NaN).  The in-place kernels must give the out-of-place bits in place.

The float64 restatements (ref_*) take `bf`: True rounds to bf16 exactly where the bf16 kernels round (LayerNorm output, q / k / v, P, the
attention output, the MLP hidden layer; the callers pass bf16-valued weights and inputs), False is exact float64.
tests/test_encoder_reference.py pins them, with bf=False, to oracle/omniparser_ref.py.

Every check returns rec / rrec records (tests/gpu_checks.py); the measured errors go to the parity report.
"""
import math
import os

import torch

from tests.gpu_checks import DEV, rec, rrec

WS, WT, HD = 7, 49, 32
EPS = 1e-5
SCALE = HD ** -0.5
GUARD = 64
NB = 256                            # distinct base rows of the row-local kernels
F32_NAN = 0x7FC0DEAD                # input guard rows (must not leak)
BF16_NAN = 0x7FA5
F32_SENT = 0x7FA5A5A5               # output guard rows (must survive)
BF16_SENT = 0x7F5A

# Gates, relative to each window's (head's) / row's own max |ref|, per (kernel, variant, group); 'interior' / 'random' = ordinary windows /
# rows, 'edge' = the last window row / column of the padded grid (padding tokens, SW-MSA regions) and the planted edge windows / rows.
# Each gate is about 3x the worst case measured on an MI355X (never more than 4x); (gate, measured) -- the measured value is also in the
# record's note.  The fused MLP on the fp32 stream and the fused attention blocks are gated relative to max |ref - x| (see row_rel /
# window_rel).  A gate of 0 is where the measured error is 0: every bf16 output equals the bf16 rounding of the float64 value (bf16-stream
# MLP edge rows, bf16 patch-embedding random tokens).  A floor of one bf16 ulp there would break the at-most-4x rule; a schedule change that
# flips one rounding must re-measure these gates, not loosen them silently.
TOL = {
    ('attn', 'mfma_expb_bf16', 'edge'): (1.5e-02, 4.76e-03),
    ('attn', 'mfma_expb_bf16', 'interior'): (1.9e-02, 6.33e-03),
    ('attn', 'mfma_expb_f32', 'edge'): (1.5e-05, 4.88e-06),
    ('attn', 'mfma_expb_f32', 'interior'): (3.2e-06, 1.05e-06),
    ('attn', 'mfma_f32_split', 'edge'): (2.3e-05, 7.48e-06),
    ('attn', 'mfma_f32_split', 'interior'): (1.9e-05, 6.24e-06),
    ('attn', 'mfma_table_bf16', 'edge'): (1.2e-02, 3.73e-03),
    ('attn', 'mfma_table_bf16', 'interior'): (6.7e-03, 2.20e-03),
    ('attn', 'mfma_table_f32', 'edge'): (5.8e-06, 1.93e-06),
    ('attn', 'mfma_table_f32', 'interior'): (2.7e-06, 8.94e-07),
    ('attn', 'scalar_bf16', 'edge'): (2.4e-02, 7.81e-03),
    ('attn', 'scalar_bf16', 'interior'): (2.4e-02, 7.75e-03),
    ('attn', 'scalar_f32', 'edge'): (6.9e-06, 2.27e-06),
    ('attn', 'scalar_f32', 'interior'): (2.8e-06, 9.32e-07),
    ('attn', 'x3_f32', 'edge'): (7.8e-05, 2.57e-05),
    ('attn', 'x3_f32', 'interior'): (7.4e-05, 2.47e-05),
    ('attn', 'x3_split', 'edge'): (7.9e-05, 2.63e-05),
    ('attn', 'x3_split', 'interior'): (8.7e-05, 2.89e-05),
    ('block', 128, 'edge'): (2.2e-02, 7.18e-03),
    ('block', 128, 'interior'): (2.3e-02, 7.47e-03),
    ('block', 256, 'edge'): (1.5e-02, 4.82e-03),
    ('block', 256, 'interior'): (1.8e-02, 5.69e-03),
    ('embed', 'generic_bf16_192', 'edge'): (2.8e-05, 9.04e-06),
    ('embed', 'generic_bf16_192', 'random'): (0.0, 0.0),
    ('embed', 'generic_f32_192', 'edge'): (9.3e-07, 3.08e-07),
    ('embed', 'generic_f32_192', 'random'): (1.1e-06, 3.56e-07),
    ('embed', 'mfma6', 'edge'): (1.1e-06, 3.38e-07),
    ('embed', 'mfma6', 'random'): (1.1e-06, 3.55e-07),
    ('embed', 'mfma8', 'edge'): (9.2e-07, 3.05e-07),
    ('embed', 'mfma8', 'random'): (2.1e-06, 6.99e-07),
    ('embed', 'tok_bf16_128', 'edge'): (1.6e-05, 5.09e-06),
    ('embed', 'tok_bf16_128', 'random'): (0.0, 0.0),
    ('embed', 'tok_f32_128', 'edge'): (1.1e-06, 3.66e-07),
    ('embed', 'tok_f32_128', 'random'): (1.4e-06, 4.43e-07),
    ('embed', 'tok_f32_96', 'edge'): (1.1e-06, 3.45e-07),
    ('embed', 'tok_f32_96', 'random'): (1.4e-06, 4.39e-07),
    ('ln', 'f32', 'edge'): (1.7e-04, 5.64e-05),
    ('ln', 'f32', 'random'): (7.2e-07, 2.39e-07),
    ('merge', 'bf16_bf16', 'edge'): (1.7e-02, 5.38e-03),
    ('merge', 'bf16_bf16', 'random'): (6.9e-03, 2.28e-03),
    ('merge', 'f32_bf16', 'edge'): (1.6e-02, 5.03e-03),
    ('merge', 'f32_bf16', 'random'): (1.6e-02, 5.21e-03),
    ('merge', 'f32_f32', 'edge'): (1.4e-04, 4.40e-05),
    ('merge', 'f32_f32', 'random'): (6.8e-07, 2.25e-07),
    ('merge', 'f32_split', 'edge'): (1.4e-04, 4.40e-05),
    ('merge', 'f32_split', 'random'): (2.3e-05, 7.59e-06),
    ('mlp', 128, 'bf16', 'edge'): (0.0, 0.0),
    ('mlp', 128, 'bf16', 'random'): (6.0e-03, 1.97e-03),
    ('mlp', 128, 'f32', 'edge'): (3.1e-03, 1.01e-03),
    ('mlp', 128, 'f32', 'random'): (2.3e-04, 7.54e-05),
    ('mlp', 256, 'bf16', 'edge'): (0.0, 0.0),
    ('mlp', 256, 'bf16', 'random'): (1.1e-02, 3.36e-03),
    ('mlp', 256, 'f32', 'edge'): (2.1e-03, 6.76e-04),
    ('mlp', 256, 'f32', 'random'): (1.6e-03, 5.07e-04),
    ('mlp', 512, 'bf16', 'edge'): (0.0, 0.0),
    ('mlp', 512, 'bf16', 'random'): (1.9e-02, 6.21e-03),
    ('mlp', 512, 'f32', 'edge'): (4.5e-03, 1.47e-03),
    ('mlp', 512, 'f32', 'random'): (2.1e-03, 6.96e-04),
}


def _tol(key):
    return TOL[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------------------------------------------------------
def rb(t, bf):
    """bf16 rounding where the bf16 kernels round (bf), identity otherwise; float64 in, float64 out"""
    return t.to(torch.bfloat16).double() if bf else t


def ln64(x, g, b, eps=EPS):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * g + b


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def rel_index():
    """[49, 49] index into the (2 WS - 1)^2 relative-position table: ((dy + 6) * 13 + (dx + 6)) for query i, key j"""
    t = torch.arange(WT)
    dy = (t // WS)[:, None] - (t // WS)[None, :]
    dx = (t % WS)[:, None] - (t % WS)[None, :]
    return (dy + WS - 1) * (2 * WS - 1) + (dx + WS - 1)


def region_ids(L, shift):
    """SW-MSA region of each coordinate s of the padded, shifted axis of length L: 0 (s < L - WS), 1 (s < L - shift), 2"""
    s = torch.arange(L)
    return torch.where(s < L - WS, 0, torch.where(s < L - shift, 1, 2))


def padded(H, W):
    return -(-H // WS) * WS, -(-W // WS) * WS


def _to_windows(t, shift):
    """[B, Hp, Wp, ...] -> rolled by -shift and partitioned: [B, nWy, nWx, 49, ...]"""
    B, Hp, Wp = t.shape[:3]
    if shift:
        t = torch.roll(t, (-shift, -shift), (1, 2))
    rest = t.shape[3:]
    t = t.reshape(B, Hp // WS, WS, Wp // WS, WS, *rest).transpose(2, 3)
    return t.reshape(B, Hp // WS, Wp // WS, WT, *rest)


def _from_windows(t, shift):
    """inverse of _to_windows"""
    B, nWy, nWx = t.shape[:3]
    rest = t.shape[4:]
    t = t.reshape(B, nWy, nWx, WS, WS, *rest).transpose(2, 3).reshape(B, nWy * WS, nWx * WS, *rest)
    if shift:
        t = torch.roll(t, (shift, shift), (1, 2))
    return t


def ref_window_attn(qkv, bqkv, table, nH, shift, bf):
    """Swin (shifted-)window attention between the qkv and proj Linears (swin_transformer.py:119-151, :209-244) from a qkv map
    qkv [B, H, W, 3C] float64: padding tokens (F.pad after norm1) carry q / k / v = the bias (bf16-rounded with bf, as the kernels
    substitute it), roll by -shift, 7x7 windows, q k^T / sqrt(32) + table[rel_index], -100 between different SW-MSA regions of the padded
    grid, softmax (P rounded with bf), P v (rounded with bf), reverse, roll back, crop -> [B, H, W, C]"""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    Hp, Wp = padded(H, W)
    full = rb(bqkv, bf).reshape(1, 1, 1, C3).expand(B, Hp, Wp, C3).clone()
    full[:, :H, :W] = qkv
    win = _to_windows(full, shift).reshape(B, Hp // WS, Wp // WS, WT, 3, nH, HD).permute(4, 0, 1, 2, 5, 3, 6)
    q, k, v = win[0], win[1], win[2]                                      # [B, nWy, nWx, nH, 49, 32]
    s = (q * SCALE) @ k.transpose(-1, -2) + table[rel_index()].permute(2, 0, 1)
    if shift:
        ry, rx = region_ids(Hp, shift).reshape(-1, WS), region_ids(Wp, shift).reshape(-1, WS)
        rid = (ry[:, None, :, None] * 3 + rx[None, :, None, :]).reshape(Hp // WS, Wp // WS, WT)
        s = s + torch.where(rid[..., :, None] != rid[..., None, :], -100.0, 0.0).double()[None, :, :, None]
    o = rb(rb(torch.softmax(s, -1), bf) @ v, bf)                          # [B, nWy, nWx, nH, 49, 32]
    y = _from_windows(o.permute(0, 1, 2, 4, 3, 5).reshape(B, Hp // WS, Wp // WS, WT, C), shift)
    return y[:, :H, :W]


def ref_attn_block(x, g, b, Wqkv, bqkv, table, Wp, bp, nH, shift, bf):
    """the attention half of a Swin block on the residual stream x [B, H, W, C]: x + proj(window attention(qkv(LN(x))))"""
    qkv = rb(rb(ln64(x, g, b), bf) @ Wqkv.T + bqkv, bf)
    return x + ref_window_attn(qkv, bqkv, table, nH, shift, bf) @ Wp.T + bp


def ref_mlp(x, g, b, W1, b1, W2, b2, bf, bf_out=False):
    """the MLP half: x + fc2(GELU(fc1(LN(x)))) (exact-erf GELU); bf_out: the bf16 residual stream's output rounding"""
    h = rb(gelu64(rb(ln64(x, g, b), bf) @ W1.T + b1), bf)
    return rb(x + h @ W2.T + b2, bf_out)


def ref_patch_embed(img, w, bias, g, be):
    """PatchEmbed (swin_transformer.py:427-443): zero-pad right / bottom to x4, conv 4x4 stride 4 (w [E, 48] = [E, 3, 4, 4]), LN -> [B, L, E]"""
    B, _, H, W = img.shape
    Hp, Wp = -(-H // 4), -(-W // 4)
    full = torch.zeros(B, 3, Hp * 4, Wp * 4, dtype=torch.float64)
    full[:, :, :H, :W] = img
    p = full.reshape(B, 3, Hp, 4, Wp, 4).permute(0, 2, 4, 1, 3, 5).reshape(B, Hp * Wp, 48)
    return ln64(p @ w.T + bias, g, be)


def merge_gather(x):
    """PatchMerging's gather (swin_transformer.py:269-296): x [B, H, W, C] zero-padded to even, quadrants (0,0), (1,0), (0,1), (1,1)
    concatenated -> [B, H2, W2, 4C]"""
    B, H, W, C = x.shape
    full = torch.zeros(B, H + H % 2, W + W % 2, C, dtype=x.dtype)
    full[:, :H, :W] = x
    return torch.cat([full[:, 0::2, 0::2], full[:, 1::2, 0::2], full[:, 0::2, 1::2], full[:, 1::2, 1::2]], -1)


def ref_patch_merge(x, g, b):
    return ln64(merge_gather(x), g, b)


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_g(seed), dtype=torch.float64) * scale


def _f32(t):
    return t.float().double()


def _bf(t):
    return t.to(torch.bfloat16).double()


def _vec(seed, n, s=0.1):
    return _f32(_randn(n, seed=seed) * s)


EDGE_ROWS = ('zeros', 'constant', 'variance below eps', 'offset 300 +- 1', 'outlier channel x50', 'scale 1e-3', 'scale 1e4')


def edge_row(kind, C, seed):
    """one LayerNorm-input row of EDGE_ROWS[kind] (fp32-valued float64)"""
    r = _randn(C, seed=seed)
    if kind == 0:
        r = torch.zeros(C, dtype=torch.float64)
    elif kind == 1:
        r = torch.full((C,), 0.5, dtype=torch.float64)
    elif kind == 2:
        r = 0.5 + 1e-4 * r               # variance ~1e-8 < eps
    elif kind == 3:
        r = 300.0 + r
    elif kind == 4:
        r[C // 3] = 50.0
    elif kind == 5:
        r = r * 1e-3
    else:
        r = r * 1e4
    return _f32(r)


def edge_rows(C, seed, scale=1.5, offset=0.2):
    """NB rows [NB, C]: rows 0..6 = EDGE_ROWS, the rest ordinary random rows"""
    x = _f32(_randn(NB, C, seed=seed) * scale + offset)
    for k in range(len(EDGE_ROWS)):
        x[k] = edge_row(k, C, seed + 1 + k)
    return x


def edge_coords(H, W, shift):
    """token coordinates next to every shift-region boundary (both sides), the corners and the padding: [(y, x)] inside H x W"""
    Hp, Wp = padded(H, W)

    def axis(L, Lp):
        s = {0, L - 1}
        for bnd in (Lp - WS, Lp - shift if shift else Lp - WS):
            for d in (-1, 0):
                s.add((bnd + d + shift) % Lp)
        return sorted(v for v in s if 0 <= v < L)
    ys, xs = axis(H, Hp), axis(W, Wp)
    return [(y, x) for y in ys for x in xs]


def plant_edge_tokens(x, shift, seed):
    """x [B, H, W, C] (fp32-valued): the EDGE_ROWS planted at edge_coords, cycling through the kinds and the images -> planted mask [B, H, W]"""
    B, H, W, C = x.shape
    m = torch.zeros(B, H, W, dtype=torch.bool)
    n = 0
    for b in range(B):
        for (y, xx) in edge_coords(H, W, shift):
            k = (n + b) % len(EDGE_ROWS)
            x[b, y, xx] = edge_row(k, C, seed + n)
            m[b, y, xx] = True
            n += 1
    return m


def image_src(B, nb, mult=7, add=1):
    """image b of a large launch is base image src[b]"""
    return (torch.arange(B, dtype=torch.int64, device=DEV) * mult + add) % nb


def row_src(R, mult=101, add=13):
    return (torch.arange(R, dtype=torch.int64, device=DEV) * mult + add) % NB


def _dev(t, dt=torch.float32):
    return t.to(dt).to(DEV).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------------------------
def window_rel(got, ref, nH, shift, x=None):
    """got (device or CPU), ref float64 [B, H, W, C] -> per (image, window, head) max |got - ref| / max |ref| of that window and head,
    [B, nWy, nWx, nH]; a non-finite value is an infinite error.  x (the fp32 residual stream the kernel added to, exact in float64): the
    denominator is max |ref - x| instead, the size of what the kernel computed -- a 300 or 1e4 residual must not hide its attention path"""
    B, H, W, C = ref.shape
    Hp, Wp = padded(H, W)
    g = got.double().cpu().reshape(B, H, W, C)
    bad = ~torch.isfinite(g)
    gp = torch.zeros(B, Hp, Wp, C, dtype=torch.float64)
    rp = torch.zeros(B, Hp, Wp, C, dtype=torch.float64)
    gp[:, :H, :W] = torch.where(bad, 0.0, g)
    rp[:, :H, :W] = ref
    sp = rp.clone()
    if x is not None:
        sp[:, :H, :W] -= x.reshape(B, H, W, C)
    d = _to_windows((gp - rp).abs(), shift).reshape(B, Hp // WS, Wp // WS, WT, nH, -1).amax((3, 5))
    r = _to_windows(sp.abs(), shift).reshape(B, Hp // WS, Wp // WS, WT, nH, -1).amax((3, 5))
    e = d / r.clamp_min(1e-300)
    bp = torch.zeros(B, Hp, Wp, dtype=torch.bool)
    bp[:, :H, :W] = bad.any(-1)
    nonfin = _to_windows(bp, shift).any(3)
    return torch.where(nonfin[..., None], float('inf'), e)


def edge_windows(B, H, W, shift, planted=None):
    """[B, nWy, nWx] bool: the last window row / column of the padded grid, and (planted [B, H, W]) windows holding a planted token"""
    Hp, Wp = padded(H, W)
    nWy, nWx = Hp // WS, Wp // WS
    e = torch.zeros(B, nWy, nWx, dtype=torch.bool)
    e[:, -1, :] = True
    e[:, :, -1] = True
    if planted is not None:
        p = torch.zeros(B, Hp, Wp, dtype=torch.bool)
        p[:, :H, :W] = planted
        e |= _to_windows(p, shift).any(3)
    return e


def row_rel(got, ref, x=None):
    """per row: max |got - ref| / max |ref| of that row -> [rows]; a non-finite value is an infinite error.  x (an fp32 residual the
    kernel added to): max |ref - x| of the row is the denominator instead"""
    g = got.double().cpu().reshape(ref.shape[0], -1)
    r = ref.reshape(ref.shape[0], -1)
    s = r if x is None else r - x.reshape(r.shape)
    e = (g - r).abs().max(1).values / s.abs().max(1).values.clamp_min(1e-300)
    return torch.where(torch.isfinite(g).all(1), e, torch.full_like(e, float('inf')))


def _gate_groups(out, name, key, groups):
    """groups: [(group, errors tensor, describe(index) -> str)]: the worst of each group against TOL[key + (group,)]"""
    for group, e, desc in groups:
        if e.numel() == 0:
            continue
        i = int(e.reshape(-1).argmax())
        err = e.reshape(-1)[i].item()
        tol, meas = _tol(key + (group,))
        note = '%s; worst %s' % (' '.join(map(str, key)), desc(i))
        if meas is not None:
            note += '; measured %.2e' % meas
        out.append(rrec('%s [%s]' % (name, group), err, tol, note))


def gate_windows(out, name, key, got, ref, nH, shift, planted=None, x=None):
    B, H, W, _ = ref.shape
    e = window_rel(got, ref, nH, shift, x)
    edge = edge_windows(B, H, W, shift, planted)[..., None].expand_as(e)
    shape = e.shape

    def desc_of(sel):
        idx = sel.nonzero()

        def d(i):
            b, wy, wx, h = idx[i].tolist()
            return 'image %d window (%d, %d) head %d' % (b, wy, wx, h)
        return d
    _gate_groups(out, name, key, [('interior', e[~edge], desc_of(~edge)), ('edge', e[edge], desc_of(edge))])
    return shape


def gate_rows(out, name, key, got, ref, edge, x=None):
    """edge: bool [rows] -- the edge rows, gated apart; x: see row_rel"""
    e = row_rel(got, ref, x)
    ie, ee = (~edge).nonzero().reshape(-1), edge.nonzero().reshape(-1)
    _gate_groups(out, name, key, [('random', e[ie], lambda i: 'row %d' % ie[i].item()), ('edge', e[ee], lambda i: 'row %d' % ee[i].item())])


# ---------------------------------------------------------------------------------------------------------------------------------------
# guarded launches
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ibits(dt):
    return torch.int32 if dt == torch.float32 else torch.int16


def guarded(rows, width, dtype, bits, fill=None):
    """[rows + GUARD, width] buffer, guard rows = bits, rows[:rows] = fill (a [rows, width] tensor or None: bits too)"""
    buf = torch.empty((rows + GUARD, width), dtype=dtype, device=DEV)
    buf.view(_ibits(dtype)).fill_(bits)
    if fill is not None:
        buf[:rows] = fill
    return buf


def kept(buf, rows, bits):
    return bool((buf[rows:].view(_ibits(buf.dtype)) == bits).all().item())


VIEW_LEAD, VIEW_OFF = 8, 8           # guard rows before / after and guard columns before a guarded_view (multiples of 8: 16-byte bases)


def guarded_view(rows, width, pitch, dtype, bits, fill=None, device=DEV, tail=VIEW_LEAD):
    """guarded() with a row pitch and guards on every side: a [VIEW_LEAD + rows + tail, pitch] buffer of `bits` and its view
    [rows, width] at row VIEW_LEAD, column VIEW_OFF (pitch >= VIEW_OFF + width), = fill where given -> (buffer, view).  The view's
    base stays 16-byte aligned whatever the pitch."""
    assert pitch >= VIEW_OFF + width
    buf = torch.empty((VIEW_LEAD + rows + tail, pitch), dtype=dtype, device=device)
    buf.view(_ibits(dtype)).fill_(bits)
    view = buf[VIEW_LEAD:VIEW_LEAD + rows, VIEW_OFF:VIEW_OFF + width]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def kept_view(buf, rows, width, bits):
    """(guard rows before and after the view of guarded_view still hold bits, so do the gap columns beside its rows)"""
    b = buf.view(_ibits(buf.dtype))
    mid = b[VIEW_LEAD:VIEW_LEAD + rows]
    rows_ok = bool((b[:VIEW_LEAD] == bits).all().item()) and bool((b[VIEW_LEAD + rows:] == bits).all().item())
    cols_ok = bool((mid[:, :VIEW_OFF] == bits).all().item()) and bool((mid[:, VIEW_OFF + width:] == bits).all().item())
    return rows_ok, cols_ok


def nan_bits(dt):
    return F32_NAN if dt == torch.float32 else BF16_NAN


def sent_bits(dt):
    return F32_SENT if dt == torch.float32 else BF16_SENT


def run_guarded(launch, ins, outs):
    """ins {name: [rows, w] device tensor} -> NaN-guarded input buffers; outs {name: (rows, w, dtype)} -> sentinel-guarded output buffers;
    launch({name: view [rows, w]}) -> ({out name: view}, problems)"""
    bufs, views, probs = {}, {}, []
    for k, t in ins.items():
        bufs[k] = guarded(t.shape[0], t.shape[1], t.dtype, nan_bits(t.dtype), t)
        views[k] = bufs[k][:t.shape[0]]
    for k, (r, w, dt) in outs.items():
        bufs[k] = guarded(r, w, dt, sent_bits(dt))
        views[k] = bufs[k][:r]
    launch(views)
    torch.cuda.synchronize()
    for k, t in ins.items():
        if not kept(bufs[k], t.shape[0], nan_bits(t.dtype)):
            probs.append('input %s: guard rows changed' % k)
    res = {}
    for k, (r, w, dt) in outs.items():
        if not kept(bufs[k], r, sent_bits(dt)):
            probs.append('output %s: a row past the end was written' % k)
        v = views[k]
        if not bool(torch.isfinite(v).all().item()):
            probs.append('%s: a valid token holds NaN / inf' % k)
        res[k] = v
    return res, probs


def guard_rec(out, tag, probs):
    out.append(rec(tag + ': guard rows untouched, no NaN / inf in valid tokens' + ('' if not probs else ' -- %s' % '; '.join(probs)), len(probs), 0))


def replicate(out, tag, run, base_in, base_out, src, twice=True):
    """run({name: gathered input [B * per, w]}) -> ({name: output [B * per, w]}, problems); base_in / base_out {name: [nb, per, w]} on the
    device.  Every output image b == base image src[b] bit for bit; the launch repeats its bits."""
    ins = {k: v.index_select(0, src).reshape(-1, v.shape[-1]) for k, v in base_in.items()}
    got, probs = run(ins)
    del ins
    bad = [k for k in base_out if not torch.equal(got[k].reshape(-1, *base_out[k].shape[1:]), base_out[k].index_select(0, src))]
    out.append(rec(tag + ': every image == its source image of the base launch, bit for bit%s' % ('' if not bad else ' -- differs: %s' % bad),
                   len(bad), 0))
    guard_rec(out, tag, probs)
    if twice:
        ins = {k: v.index_select(0, src).reshape(-1, v.shape[-1]) for k, v in base_in.items()}
        again, _ = run(ins)
        del ins
        same = all(torch.equal(got[k], again[k]) for k in base_out)
        out.append(rec(tag + ': second launch identical (deterministic)', 0 if same else 1, 0))
        del again
    del got


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def walk_counts(top=64):
    """window / tile counts k * 64 - 1, k * 64, k * 64 + 1 for k = 1, 2, 4, ... top (past 4 * 512 at top = 64), and 2 * CUs +- 1"""
    s = set()
    k = 1
    while k <= top:
        s |= {k * 64 - 1, k * 64, k * 64 + 1}
        k *= 2
    c2 = 2 * cus()
    s |= {c2 - 1, c2, c2 + 1}
    return sorted(s)


# ---------------------------------------------------------------------------------------------------------------------------------------
# window attention (ops.swin_window_attn)
# ---------------------------------------------------------------------------------------------------------------------------------------
# (H, W): every residue of H mod 7 and of W mod 7, H or W in {1, 2, 6, 7, 8}, 1 x 1, single windows, several windows
GEOMS = ((1, 1), (2, 12), (6, 11), (7, 10), (8, 8), (10, 7), (11, 6), (12, 2), (5, 6), (7, 7), (17, 20), (13, 1))
HEADS = (3, 4, 6, 8, 12, 16, 24, 32)
# impl name -> (swin_attn_impl selector, expanded bias, qkv dtype, split output)
ATTN_IMPLS = {
    'mfma_expb_bf16': (0, True, torch.bfloat16, False),
    'mfma_table_bf16': (2, False, torch.bfloat16, False),
    'scalar_bf16': (1, False, torch.bfloat16, False),
    'mfma_expb_f32': (0, True, torch.float32, False),
    'mfma_table_f32': (2, False, torch.float32, False),
    'scalar_f32': (1, False, torch.float32, False),
    'x3_split': (0, True, torch.float32, True),          # the parity engine's call: swin_attn_x3_kernel, split pairs out
    'x3_f32': (4, True, torch.float32, False),           # the same kernel, fp32 out
    'mfma_f32_split': (3, True, torch.float32, True),    # swin_attn_mfma_kernel<float>, split pairs out
}


def attn_inputs(nb, H, W, nH, shift, dt, seed):
    """base qkv [nb, H, W, 3C] (values representable in dt), bias, table with the attention edges planted in image 0:
    head nH - 1 has a zero table and window (0, 0) zero q (uniform softmax there), head 0 of the last window (an edge window) has one key
    ahead of the others by ~80 logits, head 1 (head 0 of image 1 when nH = 1) of that window has every key at +60 against every query, so
    that the -100 SW-MSA mask alone decides which keys count"""
    C = nH * HD
    rnd = _bf if dt == torch.bfloat16 else _f32
    qkv = rnd(_randn(nb, H, W, 3 * C, seed=seed))
    bqkv = _f32(_randn(3 * C, seed=seed + 1) * 0.3)
    table = _f32(_randn(169, nH, seed=seed + 2) * 0.5)
    table[:, nH - 1] = 0.0
    Hp, Wp = padded(H, W)
    nWy, nWx = Hp // WS, Wp // WS

    def toks(wy, wx):   # real tokens of shifted window (wy, wx): [(t, y, x)]
        r = []
        for t in range(WT):
            y, x = (wy * WS + t // WS + shift) % Hp, (wx * WS + t % WS + shift) % Wp
            if y < H and x < W:
                r.append((t, y, x))
        return r
    u = rnd(torch.where(_randn(HD, seed=seed + 3) > 0, 1.0, -1.0).double())
    h = nH - 1
    for (_, y, x) in toks(0, 0):
        qkv[0, y, x, h * HD:(h + 1) * HD] = 0.0
    last = toks(nWy - 1, nWx - 1)
    if last:
        c80 = rnd(u * (80.0 / (SCALE * HD)))
        for (_, y, x) in last:
            qkv[0, y, x, :HD] = u
        _, y0, x0 = last[-1]
        qkv[0, y0, x0, C:C + HD] = c80
        hb, im = (1, 0) if nH > 1 else (0, min(1, nb - 1))
        for (_, y, x) in toks(nWy - 1, nWx - 1):
            qkv[im, y, x, hb * HD:(hb + 1) * HD] = u
            qkv[im, y, x, C + hb * HD:C + (hb + 1) * HD] = rnd(u * (60.0 / (SCALE * HD)))
    return qkv, bqkv, table


class Attn:
    """one window-attention configuration: base inputs on the device, a guarded launcher, the float64 reference of the base launch"""

    def __init__(self, impl, H, W, nH, shift, nb=3, seed=11, ref=True):
        from advancedliteratemachinery_amd import ops
        self.sel, self.expb, self.dt, self.split = ATTN_IMPLS[impl]
        self.impl, self.H, self.W, self.nH, self.shift, self.nb = impl, H, W, nH, shift, nb
        self.C = nH * HD
        qkv, bqkv, table = attn_inputs(nb, H, W, nH, shift, self.dt, seed + 100 * H + W + 7 * nH)
        self.ref = ref_window_attn(qkv, bqkv, table, nH, shift, self.dt == torch.bfloat16) if ref else None
        self.qkv = _dev(qkv, self.dt).reshape(nb, H * W, 3 * self.C)
        self.bqkv, self.table = _dev(bqkv), _dev(table)
        self.bexp = ops.swin_expand_bias(self.table) if self.expb else None

    def run(self, ins):
        from advancedliteratemachinery_amd import ops
        R = ins['qkv'].shape[0]
        B = R // (self.H * self.W)
        w = 2 * self.C if self.split else self.C
        odt = torch.bfloat16 if self.split else self.dt

        def launch(v):
            ops.swin_attn_impl(self.sel)
            try:
                ops.swin_window_attn(v['qkv'], self.bqkv, self.table, B, self.H, self.W, self.C, self.nH, self.shift, out=v['out'],
                                     bias_expanded=self.bexp, out_split=self.split)
            finally:
                ops.swin_attn_impl(0)
        return run_guarded(launch, ins, {'out': (R, w, odt)})

    def value(self, out):
        """the output rows as float64 values [rows, C] (split pairs: hi + lo)"""
        if self.split:
            return out[:, :self.C].double() + out[:, self.C:].double()
        return out.double()

    def base(self, out, tag):
        got, probs = self.run({'qkv': self.qkv.reshape(-1, 3 * self.C)})
        guard_rec(out, tag + ' base', probs)
        if self.ref is not None:
            v = self.value(got['out']).reshape(self.nb, self.H, self.W, self.C)
            gate_windows(out, tag + ' vs float64 (per window and head)', ('attn', self.impl), v, self.ref, self.nH, self.shift)
        return {'out': got['out'].reshape(self.nb, self.H * self.W, -1).clone()}

    def sweep(self, out, tag, Bs, base_out, twice=True):
        for B in Bs:
            replicate(out, '%s B=%d (%d windows)' % (tag, B, B * (-(-self.H // WS)) * (-(-self.W // WS))), self.run, {'qkv': self.qkv}, base_out,
                      image_src(B, self.nb), twice)


def check_attn_geometry(impl):
    """every GEOMS shape at shift 0 and 3, at 4 and 3 heads (the parity engine's split-product call at 4 heads only; its 3-head groups run in
    check_attn_heads): float64 per window, plus a 4- and 21-image launch bit-identical to the base images"""
    out = []
    for (H, W) in GEOMS:
        for shift in (0, 3):
            for nH in ((4, 3) if impl != 'x3_split' else (4,)):
                a = Attn(impl, H, W, nH, shift)
                tag = 'window_attn[%s] %dx%d nH=%d shift=%d' % (impl, H, W, nH, shift)
                b = a.base(out, tag)
                a.sweep(out, tag, (4, 21), b, twice=False)
    return out


def check_attn_heads(impl):
    """every head count of Swin-T and Swin-B (partly empty head groups at 3, 6): float64 per window on two shapes, shift 0 and 3"""
    out = []
    for nH in HEADS:
        for (H, W) in ((8, 13), (7, 7)):
            for shift in (0, 3):
                a = Attn(impl, H, W, nH, shift, nb=2)
                a.base(out, 'window_attn[%s] %dx%d nH=%d shift=%d' % (impl, H, W, nH, shift))
    return out


def check_attn_walks(impl, nH, shapes=((7, 7, 3), (5, 6, 0)), top=64):
    """single-window images (7x7 under SW-MSA: one edge window; 5x6: padding): B = the window count, every walk_counts() count, twice, with
    guards -- each wave of the persistent kernels walks 1 .. ceil(count / grid) windows, odd and even"""
    out = []
    for (H, W, shift) in shapes:
        a = Attn(impl, H, W, nH, shift)
        tag = 'window_attn[%s] %dx%d nH=%d shift=%d' % (impl, H, W, nH, shift)
        b = a.base(out, tag)
        a.sweep(out, tag, walk_counts(top), b)
    return out


# benchmark stages for 1024 x 1024 images: (tokens per side, heads)
STAGES = ((256, 4), (128, 8), (64, 16), (32, 32))
CHUNK = {'bf16': 80, 'x3': 54}


def check_attn_stage(stage, impl):
    """the benchmark's own launch: stage `stage` of a 1024 x 1024 image, two base images against float64, then the encoder's chunk
    (80 images bf16, 54 the parity engine) bit-identical to them, twice"""
    out = []
    side, nH = STAGES[stage]
    B = CHUNK['x3' if impl.startswith('x3') else 'bf16']
    for shift in (0, 3):
        a = Attn(impl, side, side, nH, shift, nb=2)
        tag = 'window_attn[%s] stage %d %dx%d nH=%d shift=%d' % (impl, stage, side, side, nH, shift)
        b = a.base(out, tag)
        a.sweep(out, tag, (B,), b, twice=shift == 3)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# fused attention blocks (ops.swin_attn_block C = 128 / ops.swin_attn_block_packed C = 256)
# ---------------------------------------------------------------------------------------------------------------------------------------
class Block:
    def __init__(self, C, H, W, shift, nb=3, seed=21, ref=True):
        from advancedliteratemachinery_amd import ops
        from advancedliteratemachinery_amd.model.packing import pack_attn_block
        self.C, self.nH = C, C // HD
        self.H, self.W, self.shift, self.nb = H, W, shift, nb
        s = seed + 100 * H + W
        x = _f32(_randn(nb, H, W, C, seed=s) * 1.5 + 0.2)
        self.planted = plant_edge_tokens(x, shift, s + 1)
        g, b = 1 + _vec(s + 2, C), _vec(s + 3, C)
        Wqkv, bqkv = _bf(_randn(3 * C, C, seed=s + 4) / C ** 0.5 * 2), _vec(s + 5, 3 * C, 0.3)
        table = _f32(_randn(169, self.nH, seed=s + 6) * 0.5)
        Wp, bp = _bf(_randn(C, C, seed=s + 7) / C ** 0.5), _vec(s + 8, C)
        self.ref = ref_attn_block(x, g, b, Wqkv, bqkv, table, Wp, bp, self.nH, shift, True) if ref else None
        self.x64 = x
        self.x = _dev(x).reshape(nb, H * W, C)
        bexp = ops.swin_expand_bias(_dev(table))
        if C == 128:
            self.args = (_dev(g), _dev(b), _dev(Wqkv, torch.bfloat16), _dev(bqkv), bexp, _dev(Wp, torch.bfloat16), _dev(bp))
        else:
            self.args = (_dev(g), _dev(b), pack_attn_block(_dev(Wqkv, torch.bfloat16), _dev(Wp, torch.bfloat16), self.nH), _dev(bqkv), bexp,
                         _dev(bp))

    def _call(self, x, out, B):
        from advancedliteratemachinery_amd import ops
        f = ops.swin_attn_block if self.C == 128 else ops.swin_attn_block_packed
        f(x, *self.args, B, self.H, self.W, self.C, self.nH, self.shift, out=out)

    def run(self, ins):
        R = ins['x'].shape[0]
        B = R // (self.H * self.W)
        return run_guarded(lambda v: self._call(v['x'], v['out'], B), ins, {'out': (R, self.C, torch.float32)})

    def run_inplace(self, ins):
        """in place: the residual stream buffer (NaN guard rows that must stay) is the output"""
        R = ins['x'].shape[0]
        B = R // (self.H * self.W)
        buf = guarded(R, self.C, torch.float32, F32_NAN, ins['x'])
        v = buf[:R]
        self._call(v, v, B)
        torch.cuda.synchronize()
        probs = [] if kept(buf, R, F32_NAN) else ['x: guard rows changed']
        if not bool(torch.isfinite(v).all().item()):
            probs.append('x: a valid token holds NaN / inf')
        return {'out': v}, probs

    def base(self, out, tag):
        got, probs = self.run({'x': self.x.reshape(-1, self.C)})
        guard_rec(out, tag + ' base', probs)
        if self.ref is not None:
            gate_windows(out, tag + ' vs float64 (per window and head, relative to max |ref - x|)', ('block', self.C),
                         got['out'].reshape(self.nb, self.H, self.W, self.C), self.ref, self.nH, self.shift, self.planted, x=self.x64)
        b = {'out': got['out'].reshape(self.nb, self.H * self.W, self.C).clone()}
        inp, p2 = self.run_inplace({'x': self.x.reshape(-1, self.C)})
        out.append(rec(tag + ' base: in place == out of place, bit for bit' + ('' if not p2 else ' -- ' + '; '.join(p2)),
                       (0 if torch.equal(inp['out'], got['out']) else 1) + len(p2), 0))
        return b

    def sweep(self, out, tag, Bs, base_out, twice=True, inplace=True):
        for B in Bs:
            t = '%s B=%d (%d windows)' % (tag, B, B * (-(-self.H // WS)) * (-(-self.W // WS)))
            replicate(out, t, self.run, {'x': self.x}, base_out, image_src(B, self.nb), twice)
            if inplace:
                replicate(out, t + ' in place', self.run_inplace, {'x': self.x}, base_out, image_src(B, self.nb), twice=False)


def check_block_geometry(C):
    out = []
    for (H, W) in GEOMS:
        for shift in (0, 3):
            blk = Block(C, H, W, shift)
            tag = 'attn_block[C=%d] %dx%d shift=%d' % (C, H, W, shift)
            b = blk.base(out, tag)
            blk.sweep(out, tag, (4, 21), b, twice=False, inplace=False)
    return out


def check_block_walks(C, top=64):
    """single-window images: the pair kernel (C = 128) runs min(ceil(n / 2), CUs) workgroups and walks past 2 * CUs windows, the C = 256
    kernel min(n, CUs); every walk_counts() count (odd counts leave group 1 of the last pair idle), twice, in place too"""
    out = []
    for (H, W, shift) in ((7, 7, 3), (5, 6, 0)):
        blk = Block(C, H, W, shift)
        tag = 'attn_block[C=%d] %dx%d shift=%d' % (C, H, W, shift)
        b = blk.base(out, tag)
        blk.sweep(out, tag, walk_counts(top), b)
    return out


def check_block_stage(C):
    """the benchmark's own launch: stage 0 (C = 128, 256 x 256 tokens) / stage 1 (C = 256, 128 x 128) of 1024 x 1024 images, 80 images"""
    out = []
    side = 256 if C == 128 else 128
    for shift in (0, 3):
        blk = Block(C, side, side, shift, nb=2)
        tag = 'attn_block[C=%d] stage %dx%d shift=%d' % (C, side, side, shift)
        b = blk.base(out, tag)
        blk.sweep(out, tag, (CHUNK['bf16'],), b, twice=shift == 3, inplace=shift == 3)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# fused MLP (ops.swin_mlp_fused)
# ---------------------------------------------------------------------------------------------------------------------------------------
MLP_VARIANTS = {128: (0, 1, 2, 3), 256: (0, 1, 2), 512: (0, 1)}
MLP_ROWS_PER_WG = {(128, 0): 128, (128, 1): 128, (128, 2): 256, (128, 3): 256, (256, 0): 128, (256, 1): 64, (256, 2): 128, (512, 0): 128,
                   (512, 1): 64}


class Mlp:
    def __init__(self, C, stream, seed=31):
        from advancedliteratemachinery_amd.model.packing import pack_mlp
        self.C, self.dt = C, stream
        bfs = stream == torch.bfloat16
        x = edge_rows(C, seed + C)
        if bfs:
            x = _bf(x)
        g, b = 1 + _vec(seed + 1, C), _vec(seed + 2, C)
        W1, b1 = _bf(_randn(4 * C, C, seed=seed + 3) / C ** 0.5), _vec(seed + 4, 4 * C)
        W2, b2 = _bf(_randn(C, 4 * C, seed=seed + 5) / (4 * C) ** 0.5), _vec(seed + 6, C)
        self.ref = ref_mlp(x, g, b, W1, b1, W2, b2, True, bf_out=bfs)
        # fp32 stream: the error is relative to the row's max |ref - x| (x is exact), so that a 300 or 1e4 residual cannot hide the LayerNorm
        # prologue; the bf16 stream rounds its output back onto x, so there the row's max |ref| is the scale
        self.x64 = None if bfs else x
        self.edge = torch.arange(NB) < len(EDGE_ROWS)
        self.x = _dev(x, stream)
        self.args = (_dev(g), _dev(b), pack_mlp(_dev(W1, torch.bfloat16), _dev(b1), _dev(W2, torch.bfloat16)), _dev(b2))

    def run(self, ins, inplace=False):
        from advancedliteratemachinery_amd import ops
        R = ins['x'].shape[0]
        if inplace:
            buf = guarded(R, self.C, self.dt, nan_bits(self.dt), ins['x'])
            v = buf[:R]
            ops.swin_mlp_fused(v, *self.args, out=v)
            torch.cuda.synchronize()
            probs = [] if kept(buf, R, nan_bits(self.dt)) else ['x: guard rows changed']
            if not bool(torch.isfinite(v).all().item()):
                probs.append('x: a valid row holds NaN / inf')
            return {'out': v}, probs
        return run_guarded(lambda v: ops.swin_mlp_fused(v['x'], *self.args, out=v['out']), ins, {'out': (R, self.C, self.dt)})


def check_mlp(C, stream_name):
    """every variant: 256 base rows (edge rows included) against float64 per row, then every row count across the variant's workgroup tile
    bit-identical to the base rows, twice, in place too; the variants agree bit for bit"""
    from advancedliteratemachinery_amd import ops
    out = []
    stream = torch.bfloat16 if stream_name == 'bf16' else torch.float32
    m = Mlp(C, stream)
    first = None
    try:
        for v in MLP_VARIANTS[C]:
            ops.swin_mlp_variant(v)
            tag = 'mlp_fused[C=%d %s stream v%d]' % (C, stream_name, v)
            got, probs = m.run({'x': m.x})
            guard_rec(out, tag + ' base', probs)
            gate_rows(out, tag + ' vs float64 (per row%s)' % ('' if m.x64 is None else ', relative to max |ref - x|'), ('mlp', C, stream_name),
                      got['out'], m.ref, m.edge, x=m.x64)
            base = {'out': got['out'].reshape(NB, 1, C).clone()}
            if first is None:
                first = base['out']
            else:
                out.append(rec(tag + ' base == variant %d, bit for bit' % MLP_VARIANTS[C][0], 0 if torch.equal(first, base['out']) else 1, 0))
            t = MLP_ROWS_PER_WG[(C, v)]
            for R in sorted({1, t - 1, t, t + 1, 3 * t + 5, 65536 + 13}):
                src = row_src(R)
                replicate(out, '%s R=%d' % (tag, R), m.run, {'x': m.x.reshape(NB, 1, C)}, base, src)
                replicate(out, '%s R=%d in place' % (tag, R), lambda i: m.run(i, inplace=True), {'x': m.x.reshape(NB, 1, C)}, base, src,
                          twice=False)
    finally:
        ops.swin_mlp_variant(0)
    return out


def check_mlp_stage():
    """the benchmark's own launches: stage 0 (C = 128, 80 x 65 536 rows) and stage 1 (C = 256, 80 x 16 384 rows), fp32 stream, in place"""
    out = []
    for C, R in ((128, 80 * 65536), (256, 80 * 16384)):
        m = Mlp(C, torch.float32)
        tag = 'mlp_fused[C=%d f32 stream] stage R=%d' % (C, R)
        got, probs = m.run({'x': m.x})
        guard_rec(out, tag + ' base', probs)
        gate_rows(out, tag + ' base vs float64 (per row, relative to max |ref - x|)', ('mlp', C, 'f32'), got['out'], m.ref, m.edge, x=m.x64)
        base = {'out': got['out'].reshape(NB, 1, C).clone()}
        replicate(out, tag + ' in place', lambda i: m.run(i, inplace=True), {'x': m.x.reshape(NB, 1, C)}, base, row_src(R))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# patch embedding (ops.patch_embed_ln)
# ---------------------------------------------------------------------------------------------------------------------------------------
# every residue of H and of W mod 4, 1 x 1, 4-token images (one 16-token tile = 1 image at 13..16 pixels per side: 4 x 4 tokens)
PE_GEOMS = ((16, 18), (13, 15), (14, 16), (15, 17), (1, 1), (3, 2), (13, 16))
# path -> (E, out dtype, OMP355_PATCH_EMBED_SCALAR set).  csrc/norm.hip omp_patch_embed_ln: at E <= 128 (E % 8 == 0) the variable moves the
# fp32 call from the matrix-core kernel to the thread-per-token kernel (patch_embed_tok_kernel), which bf16 output takes anyway; the
# workgroup-per-16-tokens kernel (patch_embed_kernel) is reached only at E > 128 (or E % 8 != 0), never through the variable -- hence E = 192.
PE_PATHS = {
    'mfma8': (128, torch.float32, False),     # the engine's call, Swin-B
    'mfma6': (96, torch.float32, False),      # Swin-T
    'tok_f32_128': (128, torch.float32, True),
    'tok_f32_96': (96, torch.float32, True),
    'tok_bf16_128': (128, torch.bfloat16, False),
    'generic_f32_192': (192, torch.float32, False),
    'generic_bf16_192': (192, torch.bfloat16, False),
}


class Embed:
    def __init__(self, path, H, W, nb=3, seed=41):
        self.path, self.H, self.W, self.nb = path, H, W, nb
        self.E, self.dt, self.scalar = PE_PATHS[path]
        s = seed + 10 * H + W
        img = _f32(_randn(nb, 3, H, W, seed=s))
        img[1] = 0.0                                   # LayerNorm input = the conv bias
        if nb > 2:
            img[2] = 2.64                              # saturated
        E = self.E
        w = _f32(_randn(E, 48, seed=s + 1) * 0.2)
        b, g, be = _vec(s + 2, E), 1 + _vec(s + 3, E), _vec(s + 4, E)
        self.ref = ref_patch_embed(img, w, b, g, be)
        if self.dt == torch.bfloat16:
            self.ref = rb(self.ref, True)
        Hp, Wp = -(-H // 4), -(-W // 4)
        self.ntok = Hp * Wp
        edge = torch.zeros(nb, Hp, Wp, dtype=torch.bool)
        edge[1:] = True
        if H % 4:
            edge[:, -1] = True
        if W % 4:
            edge[:, :, -1] = True
        self.edge = edge.reshape(-1)
        self.img = _dev(img).reshape(nb, 1, 3 * H * W)
        self.args = (_dev(w), _dev(b), _dev(g), _dev(be))

    def run(self, ins):
        """ins['img'] [B, 3 H W]: a NaN-guarded buffer (the op allocates its output); OMP355_PATCH_EMBED_SCALAR set / unset around the call"""
        from advancedliteratemachinery_amd import ops
        B = ins['img'].shape[0]
        res = {}

        def launch(v):
            old = os.environ.get('OMP355_PATCH_EMBED_SCALAR')
            if self.scalar:
                os.environ['OMP355_PATCH_EMBED_SCALAR'] = '1'
            else:
                os.environ.pop('OMP355_PATCH_EMBED_SCALAR', None)
            try:
                res['out'] = ops.patch_embed_ln(v['img'].view(B, 3, self.H, self.W), *self.args, self.dt)[0].reshape(B * self.ntok, self.E)
            finally:
                if old is None:
                    os.environ.pop('OMP355_PATCH_EMBED_SCALAR', None)
                else:
                    os.environ['OMP355_PATCH_EMBED_SCALAR'] = old
        _, probs = run_guarded(launch, ins, {})
        if not bool(torch.isfinite(res['out']).all().item()):
            probs.append('a valid token holds NaN / inf')
        return res, probs


def check_patch_embed(path):
    """every residue of H and W mod 4: float64 per token (zero and saturated images and the padded border tokens gated apart), then image
    counts whose 16-token tile counts cross the persistent walk (ntiles > 4 * 512) bit-identical to the base images"""
    out = []
    for (H, W) in PE_GEOMS:
        e = Embed(path, H, W)
        tag = 'patch_embed[%s] %dx%d' % (path, H, W)
        got, probs = e.run({'img': e.img.reshape(e.nb, -1)})
        guard_rec(out, tag + ' base', probs)
        gate_rows(out, tag + ' vs float64 (per token)', ('embed', path), got['out'], e.ref.reshape(-1, e.E), e.edge)
        base = {'out': got['out'].reshape(e.nb, e.ntok, e.E).clone()}
        Bs = (4, 21)
        if (H, W) in ((13, 16), (15, 17)) and path.startswith('mfma'):
            Bs = walk_counts(64) + [4 * 512 * 4 + 1]    # 16 / 20 tokens per image: tile counts around every walk step
        for B in Bs:
            replicate(out, '%s B=%d (%d tokens)' % (tag, B, B * e.ntok), e.run, {'img': e.img}, base, image_src(B, e.nb), twice=B > 21)
    return out


def check_patch_embed_stage():
    """the benchmark's own launch: 1024 x 1024 images, E = 128, fp32 out, 80 images from three base images checked against float64"""
    out = []
    e = Embed('mfma8', 1024, 1024)
    tag = 'patch_embed[mfma8] 1024x1024'
    got, probs = e.run({'img': e.img.reshape(e.nb, -1)})
    guard_rec(out, tag + ' base', probs)
    gate_rows(out, tag + ' vs float64 (per token)', ('embed', 'mfma8'), got['out'], e.ref.reshape(-1, e.E), e.edge)
    base = {'out': got['out'].reshape(e.nb, e.ntok, e.E).clone()}
    replicate(out, tag + ' B=80', e.run, {'img': e.img}, base, image_src(80, e.nb))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# patch merging (ops.patch_merge_gather_ln) and the stage-output LayerNorm (ops.layernorm)
# ---------------------------------------------------------------------------------------------------------------------------------------
PM_GEOMS = ((9, 13), (1, 5), (6, 1), (7, 7), (10, 12), (1, 1), (2, 3))
PM_MODES = {'f32_f32': (torch.float32, torch.float32), 'f32_bf16': (torch.float32, torch.bfloat16), 'f32_split': (torch.float32, 'split'),
            'bf16_bf16': (torch.bfloat16, torch.bfloat16)}
PM_WIDTHS = (96, 128, 192, 256, 384, 512)


class Merge:
    def __init__(self, mode, C, H, W, nb=3, seed=51):
        from advancedliteratemachinery_amd import ops
        self.mode, self.C, self.H, self.W, self.nb = mode, C, H, W, nb
        self.idt, self.odt = PM_MODES[mode]
        s = seed + C + 10 * H + W
        x = _f32(_randn(nb, H, W, C, seed=s) * 1.5 + 0.2)
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        # edge rows: the four tokens of merged row (y2, x2) carry the quarters of an EDGE_ROWS row (the padded quarters stay zero)
        edge = torch.zeros(nb, H2, W2, dtype=torch.bool)
        n = 0
        for b in range(nb):
            for (y2, x2) in sorted({(0, 0), (H2 - 1, W2 - 1), (0, W2 - 1), (H2 - 1, 0)}):
                r = edge_row((n + b) % len(EDGE_ROWS), 4 * C, s + 100 + n)
                for q, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                    if 2 * y2 + dy < H and 2 * x2 + dx < W:
                        x[b, 2 * y2 + dy, 2 * x2 + dx] = r[q * C:(q + 1) * C]
                edge[b, y2, x2] = True
                n += 1
        if H % 2:
            edge[:, -1] = True
        if W % 2:
            edge[:, :, -1] = True
        if self.idt == torch.bfloat16:
            x = _bf(x)
        g, b_ = 1 + _vec(s + 1, 4 * C), _vec(s + 2, 4 * C)
        self.ref = rb(ref_patch_merge(x, g, b_), self.odt == torch.bfloat16).reshape(-1, 4 * C)
        self.edge = edge.reshape(-1)
        self.rows = H2 * W2
        self.x = _dev(x, self.idt).reshape(nb, H * W, C)
        self.g, self.b = _dev(g), _dev(b_)
        self.ops = ops

    def run(self, ins):
        """the input is a NaN-guarded buffer (the op allocates its output)"""
        ops, res = self.ops, {}
        B = ins['x'].shape[0] // (self.H * self.W)

        def launch(v):
            res['out'] = ops.patch_merge_gather_ln(v['x'], self.g, self.b, B, self.H, self.W, self.C, EPS,
                                                   out_dtype=ops.SPLIT if self.odt == 'split' else self.odt)[0]
        _, probs = run_guarded(launch, ins, {})
        if not bool(torch.isfinite(res['out']).all().item()):
            probs.append('a valid row holds NaN / inf')
        return res, probs

    def value(self, y):
        if self.odt == 'split':
            return y[:, :4 * self.C].double() + y[:, 4 * self.C:].double()
        return y.double()


def check_patch_merge(mode):
    """every width, odd H / W and H or W = 1: float64 per merged row (edge rows and the padded border gated apart), a guarded input (NaN
    guard rows must not reach a valid row), then 4- and 21-image launches bit-identical to the base images"""
    out = []
    for C in PM_WIDTHS:
        for (H, W) in PM_GEOMS:
            m = Merge(mode, C, H, W)
            tag = 'patch_merge[%s] C=%d %dx%d' % (mode, C, H, W)
            res, probs = m.run({'x': m.x.reshape(-1, C)})
            guard_rec(out, tag + ' base', probs)
            gate_rows(out, tag + ' vs float64 (per merged row)', ('merge', mode), m.value(res['out']), m.ref, m.edge)
            base = {'out': res['out'].reshape(m.nb, m.rows, -1).clone()}
            for B in (4, 21):
                replicate(out, '%s B=%d' % (tag, B), m.run, {'x': m.x}, base, image_src(B, m.nb), twice=False)
    return out


def check_patch_merge_stage():
    """the benchmark's own launches: the merges after stages 0, 1, 2 of 1024 x 1024 images, f32 -> bf16 for the bf16 engine's 80 images and
    f32 -> split pairs for the parity engine's 54"""
    out = []
    for mode, B in (('f32_bf16', CHUNK['bf16']), ('f32_split', CHUNK['x3'])):
        for side, C in ((256, 128), (128, 256), (64, 512)):
            m = Merge(mode, C, side, side, nb=2)
            tag = 'patch_merge[%s] stage C=%d %dx%d' % (mode, C, side, side)
            got, probs = m.run({'x': m.x.reshape(-1, C)})
            guard_rec(out, tag + ' base', probs)
            gate_rows(out, tag + ' vs float64 (per merged row)', ('merge', mode), m.value(got['out']), m.ref, m.edge)
            base = {'out': got['out'].reshape(m.nb, m.rows, -1).clone()}
            replicate(out, tag + ' B=%d' % B, m.run, {'x': m.x}, base, image_src(B, m.nb))
            del base, got, m
    return out


LN_WIDTHS = (96, 128, 192, 256, 384, 512, 768, 1024)


def check_stage_layernorm():
    """ops.layernorm as the stage outputs call it: fp32 rows -> bf16 (and -> split pairs) with the fp32 copy, every width of Swin-T and
    Swin-B; 256 base rows against float64 per row, then R = 1 .. 80 x the stage's rows bit-identical to the base rows"""
    from advancedliteratemachinery_amd import ops
    out = []
    stage_rows = {128: 80 * 65536, 256: 80 * 16384, 512: 80 * 4096, 1024: 80 * 1024}
    for C in LN_WIDTHS:
        x = edge_rows(C, 61 + C)
        g, b = 1 + _vec(62 + C, C), _vec(63 + C, C)
        ref = ln64(x, g, b)
        edge = torch.arange(NB) < len(EDGE_ROWS)
        xd, gd, bd = _dev(x), _dev(g), _dev(b)
        for mode in ('bf16', 'split'):
            def run(ins, mode=mode):
                R = ins['x'].shape[0]
                return run_guarded(lambda v: ops.layernorm(v['x'], gd, bd, out=v['y'], out_dtype=ops.SPLIT if mode == 'split' else torch.bfloat16,
                                                           out_f32=v['yf']),
                                   ins, {'y': (R, 2 * C if mode == 'split' else C, torch.bfloat16), 'yf': (R, C, torch.float32)})
            tag = 'layernorm[f32 -> %s + f32 copy] C=%d' % (mode, C)
            got, probs = run({'x': xd})
            guard_rec(out, tag + ' base', probs)
            gate_rows(out, tag + ' f32 copy vs float64 (per row)', ('ln', 'f32'), got['yf'], ref, edge)
            if mode == 'split':
                hi, lo = got['y'][:, :C], got['y'][:, C:]
                exact_hi = torch.equal(hi, got['yf'].to(torch.bfloat16))
                exact_lo = torch.equal(lo, (got['yf'] - hi.float()).to(torch.bfloat16))
                out.append(rec(tag + ': split pairs == [bf16(y) | bf16(y - hi)] of the f32 copy, bit for bit', 0 if exact_hi and exact_lo else 1, 0))
            else:
                out.append(rec(tag + ': bf16 rows == bf16(f32 copy), bit for bit', 0 if torch.equal(got['y'], got['yf'].to(torch.bfloat16)) else 1, 0))
            base = {k: v.reshape(NB, 1, -1).clone() for k, v in got.items()}
            for R in sorted({1, 15, 16, 17, 4097, stage_rows.get(C, 0) or 65536 + 13}):
                replicate(out, '%s R=%d' % (tag, R), run, {'x': xd.reshape(NB, 1, C)}, base, row_src(R), twice=R > 4097)
    return out
