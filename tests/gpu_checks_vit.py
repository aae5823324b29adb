"""The MGP-STR recogniser kernels of csrc/vit.hip at every token count and key slot, and the row statistics of the head products
(csrc/gemm.hip: OMP_STORE_ROWSTAT, csrc/vit.hip: row_stat_merge_kernel).

  * vit_attn_qkv / vit_attn (bf16): both entry points on the same q / k / v at token counts that cross the 16-key score blocks, the 32-key
    V^T blocks, the 96-key softmax chunks, odd and even query-tile counts and the pad-free slab.  They must agree bit for bit and repeat
    their bits.  Planted inputs whose float64 result is EXACT in bf16 (tests/test_vit_reference.py proves that on ref_vit_attn(bf=True)):
    the key-slot walk (every query hits one key of a permutation: the output row is that key's value row), dead keys (q = 0, one non-zero
    value row: the output is 256 / T, so a padding key that took weight shows), ties across the softmax chunks (two identical keys: the
    mean of their value rows).  A random base with a peaked softmax is gated per (row, head) against float64.  The qkv buffer is a view
    with NaN guard rows and NaN gap columns, the output a view with sentinel guard rows and gap columns, the K slab holds NaN in every
    padding row.
  * vit_patch_embed: ragged last groups of VPE_TOK tokens behind full ones, E below / not a multiple of 256, per-token gates, guard rows,
    images independent of their neighbours.
  * a3_pool: the channels-per-thread boundaries, S = 1 .. 28, T around the 64-lane stride and on the raised-LDS path, junk behind the S
    used columns of sel, want_attn off, a one-hot softmax.
  * row statistics: float64 softmax / arg-max of the fp32 logits the same product writes, planted winners in chosen columns, rows whose
    logits are all far below 0, the scalar bias path, the record of a half tile without a valid column, guard words.

The float64 restatements (ref_*) take `bf`: True rounds to bf16 exactly where the bf16 kernels round (P = exp(s - rowmax), the attention
output, the patch-embedding output), False is exact float64.  tests/test_vit_reference.py pins them, with bf=False, to
oracle/mgp_str_ref.py and to plain torch softmax attention.

Every check returns rec / rrec records (tests/gpu_checks.py); the measured errors go to the parity report.
"""
import math

import torch

from tests.gpu_checks import DEV, rec, rnd, rrec

HD = 64                             # head dimension of the ViT
MPAD = 288                          # padded keys of a slab = the most tokens the kernels take
GUARD = 64
F32_NAN = 0x7FC0DEAD                # input guards (must not leak)
BF16_NAN = 0x7FA5
F32_SENT = 0x7FA5A5A5               # output guards (must survive)
BF16_SENT = 0x7F5A

# token counts: the 16-key score blocks, the 32-key V^T blocks, the 96-key chunk ends, odd and even query-tile counts, the pad-free slab
TOKENS = (1, 15, 16, 17, 31, 32, 33, 95, 96, 97, 191, 192, 193, 256, 257, 271, 272, 273, 287, 288)

# Gates, relative to each output row's own max |ref| (attention: each (row, head)'s), per (kernel, variant, group).  Each gate is about 3x
# the worst case measured on an MI355X against the float64 restatement (never more than 4x); (gate, measured) -- the measured value is
# also in the record's note.  A gate of 0 is where the measured error is 0: every bf16 output equals the bf16 rounding of the float64 value
# (the cls row is one fp32 addition; the ragged tokens at E = 192).  A schedule change that flips one rounding must re-measure these gates,
# not loosen them silently.  'pooled C1': at C = 1 a pooled row is ONE sum of T signed terms that may cancel and is its own scale.
TOL = {
    ('attn', 17): (2.4e-04, 8.10e-05),
    ('attn', 97): (1.8e-02, 5.88e-03),
    ('attn', 257): (2.3e-02, 7.81e-03),
    ('attn', 288): (2.3e-02, 7.81e-03),
    ('embed', 'fp32', 768, 'cls'): (1.7e-07, 5.73e-08),
    ('embed', 'fp32', 768, 'ragged'): (1.2e-06, 4.05e-07),
    ('embed', 'fp32', 768, 'rest'): (1.5e-06, 4.93e-07),
    ('embed', 'bf16', 768, 'cls'): (0.0, 0.0),
    ('embed', 'bf16', 768, 'ragged'): (5.7e-03, 1.91e-03),
    ('embed', 'bf16', 768, 'rest'): (1.1e-02, 3.60e-03),
    ('embed', 'fp32', 192, 'cls'): (1.8e-07, 5.94e-08),
    ('embed', 'fp32', 192, 'ragged'): (9.8e-07, 3.26e-07),
    ('embed', 'fp32', 192, 'rest'): (1.3e-06, 4.47e-07),
    ('embed', 'bf16', 192, 'cls'): (0.0, 0.0),
    ('embed', 'bf16', 192, 'ragged'): (0.0, 0.0),
    ('embed', 'bf16', 192, 'rest'): (6.2e-03, 2.08e-03),
    ('embed', 'fp32', 100, 'cls'): (1.6e-07, 5.18e-08),
    ('embed', 'fp32', 100, 'ragged'): (9.2e-07, 3.06e-07),
    ('embed', 'fp32', 100, 'rest'): (1.4e-06, 4.73e-07),
    ('embed', 'bf16', 100, 'cls'): (0.0, 0.0),
    ('embed', 'bf16', 100, 'ragged'): (2.7e-03, 9.12e-04),
    ('embed', 'bf16', 100, 'rest'): (1.5e-02, 5.03e-03),
    ('a3', 'fp32', 'T', 'pooled'): (4.3e-06, 1.44e-06),
    ('a3', 'fp32', 'T', 'maps'): (5.6e-07, 1.88e-07),
    ('a3', 'bf16', 'T', 'pooled'): (3.8e-06, 1.25e-06),
    ('a3', 'bf16', 'T', 'maps'): (5.6e-07, 1.88e-07),
    ('a3', 'fp32', 'S', 'pooled'): (3.1e-06, 1.04e-06),
    ('a3', 'fp32', 'S', 'maps'): (5.2e-07, 1.75e-07),
    ('a3', 'bf16', 'S', 'pooled'): (3.8e-06, 1.25e-06),
    ('a3', 'bf16', 'S', 'maps'): (5.2e-07, 1.75e-07),
    ('a3', 'fp32', 'C', 'pooled'): (3.6e-06, 1.20e-06),
    ('a3', 'fp32', 'C', 'pooled C1'): (9.0e-05, 3.01e-05),
    ('a3', 'fp32', 'C', 'maps'): (4.1e-07, 1.35e-07),
    ('a3', 'bf16', 'C', 'pooled'): (3.8e-06, 1.25e-06),
    ('a3', 'bf16', 'C', 'pooled C1'): (8.2e-05, 2.73e-05),
    ('a3', 'bf16', 'C', 'maps'): (4.1e-07, 1.35e-07),
    ('a3', 'fp32', 'corner', 'pooled'): (4.3e-06, 1.42e-06),
    ('a3', 'fp32', 'corner', 'maps'): (3.6e-07, 1.21e-07),
    ('a3', 'bf16', 'corner', 'pooled'): (4.0e-06, 1.33e-06),
    ('a3', 'bf16', 'corner', 'maps'): (3.6e-07, 1.21e-07),
    ('rowstat', 'bf16'): (1.4e-06, 4.70e-07),
    ('rowstat', 'fp32'): (1.8e-06, 5.95e-07),
    ('rowstat', 'bf16x3'): (2.1e-06, 7.14e-07),
}


def _tol(key):
    return TOL[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------------------------------------------------------
def rb(t, bf):
    """bf16 rounding where the bf16 kernels round (bf), identity otherwise; float64 in, float64 out"""
    return t.to(torch.bfloat16).double() if bf else t


def ref_vit_attn(q, k, v, bf):
    """timm Attention between the qkv and proj Linears: softmax(q k^T / 8) v per head.  q, k, v float64 [..., T, 64] -> [..., T, 64].
    bf: P = exp(s - rowmax) is rounded to bf16 before P v (the row sum is taken of the unrounded exponentials, as the kernel keeps it
    in fp32), the output is rounded to bf16; the 0.125 scale is exact."""
    s = (q * 0.125) @ k.transpose(-1, -2)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return rb(rb(p, bf) @ v / p.sum(-1, keepdim=True), bf)


def ref_patch_embed(img, w, bias, cls, pos, bf):
    """timm PatchEmbed (Conv2d(3, E, 4, 4) -> flatten(2).transpose(1, 2)), cls token in front, pos_embed added (mgp_str.py:66-70).
    img [B, 3, H, W], w [E, 48] = [E, 3, 4, 4], bias / cls [E], pos [T, E] -> [B, T, E]"""
    B, _, H, W = img.shape
    Hp, Wp = H // 4, W // 4
    p = img.reshape(B, 3, Hp, 4, Wp, 4).permute(0, 2, 4, 1, 3, 5).reshape(B, Hp * Wp, 48)
    tok = p @ w.T + bias
    return rb(torch.cat([cls.reshape(1, 1, -1).expand(B, 1, -1), tok], 1) + pos, bf)


def ref_a3_pool(sel, feat):
    """token_learner.py:27-31: maps[b, s, i] = softmax_i(sel[b, i, s]), pooled[b, s] = sum_i maps[b, s, i] feat[b, i].
    sel [B, T, S], feat [B, T, C] -> (pooled [B, S, C], maps [B, S, T])"""
    maps = torch.softmax(sel.transpose(1, 2), -1)
    return maps @ feat, maps


def ref_row_stats(lg):
    """test_final.py:145-170: greedy id (the lowest index on ties) and its softmax probability of every logits row [R, V]"""
    mx = lg.max(-1, keepdim=True).values
    ar = torch.arange(lg.shape[-1]).expand_as(lg)
    ids = torch.where(lg == mx, ar, lg.shape[-1]).min(-1).values
    return ids, 1.0 / torch.exp(lg - mx).sum(-1)


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


def key_codes(T):
    """[T, 64] of +-1: dimension d of key j holds bit d % 9 of j, so two distinct keys (j < 512) differ in at least 7 dimensions"""
    j = torch.arange(T)[:, None]
    d = torch.arange(HD)[None, :]
    return (((j >> (d % 9)) & 1) * 2 - 1).double()


def walk_perm(B, nH, T):
    """pi [B, nH, T]: pi(i) = (a i + c) % T with a coprime to T and c != 0 (T > 1), another (a, c) per image and head: a permutation of
    the keys that is not the identity, so that query tile and key block differ and every key is hit from some tile"""
    pi = torch.zeros(B, nH, T, dtype=torch.int64)
    cop = [a for a in range(1, 4 * T + 2) if math.gcd(a, T) == 1]
    for b in range(B):
        for h in range(nH):
            a = cop[(3 * h + b + 1) % len(cop)]
            c = 1 + (5 * h + 7 * b) % (T - 1) if T > 1 else 0
            pi[b, h] = (a * torch.arange(T) + c) % T
    return pi


def _int_values(B, nH, T, seed, positive=False):
    """non-zero integers in [-8, 8] (positive: [1, 8]) [B, nH, T, 64], another row per (image, head, key)"""
    v = torch.randint(1, 9, (B, nH, T, HD), generator=_g(seed)).double()
    if not positive:
        v = v * (torch.randint(0, 2, (B, nH, T, HD), generator=_g(seed + 1)).double() * 2 - 1)
    return v


def walk_inputs(B, nH, T, seed=1):
    """the key-slot walk: K row j = key_codes, query i = 16 K[pi(i)], V = non-zero integers.  The hit scores 0.125 * 16 * 64 = 128, every
    other key at most 100, so output row i is V[pi(i)] exactly in bf16 arithmetic -> (q, k, v, want) [B, nH, T, 64]"""
    k = key_codes(T).expand(B, nH, T, HD).clone()
    pi = walk_perm(B, nH, T)
    idx = pi[..., None].expand(B, nH, T, HD)
    v = _int_values(B, nH, T, seed)
    return 16.0 * k.gather(2, idx), k, v, v.gather(2, idx)


def dead_inputs(B, nH, T, seed=2):
    """q = 0, K random, every V row 0 except V[T - 1] = 256: every output is 256 / T; a key beyond T that took weight would lower it"""
    q = torch.zeros(B, nH, T, HD, dtype=torch.float64)
    k = _bf(_randn(B, nH, T, HD, seed=seed + T))
    v = torch.zeros(B, nH, T, HD, dtype=torch.float64)
    v[:, :, T - 1] = 256.0
    return q, k, v, torch.full((B, nH, T, HD), 256.0 / T, dtype=torch.float64).to(torch.bfloat16).double()


def tie_pairs(T):
    """(a, b) placements of two identical keys: the same chunk of 96 keys, chunks 0 and 2 in both orders, b = T - 1"""
    s = []
    if T > 17:
        s.append((2, 17))
    if T > 200:
        s += [(3, 200), (200, 3)]
    if T > 1:
        s.append((0, T - 1))
    return s


def tie_inputs(B, nH, T, a, b, seed=3):
    """the walk with K[b] = K[a] and positive integer V rows at a and b: the queries that aimed at key a or key b now aim at both
    (16 K[a]) and must return (V[a] + V[b]) / 2 exactly, every other query its own key's row.  The walk's rows keep their best key
    in every chunk that holds a key: the running-max rescale runs with alpha = 1 (best key in chunk 0) and alpha ~ exp(-28) (best key
    in the last live chunk)"""
    q, k, v, want = walk_inputs(B, nH, T, seed)
    pi = walk_perm(B, nH, T)
    k[:, :, b] = k[:, :, a]
    pos = _int_values(B, nH, T, seed + 7, positive=True)
    v[:, :, a], v[:, :, b] = pos[:, :, a], pos[:, :, b]
    want = v.gather(2, pi[..., None].expand(B, nH, T, HD))
    both = (pi == a) | (pi == b)
    q = torch.where(both[..., None], 16.0 * k[:, :, a:a + 1], q)
    want = torch.where(both[..., None], (v[:, :, a:a + 1] + v[:, :, b:b + 1]) / 2, want)
    return q, k, v, want


def random_inputs(B, nH, T, seed=4):
    """bf16-valued q, k ~ N(0, 3^(1/2)^2), v ~ N(0, 1): scores of standard deviation ~3, a peaked softmax"""
    s = 3.0 ** 0.5
    return (_bf(_randn(B, nH, T, HD, seed=seed + T, scale=s)), _bf(_randn(B, nH, T, HD, seed=seed + T + 1, scale=s)),
            _bf(_randn(B, nH, T, HD, seed=seed + T + 2)))


def onehot_sel(B, T, S, seed=5):
    """sel [B, T, S] of -1e4 with one +1e4 per (image, map) -> (sel, chosen token [B, S]): the softmax is one-hot in fp32 and float64"""
    tok = torch.randint(0, T, (B, S), generator=_g(seed + T + S))
    sel = torch.full((B, T, S), -1e4, dtype=torch.float64)
    sel.scatter_(1, tok[:, None, :], 1e4)
    return sel, tok


def winner_bias(lg, c, margin=5.0):
    """bias [N] (fp32-valued) that lifts column c of the one-row logits lg [1, N] to `margin` above every other column"""
    N = lg.shape[-1]
    b = torch.zeros(N, dtype=torch.float64)
    others = torch.cat([lg[0, :c], lg[0, c + 1:]])
    b[c] = (others.max().item() if N > 1 else 0.0) + margin - lg[0, c].item()
    return _f32(b)


# ---------------------------------------------------------------------------------------------------------------------------------------
# errors, guards
# ---------------------------------------------------------------------------------------------------------------------------------------
def row_rel(got, ref):
    """per row of the last dimension: max |got - ref| / max |ref| of that row; a non-finite value is an infinite error"""
    g = got.double().cpu().reshape(ref.shape)
    e = (g - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)
    return torch.where(torch.isfinite(g).all(-1), e, torch.full_like(e, float('inf')))


def _gate(out, name, key, e, desc=None):
    """the worst of the errors e against TOL[key]"""
    if e.numel() == 0:
        return
    i = int(e.reshape(-1).argmax())
    tol, meas = _tol(key)
    note = 'worst at %s' % (desc(i) if desc else str(tuple(torch.unravel_index(torch.tensor(i), e.shape))))
    if meas is not None:
        note += '; measured %.2e' % meas
    out.append(rrec(name, e.reshape(-1)[i].item(), tol, note))


def _ibits(dt):
    return torch.int32 if dt == torch.float32 else torch.int16


def _filled(shape, dtype, bits):
    buf = torch.empty(shape, dtype=dtype, device=DEV)
    buf.view(_ibits(dtype)).fill_(bits)
    return buf


def _sent(dt):
    return F32_SENT if dt == torch.float32 else BF16_SENT


def _nan(dt):
    return F32_NAN if dt == torch.float32 else BF16_NAN


def _only_view_written(buf, view_rows, view_cols, bits):
    """the guarded output buffer holds the sentinel everywhere outside [GUARD : GUARD + view_rows, : view_cols]"""
    b = buf.view(_ibits(buf.dtype)).clone()
    b[GUARD:GUARD + view_rows, :view_cols] = bits
    return bool((b == bits).all().item())


def _tokens(t):
    """[B, nH, T, 64] -> token-major [B T, nH 64]"""
    B, nH, T, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * T, nH * HD)


def _heads(t, B, nH, T):
    """token-major [B T, nH 64] -> float64 [B, nH, T, 64] on the CPU"""
    return t.double().cpu().reshape(B, T, nH, HD).permute(0, 2, 1, 3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# vit_attn_qkv / vit_attn
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_attn(out, tag, q, k, v, gap=0):
    """Both entry points on bf16-valued q, k, v [B, nH, T, 64]: the fused projection is a [B T, ld] view (ld = 3 nH 64 + gap) between NaN
    guard rows with NaN gap columns, the output a [B T, nH 64] view of pitch nH 64 + 4 between sentinel rows; the slabs come from the
    identity-projection STORE_KBLK / STORE_VBLK products, K rows at and beyond T then set to NaN (V^T pad keys stay zero).  Appends the
    records every case owes (the two paths bit-identical, the second launch identical, guards) and returns the output [B, nH, T, 64]."""
    from advancedliteratemachinery_amd import _lib, ops
    B, nH, T, _ = q.shape
    E, R = nH * HD, B * T
    ld, ldo = 3 * E + gap, E + 4
    bf = torch.bfloat16
    ibuf = _filled((R + 2 * GUARD, ld), bf, BF16_NAN)
    qkv = ibuf[GUARD:GUARD + R]
    qkv[:, :3 * E] = torch.cat([_tokens(q), _tokens(k), _tokens(v)], 1).to(bf).to(DEV)
    keep = ibuf.view(torch.int16).clone()
    res = []
    for _ in range(2):
        obuf = _filled((R + 2 * GUARD, ldo), bf, BF16_SENT)
        ops.vit_attn_qkv(qkv, obuf[GUARD:GUARD + R, :E], B, T, nH)
        res.append(obuf)
    K = torch.zeros(1, B, nH, MPAD, HD, dtype=bf, device=DEV)
    Vt = torch.zeros(1, B, nH, MPAD // 32, HD, 32, dtype=bf, device=DEV)
    eye = torch.eye(E, dtype=bf, device=DEV)
    geom = (B, T, MPAD, nH, 32)
    ops.gemm(qkv[:, E:2 * E].contiguous(), eye, None, out=K, store_mode=_lib.STORE_KBLK, kv=geom)
    ops.gemm(eye, qkv[:, 2 * E:3 * E].contiguous(), None, out=Vt, store_mode=_lib.STORE_VBLK, kv=geom, M=E, N=R, K=E)
    K[0, :, :, T:] = float('nan')
    sbuf = _filled((R + 2 * GUARD, ldo), bf, BF16_SENT)
    ops.vit_attn(qkv[:, :E], K[0], Vt[0], sbuf[GUARD:GUARD + R, :E], B, T, nH, MPAD)
    torch.cuda.synchronize()
    got = res[0][GUARD:GUARD + R, :E]
    out.append(rec(tag + ': vit_attn_qkv == vit_attn on the slabs, bit for bit', 0 if torch.equal(got, sbuf[GUARD:GUARD + R, :E]) else 1, 0))
    out.append(rec(tag + ': vit_attn_qkv second launch identical', 0 if torch.equal(res[0], res[1]) else 1, 0))
    probs = []
    if not torch.equal(ibuf.view(torch.int16), keep):
        probs.append('the input buffer changed')
    for name, b in (('vit_attn_qkv', res[0]), ('vit_attn', sbuf)):
        if not _only_view_written(b, R, E, BF16_SENT):
            probs.append('%s wrote outside its output view' % name)
        if not bool(torch.isfinite(b[GUARD:GUARD + R, :E]).all().item()):
            probs.append('%s: NaN / inf in an output row' % name)
    out.append(rec(tag + ': guard rows and gap columns untouched, no NaN from a guard, a gap or a padding key%s' % ('' if not probs else ' -- ' + '; '.join(probs)),
                   len(probs), 0))
    return _heads(got, B, nH, T)


def _exact(out, tag, got, want):
    bad = (got != want).any(-1)
    note = ''
    if bad.any():
        b, h, i = bad.nonzero()[0].tolist()
        note = '%d rows differ, first: image %d head %d query %d (tile %d)' % (int(bad.sum()), b, h, i, i // 16)
    out.append(rec(tag + ': exact', float(bad.sum()), 0, note))


def check_attn_walk(B, nH, tokens=TOKENS):
    """key-slot walk at every token count, the projection pitch alternating between 3 nH 64 and 3 nH 64 + 8"""
    out = []
    for n, T in enumerate(tokens):
        q, k, v, want = walk_inputs(B, nH, T)
        tag = 'vit_attn walk[B%d nH%d T%d gap%d]' % (B, nH, T, 8 * (n & 1))
        _exact(out, tag, run_attn(out, tag, q, k, v, gap=8 * (n & 1)), want)
    return out


def check_attn_dead(B, nH, tokens):
    out = []
    for T in tokens:
        q, k, v, want = dead_inputs(B, nH, T)
        tag = 'vit_attn dead keys[B%d nH%d T%d]' % (B, nH, T)
        _exact(out, tag + ' every output is bf16(256 / T)', run_attn(out, tag, q, k, v, gap=8 * (T & 1)), want)
    return out


def check_attn_ties(B=1, nH=3, tokens=(17, 33, 97, 193, 257, 273, 288)):
    out = []
    for T in tokens:
        for (a, b) in tie_pairs(T):
            q, k, v, want = tie_inputs(B, nH, T, a, b)
            tag = 'vit_attn ties[B%d nH%d T%d keys %d = %d]' % (B, nH, T, a, b)
            _exact(out, tag, run_attn(out, tag, q, k, v), want)
    return out


def check_attn_random(T, B=3, nH=12):
    """peaked random softmax against ref_vit_attn(bf=True), every (row, head) relative to its own max |ref|"""
    out = []
    q, k, v = random_inputs(B, nH, T)
    ref = ref_vit_attn(q, k, v, True)
    for gap in (0, 8):
        tag = 'vit_attn random[B%d nH%d T%d gap%d]' % (B, nH, T, gap)
        got = run_attn(out, tag, q, k, v, gap=gap)
        e = row_rel(got, ref)
        idx = torch.ones_like(e).nonzero()
        _gate(out, tag + ' vs float64 per (row, head)', ('attn', T), e, lambda i: 'image %d head %d query %d' % tuple(idx[i].tolist()))
    return out


def _refused(out, tag, call, code, bufs):
    """call() must raise the library's error `code`; every buffer of bufs [(tensor, bits)] keeps its sentinel"""
    got = ''
    try:
        call()
        got = 'no error'
    except RuntimeError as e:
        if '(%d)' % code not in str(e):
            got = str(e)
    torch.cuda.synchronize()
    out.append(rec(tag + ': refused%s' % ('' if not got else ' -- ' + got), 0 if not got else 1, 0))
    same = all(bool((b.view(_ibits(b.dtype)) == bits).all().item()) for b, bits in bufs)
    out.append(rec(tag + ': output untouched', 0 if same else 1, 0))


def check_attn_refusals():
    from advancedliteratemachinery_amd import ops
    out = []
    B, nH, E = 1, 3, 192
    bf = torch.bfloat16
    qkv = torch.zeros(B * 289, 3 * E, dtype=bf, device=DEV)
    o = _filled((B * 289, E), bf, BF16_SENT)
    _refused(out, 'vit_attn_qkv T = 289', lambda: ops.vit_attn_qkv(qkv, o, B, 289, nH), -95, [(o, BF16_SENT)])
    q32 = torch.zeros(B * 257, 3 * E, dtype=torch.float32, device=DEV)
    o32 = _filled((B * 257, E), torch.float32, F32_SENT)
    _refused(out, 'vit_attn_qkv fp32', lambda: ops.vit_attn_qkv(q32, o32, B, 257, nH), -95, [(o32, F32_SENT)])
    K = torch.zeros(B, nH, 256, HD, dtype=bf, device=DEV)
    Vt = torch.zeros(B, nH, 8, HD, 32, dtype=bf, device=DEV)
    _refused(out, 'vit_attn Mpad = 256', lambda: ops.vit_attn(qkv[:100, :E], K, Vt, o[:100], B, 100, nH, 256), -95, [(o, BF16_SENT)])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# vit_patch_embed
# ---------------------------------------------------------------------------------------------------------------------------------------
VPE_TOK = 16
EMBED_HP, EMBED_WP = (1, 2, 8), (1, 15, 16, 17, 32, 33)


def _patch_embed(img, w, bias, cls, pos, T, E, dt):
    """omp_vit_patch_embed on an image between NaN guards into an output between sentinel rows -> (tokens [B, T, E] view, problems)"""
    from advancedliteratemachinery_amd import _lib, ops
    B, _, H, W = img.shape
    n, pad = img.numel(), GUARD * 64
    ibuf = _filled((n + 2 * pad,), torch.float32, F32_NAN)
    ibuf[pad:pad + n] = img.reshape(-1)
    obuf = _filled((B * T + 2 * GUARD, E), dt, _sent(dt))
    view = obuf[GUARD:GUARD + B * T]
    rc = _lib.lib().omp_vit_patch_embed(ops.ptr(ibuf[pad:pad + n]), ops.ptr(w), ops.ptr(bias), ops.ptr(cls), ops.ptr(pos), ops.ptr(view), ops.dt(view),
                                        B, H, W, E, ops.stream())
    _lib.check(rc, 'omp_vit_patch_embed')
    torch.cuda.synchronize()
    probs = []
    if not _only_view_written(obuf, B * T, E, _sent(dt)):
        probs.append('a row outside the output was written')
    if not bool(torch.isfinite(view).all().item()):
        probs.append('NaN / inf in a token')
    return view.reshape(B, T, E), probs


def check_patch_embed(E, dtype_name):
    """every (Hp, Wp, B) at width E: float64 per token row (the cls row, the last token of every ragged group and the rest gated apart),
    guards, and the tokens of an image must not depend on its neighbours (the images permuted: the same bits, permuted)"""
    dt = {'fp32': torch.float32, 'bf16': torch.bfloat16}[dtype_name]
    out = []
    w = _f32(_randn(E, 48, seed=E, scale=0.2))
    bias, cls = _f32(_randn(E, seed=E + 1, scale=0.1)), _f32(_randn(E, seed=E + 2, scale=0.5))
    wd, bd, cd = w.float().to(DEV), bias.float().to(DEV), cls.float().to(DEV)
    err = {'cls': [], 'ragged': [], 'rest': []}
    for Hp in EMBED_HP:
        for Wp in EMBED_WP:
            T = Hp * Wp + 1
            pos = _f32(_randn(T, E, seed=T, scale=0.3))
            pd = pos.float().to(DEV)
            img3 = _f32(_randn(3, 3, 4 * Hp, 4 * Wp, seed=100 * Hp + Wp))
            for B in (1, 3):
                tag = 'vit_patch_embed[%s E%d B%d %dx%d patches]' % (dtype_name, E, B, Hp, Wp)
                img = img3[:B]
                ref = ref_patch_embed(img, w, bias, cls, pos, dt == torch.bfloat16)
                got, probs = _patch_embed(img.float().to(DEV), wd, bd, cd, pd, T, E, dt)
                e = row_rel(got, ref)                                      # [B, T]
                px = (torch.arange(T) - 1) % Wp
                ragged = (torch.arange(T) > 0) & (px == Wp - 1) & (Wp % VPE_TOK != 0)
                for grp, m in (('cls', torch.arange(T) == 0), ('ragged', ragged), ('rest', (torch.arange(T) > 0) & ~ragged)):
                    if m.any():
                        ee = e[:, m]
                        i = int(ee.reshape(-1).argmax())
                        err[grp].append((ee.reshape(-1)[i].item(), '%s image %d token %d' % (tag, i // ee.shape[1], m.nonzero()[i % ee.shape[1]].item())))
                if B == 3:
                    perm = torch.tensor([2, 0, 1])
                    got2, probs2 = _patch_embed(img[perm].float().to(DEV), wd, bd, cd, pd, T, E, dt)
                    probs += probs2
                    if not torch.equal(got2, got[perm.to(DEV)]):
                        probs.append('the tokens of an image changed with its neighbours')
                out.append(rec(tag + ': guards untouched, finite, images independent%s' % ('' if not probs else ' -- ' + '; '.join(probs)), len(probs), 0))
    for grp, lst in err.items():
        worst = max(lst)
        tol, meas = _tol(('embed', dtype_name, E, grp))
        out.append(rrec('vit_patch_embed[%s E%d] %s tokens vs float64 (per token)' % (dtype_name, E, grp), worst[0], tol,
                        'worst at %s%s' % (worst[1], '' if meas is None else '; measured %.2e' % meas)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# a3_pool
# ---------------------------------------------------------------------------------------------------------------------------------------
A3_MODEL = (257, 27, 768)
A3_AXES = {
    'T': [(T, 27, 768) for T in (1, 63, 64, 65, 257, 288, 500)],          # the 64-lane stride; 500: the raised-LDS path (T * 112 B > 48 KB)
    'S': [(257, S, 768) for S in (1, 4, 27, 28)],
    'C': [(257, 27, C) for C in (1, 255, 256, 257, 512, 513, 768, 1023, 1024)],   # the channels-per-thread boundaries
    'corner': [(500, 28, 1024)],
}


def _sel_view(sel):
    """sel float64 [B, T, S] -> the [:, :S] column view of a [B T, 32] device buffer whose other columns hold NaN"""
    B, T, S = sel.shape
    buf = _filled((B * T, 32), torch.float32, F32_NAN)
    buf[:, :S] = sel.reshape(B * T, S).float().to(DEV)
    return buf[:, :S]


def check_a3_pool(axis, dtype_name):
    from advancedliteratemachinery_amd import ops
    dt = {'fp32': torch.float32, 'bf16': torch.bfloat16}[dtype_name]
    out = []
    ep, ep1, em = [], [], []
    for (T, S, C) in A3_AXES[axis]:
        for B in (1, 3):
            tag = 'a3_pool[%s B%d T%d S%d C%d]' % (dtype_name, B, T, S, C)
            sel = _f32(_randn(B, T, S, seed=T + S, scale=2.0))
            feat = (_bf if dt == torch.bfloat16 else _f32)(_randn(B, T, C, seed=T + C + 1))
            rp, rm = ref_a3_pool(sel, feat)
            sv, fd = _sel_view(sel), feat.to(dt).to(DEV).reshape(B * T, C)
            pooled, maps = ops.a3_pool(sv, fd, B, T, S, True)
            pooled2, none = ops.a3_pool(sv, fd, B, T, S, False)
            torch.cuda.synchronize()
            # C = 1: a pooled row is one sum of 257 signed terms that may cancel, and it is its own scale -- gated apart
            (ep1 if C == 1 else ep).append((row_rel(pooled, rp.reshape(B * S, C)).max().item(), tag))
            em.append((row_rel(maps, rm).max().item(), tag))
            out.append(rec(tag + ': want_attn=False gives the same pooled bits and no maps', 0 if none is None and torch.equal(pooled, pooled2) else 1, 0))
    for grp, lst in (('pooled', ep), ('pooled C1', ep1), ('maps', em)):
        if not lst:
            continue
        worst = max(lst)
        tol, meas = _tol(('a3', dtype_name, axis, grp))
        out.append(rrec('a3_pool[%s, %s walk] %s vs float64 (per output row)' % (dtype_name, axis, grp), worst[0], tol,
                        'worst at %s%s' % (worst[1], '' if meas is None else '; measured %.2e' % meas)))
    return out


def check_a3_onehot():
    """sel = -1e4 with one +1e4 per map: a one-hot softmax, pooled row s is the chosen token's feature row exactly"""
    from advancedliteratemachinery_amd import ops
    out = []
    for (T, S, C) in (A3_MODEL, (500, 28, 1024), (65, 4, 257)):
        for dn, dt in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
            B = 3
            sel, tok = onehot_sel(B, T, S)
            feat = _bf(_randn(B, T, C, seed=T + C + 2))
            pooled, maps = ops.a3_pool(_sel_view(sel), feat.to(dt).to(DEV).reshape(B * T, C), B, T, S, True)
            want = feat.gather(1, tok[..., None].expand(B, S, C)).reshape(B * S, C)
            hot = torch.zeros(B, S, T, dtype=torch.float64).scatter_(2, tok[..., None], 1.0)
            tag = 'a3_pool one-hot[%s T%d S%d C%d]' % (dn, T, S, C)
            out.append(rec(tag + ': pooled == the chosen feature row', float((pooled.double().cpu() != want).sum()), 0))
            out.append(rec(tag + ': maps one-hot', float((maps.double().cpu() != hot).sum()), 0))
    return out


def check_a3_refusals():
    from advancedliteratemachinery_amd import ops
    out = []
    for (T, S, C) in ((257, 29, 768), (257, 27, 1025), (1372, 27, 768)):
        sel = torch.zeros(T, 32, dtype=torch.float32, device=DEV)
        feat = torch.zeros(T, C, dtype=torch.float32, device=DEV)
        got = ''
        try:
            ops.a3_pool(sel[:, :S], feat, 1, T, S, True)
            got = 'no error'
        except RuntimeError:
            pass
        torch.cuda.synchronize()
        out.append(rec('a3_pool[T%d S%d C%d]: refused%s' % (T, S, C, '' if not got else ' -- ' + got), 0 if not got else 1, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# row statistics (ops.gemm_row_argmax_prob = OMP_STORE_ROWSTAT + omp_row_stat_merge)
# ---------------------------------------------------------------------------------------------------------------------------------------
STAT_N = (1, 38, 63, 64, 65, 127, 128, 129, 200)
STAT_M = (1, 3, 4, 5, 129)
STAT_K = 256
STAT_GUARD = 1024


class Operands:
    """A [M, K], W [N, K] (fp32-valued, W / K^(1/2)) as the operands of one engine: bf16, fp32, or bf16x3 (split-pair A rows against the
    [hi | hi | lo] image of the fp32 weight)"""

    def __init__(self, kind, M, N, seed):
        from advancedliteratemachinery_amd import ops
        A, W = rnd(M, STAT_K, seed=seed), rnd(N, STAT_K, seed=seed + 1) / STAT_K ** 0.5
        self.kind, self.M, self.N = kind, M, N
        self.kw = {}
        if kind == 'bf16':
            self.A, self.W = A.to(DEV, torch.bfloat16), W.to(DEV, torch.bfloat16)
        elif kind == 'fp32':
            self.A, self.W = A.to(DEV), W.to(DEV)
        else:
            self.A, self.W = ops.split_bf16(A.to(DEV)), ops.split_weight3(W.to(DEV))
            self.kw = dict(a_wrap=2 * STAT_K)

    def logits(self, bias):
        """the fp32 logits of the same product on the CPU, float64"""
        from advancedliteratemachinery_amd import ops
        return ops.gemm(self.A, self.W, bias, out_dtype=torch.float32, **self.kw).double().cpu()

    def stats(self, bias):
        from advancedliteratemachinery_amd import ops
        i, p = ops.gemm_row_argmax_prob(self.A, self.W, bias, **self.kw)
        return i.cpu().long(), p.double().cpu()

    def records(self, bias):
        """the raw records [M, nt, 4] and whether the guard words behind them survived"""
        from advancedliteratemachinery_amd import _lib, ops
        nt = 2 * ((self.N + 127) // 128)
        n = self.M * nt * 4
        buf = torch.full((n + STAT_GUARD,), -77.0, dtype=torch.float32, device=DEV)
        ops.gemm(self.A, self.W, bias, out=buf[:n].view(self.M, nt, 4), out_dtype=torch.float32, store_mode=_lib.STORE_ROWSTAT, ldc=self.N, **self.kw)
        torch.cuda.synchronize()
        return buf[:n].view(self.M, nt, 4).cpu(), bool((buf[n:] == -77.0).all().item())


def _stat_compare(out, errs, tag, op, bias):
    """ids and probabilities of op's row statistics against float64 softmax / arg-max of the logits of the same product"""
    lg = op.logits(bias)
    ri, rp = ref_row_stats(lg)
    gi, gp = op.stats(bias)
    bad = gi != ri
    note = ''
    if op.kind == 'bf16x3' and lg.shape[1] > 1:   # the near-tie rule of check_gemm_row_stats
        top = lg.sort(-1, descending=True).values
        near = (top[:, 0] - top[:, 1]) < 1e-4
        bad &= ~near
        note = '%d near-ties' % int(near.sum())
    out.append(rec(tag + ': ids identical, every id below N', float(bad.sum()) + float((gi >= op.N).sum()) + float((gi < 0).sum()), 0, note))
    e = ((gp - rp).abs() / rp)
    e = torch.where(torch.isfinite(gp), e, torch.full_like(e, float('inf')))
    errs.append((e.max().item(), tag))


def check_row_stats(kind):
    out, errs = [], []
    for N in STAT_N:
        for M in STAT_M:
            op = Operands(kind, M, N, seed=10 * N + M)
            tag = 'row_stats[%s %dx%dx%d]' % (kind, M, N, STAT_K)
            bias = rnd(N, seed=N + 3, scale=0.2).to(DEV)
            _stat_compare(out, errs, tag + ' random bias', op, bias)
            if M in (1, 5):
                _stat_compare(out, errs, tag + ' no bias', op, None)
                # every true logit far below 0: a padded column read as 0 would win
                _stat_compare(out, errs, tag + ' bias -30', op, torch.full((N,), -30.0, dtype=torch.float32, device=DEV))
                # the scalar bias path (a bias that is not 16-byte aligned) must give the records of the aligned bias; the record of a
                # 64-column half without a valid column is {-inf, 0}; the words behind the records stay untouched
                r0, kept0 = op.records(bias)
                ub = torch.zeros(N + 8, dtype=torch.float32, device=DEV)
                ub[1:N + 1] = bias
                r1, kept1 = op.records(ub[1:N + 1])
                out.append(rec(tag + ': unaligned bias gives the same records, bit for bit', float((r0.view(torch.int32) != r1.view(torch.int32)).sum()), 0))
                out.append(rec(tag + ': guard words behind the records untouched', 0 if kept0 and kept1 else 1, 0))
                nt = r0.shape[1]
                empty = torch.tensor([64 * h >= N for h in range(nt)])
                wrong = (r0[:, empty, 0] != -math.inf).sum() + (r0[:, empty, 1] != 0).sum() + (~torch.isfinite(r0[:, ~empty, 0])).sum() + (r0[:, ~empty, 1] < 1).sum()
                out.append(rec(tag + ': a half without a valid column holds {-inf, 0}, every other a finite maximum and a sum >= 1', float(wrong), 0,
                               '%d of %d halves empty' % (int(empty.sum()), nt)))
        # planted winners: one row, the bias lifts column c 5 above the rest
        op = Operands(kind, 1, N, seed=10 * N)
        lg0 = op.logits(None)
        for c in sorted({c for c in (0, 63, 64, 127, 128, N - 1) if c < N}):
            bias = winner_bias(lg0, c).float().to(DEV)
            tag = 'row_stats[%s 1x%dx%d] planted winner %d' % (kind, N, STAT_K, c)
            gi, _ = op.stats(bias)
            out.append(rec(tag + ': found', 0 if gi.item() == c else 1, 0, 'got %d' % gi.item()))
            _stat_compare(out, errs, tag, op, bias)
    worst = max(errs)
    tol, meas = _tol(('rowstat', kind))
    out.append(rrec('row_stats[%s] probabilities vs float64 softmax of the logits (relative)' % kind, worst[0], tol,
                    'worst at %s%s' % (worst[1], '' if meas is None else '; measured %.2e' % meas)))
    return out
