"""Row-owner chains at every row count the engine launches (csrc/dec_rows.hip for both engines, csrc/kv_rows.hip).

The chains are row-local: output row r depends on input row r and on the weights only.  So every chain is checked in two steps:
  * a BASE launch of 256 distinct rows (ordinary random rows and rows at the LayerNorm's and the arithmetic's edges) against a float64
    restatement on the CPU, every element gated relative to its own row's max |ref| (not the tensor's);
  * every larger launch builds its input on the device by gathering base rows by a fixed index map src[r], and output row r must then be
    row src[r] of the base launch BIT FOR BIT (torch.equal on the device): a 10 k- or 330 k-row launch is checked element by element against
    float64 without recomputing it.  Each of those launches runs twice (the outputs must be identical: a ring that reads a fragment before it
    lands shows up here), its x / q / qkv / logits are buf[:R] views of buffers with 64 guard rows more: the output guard rows hold a sentinel
    bit pattern that must survive, the input guard rows hold NaN that must not reach a valid row.

The float64 restatements (ref_*) take `bf`: True rounds to bf16 exactly where the bf16 chains round (LayerNorm outputs, hidden activations,
q / k / v; the caller passes bf16-valued weights and attention inputs), False is exact float64 -- the reference of the bf16x3 chains.
tests/test_rows_reference.py checks them, with bf=False, against oracle/omniparser_ref.py.

Every check returns rec / rrec records (tests/gpu_checks.py); the measured errors go to the parity report.
"""
import glob
import math
import os

import torch

from tests.gpu_checks import DEV, rec, rrec

D, FF, P = 512, 2048, 1024          # d_model, d_ff, rows of the reference's position tables
NB, GUARD = 256, 64                 # distinct base rows per chain; guard rows behind every launch's buffers
EPS = 1e-5
POSITIONS = (0, 1, P - 1)
VOCABS = (4, 124, 128, 132, 1104, 1108, 1232)
BIG_DEC = (10240, 10277)            # the benchmark's decoder rows (160 images x 64 instances) and a ragged neighbour
SWIN_R = (1, 79, 80, 81, 1000, 65536 + 13, 327680 + 13)
X3_R = (1, 47, 48, 49, 4096, 10277)
F32_GUARD = 0x7FC0DEAD              # NaN payloads: input guard rows (must not leak) and output guard rows (must survive)
BF16_GUARD = 0x7FA5
F32_SENT = 0x7FA5A5A5

# Gates, relative to each row's own max |ref|, per (engine, chain, output, rows): 'random' = the ordinary random base rows, 'edge' = the
# EDGE_ROWS (the fp32 rounding of a near-constant LayerNorm input, amplified by 1 / sqrt(eps), and of a row at 300 +- 1 is a real difference
# from exact float64 there).  Each gate is at most 4x the worst case measured on an MI355X; (gate, measured) -- the measured value is also
# in the record's note.
TOL = {
    ('bf16', 'embed', 'qkv', 'edge'): (1.5e-02, 4.78e-03),
    ('bf16', 'embed', 'qkv', 'random'): (1.3e-02, 4.33e-03),
    ('bf16', 'embed', 'x', 'edge'): (2.1e-04, 6.70e-05),
    ('bf16', 'embed', 'x', 'random'): (2.9e-05, 9.40e-06),
    ('bf16', 'ffn', 'logits', 'edge'): (1.3e-02, 4.20e-03),
    ('bf16', 'ffn', 'logits', 'random'): (1.3e-02, 4.21e-03),
    ('bf16', 'ffn', 'qkv', 'edge'): (1.4e-02, 4.59e-03),
    ('bf16', 'ffn', 'qkv', 'random'): (1.5e-02, 4.69e-03),
    ('bf16', 'ffn', 'x', 'edge'): (1.4e-03, 4.44e-04),
    ('bf16', 'ffn', 'x', 'random'): (5.7e-04, 1.89e-04),
    ('bf16', 'kv', 'K', 'all'): (1.5e-02, 5.00e-03),
    ('bf16', 'kv', 'V', 'all'): (1.8e-02, 5.68e-03),
    ('bf16', 'mid', 'q', 'edge'): (1.6e-02, 5.03e-03),
    ('bf16', 'mid', 'q', 'random'): (1.5e-02, 4.67e-03),
    ('bf16', 'mid', 'x', 'edge'): (3.0e-07, 9.90e-08),
    ('bf16', 'mid', 'x', 'random'): (6.6e-07, 2.17e-07),
    ('bf16', 'swin0', 'qkv', 'edge'): (1.1e-02, 3.52e-03),
    ('bf16', 'swin0', 'qkv', 'random'): (1.5e-02, 4.74e-03),
    ('bf16', 'swin0', 'x', 'edge'): (0.0, 0.00e+00),
    ('bf16', 'swin0', 'x', 'random'): (0.0, 0.00e+00),
    ('bf16', 'swin1', 'qkv', 'edge'): (1.5e-02, 4.76e-03),
    ('bf16', 'swin1', 'qkv', 'random'): (1.5e-02, 4.98e-03),
    ('bf16', 'swin1', 'x', 'edge'): (1.1e-03, 3.56e-04),
    ('bf16', 'swin1', 'x', 'random'): (4.8e-04, 1.59e-04),
    ('x3', 'embed', 'qkv', 'edge'): (1.2e-04, 3.91e-05),
    ('x3', 'embed', 'qkv', 'random'): (3.1e-05, 1.03e-05),
    ('x3', 'embed', 'x', 'edge'): (2.1e-04, 6.70e-05),
    ('x3', 'embed', 'x', 'random'): (2.9e-05, 9.40e-06),
    ('x3', 'ffn', 'logits', 'edge'): (5.1e-04, 1.70e-04),
    ('x3', 'ffn', 'logits', 'random'): (5.3e-05, 1.74e-05),
    ('x3', 'ffn', 'qkv', 'edge'): (5.3e-04, 1.73e-04),
    ('x3', 'ffn', 'qkv', 'random'): (2.5e-05, 8.28e-06),
    ('x3', 'ffn', 'x', 'edge'): (7.7e-05, 2.56e-05),
    ('x3', 'ffn', 'x', 'random'): (1.3e-05, 4.30e-06),
    ('x3', 'mid', 'q', 'edge'): (1.3e-04, 4.31e-05),
    ('x3', 'mid', 'q', 'random'): (2.6e-05, 8.54e-06),
    ('x3', 'mid', 'x', 'edge'): (5.6e-06, 1.85e-06),
    ('x3', 'mid', 'x', 'random'): (9.6e-06, 3.19e-06),
    ('x3', 'swin0', 'qkv', 'edge'): (7.3e-05, 2.41e-05),
    ('x3', 'swin0', 'qkv', 'random'): (1.9e-05, 6.17e-06),
    ('x3', 'swin0', 'x', 'edge'): (0.0, 0.00e+00),
    ('x3', 'swin0', 'x', 'random'): (0.0, 0.00e+00),
    ('x3', 'swin1', 'qkv', 'edge'): (4.9e-04, 1.61e-04),
    ('x3', 'swin1', 'qkv', 'random'): (2.3e-05, 7.46e-06),
    ('x3', 'swin1', 'x', 'edge'): (3.4e-05, 1.11e-05),
    ('x3', 'swin1', 'x', 'random'): (1.4e-05, 4.50e-06),
}


def _tol(eng, cls, out, group):
    return TOL[(eng, cls, out, group)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------------------------------------------------------
def rb(t, bf):
    """bf16 rounding where the bf16 chains round (bf), identity otherwise; float64 in, float64 out"""
    return t.to(torch.bfloat16).double() if bf else t


def ln64(x, g, b, eps=EPS):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * g + b


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ref_mid(x, att, Wo, bo, g2, b2, Wq, qtab, pos, bf):
    """omp_dec_rows_mid: x += att Wo^T + bo;  q = LN(x) Wq^T + qtab[pos]  -> (x', q)"""
    x1 = x + att @ Wo.T + bo
    return x1, rb(rb(ln64(x1, g2, b2), bf) @ Wq.T + qtab[pos], bf)


def ref_ffn_body(x, att, Wc, bc, g3, b3, W1, b1, W2, b2, bf, act='relu'):
    """out-projection + residual, LN, FFN (ReLU: decoder; exact-erf GELU: Swin) + residual -> x'"""
    xa = x + att @ Wc.T + bc
    h = rb(ln64(xa, g3, b3), bf) @ W1.T + b1
    h = rb(torch.relu(h) if act == 'relu' else gelu64(h), bf)
    return xa + h @ W2.T + b2


def ref_qkv_tail(x, g, b, Win, bias_row, bf):
    """next layer's norm1 + in_proj (+ position term in bias_row) / Swin norm1 + qkv: bf16(LN(x) Win^T + bias_row)"""
    return rb(rb(ln64(x, g, b), bf) @ Win.T + bias_row, bf)


def ref_head_tail(x, g, b, H, hb, bf):
    """final norm, then the prediction head h2(relu(h1(relu(h0(LN(x))))))"""
    y = rb(ln64(x, g, b), bf)
    t0 = rb(torch.relu(y @ H[0].T + hb[0]), bf)
    t1 = rb(torch.relu(t0 @ H[1].T + hb[1]), bf)
    return t1 @ H[2].T + hb[2]


def ref_embed(tok, word, ptab, pos, g, b):
    """the embedding prologue: LN(word[tok] + pos_tab[pos])"""
    return ln64(word[tok.long()] + ptab[pos], g, b)


def ref_kv(mem_pos, mem, Wk, bk, Wv, bv, bf):
    """memory projection of all slabs: K = (mem + pos) Wk^T + bk, V = mem Wv^T + bv  ([rows, n_slabs * 512] each, natural order)"""
    return rb(mem_pos @ Wk.T + bk, bf), rb(mem @ Wv.T + bv, bf)


def vt_slot(kl):
    """slot of key kl (0..31) inside a 32-key block of the V^T slabs (tests/gpu_checks.py check_kv_rows)"""
    return ((kl & 15) >> 2) * 8 + (kl >> 4) * 4 + (kl & 3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_g(seed), dtype=torch.float64) * scale


EDGE_ROWS = ('zeros', 'constant', 'variance below eps', 'offset 300 +- 1', 'outlier channel x50', 'scale 1e-3', 'scale 1e4')


def edge_rows(seed, ln_bias=None, with_att=True):
    """NB base rows (x fp32-valued, att) whose LayerNorm input x + att W^T + ln_bias (ln_bias None: x itself) reaches the edges:
    rows 0..6 = EDGE_ROWS, the rest ordinary random rows.  The LayerNorm input of the constant / small-variance rows is planted through x
    with a zero att row (the product is then exactly 0): x = c - bias in fp32."""
    x = _randn(NB, D, seed=seed, scale=2.0)
    att = _randn(NB, D, seed=seed + 1)
    bias = torch.zeros(D, dtype=torch.float64) if ln_bias is None else ln_bias
    b32 = bias.float()
    x[0] = 0.0
    att[0] = 0.0
    x[1] = (0.5 - b32).double()
    att[1] = 0.0
    x[2] = (0.5 + 1e-4 * _randn(D, seed=seed + 2).float() - b32).double()   # variance ~1e-8 < eps
    att[2] = 0.0
    x[3] = 300.0 + _randn(D, seed=seed + 3)
    x[4] = _randn(D, seed=seed + 4)
    x[4, 37] = 50.0
    x[5] *= 1e-3
    att[5] *= 1e-3
    x[6] *= 1e4
    att[6] *= 1e4
    x = x.float().double()
    return (x, att) if with_att else x


def src_map(R, mult=101, add=13):
    """row r of a launch is base row src[r]: a permutation inside every window of NB rows, shifted against the tiles"""
    return (torch.arange(R, dtype=torch.int64, device=DEV) * mult + add) % NB


def _weights(seed, x3, n, k):
    w = _randn(n, k, seed=seed) / k ** 0.5
    return w.float().double() if x3 else w.to(torch.bfloat16).double()


def _vec(seed, n, s=0.1):
    return (_randn(n, seed=seed) * s).float().double()


def _dev(t, dt=torch.float32):
    return t.to(dt).to(DEV).contiguous()


def row_rel(got, ref):
    """per row: max |got - ref| / max |ref| of that row; -> (worst, index of the worst row).  A non-finite value is an infinite error."""
    g = got.double().cpu().reshape(ref.shape[0], -1)
    r = ref.reshape(ref.shape[0], -1)
    e = (g - r).abs().max(1).values / r.abs().max(1).values.clamp_min(1e-300)
    e = torch.where(torch.isfinite(g).all(1), e, torch.full_like(e, float('inf')))
    i = int(e.argmax())
    return e[i].item(), i


def _gate(out, name, got, ref, key):
    """per-row relative error of got against the float64 ref, the random rows and the edge rows (the first len(EDGE_ROWS)) gated apart"""
    n = len(EDGE_ROWS) if key[2] != 'K' and key[2] != 'V' else 0
    for group, lo, hi in (('random' if n else 'all', n, ref.shape[0]), ('edge', 0, n)):
        if hi <= lo:
            continue
        err, i = row_rel(got[lo:hi], ref[lo:hi])
        i += lo
        tol, meas = _tol(*key, group)
        note = '%s' % ' '.join(map(str, key)) + '; worst row %d%s' % (i, ' (%s)' % EDGE_ROWS[i] if group == 'edge' else '')
        if meas is not None:
            note += '; measured %.2e' % meas
        out.append(rrec('%s [%s rows]' % (name, group), err, tol, note))


# ---------------------------------------------------------------------------------------------------------------------------------------
# launches with guard rows
# ---------------------------------------------------------------------------------------------------------------------------------------
def _guarded(R, width, dtype, fill_bits, rows=None):
    """[R + GUARD, width] buffer: rows[:R] (or uninitialised-free fill), guard rows = fill_bits"""
    buf = torch.empty((R + GUARD, width), dtype=dtype, device=DEV)
    buf.view(torch.int32 if dtype == torch.float32 else torch.int16).fill_(fill_bits)
    if rows is not None:
        buf[:R] = rows
    return buf


def _bits_kept(buf, R, fill_bits):
    v = buf[R:].view(torch.int32 if buf.dtype == torch.float32 else torch.int16)
    return bool((v == fill_bits).all().item())


class Chain:
    """one chain kind of one engine: base inputs on the device, a launcher, the output names"""

    def __init__(self, name, eng, base, launch, outs):
        self.name, self.eng, self.base, self.launch, self.outs = name, eng, base, launch, outs

    def run(self, R, src=None):
        """-> (outputs {name: [R, w] view}, problems [str]).  Input x / att / seq are gathered base rows; guards checked."""
        if src is None:
            src = torch.arange(R, device=DEV)
        bufs, probs = {}, []
        for k, (t, kind) in self.base.items():
            if kind == 'in':          # read only: NaN guard rows
                bufs[k] = _guarded(R, t.shape[1], t.dtype, F32_GUARD if t.dtype == torch.float32 else BF16_GUARD, t[src])
            elif kind == 'inout':     # the residual stream (in place): NaN guard rows that must also stay as they are
                bufs[k] = _guarded(R, t.shape[1], t.dtype, F32_GUARD, t[src])
            elif kind == 'plain':     # token ids: gathered, no guard
                bufs[k] = t[src].contiguous()
        for k, w, dt in self.outs_alloc():
            bufs[k] = _guarded(R, w, dt, F32_SENT if dt == torch.float32 else BF16_GUARD)
        self.launch({k: (v[:R] if k != 'seq' else v) for k, v in bufs.items()})
        torch.cuda.synchronize()
        for k, (t, kind) in self.base.items():
            if kind in ('in', 'inout') and not _bits_kept(bufs[k], R, F32_GUARD if bufs[k].dtype == torch.float32 else BF16_GUARD):
                probs.append('input %s: guard rows changed' % k)
        for k, w, dt in self.outs_alloc():
            if not _bits_kept(bufs[k], R, F32_SENT if dt == torch.float32 else BF16_GUARD):
                probs.append('output %s: a row past R was written' % k)
        res = {}
        for k in self.outs:
            v = bufs[k][:R]
            if not bool(torch.isfinite(v).all().item()):
                probs.append('%s: a valid row holds NaN / inf' % k)
            res[k] = v
        return res, probs

    def outs_alloc(self):
        return [(k, w, dt) for k, (w, dt) in self.out_shapes.items()]


def _compare(out, tag, got, base, src, probs):
    """got[k] == base[k][src] bit for bit, every output"""
    bad = [k for k in got if not torch.equal(got[k], base[k][src])]
    out.append(rec(tag + ': every row == its source row of the base launch, bit for bit%s' % ('' if not bad else ' -- differs: %s' % bad),
                   len(bad), 0))
    out.append(rec(tag + ': guard rows untouched, no NaN / inf in valid rows' + ('' if not probs else ' -- %s' % '; '.join(probs)), len(probs), 0))


def _sweep(out, ch, tag, Rs, base, twice=True, src_of=src_map):
    """every R: bit-identical to the base launch through src; run twice (deterministic)"""
    for R in Rs:
        src = src_of(R)
        got, probs = ch.run(R, src)
        _compare(out, '%s R=%d' % (tag, R), got, base, src, probs)
        if twice:
            again, _ = ch.run(R, src)
            same = all(torch.equal(got[k], again[k]) for k in got)
            out.append(rec('%s R=%d: second launch identical (deterministic)' % (tag, R), 0 if same else 1, 0))
        del got


# ---------------------------------------------------------------------------------------------------------------------------------------
# decoder chains
# ---------------------------------------------------------------------------------------------------------------------------------------
def _att_dev(att, x3):
    from advancedliteratemachinery_amd import ops
    if x3:
        return ops.split_bf16(_dev(att))       # split pairs [NB, 1024]
    return _dev(att, torch.bfloat16)


def _dec_setup(x3, seed):
    """weights of one decoder layer pair (mid + ffn) with their packed streams, float64 copies (bf16- / fp32-valued as the engine sees them)"""
    W = dict(Wo=_weights(seed + 1, x3, D, D), Wq=_weights(seed + 2, x3, D, D), Wc=_weights(seed + 3, x3, D, D), W1=_weights(seed + 4, x3, FF, D),
             W2=_weights(seed + 5, x3, D, FF), Win=_weights(seed + 6, x3, 3 * D, D), H0=_weights(seed + 7, x3, D, D), H1=_weights(seed + 8, x3, D, D))
    v = dict(bo=_vec(seed + 10, D), g2=1 + _vec(seed + 11, D), b2=_vec(seed + 12, D), bc=_vec(seed + 13, D), g3=1 + _vec(seed + 14, D),
             b3=_vec(seed + 15, D), b1=_vec(seed + 16, FF), bb2=_vec(seed + 17, D), gt=1 + _vec(seed + 18, D), bt=_vec(seed + 19, D),
             hb0=_vec(seed + 20, D), hb1=_vec(seed + 21, D))
    v['qtab'] = (_randn(P, D, seed=seed + 22) * 0.3).float().double()
    v['tab'] = (_randn(P, 3 * D, seed=seed + 23) * 0.3).float().double()
    W.update(v)
    return W


def _wdev(W, k, x3):
    return _dev(W[k], torch.float32 if x3 else torch.bfloat16)


def dec_chain(kind, x3, W, pos, vocab=1104, seed=100):
    """-> (Chain, float64 reference of the base launch {out: [NB, w]}) for kind in mid / ffn_qkv / ffn_head / embed"""
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.model import packing
    bf = not x3
    eng = 'x3' if x3 else 'bf16'
    odt = torch.float32 if x3 else torch.bfloat16
    dpos = torch.tensor([pos, 0], dtype=torch.int32, device=DEV)
    wd = lambda k: _wdev(W, k, x3)        # noqa: E731
    vd = lambda k: _dev(W[k])             # noqa: E731
    if kind == 'embed':
        V = 1104
        ptab = (_randn(P, D, seed=seed + 40) * 0.5).float().double()
        word = _randn(V, D, seed=seed + 41).float().double()
        p32 = ptab[pos].float()
        word[1] = 300.0 + _randn(D, seed=seed + 42)
        word[2] = _randn(D, seed=seed + 43)
        word[2, 37] = 50.0
        word[3] *= 1e-3
        word[4] *= 1e4
        word[5] = (-p32).double()                                                    # LayerNorm input 0
        word[6] = (0.5 - p32).double()                                               # constant
        word[7] = (0.5 + 1e-4 * _randn(D, seed=seed + 44).float() - p32).double()    # variance below eps
        word = word.float().double()
        tok = torch.randint(0, V, (NB,), generator=_g(seed + 45), dtype=torch.int32)
        tok[:9] = torch.tensor([5, 6, 7, 1, 2, 3, 4, 0, V - 1], dtype=torch.int32)
        ge, be = 1 + _vec(seed + 46, D), _vec(seed + 47, D)
        xe = ref_embed(tok, word, ptab, pos, ge, be)
        ref = dict(x=xe, qkv=ref_qkv_tail(xe, W['gt'], W['bt'], W['Win'], W['tab'][pos], bf))
        stream, stride = packing.pack_rows_embed_qkv(wd('Win'))
        seq = tok[:, None].expand(NB, P).contiguous().to(DEV)                        # every column the same token: seq[r, pos]
        emb = (_dev(word), _dev(ptab), _dev(ge), _dev(be))
        tabd, gtd, btd = vd('tab'), vd('gt'), vd('bt')

        def launch(b):
            ops.dec_rows_ffn(b['x'], stream, stride, dpos, gtd, btd, embed=(b['seq'],) + emb, bias_tab=tabd, qkv=b['qkv'], x3=x3,
                             xcd_mask=launch.mask)
        x_in = torch.empty(NB, D, device=DEV)
        x_in.view(torch.int32).fill_(F32_GUARD)  # the prologue writes x: its input rows are NaN too
        ch = Chain('embed', eng, dict(x=(x_in, 'inout'), seq=(seq, 'plain')), launch, ('x', 'qkv'))
        ch.out_shapes = dict(qkv=(3 * D, odt))
        launch.mask = 0
        ch.cls = 'embed'
        return ch, ref
    ln_bias = W['bo'] if kind == 'mid' else W['bc']
    x, att = edge_rows(seed, ln_bias)
    att = rb(att, bf).float().double() if bf else att.float().double()
    base = dict(x=(_dev(x), 'inout'), att=(_att_dev(att, x3), 'in'))
    if kind == 'mid':
        x1, q = ref_mid(x, att, W['Wo'], W['bo'], W['g2'], W['b2'], W['Wq'], W['qtab'], pos, bf)
        ref = dict(x=x1, q=q)
        stream, stride = packing.pack_rows_mid(wd('Wo'), wd('Wq'))
        bod, g2d, b2d, qtd = vd('bo'), vd('g2'), vd('b2'), vd('qtab')

        def launch(b):
            ops.dec_rows_mid(b['att'], b['x'], stream, stride, bod, g2d, b2d, qtd, dpos, q=b['q'], x3=x3, xcd_mask=launch.mask, pos_mod=launch.pos_mod)
        ch = Chain('mid', eng, base, launch, ('x', 'q'))
        ch.out_shapes = dict(q=(D, odt))
        launch.pos_mod = 0          # > 0: row r sits at position r % pos_mod and dpos (ch.dpos: the check moves it) is not read
        ch.dpos = dpos
    else:
        x2 = ref_ffn_body(x, att, W['Wc'], W['bc'], W['g3'], W['b3'], W['W1'], W['b1'], W['W2'], W['bb2'], bf)
        common = dict(out_b=vd('bc'), ln_g=vd('g3'), ln_b=vd('b3'), ff1_b=vd('b1'), ff2_b=vd('bb2'), x3=x3)
        gtd, btd = vd('gt'), vd('bt')
        if kind == 'ffn_qkv':
            ref = dict(x=x2, qkv=ref_qkv_tail(x2, W['gt'], W['bt'], W['Win'], W['tab'][pos], bf))
            stream, stride = packing.pack_rows_ffn_qkv(wd('Wc'), wd('W1'), wd('W2'), wd('Win'))
            tabd = vd('tab')

            def launch(b):
                ops.dec_rows_ffn(b['x'], stream, stride, dpos, gtd, btd, att=b['att'], bias_tab=tabd, qkv=b['qkv'], xcd_mask=launch.mask, **common)
            ch = Chain('ffn_qkv', eng, base, launch, ('x', 'qkv'))
            ch.out_shapes = dict(qkv=(3 * D, odt))
        else:
            H2 = _weights(seed + 50 + vocab, x3, vocab, D)
            hb2 = _vec(seed + 51 + vocab, vocab)
            ref = dict(x=x2, logits=ref_head_tail(x2, W['gt'], W['bt'], (W['H0'], W['H1'], H2), (W['hb0'], W['hb1'], hb2), bf))
            h2d = H2.float() if x3 else H2.to(torch.bfloat16)
            stream, stride = packing.pack_rows_ffn_head(wd('Wc'), wd('W1'), wd('W2'), wd('H0'), wd('H1'), h2d.to(DEV))
            hbd = (vd('hb0'), vd('hb1'), _dev(hb2))

            def launch(b):
                ops.dec_rows_ffn(b['x'], stream, stride, dpos, gtd, btd, att=b['att'], head_b=hbd, logits=b['logits'], vocab=vocab,
                                 xcd_mask=launch.mask, **common)
            ch = Chain('ffn_head[vocab %d]' % vocab, eng, base, launch, ('x', 'logits'))
            ch.out_shapes = dict(logits=(vocab, torch.float32))
    launch.mask = 0
    ch.cls = 'mid' if kind == 'mid' else 'ffn'
    return ch, ref


def _base_vs_ref(out, ch, ref, tag):
    got, probs = ch.run(NB)
    for k in ch.outs:
        _gate(out, '%s %s vs float64 (per-row relative)' % (tag, k), got[k], ref[k], (ch.eng, ch.cls, k))
    out.append(rec(tag + ': guard rows untouched, no NaN / inf in valid rows' + ('' if not probs else ' -- %s' % '; '.join(probs)), len(probs), 0))
    return got


def fixture_vocabs():
    """num_classes of every committed fixture's args (tests/golden/*.pt)"""
    from advancedliteratemachinery_amd.utils.parser import make_args
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    vs = set()
    for f in sorted(glob.glob(os.path.join(here, '*.pt'))):
        d = torch.load(f, map_location='cpu', weights_only=False)
        c = d.get('case') if isinstance(d, dict) else None
        if isinstance(c, dict) and isinstance(c.get('args'), dict):
            vs.add(make_args(**c['args']).num_classes)
    return sorted(vs)


def tile_sweep():
    """-> (row counts of the bf16 decoder sweep, {mid: tiles the automatic rule can choose}, {mid: tiles the sweep reaches}).
    The tile boundaries come from ops.rows_tile_choice (the rule itself), not from constants."""
    from advancedliteratemachinery_amd import ops
    half = torch.cuda.get_device_properties(0).multi_processor_count // 2
    top = 80 * half + 1000
    Rs = {1, 15, 16, 17, 200} | set(BIG_DEC)
    can, reached = {}, {}
    for mid in (False, True):
        ch = [ops.rows_tile_choice(R, mid) for R in range(1, top + 1)]
        can[mid] = set(ch)
        for R in range(1, top):
            if ch[R - 1] != ch[R]:
                Rs |= {R, R + 1}
    for mid in (False, True):
        reached[mid] = {ops.rows_tile_choice(R, mid) for R in Rs}
    return sorted(Rs), can, reached


def check_rows_tile_rule():
    """the automatic tile rule (csrc/dec_rows.hip rows_rtt) against its statement: the smallest tile of {16 (mid only), 32, 48, 64, 80} rows
    that keeps a launch on half the chip's CUs, else 80; and the sweep of the decoder checks reaches every tile it can choose"""
    from advancedliteratemachinery_amd import ops
    half = torch.cuda.get_device_properties(0).multi_processor_count // 2
    out = []
    for mid in (False, True):
        tiles = (16, 32, 48, 64, 80) if mid else (32, 48, 64, 80)
        bad = 0
        for R in range(1, 80 * half + 1000):
            want = next((t for t in tiles[:-1] if -(-R // t) <= half), 80)
            bad += ops.rows_tile_choice(R, mid) != want
        out.append(rec('rows_tile_choice(R, mid=%s) == smallest tile keeping ceil(R / tile) <= %d workgroups, R = 1 .. %d' % (mid, half, 80 * half + 999), bad, 0))
    Rs, can, reached = tile_sweep()
    for mid in (False, True):
        out.append(rec('decoder sweep %s reaches every tile the rule chooses for %s: %s (reached %s)'
                       % (Rs, 'mid' if mid else 'ffn', sorted(can[mid]), sorted(reached[mid])), len(can[mid] - reached[mid]), 0))
    return out


def check_dec_chain(kind, x3=False):
    """one decoder chain kind: float64 at every position (and, for the head, every vocabulary) on the base rows; then the row-count sweep
    (bf16: auto tile + every forced tile; x3: its 48-row tile) bit-identical to the base launch, twice, with guards"""
    from advancedliteratemachinery_amd import ops
    out = []
    eng = 'x3' if x3 else 'bf16'
    W = _dec_setup(x3, 0)
    tag0 = 'rows[%s] %s' % (eng, kind)
    if kind == 'ffn_head':
        vocabs = sorted(set(VOCABS) | set(fixture_vocabs()))
        out.append(rec(tag0 + ': every vocabulary %% 4 == 0 (%s)' % vocabs, sum(v % 4 != 0 for v in vocabs), 0))
        for V in vocabs:
            ch, ref = dec_chain(kind, x3, W, P - 1, vocab=V)
            base = _base_vs_ref(out, ch, ref, '%s vocab=%d R=%d' % (tag0, V, NB))
            _sweep(out, ch, '%s vocab=%d' % (tag0, V), (1, 17, 129), base, twice=False)
        ch, ref = dec_chain(kind, x3, W, P - 1, vocab=1104)
    else:
        for pos in POSITIONS:   # the last one (P - 1) is the sweep's
            ch, ref = dec_chain(kind, x3, W, pos)
            _base_vs_ref(out, ch, ref, '%s pos=%d R=%d' % (tag0, pos, NB))
    if x3:
        base = ch.run(NB)[0]
        _sweep(out, ch, tag0 + ' pos=%d' % (P - 1), X3_R, base)
        return out
    mid = kind == 'mid'
    Rs, _, _ = tile_sweep()
    try:
        # the base launch at every tile: the auto tile at 256 rows and every forced one
        ops.rows_tile(0)
        auto_t = ops.rows_tile_choice(NB, mid)
        base = {auto_t: ch.run(NB)[0]}
        for rtt in (2, 3, 4, 5):
            ops.rows_tile(rtt)
            got = ch.run(NB)[0]
            if 16 * rtt not in base:
                base[16 * rtt] = got
            same = all(torch.equal(got[k], base[auto_t][k]) for k in got)
            out.append(rec('%s: base launch at %d rows per workgroup == at %d (auto), bit for bit' % (tag0, 16 * rtt, auto_t), 0 if same else 1, 0))
            # held at this forced tile: a ragged large launch with another row placement
            src2 = lambda R: src_map(R, 37, 101)    # noqa: E731
            _sweep(out, ch, '%s tile %d (forced)' % (tag0, 16 * rtt), (4097,), base[16 * rtt], twice=False, src_of=src2)
        ops.rows_tile(0)
        for R in Rs:
            t = ops.rows_tile_choice(R, mid)
            _sweep(out, ch, '%s auto tile %d' % (tag0, t), (R,), base[t])
    finally:
        ops.rows_tile(0)
    return out


MID_POS_MODS = (1, 2, 6, 7, P)      # P: the largest the check's qtab has rows for
MID_POS_ROWS = (1, 15, 16, 17, 200, 2049)


def ref_mid_rows(W, x, att, pos_of_row):
    """ref_mid with a position per row (bf16 chains) -> (x', q): row r at position pos_of_row[r]"""
    x1, q = zip(*[ref_mid(x[r:r + 1], att[r:r + 1], W['Wo'], W['bo'], W['g2'], W['b2'], W['Wq'], W['qtab'], int(pos_of_row[r]), True)
                  for r in range(x.shape[0])])
    return torch.cat(x1), torch.cat(q)


def one_position_launches(ch, positions):
    """the one-position form of the mid chain on the NB base rows at every position in `positions`
    -> (x' [NB, D] of the first, q [len(positions), NB, D], positions whose x' differs from the first's)"""
    xb, ab = ch.base['x'][0], ch.base['att'][0]
    q = torch.empty((len(positions), NB, D), dtype=torch.bfloat16, device=DEV)
    x0, differ = None, torch.zeros((), dtype=torch.int64, device=DEV)
    ch.launch.pos_mod = 0
    for i, pos in enumerate(positions):
        ch.dpos[0] = pos
        x = xb.clone()
        ch.launch(dict(att=ab, x=x, q=q[i]))
        if x0 is None:
            x0 = x
        differ += (x.view(torch.int32) != x0.view(torch.int32)).any()
    torch.cuda.synchronize()
    return x0, q, int(differ.item())


def compare_pos_mod(out, tag, got, probs, src, L, x0, qpos):
    """row r of a pos_mod = L launch of the base rows src[r] == row src[r] of the one-position launch at position r % L, bit for bit"""
    pos = torch.arange(src.shape[0], device=src.device) % L
    bad = [k for k, want in (('x', x0[src]), ('q', qpos[pos, src])) if not torch.equal(got[k], want)]
    out.append(rec(tag + ': every row == its row of the one-position launch at r %% %d, bit for bit%s' % (L, '' if not bad else ' -- differs: %s' % bad),
                   len(bad), 0))
    out.append(rec(tag + ': guard rows untouched, no NaN / inf in valid rows' + ('' if not probs else ' -- %s' % '; '.join(probs)), len(probs), 0))


_MID_POS_BASE = []


def mid_pos_base():
    """(weights, chain, base x / att on the host, one-position launches at every position) -- launched once, shared by every pos_mod"""
    from advancedliteratemachinery_amd import ops
    if not _MID_POS_BASE:
        W = _dec_setup(False, 0)
        ch, _ = dec_chain('mid', False, W, 0)
        ops.rows_tile(0)
        _MID_POS_BASE.append((W, ch, ch.base['x'][0].double().cpu(), ch.base['att'][0].double().cpu()) + one_position_launches(ch, list(range(P))))
    return _MID_POS_BASE[0]


def check_dec_mid_pos_mod(L):
    """omp_dec_rows_args.pos_mod (dec_rows_mid_kernel<RTT, E, ROWPOS>: the batched prompt prefill's form of the mid chain): float64 with a
    position per row, and bit for bit the one-position launch at each row's position, at the auto tiles (16 rows up to 2048, 32 at 2049) and
    at every forced tile; d_pos holds a position no row of the launch sits at (it is not read)"""
    from advancedliteratemachinery_amd import ops
    out = []
    W, ch, x_h, att_h, x0, qpos, differ = mid_pos_base()
    tag0 = 'rows[bf16] mid pos_mod'
    try:
        ops.rows_tile(0)
        out.append(rec(tag0 + ': x is the same at every position 0 .. %d (one-position launches)' % (P - 1), differ, 0))
        out.append(rec(tag0 + ': auto tile 16 at R = 200, 32 at R = 2049 (got %d, %d)' % (ops.rows_tile_choice(200, True), ops.rows_tile_choice(2049, True)),
                       int(ops.rows_tile_choice(200, True) != 16) + int(ops.rows_tile_choice(2049, True) != 32), 0))
        ch.launch.pos_mod = L
        ch.dpos[0] = P - 3 if L < P else 0        # not a position of this launch (L = P: every position is one; row 0's then)
        tag = '%s=%d' % (tag0, L)
        # float64: the NB base rows in order, row r at position r % L
        got, probs = ch.run(NB)
        rx, rq = ref_mid_rows(W, x_h, att_h, [r % L for r in range(NB)])
        _gate(out, tag + ' R=%d x vs float64 (per-row relative)' % NB, got['x'], rx, ('bf16', 'mid', 'x'))
        _gate(out, tag + ' R=%d q vs float64 (per-row relative)' % NB, got['q'], rq, ('bf16', 'mid', 'q'))
        compare_pos_mod(out, tag + ' R=%d' % NB, got, probs, torch.arange(NB, device=DEV), L, x0, qpos)
        for R in MID_POS_ROWS:
            src = src_map(R)
            got, probs = ch.run(R, src)
            compare_pos_mod(out, '%s R=%d auto tile %d' % (tag, R, ops.rows_tile_choice(R, True)), got, probs, src, L, x0, qpos)
        for rtt in (2, 3, 4, 5):
            ops.rows_tile(rtt)
            src = src_map(4097, 37, 101)
            got, probs = ch.run(4097, src)
            compare_pos_mod(out, '%s R=4097 tile %d (forced)' % (tag, 16 * rtt), got, probs, src, L, x0, qpos)
        ops.rows_tile(0)
        if L != 6:
            return out
        # the masked grid
        ch.launch.pos_mod = 6
        src = src_map(200)
        plain, _ = ch.run(200, src)
        ch.launch.mask = 0x0F
        got, probs = ch.run(200, src)
        same = all(torch.equal(got[k], plain[k]) for k in got)
        out.append(rec(tag0 + '=6 R=200: xcd_mask 0x0F == unmasked, bit for bit%s' % ('' if not probs else ' -- ' + '; '.join(probs)), (0 if same else 1) + len(probs), 0))
        compare_pos_mod(out, tag0 + '=6 R=200 xcd_mask 0x0F', got, probs, src, 6, x0, qpos)
    finally:
        ch.launch.mask, ch.launch.pos_mod = 0, 0
        ops.rows_tile(0)
    return out


def check_dec_mid_pos_mod_refusals():
    """pos_mod < 0, and pos_mod with the split-pair chain: OMP_ERR_INVALID, x keeps its bits and q its sentinels"""
    out = []
    for x3, pos_mod in ((False, -1), (True, 6), (True, -1)):
        ch, _ = dec_chain('mid', x3, _dec_setup(x3, 0), 0)
        inner, err = ch.launch, []

        def launch(b):
            try:
                inner(b)
            except RuntimeError as e:
                err.append(str(e))
        inner.pos_mod = pos_mod
        ch.launch = launch
        R = 200
        src = src_map(R)
        got, probs = ch.run(R, src)
        probs = [p for p in probs if 'valid row holds NaN' not in p]       # q keeps its sentinel, a NaN payload
        name = 'rows[%s] mid pos_mod=%d' % (ch.eng, pos_mod)
        ok = len(err) == 1 and '(-22)' in err[0] and 'omp_dec_rows_mid: pos_mod' in err[0]
        out.append(rec(name + ': refused with -22%s' % ('' if ok else ' -- %s' % (err or 'no error')), 0 if ok else 1, 0))
        qi = got['q'].view(torch.int32 if got['q'].dtype == torch.float32 else torch.int16)
        kept = bool((qi == (F32_SENT if got['q'].dtype == torch.float32 else BF16_GUARD)).all().item()) and \
            torch.equal(got['x'].view(torch.int32), ch.base['x'][0][src].view(torch.int32))
        out.append(rec(name + ': nothing written (x its bits, q its sentinels, guard rows)%s' % ('' if not probs else ' -- ' + '; '.join(probs)),
                       (0 if kept else 1) + len(probs), 0))
    return out


def check_dec_rows_xcd_branches():
    """omp_dec_rows_args.xcd_mask on both branches of xcd_grid (csrc/dec_rows.hip): at R = 200 the tiles fit the masked XCDs in one round (the
    mask applies), at R = 10 240 they fit 0x0F exactly (128 tiles of 80), at R = 10 277 they do not (129 tiles: every block is a tile).
    Every output identical to the unmasked launch, bit for bit, for every decoder chain kind."""
    from advancedliteratemachinery_amd import ops
    out = []
    W = _dec_setup(False, 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for kind in ('mid', 'ffn_qkv', 'ffn_head', 'embed'):
        ch, _ = dec_chain(kind, False, W, P - 1)
        for R in (200, 10240, 10277):
            src = src_map(R)
            ch.launch.mask = 0
            ref, _ = ch.run(R, src)
            t = ops.rows_tile_choice(R, kind == 'mid')
            for mask in (0x0F, 0x04):
                ch.launch.mask = mask
                got, probs = ch.run(R, src)
                fits = -(-R // t) <= bin(mask).count('1') * (cus // 8)
                same = all(torch.equal(got[k], ref[k]) for k in got)
                out.append(rec('rows[bf16] %s R=%d (%d tiles of %d): xcd_mask 0x%02X (%s) == unmasked, bit for bit%s'
                               % (kind, R, -(-R // t), t, mask, 'mask applies' if fits else 'tiles do not fit: no mask', '' if not probs else ' -- ' + '; '.join(probs)),
                               (0 if same else 1) + len(probs), 0))
            ch.launch.mask = 0
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# Swin stage-2 chains
# ---------------------------------------------------------------------------------------------------------------------------------------
def swin_chain(mode, x3, seed=300):
    """mode 0 (norm1 + qkv), 1 (proj + residual, norm2, fc1 + GELU, fc2 + residual), '1q' (1 + the next block's norm1 + qkv)"""
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.model import packing
    bf = not x3
    eng = 'x3' if x3 else 'bf16'
    odt = torch.float32 if x3 else torch.bfloat16
    wdt = torch.float32 if x3 else torch.bfloat16
    Wqkv, bqkv = _weights(seed + 1, x3, 3 * D, D), _vec(seed + 2, 3 * D)
    Wp, bp = _weights(seed + 3, x3, D, D), _vec(seed + 4, D)
    W1, b1 = _weights(seed + 5, x3, FF, D), _vec(seed + 6, FF)
    W2, b2 = _weights(seed + 7, x3, D, FF), _vec(seed + 8, D)
    g1, be1, g2, be2 = 1 + _vec(seed + 9, D), _vec(seed + 10, D), 1 + _vec(seed + 11, D), _vec(seed + 12, D)
    wd = lambda t: _dev(t, wdt)            # noqa: E731
    if mode == 0:
        x = edge_rows(seed, None, with_att=False)
        ref = dict(x=x, qkv=ref_qkv_tail(x, g1, be1, Wqkv, bqkv, bf))
        s = packing.pack_rows_embed_qkv(wd(Wqkv))
        n1, bq = (_dev(g1), _dev(be1)), _dev(bqkv)

        def launch(b):
            ops.swin_rows_qkv(b['x'], n1, bq, s[0], s[1], qkv=b['qkv'], x3=x3)
        ch = Chain('swin mode 0', eng, dict(x=(_dev(x), 'inout')), launch, ('x', 'qkv'))
        ch.out_shapes = dict(qkv=(3 * D, odt))
    else:
        tail = mode == '1q'
        x, att = edge_rows(seed, bp)
        att = rb(att, bf).float().double() if bf else att.float().double()
        x2 = ref_ffn_body(x, att, Wp, bp, g2, be2, W1, b1, W2, b2, bf, act='gelu')
        ref = dict(x=x2)
        if tail:
            ref['qkv'] = ref_qkv_tail(x2, g1, be1, Wqkv, bqkv, bf)
        s = (packing.pack_rows_ffn_qkv(wd(Wp), wd(W1), wd(W2), wd(Wqkv)) if tail else packing.pack_rows_ffn(wd(Wp), wd(W1), wd(W2)))
        args = (_dev(bp), (_dev(g2), _dev(be2)), _dev(b1), _dev(b2))
        nxt = dict(next_n1=(_dev(g1), _dev(be1)), next_qkv_b=_dev(bqkv)) if tail else {}

        def launch(b):
            ops.swin_rows_block(b['x'], b['att'], s[0], s[1], *args, qkv=b.get('qkv'), x3=x3, **nxt)
        ch = Chain('swin mode 1' + (' + next qkv' if tail else ''), eng, dict(x=(_dev(x), 'inout'), att=(_att_dev(att, x3), 'in')), launch,
                   ('x', 'qkv') if tail else ('x',))
        ch.out_shapes = dict(qkv=(3 * D, odt)) if tail else {}
    launch.mask = 0
    ch.cls = 'swin0' if mode == 0 else 'swin1'
    return ch, ref


def check_swin_chain(mode, x3=False):
    out = []
    ch, ref = swin_chain(mode, x3)
    tag = 'rows[%s] %s' % (ch.eng, ch.name)
    base = _base_vs_ref(out, ch, ref, '%s R=%d' % (tag, NB))
    Rs = SWIN_R + ((47, 48, 49) if x3 else ())
    _sweep(out, ch, tag, sorted(Rs), base)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the memory projection
# ---------------------------------------------------------------------------------------------------------------------------------------
NL, NH = 12, 8


def _kv_setup(seed=500):
    from advancedliteratemachinery_amd.model import packing
    Wk = _weights(seed + 1, False, NL * D, D)
    Wv = _weights(seed + 2, False, NL * D, D)
    bk, bv = _vec(seed + 3, NL * D), _vec(seed + 4, NL * D)
    sk = packing.pack_kv_rows_k(_dev(Wk, torch.bfloat16))
    sv = packing.pack_kv_rows_v(_dev(Wv, torch.bfloat16))
    return dict(Wk=Wk, Wv=Wv, bk=bk, bv=bv, sk=sk, sv=sv, bkd=_dev(bk), bvd=_dev(bv))


def _kv_rows_in(B, M, seed):
    """memory rows of B images (bf16-valued float64): random, with zero / 1e-3 / 1e4 / offset / outlier rows planted in every image"""
    mem = _randn(B * M, D, seed=seed)
    pos = _randn(B * M, D, seed=seed + 1) * 0.5
    for b in range(B):
        r = b * M
        mem[r] = 0.0
        mem[r + 1] *= 1e-3
        mem[r + 2] *= 1e4
        mem[r + 3] += 300.0
        mem[r + 4, 37] = 50.0
    mem = mem.to(torch.bfloat16).double()
    return mem, (mem + pos).to(torch.bfloat16).double()


def _kv_run(S, mem, mem_pos, B, M):
    from advancedliteratemachinery_amd import ops
    Mpad = (M + 31) // 32 * 32
    K = torch.zeros(NL, B, NH, Mpad, 64, dtype=torch.bfloat16, device=DEV)
    Vt = torch.zeros(NL, B, NH, Mpad // 32, 64, 32, dtype=torch.bfloat16, device=DEV)
    ops.kv_project_rows(mem_pos, S['sk'][0], S['sk'][1], S['bkd'], K, B, M, Mpad, NL, False)
    ops.kv_project_rows(mem, S['sv'][0], S['sv'][1], S['bvd'], Vt, B, M, Mpad, NL, True)
    torch.cuda.synchronize()
    return K, Vt


def _vt_natural(Vt):
    """V^T slabs [NL, B, nH, Mpad/32, 64, 32 slots] -> V [NL, B, nH, Mpad, 64]"""
    slot = vt_slot(torch.arange(32, device=Vt.device))
    v = Vt[..., slot].transpose(-1, -2)
    return v.reshape(Vt.shape[0], Vt.shape[1], Vt.shape[2], -1, 64)


def check_kv_rows_full():
    """omp_kv_project_rows: every K and V^T slab entry of every slab against float64, relative to each (slab, key) row's own max; M = 3072
    (one image) and M = 64 / 192 (three images) and 4096 (one image)"""
    out = []
    S = _kv_setup()
    for B, M in ((1, 3072), (3, 64), (3, 192), (1, 4096)):
        mem, mem_pos = _kv_rows_in(B, M, 600 + M)
        K, Vt = _kv_run(S, _dev(mem, torch.bfloat16), _dev(mem_pos, torch.bfloat16), B, M)
        kr, vr = ref_kv(mem_pos, mem, S['Wk'], S['bk'], S['Wv'], S['bv'], True)
        to_slab = lambda t: t.reshape(B, M, NL, D).permute(2, 0, 1, 3).reshape(NL * B * M, D)   # noqa: E731  rows (slab, image, key)
        nat = lambda t: t[:, :, :, :M].permute(0, 1, 3, 2, 4).reshape(NL * B * M, D)          # noqa: E731  [NL, B, nH, M, 64] -> same rows
        tag = 'kv_rows full[B=%d, M=%d]' % (B, M)
        _gate(out, tag + ' K vs float64 (per (slab, key) row)', nat(K), to_slab(kr), ('bf16', 'kv', 'K'))
        _gate(out, tag + ' V^T vs float64 (per (slab, key) row)', nat(_vt_natural(Vt)), to_slab(vr), ('bf16', 'kv', 'V'))
        del K, Vt
    return out


def check_kv_rows_batch():
    """a B = 40, M = 3072 call: every image's K and V^T slabs identical, bit for bit, to that image projected alone"""
    out = []
    S = _kv_setup()
    B, M = 40, 3072
    g = torch.Generator(device=DEV).manual_seed(700)
    mem = torch.randn(B * M, D, generator=g, device=DEV).to(torch.bfloat16)
    mem_pos = (mem.float() + 0.5 * torch.randn(B * M, D, generator=g, device=DEV)).to(torch.bfloat16)
    K, Vt = _kv_run(S, mem, mem_pos, B, M)
    bad = []
    for b in range(B):
        k1, v1 = _kv_run(S, mem[b * M:(b + 1) * M].contiguous(), mem_pos[b * M:(b + 1) * M].contiguous(), 1, M)
        if not (torch.equal(k1[:, 0], K[:, b]) and torch.equal(v1[:, 0], Vt[:, b])):
            bad.append(b)
    out.append(rec('kv_rows[B=%d, M=%d]: every image == that image projected alone, bit for bit%s' % (B, M, '' if not bad else ' -- images %s' % bad), len(bad), 0))
    return out
