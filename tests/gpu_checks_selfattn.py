"""The three causal self-attention step kernels of csrc/decoder.hip at every cache position where their loops change shape:

  head   dec_self_attn_kernel        one wave per (row, head), 32 keys per outer iteration      fp32 / bf16   omp_debug_self_attn_impl(1)
  row    dec_self_attn_row_kernel    one wave per row, groups of U = 4 keys                       fp32 / bf16   omp_debug_self_attn_impl(2)
  fused  dec_fused_self_attn_kernel  LN1 + q | k | v of one head + append + attention, 64-key chunks in a ring of 3 (it wraps at
                                     positions 192 and 384), 4-row tiles                          bf16, EMBED off / on   ops.fused_self_attn

A launch has one row per target key (R = pos + 1 unless a case says otherwise); every row owns its cache.  Planted inputs (all values exact
in bf16; tests/test_selfattn_reference.py proves the stated outputs and that a lost, shifted, stale or skipped key breaks the gates):

  * uniform walk: every key is 0 (all scores 0), V is 0 except the row's target key, which holds the row's pattern u: the output is
    u / (pos + 1); a dropped target gives 0, a doubled one twice the value.  The target of the last row is `pos`, the key held in registers.
  * peaked walk: V[j] is a pattern of j, the target key is 4 q (score 32, every other key 0 and score 0): the output is V[target].
  The fused kernel runs them with W = 0, so q, k_new, v_new are bias_tab[pos] for EVERY row: there the new value is a pattern w shared by
  all rows (uniform: (u + w) / (pos + 1), the last row w / (pos + 1)), the new key 4 q for all rows and the cached target 8 q (score 64,
  the new key 32, the rest 0; the last row aims at the new key).
  * ramps: scores rising / falling by a fixed step to +80, so that the running maximum changes at every key / never.
  * random base (randn x 1.5) and, for the fused kernel, its LayerNorm + projection against a float64 mirror of its rounding points.

Every launch: cache positions above `pos`, position `pos` itself, the guard rows of the caches, of `out` and of x_out hold a NaN pattern
beforehand; afterwards every cache word but position `pos` is bit-identical, position `pos` holds the new k / v, the guards are untouched and
the outputs are finite.  No case launches with pos >= Lmax: the position lives in device memory and the host cannot refuse it.

The float64 restatements (ref_*) run on whatever device their operands are on (the GPU checks keep the large ones on the device) and read
the bytes the kernel was given.  Checks return rec / rrec records (tests/gpu_checks.py)."""
import contextlib

import torch
import torch.nn.functional as F

from tests.gpu_checks import DEV, rec, rrec

D, HD, NH = 512, 64, 8
LMAX = 450
GUARD = 4                           # a dead row of a 4-row tile that wrote would land here
F32_NAN = 0x7FC0DEAD
BF16_NAN = 0x7FA5
EPS = 1e-5
VOCAB = 512

# 0..9; every multiple of 32 up to 128 and of 64 up to 448 with both neighbours; Lmax - 1
POSITIONS = sorted(set(range(10)) | {m + e for m in range(32, 129, 32) for e in (-1, 0, 1)}
                   | {m + e for m in range(64, 449, 64) for e in (-1, 0, 1)} | {LMAX - 1})
LONG_POS, LONG_LMAX = 1023, 1024
LONG_TARGETS = sorted(set(range(0, 1024, 16)) | {0, 1022, 1023})

# per (row, head), relative to its largest stated value.  bf16: the one output rounding stays below 2^-8 of each value (half a step of 2^-7
# of its power of two; measured 3.5e-3 on an MI355X), the fp32 noise under it is ~1e-7.  fp32: exact terms, one reciprocal and one multiply
# (measured 8e-8).  A lost or doubled key is an error of 1 / 3 or more, a misread one of 2 / 7 or more (tests/test_selfattn_reference.py).
WALK_GATE = {torch.bfloat16: 2.0 ** -8, torch.float32: 1e-6}
# the project's gates (check_self_attn), absolute.  Measured worst on an MI355X: fp32 1.8e-5 (the row kernel on the falling ramp at position
# 129: scores of 80 log2(e) = 115 in fp32 are good to ~1e-5, which the exponential turns into a relative error of the weights; 7.6e-6 for the
# (row, head) kernel, 3e-6 on random data), bf16 1.5e-2
GATE = {torch.float32: 2e-5, torch.bfloat16: 3e-2}
LN_GATE = 2e-5                                       # check_dec_embed_ln
STEP_FLOOR = 2e-5   # below |value| ~ 4e-3 a bf16 step is smaller than the fp32 accumulation error of a 512-term product: the unit is the fp32 gate

DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}
KERNELS = ('head', 'row', 'fused', 'fused_embed')


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------------------------------------------------------
def rb(t, bf):
    return t.to(torch.bfloat16).double() if bf else t


def ref_attn(q, K, V, nH, bf=False, ksrc=None, vsrc=None, weight=None, chunk=64):
    """softmax(q K^T / 8) V per head over ALL keys given.  q [R, d], K / V [R, L, d] float64 (d = 64 nH) -> [R, d]; bf rounds the output.
    The mutants of tests/test_selfattn_reference.py: ksrc / vsrc [L] = the key whose K / V row slot j reads, weight [R, L] = how often a key
    counts (0 = dropped, 2 = taken twice)."""
    R, L, d = K.shape
    out = []
    for r0 in range(0, R, chunk):
        k, v = K[r0:r0 + chunk], V[r0:r0 + chunk]
        if ksrc is not None:
            k = k[:, ksrc]
        if vsrc is not None:
            v = v[:, vsrc]
        n = k.shape[0]
        s = torch.einsum('rhd,rlhd->rhl', q[r0:r0 + chunk].reshape(n, nH, HD) * 0.125, k.reshape(n, L, nH, HD))
        p = torch.exp(s - s.amax(-1, keepdim=True))
        if weight is not None:
            p = p * weight[r0:r0 + chunk, None, :]
        out.append((torch.einsum('rhl,rlhd->rhd', p, v.reshape(n, L, nH, HD)) / p.sum(-1, keepdim=True)).reshape(n, d))
    return rb(torch.cat(out), bf)


def ref_ln(x, g, b, eps=EPS):
    return F.layer_norm(x, (x.shape[-1],), g, b, eps)


def ref_embed(word, pos_row, tok, g, b, eps=EPS):
    """DecoderEmbeddings at one position: LN(word[token] + position)  (the reference of check_dec_embed_ln)"""
    return ref_ln(word[tok.long()] + pos_row, g, b, eps)


def ref_fused_qkv(x, ln_g, ln_b, W, bias_row, bf, eps=EPS):
    """the fused kernel's q | k | v rows [R, 1536] at its rounding points: LN1 in float64 -> bf16, the product in float64 + bias -> bf16"""
    return rb(rb(ref_ln(x, ln_g, ln_b, eps), bf) @ W.T + bias_row, bf)


def head_rel(got, want, nH):
    """per (row, head): max |got - want| / max |want|; a non-finite value is an infinite error -> [R, nH]"""
    g, w = got.double().reshape(-1, nH, HD), want.reshape(-1, nH, HD)
    e = (g - w).abs().amax(-1) / w.abs().amax(-1).clamp_min(1e-300)
    return torch.where(torch.isfinite(g).all(-1), e, torch.full_like(e, float('inf')))


def bf16_steps(got, ref, floor=STEP_FLOOR):
    """max |got - bf16(ref)| in bf16 steps of bf16(ref); near zero the unit is `floor`"""
    r = ref.to(torch.bfloat16).double()
    unit = torch.exp2(torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126))) - 7).clamp_min(floor)
    return ((got.double() - r).abs() / unit).max().item()


# ---------------------------------------------------------------------------------------------------------------------------------------
# planted inputs (float64, exact in bf16)
# ---------------------------------------------------------------------------------------------------------------------------------------
def q_dir(d, dev='cpu'):
    """[d] of +-1: the query of every planted case"""
    c = torch.arange(d, device=dev)
    return (((c * 7 + c // HD * 3) % 5 < 2).double() * 2 - 1)


def u_pat(rows, d, dev='cpu'):
    """[len(rows), d] of non-zero integers in [-16, 17], another pattern per row index"""
    r = torch.as_tensor(rows, dtype=torch.int64, device=dev)[:, None]
    c = torch.arange(d, device=dev)[None, :]
    u = (r * 37 + c * 11) % 33 - 16
    return torch.where(u == 0, 17, u).double()


def v_pat(keys, d, dev='cpu'):
    """[len(keys), d]: dimension c of key j holds +-(1 + (j + c) % 7), the sign bit c % 10 of j: two keys below 1024 differ in sign in at least
    6 dimensions of every head"""
    j = torch.as_tensor(keys, dtype=torch.int64, device=dev)[:, None]
    c = torch.arange(d, device=dev)[None, :]
    return ((((j >> (c % 10)) & 1) * 2 - 1) * (1 + (j + c) % 7)).double()


class Plant:
    """q, kn, vn [R, d] (this step's row of qkv), Kc, Vc [R, pos, d] (the cache below pos), targets [R]"""

    def __init__(self, pos, targets, d, dev):
        self.pos, self.d, self.R = pos, d, len(targets)
        self.t = torch.as_tensor(targets, dtype=torch.int64, device=dev)
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
        self.q = q_dir(d, dev).expand(self.R, d).clone()
        self.kn, self.vn, self.Kc, self.Vc = z(self.R, d), z(self.R, d), z(self.R, pos, d), z(self.R, pos, d)

    def put(self, cache, new, rows_value):
        """the target key of every row <- its row of rows_value: cache slot t below pos, the new key at pos"""
        old = self.t < self.pos
        r = torch.arange(self.R, device=self.t.device)
        cache[r[old], self.t[old]] = rows_value[old]
        new[~old] = rows_value[~old]

    def all_keys(self):
        """K, V [R, pos + 1, d] as the kernel sees them after the append"""
        return torch.cat([self.Kc, self.kn[:, None]], 1), torch.cat([self.Vc, self.vn[:, None]], 1)


def plant_uniform(pos, targets, d=D, shared=False, dev='cpu'):
    """all keys 0; V = 0 but the target <- u_pat(row).  shared (the fused kernel): the new value is one pattern w for every row"""
    p = Plant(pos, targets, d, dev)
    u = u_pat(list(range(p.R)), d, dev)
    p.put(p.Vc, p.vn, u)
    if shared:
        p.vn[:] = u_pat([p.R + 5], d, dev)
    return p


def plant_peaked(pos, targets, d=D, shared=False, dev='cpu'):
    """V[j] = v_pat(j) in every row; the target key = 4 q, the rest 0.  shared: the new key is 4 q for every row and a cached target 8 q"""
    p = Plant(pos, targets, d, dev)
    p.Vc[:] = v_pat(list(range(pos)), d, dev)
    p.vn[:] = v_pat([pos], d, dev)
    p.put(p.Kc, p.kn, (8.0 if shared else 4.0) * p.q)
    if shared:
        p.kn[:] = 4.0 * p.q
    return p


def want_uniform(p, shared):
    """the stated output of the uniform walk, float64"""
    u = u_pat(list(range(p.R)), p.d, p.t.device)
    if shared:
        w = u_pat([p.R + 5], p.d, p.t.device)
        u = torch.where((p.t < p.pos)[:, None], u + w, w.expand_as(u))
    return u / (p.pos + 1)


def want_peaked(p):
    return v_pat(p.t.tolist(), p.d, p.t.device)


def plant_ramp(pos, R, rising, dt, d=D, seed=0, dev='cpu'):
    """key j = c_j q with c_j = 10 j / pos (rising) or 10 (pos - j) / pos, rounded to dt: scores 80 j / pos; V random, the new value shared"""
    p = Plant(pos, [0] * R, d, dev)
    j = torch.arange(pos + 1, dtype=torch.float64)
    c = (10.0 * (j if rising else pos - j) / max(pos, 1)).to(dt).double().to(dev)
    p.Kc[:] = c[:pos, None] * p.q[0] + 0.0         # + 0.0: no -0 where c is 0 (the fused kernel's 0 W + bias gives +0)
    p.kn[:] = c[pos] * p.q[0] + 0.0
    g = torch.Generator().manual_seed(1000 * pos + seed)
    p.Vc[:] = (torch.randn(R, pos, d, generator=g) * 1.5).to(dt).double().to(dev)
    p.vn[:] = (torch.randn(1, d, generator=g) * 1.5).to(dt).double().to(dev)
    return p


def plant_random(pos, R, dt, d=D, seed=0, shared=False, dev='cpu'):
    """randn x 1.5 everywhere, rounded to dt.  shared: one q, k_new, v_new for all rows"""
    p = Plant(pos, [0] * R, d, dev)
    g = torch.Generator().manual_seed(7919 * pos + 31 * R + seed)
    r = lambda *s: (torch.randn(*s, generator=g) * 1.5).to(dt).double().to(dev)
    n = 1 if shared else R
    p.q[:], p.kn[:], p.vn[:] = r(n, d), r(n, d), r(n, d)
    p.Kc[:], p.Vc[:] = r(R, pos, d), r(R, pos, d)
    return p


# ---------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm inputs whose bf16 rounding an fp32 evaluation cannot flip
# ---------------------------------------------------------------------------------------------------------------------------------------
def near_tie(y):
    """elements of float64 y (|y| >= 2^-9) within 2^-17 |y| + 2^-21 of the midpoint between two bf16 neighbours: an fp32 evaluation of y
    (relative error of a few 2^-24) could round them to the other neighbour.  Below 2^-9 a flip moves a 512-term product by less than 5e-6."""
    a = y.abs()
    ulp = torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0 ** -126))) - 7)
    dist = ulp / 2 - (y - y.to(torch.bfloat16).double()).abs()
    return (dist < a * 2.0 ** -17 + 2.0 ** -21) & (a >= 2.0 ** -9)


def settle(x, fn):
    """nudge the fp32-valued rows x until no element of fn(x) is near_tie -> x.  The bound on the appended k / v (one bf16 step)
    holds only when the reference's LN1 rounding is the kernel's: a flipped rounding of an LN value of 2 moves a product by up to 5e-4."""
    for it in range(200):
        m = near_tie(fn(x))
        if not m.any():
            return x
        x = (x + m * 1e-3 * (1 + it % 5)).float().double()
    raise AssertionError('settle: the LayerNorm rows did not settle')


# ---------------------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ibits(dt):
    return torch.int32 if dt == torch.float32 else torch.int16


def _nan(dt):
    return F32_NAN if dt == torch.float32 else BF16_NAN


def _filled(shape, dt):
    buf = torch.empty(shape, dtype=dt, device=DEV)
    buf.view(_ibits(dt)).fill_(_nan(dt))
    return buf


def _is_nan_fill(t):
    return bool((t.view(_ibits(t.dtype)) == _nan(t.dtype)).all().item())


def _same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(_ibits(a.dtype)), b.contiguous().view(_ibits(b.dtype))))


@contextlib.contextmanager
def self_attn_impl(which):
    from advancedliteratemachinery_amd import ops
    ops.self_attn_impl(which)
    try:
        yield
    finally:
        ops.self_attn_impl(0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class FusedArgs:
    """the operands of the fused kernel besides the caches.  W = None: zero weights, so that q | k | v = bf16(bias_tab[pos]).  bias_tab and
    pos_tab hold NaN in every row but `pos`, word row 0 (the token of every seq entry but column pos) is NaN."""

    def __init__(self, R, pos, Lmax, bias_row, embed, seed, W=None, x=None, word_rows=None):
        g = _gen(seed)
        self.R, self.pos, self.embed = R, pos, embed
        self.ln_g = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
        self.ln_b = (0.1 * torch.randn(D, generator=g)).to(DEV)
        self.W = torch.zeros(3 * D, D, dtype=torch.bfloat16, device=DEV) if W is None else W.to(DEV, torch.bfloat16)
        self.bias_tab = _filled((Lmax, 3 * D), torch.float32)
        self.bias_tab[pos] = bias_row.float().to(DEV)
        xr = torch.randn(R, D, generator=g)            # drawn whether used or not: the same seed gives the same operands
        self.x = (xr if x is None else x.float()).to(DEV)
        if embed:
            self.tok = (1 + (torch.arange(R) * 5) % (VOCAB - 1)).to(torch.int32)
            word = torch.randn(VOCAB, D, generator=g)
            if word_rows is not None:
                word[self.tok.long()] = word_rows.float()
            word[0] = float('nan')
            self.word = word.to(DEV)
            self.pos_tab = _filled((Lmax, D), torch.float32)
            self.pos_tab[pos] = (0.5 * torch.randn(D, generator=g)).to(DEV)
            self.emb_g = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
            self.emb_b = (0.1 * torch.randn(D, generator=g)).to(DEV)
            self.seq = torch.zeros(R, Lmax + 3, dtype=torch.int32, device=DEV)
            self.seq[:, pos] = self.tok.to(DEV)
            self.xbuf = _filled((R + GUARD, D), torch.float32)
            self.x = None

    def ref_x(self):
        """the rows LN1 reads, float64 on the CPU: x, or the embedded rows"""
        if not self.embed:
            return self.x.double().cpu()
        return ref_embed(self.word.double().cpu(), self.pos_tab[self.pos].double().cpu(), self.tok, self.emb_g.double().cpu(), self.emb_b.double().cpu())

    def launch(self, kc, vc, o, dpos):
        from advancedliteratemachinery_amd import ops
        emb = (self.seq, self.word, self.pos_tab, self.emb_g, self.emb_b, self.xbuf[:self.R]) if self.embed else None
        ops.fused_self_attn(self.x, self.ln_g, self.ln_b, self.W, self.bias_tab, kc, vc, o, dpos, eps=EPS, embed=emb)


def fused_bias_row(p):
    """bias_tab[pos] that makes the fused kernel (W = 0) see the plant: its q, k_new, v_new must be the same in every row"""
    for t in (p.q, p.kn, p.vn):
        assert bool((t == t[:1]).all()), 'the fused kernel with W = 0 gives every row the same q, k_new, v_new'
    return torch.cat([p.q[0], p.kn[0], p.vn[0]])


def run_step(out, tag, kern, dt, p, Lmax, nH=NH, fused=None):
    """One launch of `kern` on plant p (values exact in dt): caches [R + GUARD, Lmax, d] and out [R + GUARD, d] pre-filled with NaN bits, the
    plant below pos.  Appends the memory-discipline record; -> (out rows [R, d], appended k [R, d], appended v [R, d]) on the device."""
    from advancedliteratemachinery_amd import ops
    R, pos, d = p.R, p.pos, p.d
    assert 0 <= pos < Lmax and R > 0, 'a launch with pos >= Lmax writes out of bounds'
    kbuf, vbuf, obuf = _filled((R + GUARD, Lmax, d), dt), _filled((R + GUARD, Lmax, d), dt), _filled((R + GUARD, d), dt)
    Kc, Vc = p.Kc.to(DEV, dt), p.Vc.to(DEV, dt)
    kbuf[:R, :pos], vbuf[:R, :pos] = Kc, Vc
    dpos = torch.tensor([pos], dtype=torch.int32, device=DEV)
    if kern in ('fused', 'fused_embed'):
        assert dt == torch.bfloat16 and d == D
        fused = fused or FusedArgs(R, pos, Lmax, fused_bias_row(p), kern == 'fused_embed', seed=pos + R)
        fused.launch(kbuf[:R], vbuf[:R], obuf[:R], dpos)
    else:
        qkv = torch.cat([p.q, p.kn, p.vn], 1).to(DEV, dt)
        with self_attn_impl({'head': 1, 'row': 2}[kern]):
            ops.dec_self_attn_step(qkv, kbuf[:R], vbuf[:R], obuf[:R], dpos, nH)
    torch.cuda.synchronize()
    probs = []
    for name, buf, plant in (('K', kbuf, Kc), ('V', vbuf, Vc)):
        if not _same_bits(buf[:R, :pos], plant):
            probs.append('%s cache changed below pos' % name)
        if not _is_nan_fill(buf[:R, pos + 1:]):
            probs.append('%s cache written above pos' % name)
        if not _is_nan_fill(buf[R:]):
            probs.append('%s cache guard rows written' % name)
        if not bool(torch.isfinite(buf[:R, pos]).all().item()):
            probs.append('%s cache: position pos not written / not finite' % name)
    if not _is_nan_fill(obuf[R:]):
        probs.append('out guard rows written')
    if not bool(torch.isfinite(obuf[:R]).all().item()):
        probs.append('NaN / inf in an output row')
    if fused is not None and fused.embed:
        if not _is_nan_fill(fused.xbuf[R:]):
            probs.append('x_out guard rows written')
        if not bool(torch.isfinite(fused.xbuf[:R]).all().item()):
            probs.append('NaN / inf in x_out')
    out.append(rec(tag + ': caches bit-identical but position pos, guards untouched, outputs finite%s' % ('' if not probs else ' -- ' + '; '.join(probs)),
                   len(probs), 0))
    return obuf[:R], kbuf[:R, pos].clone(), vbuf[:R, pos].clone()


def _appended(out, tag, kpos, vpos, p, dt):
    ok = _same_bits(kpos, p.kn.to(DEV, dt)) and _same_bits(vpos, p.vn.to(DEV, dt))
    out.append(rec(tag + ': position pos holds exactly this step\'s k and v', 0 if ok else 1, 0))


def _x_out(out, tag, fa):
    e = (fa.xbuf[:fa.R].double().cpu() - fa.ref_x()).abs().max().item()
    out.append(rec(tag + ': x_out vs float64 LN(word[token] + position)', e, LN_GATE))


def _on_dev(p):
    """the float64 operands of ref_attn from the bytes the kernel got, on the device"""
    K, V = p.all_keys()
    return p.q.to(DEV), K.to(DEV), V.to(DEV)


def _is_fused(kern):
    return kern in ('fused', 'fused_embed')


def _walk_case(out, kern, dn, pos, Lmax, targets):
    dt = DTYPES[dn]
    shared = _is_fused(kern)
    worst = {}
    for walk, plant in (('uniform', plant_uniform), ('peaked', plant_peaked)):
        p = plant(pos, targets, D, shared, DEV)
        tag = 'self_attn %s walk[%s %s pos%d R%d]' % (walk, kern, dn, pos, p.R)
        fa = FusedArgs(p.R, pos, Lmax, fused_bias_row(p), kern == 'fused_embed', seed=pos) if shared else None
        got, kpos, vpos = run_step(out, tag, kern, dt, p, Lmax, fused=fa)
        _appended(out, tag, kpos, vpos, p, dt)
        if fa is not None and fa.embed:
            _x_out(out, tag, fa)
        want = ref_attn(*_on_dev(p), NH)
        e = head_rel(got, want, NH)
        i = int(e.reshape(-1).argmax())
        out.append(rec(tag + ' vs float64 per (row, head)', e.reshape(-1)[i].item(), WALK_GATE[dt], 'worst at row %d (target %d) head %d' % (i // NH, int(p.t[i // NH]), i % NH)))
        worst[walk] = e.max().item()
    return worst


def check_walks(kern, dn, positions):
    """both walks at every position of `positions`, one row per target key 0 .. pos, Lmax = 450"""
    out, worst = [], {}
    for pos in positions:
        for walk, e in _walk_case(out, kern, dn, pos, LMAX, list(range(pos + 1))).items():
            worst[walk] = max(worst.get(walk, (0.0, 0)), (e, pos))
    for walk, (e, pos) in worst.items():
        out.append(rrec('self_attn %s walk[%s %s positions %d..%d] worst (row, head)' % (walk, kern, dn, positions[0], positions[-1]), e, WALK_GATE[DTYPES[dn]],
                        'worst at pos %d' % pos))
    return out


def check_walk_long(kern):
    """the fused kernel at pos = 1023 of Lmax = 1024: every 16th key, keys 1022 and 1023 (16 chunks, the ring wraps five times)"""
    out = []
    for walk, e in _walk_case(out, kern, 'bf16', LONG_POS, LONG_LMAX, LONG_TARGETS).items():
        out.append(rrec('self_attn %s walk[%s bf16 pos %d] worst (row, head)' % (walk, kern, LONG_POS), e, WALK_GATE[torch.bfloat16]))
    return out


RAMP_POS = (9, 129, 200, 449)
RANDOM_POS = (0, 36, 129, 200)
RANDOM_R = (1, 3, 4, 5, 70)


def _vs_float64(out, tag, kern, dt, p, Lmax, nH=NH):
    """launch, memory discipline, the append, and max |out - float64| against the project's gate"""
    got, kpos, vpos = run_step(out, tag, kern, dt, p, Lmax, nH=nH)
    _appended(out, tag, kpos, vpos, p, dt)
    e = (got.double() - ref_attn(*_on_dev(p), nH)).abs().max().item()
    out.append(rec(tag + ' vs float64', e, GATE[dt]))
    return e


def check_ramps(kern, dn):
    dt = DTYPES[dn]
    out, worst = [], (0.0, '')
    for pos in RAMP_POS:
        for rising in (True, False):
            p = plant_ramp(pos, 5, rising, dt, dev=DEV)
            tag = 'self_attn %s ramp[%s %s pos%d R5]' % ('rising' if rising else 'falling', kern, dn, pos)
            worst = max(worst, (_vs_float64(out, tag, kern, dt, p, pos + 3), tag))
    out.append(rrec('self_attn ramps[%s %s] worst vs float64' % (kern, dn), worst[0], GATE[dt], 'worst at ' + worst[1]))
    return out


def check_random(kern, dn):
    dt = DTYPES[dn]
    out, worst = [], (0.0, '')
    for pos in RANDOM_POS:
        for R in RANDOM_R:
            p = plant_random(pos, R, dt, shared=_is_fused(kern), dev=DEV)
            tag = 'self_attn random[%s %s pos%d R%d]' % (kern, dn, pos, R)
            worst = max(worst, (_vs_float64(out, tag, kern, dt, p, pos + 2), tag))
    out.append(rrec('self_attn random[%s %s] worst vs float64' % (kern, dn), worst[0], GATE[dt], 'worst at ' + worst[1]))
    return out


def check_random_heads(dn):
    """dec_self_attn_kernel at nH = 6, 3, 1 (d = 64 nH): the h >= nH early return of the last 4-head workgroup"""
    dt = DTYPES[dn]
    out, worst = [], (0.0, '')
    for nH in (6, 3, 1):
        for pos in (0, 36, 129):
            for R in (1, 5):
                p = plant_random(pos, R, dt, d=HD * nH, seed=nH, dev=DEV)
                tag = 'self_attn random[head %s nH%d pos%d R%d]' % (dn, nH, pos, R)
                worst = max(worst, (_vs_float64(out, tag, 'head', dt, p, pos + 2, nH=nH), tag))
    out.append(rrec('self_attn random[head %s nH 6 / 3 / 1] worst vs float64' % dn, worst[0], GATE[dt], 'worst at ' + worst[1]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fused kernel's LayerNorm + projection
# ---------------------------------------------------------------------------------------------------------------------------------------
PROJ_R = (1, 2, 3, 4, 5, 8, 13, 63)
PROJ_POS = (0, 63, 64, 200)


def proj_inputs(R, seed):
    """random bf16 W (q | k | v ~ N(0, 1.5^2)), a random bias row and random fp32 rows (x, or the word rows with EMBED, before they are
    settled) -> dict of CPU float64 tensors"""
    g = _gen(seed)
    W = (torch.randn(3 * D, D, generator=g) * (1.5 / D ** 0.5)).to(torch.bfloat16).double()
    bias = (torch.randn(3 * D, generator=g) * 0.5).double()
    rows = torch.randn(R, D, generator=g).double()
    return dict(W=W, bias=bias, rows=rows)


def check_fused_projection(embed):
    out, worst_o, worst_s = [], (0.0, ''), (0.0, '')
    bf = torch.bfloat16
    for pos in PROJ_POS:
        for R in PROJ_R:
            tag = 'fused_self_attn projection[%s pos%d R%d]' % ('embed' if embed else 'x', pos, R)
            Lmax = pos + 2
            i = proj_inputs(R, seed=100 * pos + R)
            fa = FusedArgs(R, pos, Lmax, i['bias'], embed, seed=pos + R, W=i['W'], x=i['rows'])
            g1, b1 = fa.ln_g.double().cpu(), fa.ln_b.double().cpu()
            if embed:
                word, ge, be, pe = fa.word.double().cpu(), fa.emb_g.double().cpu(), fa.emb_b.double().cpu(), fa.pos_tab[pos].double().cpu()
                rows = settle(word[fa.tok.long()], lambda w: ref_ln(ref_ln(w + pe, ge, be).float().double(), g1, b1))
                fa = FusedArgs(R, pos, Lmax, i['bias'], True, seed=pos + R, W=i['W'], x=i['rows'], word_rows=rows)
                x = fa.ref_x().float().double()          # the kernel holds the embedded row in fp32
            else:
                x = settle(i['rows'], lambda v: ref_ln(v, g1, b1))
                fa = FusedArgs(R, pos, Lmax, i['bias'], False, seed=pos + R, W=i['W'], x=x)
            qkv = ref_fused_qkv(x, g1, b1, i['W'], fa.bias_tab[pos].double().cpu(), True)
            p = plant_random(pos, R, bf, seed=5, dev=DEV)
            p.q, p.kn, p.vn = qkv[:, :D].to(DEV), qkv[:, D:2 * D].to(DEV), qkv[:, 2 * D:].to(DEV)
            got, kpos, vpos = run_step(out, tag, 'fused_embed' if embed else 'fused', bf, p, Lmax, fused=fa)
            s = max(bf16_steps(kpos, p.kn), bf16_steps(vpos, p.vn))
            out.append(rec(tag + ': appended k, v within one bf16 step of the float64 mirror', s, 1.0))
            worst_s = max(worst_s, (s, tag))
            # the attention in float64 over the cache bytes: the k / v the kernel appended, the mirror's q
            K = torch.cat([p.Kc, kpos.double()[:, None]], 1)
            V = torch.cat([p.Vc, vpos.double()[:, None]], 1)
            e = (got.double() - ref_attn(p.q, K, V, NH)).abs().max().item()
            out.append(rec(tag + ' out vs float64', e, GATE[bf]))
            worst_o = max(worst_o, (e, tag))
            if embed:
                _x_out(out, tag, fa)
                # every head's workgroup embeds the rows again and only head 0 writes them: the same step from x = x_out (EMBED off) must
                # append the same k, v and give the same output in every head, bit for bit
                fb = FusedArgs(R, pos, Lmax, i['bias'], False, seed=pos + R, W=i['W'], x=fa.xbuf[:R].cpu())
                fb.ln_g, fb.ln_b = fa.ln_g, fa.ln_b
                got2, kpos2, vpos2 = run_step(out, tag + ' from x_out', 'fused', bf, p, Lmax, fused=fb)
                same = _same_bits(got, got2) and _same_bits(kpos, kpos2) and _same_bits(vpos, vpos2)
                out.append(rec(tag + ': every head saw the rows head 0 wrote to x_out (EMBED off on x_out gives the same bits)', 0 if same else 1, 0))
    kind = 'embed' if embed else 'x'
    out.append(rrec('fused_self_attn projection[%s] worst out vs float64' % kind, worst_o[0], GATE[bf], 'worst at ' + worst_o[1]))
    out.append(rrec('fused_self_attn projection[%s] worst appended k / v in bf16 steps' % kind, worst_s[0], 1.0, 'worst at ' + worst_s[1]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
ERR_INVALID = -22


def _refused(out, tag, call, bufs):
    """call() returns OMP_ERR_INVALID and sets the error text; every buffer of bufs keeps its NaN fill"""
    from advancedliteratemachinery_amd import _lib
    _lib.lib().omp_debug_sample_impl(99)          # another entry's error text (the selector stays as it is): the call below must replace it
    rc = call()
    text = _lib.lib().omp_last_error().decode('utf-8', 'replace')
    torch.cuda.synchronize()
    ok = rc == ERR_INVALID and text.startswith(tag.split(' ')[0])
    out.append(rec(tag + ': refused with the error text set%s' % ('' if ok else ' -- rc %d, text %r' % (rc, text)), 0 if ok else 1, 0))
    out.append(rec(tag + ': nothing written', 0 if all(_is_nan_fill(b) for b in bufs) else 1, 0))


def check_refusals():
    from advancedliteratemachinery_amd import _lib, ops
    out = []
    h = _lib.lib()
    R, Lmax = 4, 8
    dpos = torch.zeros(1, dtype=torch.int32, device=DEV)
    for dn, dt in DTYPES.items():
        qkv = torch.zeros(R, 3 * D, dtype=dt, device=DEV)
        kc, vc, o = _filled((R, Lmax, D), dt), _filled((R, Lmax, D), dt), _filled((R, D), dt)
        bufs = (kc, vc, o)

        def step(qkv=qkv, kc=kc, vc=vc, o=o, dpos=dpos, dtype=ops.dt(dt), R=R, nH=NH, d=D, Lmax=Lmax):
            return h.omp_dec_self_attn_step(ops.ptr(qkv), ops.ptr(kc), ops.ptr(vc), ops.ptr(o), ops.ptr(dpos), dtype, R, nH, d, Lmax, ops.stream())
        for impl in (1, 2):
            with self_attn_impl(impl):
                t = 'omp_dec_self_attn_step [%s impl %d]' % (dn, impl)
                _refused(out, t + ' d != 64 nH', lambda: step(nH=7), bufs)
                _refused(out, t + ' d = 0', lambda: step(nH=0, d=0), bufs)
                _refused(out, t + ' bad dtype', lambda: step(dtype=2), bufs)
                _refused(out, t + ' bad dtype -1', lambda: step(dtype=-1), bufs)
                for name in ('qkv', 'kc', 'vc', 'o', 'dpos'):
                    _refused(out, t + ' null %s' % name, lambda: step(**{name: None}), bufs)
                _refused(out, t + ' R = 0', lambda: step(R=0), bufs)
                _refused(out, t + ' R = -1', lambda: step(R=-1), bufs)
        with self_attn_impl(2):
            q6 = torch.zeros(R, 3 * 384, dtype=dt, device=DEV)
            _refused(out, 'omp_dec_self_attn_step [%s] the row kernel with nH = 6' % dn, lambda: step(qkv=q6, nH=6, d=384), bufs)
    bf = torch.bfloat16
    kc, vc, o, xo = _filled((R, Lmax, D), bf), _filled((R, Lmax, D), bf), _filled((R, D), bf), _filled((R, D), torch.float32)
    bufs = (kc, vc, o, xo)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    a = dict(x=f32(R, D), ln_g=f32(D), ln_b=f32(D), W=torch.zeros(3 * D, D, dtype=bf, device=DEV), bias_tab=f32(Lmax, 3 * D), kc=kc, vc=vc, o=o, dpos=dpos,
             R=R, Lmax=Lmax, seq=torch.zeros(R, Lmax, dtype=torch.int32, device=DEV), seq_ld=Lmax, word=f32(4, D), pos_tab=f32(Lmax, D), emb_g=f32(D), emb_b=f32(D),
             x_out=xo, embed=0)

    def fused(**kw):
        v = dict(a, **kw)
        P = ops.ptr
        return h.omp_debug_fused_self_attn(P(v['x']), P(v['ln_g']), P(v['ln_b']), EPS, P(v['W']), P(v['bias_tab']), P(v['kc']), P(v['vc']), P(v['o']), P(v['dpos']),
                                           v['R'], v['Lmax'], P(v['seq']), v['seq_ld'], P(v['word']), P(v['pos_tab']), P(v['emb_g']), P(v['emb_b']), P(v['x_out']),
                                           v['embed'], ops.stream())
    t = 'omp_debug_fused_self_attn'
    for name in ('x', 'ln_g', 'ln_b', 'W', 'bias_tab', 'kc', 'vc', 'o', 'dpos'):
        _refused(out, t + ' null %s' % name, lambda: fused(**{name: None}), bufs)
    for name in ('seq', 'word', 'pos_tab', 'emb_g', 'emb_b', 'x_out', 'ln_g', 'kc', 'dpos'):
        _refused(out, t + ' embed, null %s' % name, lambda: fused(embed=1, **{name: None}), bufs)
    _refused(out, t + ' embed, seq_ld = 0', lambda: fused(embed=1, seq_ld=0), bufs)
    for embed in (0, 1):
        _refused(out, t + ' embed %d, R = 0' % embed, lambda: fused(embed=embed, R=0), bufs)
        _refused(out, t + ' embed %d, R = -4' % embed, lambda: fused(embed=embed, R=-4), bufs)
        _refused(out, t + ' embed %d, Lmax = 0' % embed, lambda: fused(embed=embed, Lmax=0), bufs)
    return out
