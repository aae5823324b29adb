"""omp_gemm_bias_act (csrc/gemm.hip and the tile-kernel units csrc/gemm256.hip, gemm4w.hip, gemm4wr.hip, gemm4wp.hip) at every ragged edge, pitch and few-row count: the 128x128 / 64x64 DMA tile
kernels (selectors 5, 6), the 256x256 tile kernels (9, 10, 16, 20), gemm_rows (3) and the split-K gemm_small with its fused LayerNorm
prologue (4), forced with ops.force_gemm_kernel.

Every launch goes through run_case:
  * the destination (and the second destination) is a VIEW into a larger buffer of sentinel bits: ldc > N, gap columns on both sides,
    guard rows before row 0 and after row M - 1.  After the launch every sentinel must be there bit for bit (gate 0);
  * A, W and the residual are views with lda > K, ldw > K, ldr > N whose gap columns and guard rows hold NaN (the few-row sweeps: NaN in
    every row of A from M to 63); the output must be finite (gate 0) and equal the float64 restatement;
  * pitch classes: 'vec' (ldc and ldr multiples of the 16-byte chunk), 'scalar' (ldc not a multiple of 4 elements: store4 element by
    element), 'ldr_odd' (ldc even, ldr odd);
  * out is residual (in place) must equal out of place bit for bit;
  * bias 'table' (bias_row_mod / bias_row_off: row m takes table row (off + m) % mod): the device table has exactly mod rows between NaN
    guard rows, and next to float64 every row must equal, bit for bit, its row of the one-row launch (bias_row = [j]) of its table row.
Stray accesses are detected BY VALUE only: nothing here looks at a kernel's code or provokes a fault.

ref_gemm / ref_ln_gemm are the float64 restatements (tests/test_gemm_reference.py pins them to plain torch and to tests/fake_ops.gemm, and
proves on the CPU -- a fake launch with one seeded defect at a time -- that run_case notices what it is for).

Every check returns rec / rrec records (tests/gpu_checks.py); the measured errors go to the parity report.
"""
import functools
import math

import torch
import torch.nn.functional as F

from tests.gpu_checks import DEV, rec, rnd, rrec
from tests.gpu_checks_encoder import VIEW_LEAD, VIEW_OFF, gelu64, guarded_view, kept_view, nan_bits, sent_bits

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2      # include/omp355.h: OMP_ACT_*
ACT_NAMES = {ACT_NONE: 'none', ACT_GELU: 'gelu', ACT_RELU: 'relu'}
DT = {'bf16': torch.bfloat16, 'fp32': torch.float32}
ERR_INVALID, ERR_UNSUPPORTED = -22, -95     # OMP_ERR_*
TILE = {5: 128, 6: 64, 9: 256, 10: 256, 16: 256, 20: 256}
SEL_CLASS = {5: 'dma', 6: 'dma', 9: 'tile256', 10: 'tile256', 16: 'tile256', 20: 'tile256', 3: 'rows', 4: 'small'}
# K tiles of 128 bytes per ring (the depth NS read from the kernel's file): 1, 2, NS - 1, NS, NS + 1, 2 NS + 1 where the selector takes them
#   5: gemm_dma<128, 128, NS = 2>;  6: gemm_dma<64, 64, NS = 8> up to 512 tiles (NS = 4 above: check_ring4)
#   9: gemm_256, two 64 KB buffers (NS = 2), K >= 128;  10: gemm_4w, ring of 5 operand-tile slots, K = 64 allowed
#   16 / 20: gemm_4w_r / gemm_4w_p, NS = 5 X tiles, K % 256 == 0: the multiples of four tiles around NS - 1, NS + 1 and 2 NS + 1
K_TILES = {5: (1, 2, 3, 5), 6: (1, 2, 7, 8, 9, 17), 9: (2, 3, 5), 10: (1, 2, 3, 4, 5, 6, 11), 16: (4, 8, 12), 20: (4, 8, 12)}

# Gates, relative to each output row's own max |ref|, per (selector class, operand type, destination type, activation).  Each gate is
# about 3x the worst case measured on an MI355X against the float64 restatement (never more than 4x; the headroom is for box-to-box
# differences in fp32 summation order only); (gate, measured).  On top of its gate every case is held to the absolute gates
# check_gemm has always used (_cap).  A key that is not in the table could not be measured: its cases are held to _cap alone and say so.
# 'ln offset' is the planted LayerNorm row of mean 1e3 and unit spread (its fp32 mean carries 1e3 * 2^-24 per element).
TOL = {
    ('dma', 'bf16', 'bf16', 'gelu'): (1.2e-02, 3.91e-03),
    ('dma', 'bf16', 'bf16', 'none'): (1.9e-02, 6.17e-03),
    ('dma', 'bf16', 'bf16', 'relu'): (1.4e-03, 4.81e-04),
    ('dma', 'bf16', 'fp32', 'gelu'): (7.7e-07, 2.56e-07),
    ('dma', 'bf16', 'fp32', 'none'): (7.8e-07, 2.62e-07),
    ('dma', 'bf16', 'fp32', 'relu'): (8.9e-07, 2.97e-07),
    ('dma', 'bf16', 'split', 'gelu'): (4.6e-05, 1.52e-05),
    ('dma', 'bf16', 'split', 'none'): (3.5e-05, 1.18e-05),
    ('dma', 'fp32', 'fp32', 'gelu'): (5.0e-06, 1.65e-06),
    ('dma', 'fp32', 'fp32', 'none'): (3.4e-06, 1.12e-06),
    ('dma', 'fp32', 'fp32', 'relu'): (2.5e-06, 8.31e-07),
    ('ln', 'bf16', 'bf16', 'none'): (1.2e-02, 4.07e-03),
    ('ln', 'bf16', 'bf16', 'relu'): (5.1e-03, 1.70e-03),
    ('ln', 'bf16', 'fp32', 'none'): (5.4e-04, 1.81e-04),
    ('ln', 'fp32', 'fp32', 'none'): (1.6e-06, 5.26e-07),
    ('ln', 'fp32', 'fp32', 'relu'): (1.8e-06, 6.15e-07),
    ('ln offset', 'bf16', 'bf16', 'none'): (2.1e-02, 6.90e-03),
    ('ln offset', 'bf16', 'bf16', 'relu'): (1.9e-02, 6.17e-03),
    ('ln offset', 'bf16', 'fp32', 'none'): (1.3e-03, 4.21e-04),
    ('ln offset', 'fp32', 'fp32', 'none'): (2.1e-04, 7.06e-05),
    ('ln offset', 'fp32', 'fp32', 'relu'): (2.2e-04, 7.19e-05),
    ('rows', 'bf16', 'bf16', 'gelu'): (4.7e-05, 1.58e-05),
    ('rows', 'bf16', 'bf16', 'none'): (1.7e-02, 5.59e-03),
    ('rows', 'bf16', 'bf16', 'relu'): (1.1e-02, 3.65e-03),
    ('rows', 'bf16', 'fp32', 'gelu'): (1.5e-06, 4.94e-07),
    ('rows', 'bf16', 'fp32', 'none'): (2.0e-06, 6.56e-07),
    ('rows', 'bf16', 'fp32', 'relu'): (1.6e-06, 5.20e-07),
    ('rows', 'bf16', 'split', 'none'): (3.2e-05, 1.07e-05),
    ('rows', 'fp32', 'fp32', 'gelu'): (4.1e-06, 1.37e-06),
    ('rows', 'fp32', 'fp32', 'none'): (7.0e-06, 2.32e-06),
    ('rows', 'fp32', 'fp32', 'relu'): (3.8e-06, 1.27e-06),
    ('small', 'bf16', 'bf16', 'gelu'): (4.7e-05, 1.58e-05),
    ('small', 'bf16', 'bf16', 'none'): (1.7e-02, 5.59e-03),
    ('small', 'bf16', 'bf16', 'relu'): (1.1e-02, 3.65e-03),
    ('small', 'bf16', 'fp32', 'gelu'): (7.8e-07, 2.61e-07),
    ('small', 'bf16', 'fp32', 'none'): (9.3e-07, 3.10e-07),
    ('small', 'bf16', 'fp32', 'relu'): (7.3e-07, 2.43e-07),
    ('small', 'fp32', 'fp32', 'gelu'): (2.9e-06, 9.69e-07),
    ('small', 'fp32', 'fp32', 'none'): (2.6e-06, 8.67e-07),
    ('small', 'fp32', 'fp32', 'relu'): (2.6e-06, 8.61e-07),
    ('tile256', 'bf16', 'bf16', 'gelu'): (1.2e-02, 3.91e-03),
    ('tile256', 'bf16', 'bf16', 'none'): (1.9e-02, 6.17e-03),
    ('tile256', 'bf16', 'bf16', 'relu'): (1.4e-03, 4.81e-04),
    ('tile256', 'bf16', 'fp32', 'gelu'): (7.7e-07, 2.56e-07),
    ('tile256', 'bf16', 'fp32', 'none'): (7.8e-07, 2.62e-07),
    ('tile256', 'bf16', 'fp32', 'relu'): (5.5e-07, 1.82e-07),
    ('tile256', 'bf16', 'split', 'gelu'): (4.6e-05, 1.52e-05),
}

WORST = {}   # key -> worst measured value of this process (tools that re-measure the table read it)


def _cap(ref, out_kind, key=('',)):
    """the gates of tests/gpu_checks.py for the same case: fp32 destinations 2e-4 absolute, bf16 max(3e-2, 2^-8 max |ref|), split pair
    rows (hi + lo) the 4e-5 max(1, max |ref|) of check_gemm_x3.  Behind the LayerNorm prologue check_gemm_small doubles its gate, by
    operand type (fp32 4e-4, bf16 6e-2): the normalised row is rounded to the operand type, and an fp32 LayerNorm may round an element
    to the other bf16 neighbour than the float64 one does, whatever the destination holds."""
    top = ref.abs().max().item()
    if key[0].startswith('ln'):
        return 4e-4 if key[1] == 'fp32' else max(6e-2, 2.0 ** -7 * top)
    if out_kind == 'bf16':
        return max(3e-2, 2.0 ** -8 * top)
    return 2e-4 if out_kind == 'fp32' else 4e-5 * max(1.0, top)


def krec(kind, name, err, tol, note='', report=False):
    r = (rrec if report else rec)(name, err, tol, note)
    r['kind'] = kind
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------------------------------------------------------
def ref_gemm(A, W, bias=None, bias_mode='n', act=ACT_NONE, residual=None, out='fp64', row=0, mod=0, off=0):
    """act(A W^T + bias) + residual in float64 on the operands as the kernel sees them (already rounded to the operand type).
    bias_mode: 'n' bias[n], 'm' bias[m], 'row' bias[row][n] of a table, 'table' the table's per-row form: row m takes
    bias[(off + m) % mod][n].  GELU is the erf form.  out: 'fp64' unrounded (fp32 destinations are compared with it), 'bf16' rounded
    once to bf16, 'split' -> (hi plane, lo plane) of the split-bf16 pair rows."""
    y = A.double() @ W.double().t()
    if bias is not None:
        b = bias.double()
        if bias_mode == 'table':
            for m in range(y.shape[0]):
                y[m] += b[(off + m) % mod]
        else:
            y = y + (b[:, None] if bias_mode == 'm' else b[row] if bias_mode == 'row' else b)
    y = gelu64(y) if act == ACT_GELU else (y.clamp_min(0.0) if act == ACT_RELU else y)
    if residual is not None:
        y = y + residual.double()
    if out == 'bf16':
        return y.to(torch.bfloat16).double()
    if out == 'split':
        hi = y.to(torch.bfloat16).double()
        return hi, (y - hi).to(torch.bfloat16).double()
    return y


def ref_ln_gemm(X, g, b, eps, W, dtype, **kw):
    """ref_gemm behind F.layer_norm in float64; the normalised row is rounded to the operand type, where the prologue of gemm_small
    rounds it on its way into LDS"""
    K = X.shape[-1]
    y = F.layer_norm(X.double(), (K,), g.double(), b.double(), eps)
    return ref_gemm(y.to(dtype).double(), W, **kw)


def wrap_a(A, K, a_wrap):
    """the A operand a bf16x3 product reads: K columns of a [M, a_wrap] pair row, the columns beyond a_wrap wrap back ([hi | lo | hi])"""
    return torch.cat([A, A[:, :K - a_wrap]], 1) if a_wrap else A


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def case(sel, dtn, out, M, N, K, bias='n', act=ACT_NONE, res=False, inplace=False, c2=False, trans=0, a_wrap=0, pitch='vec', ln=None,
         rows=None, seed=1, plant=False, tail=VIEW_LEAD, mod=0, off=0, one=None, hint=False):
    """sel: selector; dtn: operand type; out: 'bf16' / 'fp32' / 'split'; bias: None / 'n' / 'm' / 'row' / 'table'; res: residual of the
    destination's type; inplace: out is residual; c2: second destination; trans: trans_rows (> 0: M = 3 * trans, transposed store with
    trans_ld > trans_rows); a_wrap: A is [M, a_wrap] pair rows; ln: eps of the fused LayerNorm (A is the fp32 stream); rows: rows of
    the host operands (>= M; the launch takes the first M -- rows are independent); plant: LayerNorm edge rows; tail: NaN rows behind A.
    bias 'table': a device table of exactly `mod` rows between NaN guard rows; row m takes row (off + m) % mod (bias_row_mod /
    bias_row_off), or, one = j, every row takes row j through bias_row = [j] (the one-row form on the same table); hint: the split-K
    hint (small_m_splitk)"""
    return dict(sel=sel, dtn=dtn, out=out, M=M, N=N, K=K, bias=bias, act=act, res=res or inplace, inplace=inplace, c2=c2, trans=trans,
                a_wrap=a_wrap, pitch=pitch, ln=ln, rows=rows or M, seed=seed, plant=plant, tail=tail, mod=mod, off=off, one=one, hint=hint)


def tol_key(c):
    cls = 'ln' if c['ln'] is not None else SEL_CLASS[c['sel']]
    return (cls, c['dtn'], c['out'], ACT_NAMES[c['act']])


def tag(c):
    t = 'gemm[k%d,%s->%s,%dx%dx%d' % (c['sel'], c['dtn'], c['out'], c['M'], c['N'], c['K'])
    t += ',bias %s' % c['bias'] if c['bias'] else ',no bias'
    if c['bias'] == 'table':
        t += ' of %d rows, ' % c['mod'] + ('(%d + m) %% %d' % (c['off'], c['mod']) if c['one'] is None else 'row %d' % c['one'])
    if c['act']:
        t += ',' + ACT_NAMES[c['act']]
    for k, s in (('inplace', 'in place'), ('c2', 'C2'), ('trans', 'trans_out'), ('a_wrap', 'a_wrap'), ('plant', 'planted rows')):
        if c[k]:
            t += ',' + s
    if c['res'] and not c['inplace']:
        t += ',residual'
    if c['ln'] is not None:
        t += ',LN eps %g' % c['ln']
    return t + ',%s]' % c['pitch']


LN_CONST, LN_OFFSET = 0.75, 1e3


def ln_plant_rows(M):
    """(constant row, offset row) among the M rows of a planted LayerNorm case, None where there is no room: row 0 is constant from
    M = 2, row M - 1 the offset row from M = 3 (a random row stays in every launch: the two eps values must give different outputs)"""
    return (0 if M >= 2 else None, M - 1 if M >= 3 else None)


PTABLE_ROWS = 7   # rows of the host table the per-row bias cases cut theirs from (the first `mod`)


@functools.lru_cache(maxsize=6)
def host(dtn, rows, N, K, a_wrap, seed, ln):
    """CPU operands, rounded to the types the kernel reads them in"""
    dt = DT[dtn]
    ka = a_wrap or K
    h = dict(W=(rnd(N, K, seed=seed + 1) / math.sqrt(K)).to(dt), bias_n=rnd(N, seed=seed + 2), bias_m=rnd(rows, seed=seed + 3),
             table=rnd(5, N, seed=seed + 4), ptable=rnd(PTABLE_ROWS, N, seed=seed + 9), res_bf16=rnd(rows, N, seed=seed + 5).to(torch.bfloat16), res_fp32=rnd(rows, N, seed=seed + 6))
    if ln:
        h['A'] = rnd(rows, K, seed=seed) * 1.5 + 0.2
        h['g'], h['b'] = rnd(K, seed=seed + 7) * 0.1 + 1, rnd(K, seed=seed + 8) * 0.1
    else:
        h['A'] = rnd(rows, ka, seed=seed).to(dt)
    return h


LN_LOW = 0.03   # spread of the low-variance row: its variance 9e-4 is of the order of the larger eps


def ln_low_row(M):
    """the row of a planted LayerNorm case that holds 0.2 + LN_LOW * noise: between eps = 1e-5 and 1e-3 its scale 1 / sqrt(var + eps)
    moves by a third, so the two outputs differ by construction, not by the chance of a bf16 rounding falling the other way"""
    return min(1, M - 1)


def plant_ln(X, M):
    """X [M, K] fp32 -> copy with the planted rows of ln_plant_rows and ln_low_row"""
    X = X.clone()
    X[ln_low_row(M)] = 0.2 + LN_LOW * rnd(X.shape[1], seed=78)
    rc, ro = ln_plant_rows(M)
    if ro is not None:
        X[ro] = LN_OFFSET + rnd(X.shape[1], seed=77)
    if rc is not None:
        X[rc] = LN_CONST
    return X


def _pitches(c, width):
    base = (VIEW_OFF + width + 7) // 8 * 8 + 8
    ldc, ldr = {'vec': (base, base + 8), 'scalar': (base + 1, base + 8), 'ldr_odd': (base, base + 9)}[c['pitch']]
    return ldc, (ldc if c['inplace'] else ldr)


def _pitch_in(width, extra):
    return (VIEW_OFF + width + 7) // 8 * 8 + extra


def reference(c, h, A):
    """float64 (out, out2, raw, raw2) of case c on host operands h with the A rows `A` ([M, ...]): out / out2 as the destination holds
    them (rounded once to bf16; a (hi, lo) pair for split rows), raw / raw2 the unrounded values the absolute gates are taken against"""
    M = c['M']
    bias = {None: None, 'n': h['bias_n'], 'm': h['bias_m'][:M], 'row': h['table'], 'table': h['ptable'][:c['mod']]}[c['bias']]
    res = h['res_' + ('bf16' if c['out'] == 'bf16' else 'fp32')][:M] if c['res'] else None
    kw = dict(bias=bias, bias_mode=c['bias'] or 'n', act=c['act'], row=3, mod=c['mod'], off=c['off'])
    if c['bias'] == 'table' and c['one'] is not None:
        kw.update(bias_mode='row', row=c['one'])
    if c['ln'] is not None:
        f = lambda **k: ref_ln_gemm(A, h['g'], h['b'], c['ln'], h['W'], DT[c['dtn']], **k)
    else:
        f = lambda **k: ref_gemm(wrap_a(A, c['K'], c['a_wrap']), h['W'], **k)
    out = f(residual=res, out=c['out'] if c['out'] != 'fp32' else 'fp64', **kw)
    out2 = f(out=c['out'] if c['out'] != 'fp32' else 'fp64', **kw) if c['c2'] else None
    raw = f(residual=res, out='fp64', **kw)
    raw2 = f(out='fp64', **kw) if c['c2'] else None
    return out, out2, raw, raw2


def gpu_launch(call):
    """omp_gemm_bias_act on the views of `call`, its selector forced (and 0 restored)"""
    from advancedliteratemachinery_amd import ops
    ops.force_gemm_kernel(0 if call['hint'] else call['sel'])   # under the split-K hint the library's own rule must answer 4 (the prefill's path)
    try:
        ops.gemm(call['A'], call['W'], call['bias'], residual=call['residual'], act=call['act'], out=call['out'],
                 out_dtype=ops.SPLIT if call['split'] else None, M=call['M'], N=call['N'], K=call['K'], ldc=call['ldc'],
                 bias_row=call['bias_row'], bias_row_stride=call['bias_row_stride'], trans_rows=call['trans_rows'], trans_ld=call['trans_ld'],
                 ln=call['ln'], ln_eps=call['ln_eps'], bias_along_m=call['bias_mode'] == 'm', out_noresidual=call['out2'], a_wrap=call['a_wrap'],
                 bias_row_mod=call['bias_row_mod'], bias_row_off=call['bias_row_off'], small_m=call['hint'], store_mode=call.get('store_mode', 0),
                 kv=call.get('kv'))
    finally:
        ops.force_gemm_kernel(0)
    torch.cuda.synchronize()


def run_case(c, launch=gpu_launch, device=DEV, A=None, report=True, expect=None, expect_msg=None):
    """Build the guarded views of case c, launch, check -> (records, outputs {name: clone of the destination view}).
    A: host A rows [M, ...] instead of the case's own (planted inputs).  expect: an OMP_ERR_* code the call must be refused with (nothing
    runs: every destination keeps its sentinels); expect_msg: a text the refusal's message (behind the code) must hold."""
    out = []
    M, N, K, dt = c['M'], c['N'], c['K'], DT[c['dtn']]
    h = host(c['dtn'], c['rows'], N, K, c['a_wrap'], c['seed'], c['ln'] is not None)
    if A is None:
        A = h['A'][:M]
        if c['plant']:
            A = plant_ln(A, M)
    odt = torch.float32 if c['out'] == 'fp32' else torch.bfloat16
    name = tag(c)
    # inputs between NaN
    _, Av = guarded_view(M, A.shape[1], _pitch_in(A.shape[1], 8), A.dtype, nan_bits(A.dtype), A.to(device), device, tail=c['tail'])
    _, Wv = guarded_view(N, K, _pitch_in(K, 16), dt, nan_bits(dt), h['W'].to(device), device)
    # destinations between sentinels
    if c['trans']:
        tr, Bn = c['trans'], M // c['trans']
        crows, cw = Bn * N, tr
    else:
        crows, cw = M, (2 * N if c['out'] == 'split' else N)
    ldc, ldr = _pitches(c, cw)
    res_h = h['res_' + ('bf16' if c['out'] == 'bf16' else 'fp32')][:M] if c['res'] else None
    Cb, Cv = guarded_view(crows, cw, ldc, odt, sent_bits(odt), res_h.to(device) if c['inplace'] else None, device)
    Rv = None
    if c['inplace']:
        Rv = Cv
    elif c['res']:
        _, Rv = guarded_view(M, N, ldr, odt, nan_bits(odt), res_h.to(device), device)
    C2b = C2v = None
    if c['c2']:
        C2b, C2v = guarded_view(M, N, ldc + 16, odt, sent_bits(odt), None, device)
    bias = {None: None, 'n': h['bias_n'], 'm': h['bias_m'][:M].contiguous(), 'row': h['table'], 'table': h['ptable'][:c['mod']]}[c['bias']]
    bias_row, bias_ld, per_row = (3 if c['bias'] == 'row' else None), (N if c['bias'] == 'row' else 0), False
    if c['bias'] == 'table':   # exactly mod rows between NaN rows, at a pitch of its own: a read of any other row shows up by value
        bias_ld = _pitch_in(N, 4)
        _, bias = guarded_view(c['mod'], N, bias_ld, torch.float32, nan_bits(torch.float32), bias.to(device), device)
        bias_row, per_row = c['one'], c['one'] is None
    call = dict(sel=c['sel'], A=Av, W=Wv, bias=None if bias is None else bias.to(device), bias_mode=c['bias'],
                bias_row=torch.tensor([bias_row], dtype=torch.int32, device=device) if bias_row is not None else None,
                bias_row_stride=bias_ld, bias_row_mod=c['mod'] if per_row else 0, bias_row_off=c['off'] if per_row else 0, hint=c['hint'],
                residual=Rv, act=c['act'], out=Cv, out2=C2v, split=c['out'] == 'split',
                M=M, N=N, K=K, ldc=ldc, trans_rows=c['trans'], trans_ld=ldc if c['trans'] else 0, a_wrap=c['a_wrap'],
                ln=None if c['ln'] is None else (h['g'].to(device), h['b'].to(device)), ln_eps=c['ln'] if c['ln'] is not None else 1e-5)
    err = ''
    try:
        launch(call)
    except RuntimeError as e:
        err = str(e)
    if expect is not None:
        why = '' if '(%d)' % expect in err and (expect_msg or '') in err.partition('): ')[2] else (err or 'no error')
        out.append(krec('refusal', name + ': refused with %d%s' % (expect, '' if not why else ' -- ' + why), 0 if not why else 1, 0))
    elif err:
        out.append(krec('launch', name + ': ' + err, 1, 0))
        return out, {}
    # gate 0: the sentinels
    probs = []
    for nm, (buf, r, w) in dict(C=(Cb, crows, cw), C2=(C2b, M, N)).items():
        if buf is not None:
            rows_ok, cols_ok = kept_view(buf, r, w, sent_bits(odt))
            probs += [] if rows_ok else ['%s: a guard row was written' % nm]
            probs += [] if cols_ok else ['%s: a gap column was written' % nm]
            if expect is not None and not c['inplace'] and not _all_bits(buf, sent_bits(odt)):
                probs.append('%s: a refused call wrote' % nm)
    out.append(krec('guards', name + ': sentinels bit-identical%s' % ('' if not probs else ' -- ' + '; '.join(probs)), len(probs), 0))
    if expect is not None:
        return out, {}
    outs = {'C': Cv.clone()}
    if C2v is not None:
        outs['C2'] = C2v.clone()
    # gate 0: no NaN from a gap column, a guard row or a row at or beyond M
    bad = sum(int((~torch.isfinite(v)).sum().item()) for v in outs.values())
    out.append(krec('nan', name + ': output finite', bad, 0, '%d NaN / inf elements' % bad))
    # the float64 restatement
    ref, ref2, raw, raw2 = reference(c, h, A)
    raw = raw.to(device)
    key = tol_key(c)
    if c['out'] == 'split':
        got = Cv[:, :N].double() + Cv[:, N:].double()
        want = (ref[0] + ref[1]).to(device)
    elif c['trans']:
        got = Cv.double().reshape(Bn, N, tr).permute(0, 2, 1).reshape(M, N)
        want = ref.to(device)
    else:
        got, want = Cv.double(), ref.to(device)
    groups = [('', got, want, key, raw)]
    if c['plant'] and ln_plant_rows(M)[1] is not None:   # the offset row has a gate of its own
        ro = ln_plant_rows(M)[1]
        keep = torch.arange(M, device=device) != ro
        groups = [('', got[keep], want[keep], key, raw[keep]), (' offset row', got[ro:ro + 1], want[ro:ro + 1], ('ln offset',) + key[1:], raw[ro:ro + 1])]
    if C2v is not None:
        groups.append((' C2', C2v.double(), ref2.to(device), key, raw2.to(device)))
    for sfx, g, w, k, rw in groups:
        gate(out, name + sfx, k, g, w, rw, c['out'], report)
    return out, outs


def _all_bits(buf, bits):
    return bool((buf.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32) == bits).all().item())


def gate(out, name, key, got, want, raw, out_kind, report=True):
    """per output row against that row's max |ref| of the reference as the destination holds it (the table's gate), and the absolute
    gate of the existing checks, which those take against the UNROUNDED reference `raw`: against the rounded one a single bf16 rounding
    that falls the other way is a whole ulp (2^-7 of the element), which the 2^-8 max |ref| of check_gemm was never meant to admit"""
    d = (got - want).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    rel = (d.amax(1) / want.abs().amax(1).clamp_min(1e-30)).max().item()
    WORST[key] = max(WORST.get(key, 0.0), rel)
    g = TOL.get(key)
    da = (got - raw).abs()
    da = torch.where(torch.isfinite(da), da, torch.full_like(da, float('inf'))).max().item()
    if g is not None:
        out.append(krec('value', name + ': per row vs float64', rel, g[0], 'relative to the row\'s max |ref|; gate %s measured %.2e' % (key, g[1]), report))
    out.append(krec('value' if g is None else 'cap', name + ': absolute%s' % ('' if g is not None else ' (no measured gate for %s)' % (key,)),
                    da, _cap(raw, out_kind, key), 'rel %.3e' % rel, report and g is None))


def fold(records, name):
    """the records of a sweep: every failing one, and per kind the worst of the passing ones under one name (reported)"""
    out = [r for r in records if not r['ok']]
    for kind in sorted({r['kind'] for r in records}):
        rs = [r for r in records if r['kind'] == kind and r['ok']]
        if rs:
            w = max(rs, key=lambda r: r['err'] / r['tol'] if r['tol'] > 0 else r['err'])
            out.append(krec(kind, '%s: %s, worst of %d: %s' % (name, kind, len(rs), w['name']), w['err'], w['tol'], w['note'], True))
    return out


def same_bits(out, name, a, b):
    ib = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    neq = int((a.contiguous().view(ib) != b.contiguous().view(ib)).sum().item())
    out.append(krec('bits', name, neq, 0, 'elements that differ, of %d' % a.numel()))


def accepts(c):
    """what the selector's *_ok predicate (and the host checks of omp_gemm_bias_act) take of a case, restated from csrc/gemm_common.h"""
    s, bf = c['sel'], c['dtn'] == 'bf16'
    if c['out'] == 'split' and (not bf or c['N'] % 8 or c['res'] or c['trans']):
        return False
    if c['a_wrap'] and not bf:
        return False
    if c['c2'] and (c['pitch'] != 'vec' or c['M'] <= 64 or c['N'] % 8 or not c['res']):
        return False
    if s in (3, 5, 6):
        return True
    if s == 4:
        return c['M'] <= 64 and c['K'] % (128 if bf else 64) == 0 and not c['trans'] and not c['a_wrap'] and c['out'] != 'split'
    ok = bf and not c['trans'] and c['N'] % 8 == 0 and c['bias'] != 'm' and c['pitch'] == 'vec'
    ok = ok and (c['K'] >= 128 or (s == 10 and c['K'] == 64)) and c['K'] % 64 == 0
    if s in (16, 20):
        ok = ok and c['K'] % 256 == 0
    if s == 20:
        ok = ok and c['M'] % 256 == 0 and c['N'] % 256 == 0
    return ok


def run_tile(out, c, base=None):
    """run_case, and for the 256x256 kernels the bit equality with selector 5 on the same guarded views that check_gemm_4w claims"""
    recs, o = run_case(c)
    out += recs
    if c['sel'] in (9, 10, 16, 20) and o:
        if base is None:
            r5, base = run_case(dict(c, sel=5), report=False)
            out += [r for r in r5 if not r['ok']]
        for k in o:
            same_bits(out, tag(c) + ': %s == selector 5 bit for bit' % k, o[k], base[k])
    return o


# ---------------------------------------------------------------------------------------------------------------------------------------
# the tile kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
def _kt(dtn):
    return 64 if dtn == 'bf16' else 32          # elements of a 128-byte K tile


def check_tile_mn(sel, dtn):
    """M in {1, T - 1, T, T + 1, 2 T + 17} x N in {8, T - 8, T, T + 8, T + 3 (5, 6)} at K = 2 tiles: bias + residual, vector pitches"""
    T = TILE[sel]
    Ms, Ns = (1, T - 1, T, T + 1, 2 * T + 17), (8, T - 8, T, T + 8) + ((T + 3,) if sel in (5, 6) else ())
    if sel == 20:
        Ms, Ns = (256, 512), (256, 512)
    K = 2 * _kt(dtn) if sel not in (16, 20) else 256
    recs = []
    for N in Ns:
        for M in Ms:
            c = case(sel, dtn, dtn, M, N, K, res=True, rows=max(Ms), seed=N)
            if accepts(c):
                run_tile(recs, c)
    return fold(recs, 'gemm[k%d,%s] M x N edges' % (sel, dtn))


def check_tile_k(sel, dtn):
    """K = 1, 2, NS - 1, NS, NS + 1, 2 NS + 1 tiles of the selector's ring at the ragged corner (T + 1, T + 8) and at (2 T + 17, T - 8)"""
    T = TILE[sel]
    shapes = ((T + 1, T + 8), (2 * T + 17, T - 8)) if sel != 20 else ((256, 512), (512, 256))
    recs = []
    for nt in K_TILES[sel]:
        for (M, N) in shapes:
            for act in (ACT_NONE, ACT_GELU):
                c = case(sel, dtn, dtn, M, N, nt * _kt(dtn), act=act, res=act == ACT_NONE, seed=nt)
                if accepts(c):
                    run_tile(recs, c)
    return fold(recs, 'gemm[k%d,%s] K tiles %s' % (sel, dtn, K_TILES[sel]))


def check_ring4(dtn):
    """the 4-stage ring of the 64x64 kernel (more than 512 tiles): one 1500 x 1600 product at K = 1, 3, 4 and 5 tiles"""
    recs = []
    for nt in (1, 3, 4, 5):
        recs += run_case(case(6, dtn, dtn, 1500, 1600, nt * _kt(dtn), res=True, seed=nt))[0]
    return fold(recs, 'gemm[k6,%s] 4-stage ring, 1500x1600' % dtn)


def epilogues(sel, dtn, M, N, K, pitch):
    """the epilogue cases of a shape (those the host checks take; the selector's own refusals are filtered by accepts)"""
    other = 'fp32' if dtn == 'bf16' else None
    cs = [case(sel, dtn, dtn, M, N, K, bias=None, pitch=pitch),
          case(sel, dtn, dtn, M, N, K, pitch=pitch),
          case(sel, dtn, dtn, M, N, K, bias='row', pitch=pitch),
          case(sel, dtn, dtn, M, N, K, bias='m', pitch=pitch),
          case(sel, dtn, dtn, M, N, K, bias='m', act=ACT_GELU, res=True, pitch=pitch),
          case(sel, dtn, dtn, M, N, K, act=ACT_GELU, pitch=pitch),
          case(sel, dtn, dtn, M, N, K, act=ACT_RELU, pitch=pitch),
          case(sel, dtn, dtn, M, N, K, res=True, pitch=pitch),
          case(sel, dtn, dtn, M, N, K, res=True, c2=True, pitch=pitch),
          case(sel, dtn, dtn, 3 * (M // 3), N, K, trans=M // 3, pitch=pitch)]
    if other:
        cs += [case(sel, dtn, 'fp32', M, N, K, res=True, pitch=pitch),
               case(sel, dtn, 'fp32', M, N, K, act=ACT_GELU, pitch=pitch),
               case(sel, dtn, 'fp32', M, N, K, bias='m', res=True, pitch=pitch),
               case(sel, dtn, 'fp32', M, N, K, res=True, c2=True, pitch=pitch),
               case(sel, dtn, 'split', M, N, K, act=ACT_GELU, pitch=pitch),
               case(sel, dtn, 'split', M, N, K, bias='m', pitch=pitch),
               case(sel, dtn, dtn, M, N, 384, a_wrap=256, pitch=pitch),
               case(sel, dtn, 'fp32', M, N, 384, a_wrap=256, res=True, pitch=pitch)]
    return cs


def check_tile_epilogues(sel, dtn):
    """every epilogue at the ragged corner (T + 1, T + 8) and at one even shape (2 T, 2 T), on vector pitches and (5, 6) on the scalar
    store4 pitches.  Not folded: the bias_along_m records are the ones the fix of the vector epilogue is judged by."""
    T, out = TILE[sel], []
    K = 256 if sel in (16, 20) else 2 * _kt(dtn)
    shapes = ((T + 1, T + 8), (2 * T, 2 * T)) if sel != 20 else ((256, 512),)
    for (M, N) in shapes:
        for pitch in ('vec', 'scalar'):
            for c in epilogues(sel, dtn, M, N, K, pitch):
                if accepts(c):
                    run_tile(out, c)
    return out


def check_tile_pitches(sel, dtn):
    """the three pitch classes with a bf16 and an fp32 destination (bias, ReLU, residual) at the ragged corner and at (T - 1, T + 3)"""
    T, out = TILE[sel], []
    K = 256 if sel in (16, 20) else 2 * _kt(dtn)
    for (M, N) in ((T + 1, T + 8), (T - 1, T + 3)) if sel != 20 else ((256, 256),):
        for pitch in ('vec', 'scalar', 'ldr_odd'):
            for o in ((dtn, 'fp32') if dtn == 'bf16' else ('fp32',)):
                for bias in ('n', 'm'):
                    c = case(sel, dtn, o, M, N, K, bias=bias, act=ACT_RELU, res=True, pitch=pitch)
                    if accepts(c):
                        run_tile(out, c)
    return out


def check_tile_refusals(sel):
    """one combination the selector refuses: OMP_ERR_UNSUPPORTED, nothing launched (the destination keeps every sentinel)"""
    out = []
    if sel in (5, 6):
        return out   # they take every product (GEMM_SELECTORS: ok = nullptr)
    M, N = (257, 264) if sel != 20 else (256, 256)
    refused = [case(sel, 'bf16', 'bf16', M, N, 256, bias='m'),            # bias_along_m with a plain destination
               case(sel, 'bf16', 'bf16', M, N, 256, pitch='scalar'),      # ldc % 8 != 0
               case(sel, 'fp32', 'fp32', M, N, 256)]                      # bf16 operands only
    if sel == 16:
        refused.append(case(sel, 'bf16', 'bf16', M, N, 320))              # K % 256 != 0
    if sel == 20:
        refused.append(case(sel, 'bf16', 'bf16', 257, 256, 256))          # M % 256 != 0
    for c in refused:
        out += run_case(c, expect=ERR_UNSUPPORTED)[0]
    return out


def check_inplace(sel, dtn):
    """out is residual == out of place, bit for bit (selectors 3, 4, 6), bf16 and fp32 destinations, vector and scalar pitches"""
    out = []
    shapes = ((65, 72), (130, 67)) if sel == 6 else ((1, 16), (17, 20), (49, 67), (64, 512))
    for (M, N) in shapes:
        for o in ((dtn, 'fp32') if dtn == 'bf16' else ('fp32',)):
            for pitch in ('vec', 'scalar'):
                c = case(sel, dtn, o, M, N, 512, res=True, act=ACT_RELU, pitch=pitch, tail=64)
                ra, a = run_case(c)
                rb, b = run_case(dict(c, inplace=True))
                out += ra + rb
                if a and b:
                    same_bits(out, tag(c) + ': in place == out of place', b['C'], a['C'])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the few-row kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
FEW_N = (16, 20, 67, 512)
FEW_K = {'bf16': (128, 512, 1152, 2048), 'fp32': (64, 128, 512, 1152, 2048)}
EDGE_M = (1, 16, 17, 32, 33, 48, 49, 64)


def check_few_rows(sel, dtn, K):
    """every M from 1 to 64 at N in FEW_N: operands built once per (N, K) with 64 rows, NaN in every row of A at or beyond M (64 NaN
    rows behind the view), the reference sliced (rows are independent).  fp32 destination with an in-place fp32 residual: the
    decoder step's product"""
    recs = []
    for N in FEW_N:
        for M in range(1, 65):
            recs += run_case(case(sel, dtn, 'fp32', M, N, K, inplace=True, rows=64, seed=N, tail=64), report=False)[0]
    return fold(recs, 'gemm[k%d,%s,K=%d] M = 1..64 x N in %s' % (sel, dtn, K, FEW_N))


def check_few_epilogues(sel, dtn):
    """bias_row, bias_along_m, ReLU into the operand type, GELU, no bias at the MF template boundaries; selector 3: one a_wrap product"""
    recs = []
    for (N, K) in ((20, 128), (67, 1152), (512, 512)):
        for M in EDGE_M:
            for kw in (dict(bias='row'), dict(bias='m'), dict(bias='m', act=ACT_RELU, res=True), dict(act=ACT_RELU), dict(act=ACT_GELU), dict(bias=None)):
                for o in ((dtn, 'fp32') if dtn == 'bf16' else ('fp32',)):
                    for pitch in ('vec', 'scalar'):
                        recs += run_case(case(sel, dtn, o, M, N, K, rows=64, seed=N, tail=64, pitch=pitch, **kw), report=False)[0]
    out = fold(recs, 'gemm[k%d,%s] few-row epilogues' % (sel, dtn))
    if sel == 3 and dtn == 'bf16':
        for M in (17, 64):
            out += run_case(case(3, 'bf16', 'fp32', M, 67, 384, a_wrap=256, res=True, tail=64))[0]
            out += run_case(case(3, 'bf16', 'split', M, 72, 384, a_wrap=256, tail=64))[0]
        out += run_case(case(3, 'bf16', 'bf16', 39, 67, 512, trans=13, tail=64))[0]
    if sel == 4:
        out += run_case(case(4, dtn, dtn, 65, 64, 512), expect=ERR_UNSUPPORTED)[0]              # M > 64
        out += run_case(case(4, dtn, dtn, 16, 64, 512, trans=8), expect=ERR_UNSUPPORTED)[0]     # trans_out
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the LayerNorm prologue of gemm_small
# ---------------------------------------------------------------------------------------------------------------------------------------
LN_K = {'bf16': (128, 384, 512, 1024), 'fp32': (64, 128, 384, 512, 1024)}
LN_EPS = (1e-5, 1e-3)


def check_ln(dtn, K):
    """selector 4 behind ln=: every M from 1 to 64 at K = 384 (nch = 96: the second pass of 64 lanes is partial) and K = 512, the MF
    boundaries at the other K; the fp32 stream has lda > K with NaN gap columns and NaN in every row at or beyond M; planted rows (a
    constant row, a row of mean 1e3 and unit spread, row M - 1); two eps values whose outputs must differ and match their references."""
    out, recs = [], []
    Ms = range(1, 65) if K in (384, 512) else (1, 16, 17, 48, 49, 64)
    for M in Ms:
        for N in ((67,) if M not in EDGE_M else (20, 67, 512)):
            got = {}
            if dtn == 'fp32' and M > 32 and 16384 + 64 * (4 * K + 16) > 160 * 1024:
                # 64 normalised fp32 rows of K > 544 do not fit the 160 KB of LDS: a clean OMP_ERR_INVALID, nothing launched
                recs += run_case(case(4, dtn, dtn, M, N, K, ln=LN_EPS[0], rows=64, seed=K + N, plant=True, tail=64), report=False, expect=ERR_INVALID)[0]
                continue
            for eps in LN_EPS:
                c = case(4, dtn, dtn, M, N, K, act=ACT_RELU if N == 20 else ACT_NONE, ln=eps, rows=64, seed=K + N, plant=True, tail=64)
                r, o = run_case(c, report=False)
                recs += r
                got[eps] = o.get('C')
            if all(v is not None for v in got.values()):
                differ = not torch.equal(got[LN_EPS[0]], got[LN_EPS[1]])
                recs.append(krec('eps', 'gemm[k4,%s,LN,%dx%dx%d]: eps = %g and %g give different outputs' % ((dtn, M, N, K) + LN_EPS), 0 if differ else 1, 0))
            if M in EDGE_M and M >= 2 and N == 67 and got[LN_EPS[0]] is not None:
                recs += ln_constant_row(dtn, M, N, K, got[LN_EPS[0]])
    out += fold(recs, 'gemm[k4,%s,LN,K=%d]' % (dtn, K))
    # fp32 destination of the bf16 engine (the decoder's q / k projections keep fp32)
    if dtn == 'bf16':
        for M in (17, 64):
            out += run_case(case(4, dtn, 'fp32', M, 67, K, ln=1e-5, rows=64, seed=K, plant=True, tail=64, pitch='scalar'))[0]
    return out


def ln_constant_row(dtn, M, N, K, o1, launch=gpu_launch, device=DEV):
    """the constant row has variance 0: its normalised row is beta EXACTLY, so its output row (o1: the destination of the LayerNorm
    launch at eps 1e-5) must equal, bit for bit, the row the same kernel gives without the prologue for an A row that holds beta
    rounded to the operand type"""
    c = case(4, dtn, dtn, M, N, K, act=ACT_RELU if N == 20 else ACT_NONE, rows=64, seed=K + N, tail=64)
    Ab = host(dtn, 64, N, K, 0, K + N, True)['b'].to(DT[dtn]).reshape(1, K).expand(M, K).contiguous()
    r2, o2 = run_case(c, launch, device, A=Ab, report=False)
    out = [r for r in r2 if not r['ok']]
    if o2:
        rc = ln_plant_rows(M)[0]
        same_bits(out, tag(dict(c, ln=1e-5, plant=True)) + ': constant row == the product of the rounded beta, bit for bit', o1[rc], o2['C'][rc])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the bias table's per-row form (bias_row_mod / bias_row_off: the batched prompt prefill's products)
# ---------------------------------------------------------------------------------------------------------------------------------------
TABLE_MODS = (1, 2, 6, 7)


def table_offs(mod):
    """0, a small offset and one beyond the table (mod + 3: no multiple of mod at mod 2, 6, 7)"""
    return (0, 4, mod + 3)


def one_row_outputs(c, launch=gpu_launch, device=DEV, rows=None):
    """the one-row form of table case c (bias_row = [j], the same forced selector, the same operands) for every j in `rows` (all of the
    table) -> (records, {j: outputs}).  Each launch is held to float64 like any other case."""
    recs, ones = [], {}
    for j in (range(c['mod']) if rows is None else rows):
        r, o = run_case(dict(c, one=j, off=0), launch, device, report=False)
        recs += r
        ones[j] = o
    return recs, ones


def table_bits(out, c, outs, ones):
    """the property the prefill pass rests on: row m of the per-row launch == row m of the one-row launch of table row (off + m) % mod,
    bit for bit, in every destination"""
    M = c['M']
    idx = (c['off'] + torch.arange(M)) % c['mod']
    for k in outs:
        if any(k not in ones.get(j, {}) for j in set(idx.tolist())):
            out.append(krec('bits', tag(c) + ': %s: a one-row launch is missing' % k, 1, 0))
            continue
        want = torch.stack([ones[int(j)][k][m] for m, j in enumerate(idx.tolist())])
        same_bits(out, tag(c) + ': %s row m == the one-row form of table row (off + m) %% mod, bit for bit' % k, outs[k], want)


def run_table(c, launch=gpu_launch, device=DEV, ones=None):
    """both gates of a per-row table case: float64 (run_case) and bit equality with the one-row form -> records"""
    recs, outs = run_case(c, launch, device, report=False)
    if ones is None:
        r1, ones = one_row_outputs(c, launch, device, rows=sorted({(c['off'] + m) % c['mod'] for m in range(c['M'])}))
        recs += r1
    if outs:
        table_bits(recs, c, outs, ones)
    return recs


SMALL_TYPES = (('bf16', 'bf16'), ('bf16', 'fp32'), ('fp32', 'fp32'))
LN_TIE_MARGIN = 16 * 2.0 ** -24   # of max(1, |y|): the mean of K terms, the variance, its inverse root, the scale and the shift each round in fp32


def ln_resolvable(X, g, b, eps, W, margin=LN_TIE_MARGIN, share=0.1):
    """False when an element of the float64-normalised rows lies within `margin` * max(1, |y|) of the midpoint of two neighbouring bf16
    values AND rounding it the other way could move an output of its row by more than `share` of the tightest gate of a bf16 LayerNorm
    case (one bf16 step of the element times the largest |w| of its column of W^T, against the row's max |y W^T|).
    ref_ln_gemm rounds the normalised row to bf16 where the prologue does; that close to a tie no fp32 LayerNorm can tell which way the
    float64 value rounds, the operand element moves by a whole bf16 step and the row's float64 reference is the reference of another
    operand -- 6e-4 of the row's max at 64 x 16 x 128 on an MI355X, where one element of 8192 (-1.5117188) sat 3e-8 (relative) from a tie.
    Decided from the float64 values and the formats alone, never from a kernel's output."""
    y = F.layer_norm(X.double(), (X.shape[-1],), g.double(), b.double(), eps)
    yb = y.to(torch.bfloat16)
    bits = yb.view(torch.int16).to(torch.int32)
    dist, step = torch.full_like(y, float('inf')), torch.zeros_like(y)
    for d in (1, -1):
        nb = (bits + d).clamp(-32768, 32767).to(torch.int16).view(torch.bfloat16).double()
        mid = (yb.double() + nb) / 2
        ok = torch.isfinite(mid)
        dist = torch.minimum(dist, torch.where(ok, (y - mid).abs(), torch.full_like(y, float('inf'))))
        step = torch.maximum(step, torch.where(ok, (yb.double() - nb).abs(), torch.zeros_like(y)))
    effect = step * W.double().abs().amax(0)[None, :] / (yb.double() @ W.double().t()).abs().amax(1, keepdim=True).clamp_min(1e-30)
    gate = min(v[0] for k, v in TOL.items() if k[0] == 'ln' and k[1] == 'bf16')
    return not bool(((dist <= margin * y.abs().clamp_min(1.0)) & (effect > share * gate)).any().item())


def ln_seed(dtn, N, K, eps, first):
    """the first seed of first, first + 1000, ... whose 64 LayerNorm input rows are resolvable (bf16 operands; fp32 operands are not rounded)"""
    if dtn != 'bf16':
        return first
    for seed in range(first, first + 1000 * 500, 1000):
        h = host(dtn, 64, N, K, 0, seed, True)
        if ln_resolvable(h['A'], h['g'], h['b'], eps, h['W']):
            return seed
    raise AssertionError('no resolvable LayerNorm input among 500 seeds')


def check_table_small(dtn, out, ln):
    """selector 4 under the split-K hint: M at every MF boundary (below 16 MF the lanes of rows beyond M form a table index too), N in
    (16, 20, 512), one K tile group, every (mod, off).  The one-row launches are shared by the twelve (mod, off) of a shape: every
    table is the first `mod` rows of one host table, and a row's bits cannot depend on how many rows lie behind it.  Behind the LayerNorm
    prologue the bf16 operand rows are drawn from the first seed whose normalised rows stay clear of a bf16 rounding tie (ln_resolvable)."""
    recs = []
    K = 128 if dtn == 'bf16' else 64
    for N in (16, 20, 512):
        seed = ln_seed(dtn, N, K, 1e-5, N) if ln else N
        for M in EDGE_M:
            base = case(4, dtn, out, M, N, K, bias='table', mod=PTABLE_ROWS, ln=1e-5 if ln else None, rows=64, seed=seed, tail=64, hint=True,
                        pitch='scalar' if N == 20 else 'vec')
            r1, ones = one_row_outputs(base)
            recs += r1
            for mod in TABLE_MODS:
                for off in table_offs(mod):
                    recs += run_table(dict(base, mod=mod, off=off), ones=ones)
    return fold(recs, 'gemm[k4,%s->%s%s] per-row bias table' % (dtn, out, ',LN' if ln else ''))


def table_epilogues(sel, M, N, K, pitch):
    """the epilogues a per-row table goes with, as accepts() filters them: plain / ReLU / GELU into bf16 and fp32, split pairs, the
    fp32 residual in place (the pass's own form), residual + C2"""
    kw = dict(bias='table', pitch=pitch)
    cs = [case(sel, 'bf16', 'bf16', M, N, K, **kw),
          case(sel, 'bf16', 'bf16', M, N, K, act=ACT_RELU, **kw),
          case(sel, 'bf16', 'bf16', M, N, K, act=ACT_GELU, **kw),
          case(sel, 'bf16', 'fp32', M, N, K, inplace=True, **kw),
          case(sel, 'bf16', 'fp32', M, N, K, act=ACT_GELU, **kw),
          case(sel, 'bf16', 'fp32', M, N, K, act=ACT_RELU, res=True, **kw),
          case(sel, 'bf16', 'fp32', M, N, K, res=True, c2=True, **kw),
          case(sel, 'bf16', 'bf16', M, N, K, res=True, c2=True, **kw),
          case(sel, 'bf16', 'split', M, N, K, **kw),
          case(sel, 'bf16', 'split', M, N, K, act=ACT_GELU, **kw)]
    return [c for c in cs if accepts(c)]


TABLE_TILE_SHAPES = {6: ((65, 127, 129), (64, 72, 67)), 5: ((129, 257), (128, 136, 131))}
TABLE_TILE_MODS = ((6, 4), (7, 10), (2, 5), (1, 4))   # (mod, off), taken in turn: off is no multiple of mod but at mod 1, M >= 2 mod + 1


def check_table_tile(sel, N):
    """selectors 5 / 6 at ragged M, N = tile, tile + 8 and tile + 3 (the 4-value path at the edge), vector and scalar pitches, every
    epilogue of table_epilogues; fp32 operands once per pitch"""
    recs, i = [], 0
    for M in TABLE_TILE_SHAPES[sel][0]:
        for pitch in ('vec', 'scalar'):
            cs = table_epilogues(sel, M, N, 128, pitch)
            if M == TABLE_TILE_SHAPES[sel][0][0]:
                cs.append(case(sel, 'fp32', 'fp32', M, N, 64, bias='table', res=True, pitch=pitch))
            for c in cs:
                mod, off = TABLE_TILE_MODS[i % len(TABLE_TILE_MODS)]
                i += 1
                recs += run_table(dict(c, mod=mod, off=off))
    return fold(recs, 'gemm[k%d,N=%d] per-row bias table' % (sel, N))


def check_table_ring4():
    """the 4-stage ring of the 64x64 kernel (more than 512 tiles) with a per-row table: one 1025 x 2048 product of one K tile pair"""
    return fold(run_table(case(6, 'bf16', 'bf16', 1025, 2048, 128, bias='table', mod=7, off=10)), 'gemm[k6] per-row bias table, 4-stage ring, 1025x2048')


STORE_KBLK = 2   # include/omp355.h: OMP_STORE_KBLK


def check_table_refusals():
    """what omp_gemm_bias_act refuses of a per-row table: OMP_ERR_INVALID, a message that names the entry point, every sentinel kept"""
    out = []

    def refused(c, **change):
        launch = (lambda call: gpu_launch(dict(call, **change)))
        out.extend(run_case(c, launch, expect=ERR_INVALID, expect_msg='omp_gemm_bias_act')[0])
    few = case(0, 'bf16', 'bf16', 64, 64, 128, bias='table', mod=6, off=4)
    big = case(6, 'bf16', 'bf16', 129, 64, 128, bias='table', mod=6, off=4)
    refused(few)                                                            # M <= 64, no split-K hint, no forced tile kernel
    refused(dict(few, sel=3))                                               # ... nor under a forced kernel without the table
    refused(big, bias_mode='m')                                             # bias_along_m
    refused(big, trans_rows=43, trans_ld=64)                                # trans_out
    refused(dict(big, M=128), store_mode=STORE_KBLK, kv=(1, 128, 128, 1, 16))   # a blocked K store
    refused(big, bias_row_stride=63)                                        # bias_row_stride < N
    refused(big, bias=None)                                                 # a null bias
    refused(big, bias_row_off=-1)                                           # a negative bias_row_off
    refused(big, bias_row_mod=-1)                                           # a negative bias_row_mod
    return out
