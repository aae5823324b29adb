"""The kernels between the encoder and the decoders at their edges: the FPN fuse (csrc/fpn.hip omp_fpn_fuse), the split-bf16 producer
(csrc/norm.hip omp_split_bf16), the row-owner K / V^T memory projection (csrc/kv_rows.hip omp_kv_project_rows), the cached memory slabs of
Decoder.project_memory (model/transformer.py) and the device pre-processing (utils/preprocess.py DevicePreprocessor).

They build the memory every decoder step of every image reads, so every ELEMENT is held to a float64 restatement here, inputs and outputs
sit between guard rows (tests/gpu_checks_encoder.py: NaN before / after an input, a sentinel before / after an output), and a batched launch
must repeat its one-image launches bit for bit.  Where a gate is not bit-exactness it is derived, not measured:

  * FPN, fp32: 4 x the distance of oracle.fpn in float32 from oracle.fpn in float64 ON THE SAME CASE (both run on the CPU; the kernel's index
    and weight arithmetic is the float32 one, the factor is for another add order and fused multiply-adds);
  * FPN, bf16: one bf16 ulp of the bf16-rounded float64 restatement per element (an fp32 bilinear can carry a value across one rounding
    boundary), never less than the fp32 gate of that case (cancellation near zero);
  * K / V^T products: |got - ref| <= 1.5 ulp(ref) + 513 * 2^-24 * (sum_k |a_k| |w_k| + |bias|): 512 exact products and 513 fp32 additions
    in any order, half an ulp of the output format for the final rounding and one more for a rounding that flips (product_gate);
  * the split-plane slabs of the parity engine: hi + lo within the 6e-5 of gpu_checks.check_cross_attn_split.

tests/test_neck_reference.py pins the restatements and helpers of this module on the CPU.  Every check returns rec / rrec records; the
measured values go to the parity report, and every check ends with a summary record (gated elements, worst error / gate).
"""
import torch
import torch.nn.functional as F

from tests import gpu_checks_encoder as E
from tests.gpu_checks import DEV, ENGINES, rec, rrec
from tests.gpu_checks_encoder import edge_rows, guard_rec, guarded, guarded_view, image_src, replicate, run_guarded

FC = 256                             # FPN channels per level
LEAD = E.VIEW_LEAD                   # guard rows in front of a buffer
U32 = 2.0 ** -24                     # unit roundoff of the fp32 accumulators
SPLIT_TOL = 6e-5                     # hi + lo of the split-plane slabs (gpu_checks.check_cross_attn_split)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_g(seed), dtype=torch.float64) * scale


def _valued(t, dt):
    """float64 tensor holding values of dt"""
    return t.to(dt).double()


# ---------------------------------------------------------------------------------------------------------------------------------------
# gates
# ---------------------------------------------------------------------------------------------------------------------------------------
def ulp_of(ref, dt):
    """the spacing of dt's numbers at |ref| (float64 in, float64 out; 0 at 0)"""
    bits = 7 if dt == torch.bfloat16 else 23
    _, e = torch.frexp(ref.abs())                                  # |ref| = m 2^e, m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 1 - bits))


def product_gate(ref, absprod, dt):
    """the derived gate of a K = 512 product + bias accumulated in fp32 and rounded to dt (module docstring); absprod = sum |a| |w| + |bias|"""
    return 1.5 * ulp_of(ref, dt) + 513 * U32 * absprod


def outside(got, ref, gate):
    """-> (elements outside the gate, worst |got - ref| / gate, elements); a non-finite element is outside; gate: tensor or number"""
    got, ref = got.double().cpu().reshape(-1), ref.reshape(-1)
    gate = torch.as_tensor(gate, dtype=torch.float64)
    gate = gate.expand(ref.shape) if gate.dim() == 0 else gate.reshape(-1)
    d = (got - ref).abs()
    d = torch.where(torch.isfinite(got), d, torch.full_like(d, float('inf')))
    ratio = torch.where(gate > 0, d / gate.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float('inf'))))
    return int((d > gate).sum().item()), (ratio.max().item() if ratio.numel() else 0.0), ref.numel()


class Tally(object):
    """gated elements and the worst error / gate of one check -> its summary record"""

    def __init__(self, name):
        self.name, self.n, self.worst = name, 0, 0.0

    def gate(self, out, name, got, ref, gate, note=''):
        bad, worst, n = outside(got, ref, gate)
        self.n += n
        self.worst = max(self.worst, worst)
        out.append(rrec(name + ': elements outside the gate', bad, 0, '%d elements, worst |err| / gate %.3f%s' % (n, worst, '; ' + note if note else '')))
        return worst

    def exact(self, n):
        self.n += n

    def summary(self, out):
        out.append(rrec('%s: summary' % self.name, 0, 0, '%d gated elements, worst |err| / gate %.3f' % (self.n, self.worst)))
        return out


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def lead_kept(buf, lead, bits):
    return bool((_bits(buf)[:lead] == bits).all().item())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. FPN fuse
# ---------------------------------------------------------------------------------------------------------------------------------------
FPN_STARTS = ((1, 1), (2, 3), (3, 5), (7, 9), (13, 8), (1, 40), (65, 3), (38, 51))     # (h2, w2) = ceil(H / 4), ceil(W / 4) of an image
FPN_INPUTS = ('random', 'l2 only', 'l3 only', 'l4 only', 'l5 only')


def level_chain(h2, w2):
    """the four level sizes a Swin backbone produces from (h2, w2): PatchMerging halves with ceil"""
    s = [(h2, w2)]
    for _ in range(3):
        s.append((-(-s[-1][0] // 2), -(-s[-1][1] // 2)))
    return tuple(s)


def fpn_inputs(sizes, kind, dt, nb=2):
    """laterals l2 .. l5, NCHW float64 [nb, 256, h, w] holding values of dt; kind FPN_INPUTS: random, or one level random and the others zero"""
    k = FPN_INPUTS.index(kind) - 1
    return [_valued(_randn(nb, FC, h, w, seed=1000 * i + 31 * h + w), dt) if k < 0 or k == i else torch.zeros(nb, FC, h, w, dtype=torch.float64)
            for i, (h, w) in enumerate(sizes)]


def fpn_oracle(lat, dtype):
    """oracle.fpn with identity 1x1 weights on the CPU in `dtype` -> float64 [nb, 1024, h3, w3]"""
    from oracle import omniparser_ref as O
    eye = torch.eye(FC, dtype=dtype).reshape(FC, FC, 1, 1)
    return O.fpn({'fpn.fpn_in.%d.weight' % i: eye for i in range(4)}, [t.to(dtype) for t in lat]).double()


def ref_fpn(lat, bf):
    """float64 restatement of fpn.py:21-45 without the 1x1 convs: p5 = l5, p_k = l_k + nearest(p_{k+1}) -- with bf every sum rounded to bf16,
    where the reference's bf16 tensors round and csrc/fpn.hip pyramid_at does -- then p2, p4, p5 resampled bilinearly (align_corners = False)
    to l3's size and (p2, p3, p4, p5) concatenated; with bf the result is rounded to bf16 once more (the output tensor)."""
    l2, l3, l4, l5 = lat
    p5 = E.rb(l5, bf)
    p4 = E.rb(l4 + F.interpolate(p5, size=l4.shape[2:], mode='nearest'), bf)
    p3 = E.rb(l3 + F.interpolate(p4, size=l3.shape[2:], mode='nearest'), bf)
    p2 = E.rb(l2 + F.interpolate(p3, size=l2.shape[2:], mode='nearest'), bf)
    sz = l3.shape[2:]
    return E.rb(torch.cat([F.interpolate(p2, size=sz, mode='bilinear'), p3, F.interpolate(p4, size=sz, mode='bilinear'),
                           F.interpolate(p5, size=sz, mode='bilinear')], 1), bf)


def token_major(t, stride=1):
    """NCHW [nb, C, h, w] -> the stride-`stride` grid, token-major [nb, ho * wo, C]"""
    t = t[:, :, ::stride, ::stride]
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1])


def level_slices_ok(y, kind):
    """one-level inputs: slice j of the output (p2, p3, p4, p5) is non-zero exactly for j <= the level that was fed (the top-down path adds
    a level into the finer ones only); y [tokens, 1024]"""
    k = FPN_INPUTS.index(kind) - 1
    nz = [bool((y[:, j * FC:(j + 1) * FC] != 0).any().item()) for j in range(4)]
    return nz == [j <= k for j in range(4)], nz


def fpn_launch(tm, B, sizes, stride, dt):
    """omp_fpn_fuse on laterals tm (four [B * h * w, 256] device tensors) placed between NaN guard rows, into an output between sentinel
    guard rows -> (output view [B * ho * wo, 1024], problems)"""
    from advancedliteratemachinery_amd import _lib, ops
    nanb, sentb = E.nan_bits(dt), E.sent_bits(dt)
    ins = []
    for t in tm:
        buf = guarded(LEAD + t.shape[0], FC, dt, nanb)
        buf[LEAD:LEAD + t.shape[0]] = t
        ins.append(buf)
    (h2, w2), (h3, w3), (h4, w4), (h5, w5) = sizes
    ho, wo = -(-h3 // stride), -(-w3 // stride)
    R = B * ho * wo
    obuf = guarded(LEAD + R, 4 * FC, dt, sentb)
    y = obuf[LEAD:LEAD + R]
    rc = _lib.lib().omp_fpn_fuse(*[ops.ptr(b[LEAD:]) for b in ins], ops.ptr(y), ops.dt(dt), B, h2, w2, h3, w3, h4, w4, h5, w5, stride, ops.stream())
    _lib.check(rc, 'omp_fpn_fuse')
    torch.cuda.synchronize()
    probs = []
    for i, (b, t) in enumerate(zip(ins, tm)):
        if not (lead_kept(b, LEAD, nanb) and E.kept(b, LEAD + t.shape[0], nanb)):
            probs.append('input l%d: guard rows changed' % (i + 2))
    if not lead_kept(obuf, LEAD, sentb):
        probs.append('output: a row before the start was written')
    if not E.kept(obuf, LEAD + R, sentb):
        probs.append('output: a row past the end was written')
    if not bool(torch.isfinite(y).all().item()):
        probs.append('output: a valid token holds NaN / inf (a read outside a map)')
    return y, probs


def check_fpn_geometry(dtype_name=None):
    out = []
    for dn in (('fp32', 'bf16') if dtype_name is None else (dtype_name,)):
        dt = {'fp32': torch.float32, 'bf16': torch.bfloat16}[dn]
        tally = Tally('fpn_geometry[%s]' % dn)
        for start in FPN_STARTS:
            sizes = level_chain(*start)
            for kind in FPN_INPUTS:
                lat = fpn_inputs(sizes, kind, dt)
                r64 = fpn_oracle(lat, torch.float64)
                d32 = (fpn_oracle(lat, torch.float32) - r64).abs().max().item()       # the oracle's own float32 error on this case
                ref = r64 if dt == torch.float32 else ref_fpn(lat, True)
                dev = [token_major(t).to(dt).to(DEV).contiguous() for t in lat]       # [2, h * w, 256]
                for stride in (1, 2):
                    tag = 'fpn_geometry[%s,%dx%d,%s,stride%d]' % (dn, start[0], start[1], kind, stride)
                    y, probs = fpn_launch([t.reshape(-1, FC) for t in dev], 2, sizes, stride, dt)
                    r = token_major(ref, stride).reshape(-1, 4 * FC)
                    if dt == torch.float32:
                        gate, note = 4 * d32, 'oracle fp32 vs fp64 on this case %.3e, gate 4 x that' % d32
                        out.append(rrec(tag + ': max |kernel - fp64|', (y.double().cpu() - r).abs().max().item(), gate, note))
                    else:
                        gate, note = torch.clamp_min(ulp_of(r, dt), 4 * d32), 'gate: one bf16 ulp of the reference, floor 4 x %.3e' % d32
                    tally.gate(out, tag, y, r, gate, note)
                    guard_rec(out, tag, probs)
                    if kind != 'random':
                        ok, nz = level_slices_ok(y, kind)
                        out.append(rec(tag + ': non-zero output slices (p2, p3, p4, p5) = %s' % nz, 0 if ok else 1, 0))
                    else:
                        # the one-image launches; the two-image launch above and every slot of a five-image launch must repeat them
                        base = torch.stack([fpn_launch([t[i] for t in dev], 1, sizes, stride, dt)[0] for i in range(2)])
                        out.append(rec(tag + ': B = 2 launch == the two B = 1 launches, bit for bit', 0 if torch.equal(y.reshape(base.shape), base) else 1, 0))

                        def run(ins, stride=stride):
                            yy, pp = fpn_launch([ins['l%d' % (i + 2)] for i in range(4)], 5, sizes, stride, dt)
                            return {'y': yy}, pp
                        replicate(out, tag + ' B = 5', run, {'l%d' % (i + 2): t for i, t in enumerate(dev)}, {'y': base}, image_src(5, 2))
        tally.summary(out)
    return out


def check_fpn_geometry_fp32():
    return check_fpn_geometry('fp32')


def check_fpn_geometry_bf16():
    return check_fpn_geometry('bf16')


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. split-bf16 producer with row pitches
# ---------------------------------------------------------------------------------------------------------------------------------------
SPLIT_ROWS = (1, 63, 64, 65, 333)
SPLIT_C = (4, 96, 512)


def split_inputs(C, rows=333, seed=77):
    """fp32-valued float64 [rows, C]: row 0 cycles through the planted kinds column by column (a one-row launch sees them all), rows 1 .. 4
    hold one kind each -- values that round UP in hi (lo negative), both signs of zero, magnitudes 2^-100 .. 2^100 of both signs -- then the
    LayerNorm edge rows of tests/gpu_checks_encoder.py and ordinary rows.  No subnormal and no non-finite value, in x, hi or lo."""
    n = rows * C
    i = torch.arange(n, dtype=torch.float64)
    mant = 1.0 + torch.rand(n, generator=_g(seed), dtype=torch.float64)
    sign = torch.where(torch.rand(n, generator=_g(seed + 1), dtype=torch.float64) < 0.5, -1.0, 1.0)
    up = sign * (1.0 + (torch.randint(0, 128, (n,), generator=_g(seed + 2)).double() + 0.75) / 128.0) * 2.0 ** torch.randint(-3, 4, (n,), generator=_g(seed + 3)).double()
    zero = torch.where(i % 2 == 0, 0.0, -0.0)
    col = i % C                                                  # a magnitude row: 2^100 in column 0, 2^-100 in column 1, then inwards
    mag = sign * mant * 2.0 ** (torch.where(col % 2 == 0, 1.0, -1.0) * (100 - (torch.div(col, 2, rounding_mode='floor') * 7) % 101))
    kinds = [up.float().double().reshape(rows, C), zero.reshape(rows, C), mag.float().double().reshape(rows, C)]
    x = torch.cat([edge_rows(C, seed + 4), _valued(_randn(rows, C, seed=seed + 5) * 3, torch.float32)])[:rows].clone()
    x[5:] = x[:rows - 5].clone()
    col = torch.arange(C) % 3
    x[0] = torch.stack([k[0] for k in kinds])[col, torch.arange(C)]
    for r, k in enumerate(kinds):
        x[1 + r] = k[1 + r]
    x[4] = torch.where(torch.arange(C) % 2 == 0, kinds[0][4], kinds[2][4])
    return x


def split_ref(x):
    """fp32 [rows, C] -> (hi, lo) bf16: hi = bf16(x), lo = bf16(x - hi), the CPU's arithmetic"""
    x = x.float()
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def split_expected(x, triple):
    """the planes omp_split_bf16 writes: [hi | lo] or [hi | hi | lo], bf16 [rows, 2 C or 3 C]"""
    hi, lo = split_ref(x)
    return torch.cat([hi, hi, lo] if triple else [hi, lo], 1)


def check_split_bf16_pitch():
    from advancedliteratemachinery_amd import ops
    out = []
    tally = Tally('split_bf16_pitch')
    f32, bf = torch.float32, torch.bfloat16
    for C in SPLIT_C:
        X = split_inputs(C).float()
        for rows in SPLIT_ROWS:
            x = X[:rows]
            for triple in (False, True):
                n = 3 if triple else 2
                want = split_expected(x, triple).view(torch.int16)
                for case in ('dense', 'pitched input', 'pitched output'):
                    tag = 'split_bf16_pitch[%d x %d, %s, %s]' % (rows, C, 'hi|hi|lo' if triple else 'hi|lo', case)
                    if case == 'dense':
                        res, probs = run_guarded(lambda v: ops.split_bf16(v['x'], triple=triple, out=v['y']), {'x': x.to(DEV)}, {'y': (rows, n * C, bf)})
                        y = res['y']
                    elif case == 'pitched input':      # a column slice of a wider fp32 tensor of NaN: ldx > C
                        ibuf, xv = guarded_view(rows, C, E.VIEW_OFF + C + 12, f32, E.nan_bits(f32), x.to(DEV))
                        res, probs = run_guarded(lambda v: ops.split_bf16(xv, triple=triple, out=v['y']), {}, {'y': (rows, n * C, bf)})
                        y = res['y']
                        if not all(E.kept_view(ibuf, rows, C, E.nan_bits(f32))):
                            probs.append('input: guard rows / columns changed')
                    else:                              # out = a column slice of a wider bf16 tensor of sentinels: ldy > n C
                        obuf, y = guarded_view(rows, n * C, E.VIEW_OFF + n * C + 20, bf, E.sent_bits(bf))
                        _, probs = run_guarded(lambda v: ops.split_bf16(v['x'], triple=triple, out=y), {'x': x.to(DEV)}, {})
                        rows_ok, cols_ok = E.kept_view(obuf, rows, n * C, E.sent_bits(bf))
                        if not rows_ok:
                            probs.append('output: a guard row was written')
                        if not cols_ok:
                            probs.append('output: a sentinel column beside the rows was written')
                    bad = int((y.contiguous().view(torch.int16).cpu() != want).sum().item())
                    tally.exact(want.numel())
                    out.append(rrec(tag + ': plane elements whose bits differ from bf16(x), bf16(x - hi)', bad, 0))
                    guard_rec(out, tag, probs)
    return tally.summary(out)


# ---------------------------------------------------------------------------------------------------------------------------------------
# slab layouts (DESIGN.md "cross-attention memory layout"; tests/fake_ops.py restates the writers)
# ---------------------------------------------------------------------------------------------------------------------------------------
def vt_slot(k):
    """slot of key k (0 .. 31) inside a 32-key block of V^T: the order the first cross-attention product delivers P"""
    return 8 * ((k & 15) >> 2) + 4 * (k >> 4) + (k & 3)


def k_natural(K, split=False):
    """K slab [NL, B, nH, Mpad, 64] (split: [NL, B, nH, Mpad / 32, 2 planes, 32, 64]) -> [planes, NL, B, nH, Mpad, 64]"""
    if not split:
        return K[None]
    K = K.movedim(-3, 0)
    return K.reshape(*K.shape[:4], -1, 64)


def vt_natural(Vt, split=False):
    """V^T slab [NL, B, nH, Mpad / KB, 64, KB] (split: [.., Mpad / 32, 2 planes, 64, 32]) -> [planes, NL, B, nH, Mpad, 64], keys in natural
    order: a 32-key block stores key k in slot vt_slot(k), a 16-key block (the fp32 slabs) in slot k"""
    V = Vt.movedim(-3, 0) if split else Vt[None]
    if V.shape[-1] == 32:
        V = V[..., vt_slot(torch.arange(32, device=V.device))]
    V = V.transpose(-1, -2)                                   # [.., blocks, KB, 64]
    return V.reshape(*V.shape[:4], -1, 64)


def slab_order(y, B, M):
    """token-major product y [B * M, NL * 512] -> [NL, B, 8, M, 64]"""
    return y.reshape(B, M, -1, 8, 64).permute(2, 0, 3, 1, 4)


def product64(a, w, bias):
    """float64 (a W^T + bias, |a| |W|^T + |bias|) of operands given as float64"""
    return a @ w.t() + bias, a.abs() @ w.abs().t() + bias.abs()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. row-owner memory projection
# ---------------------------------------------------------------------------------------------------------------------------------------
KV_DIRECT = tuple((ns, B, M) for ns in (1, 2) for (B, M) in ((1, 64), (5, 64), (2, 128)))
KV_ENGINE = ((1, 64), (3, 192))
KV_MPAD = (96, 128)                  # M = 64 inside larger slabs


def kv_inputs(B, M, n_slabs, seed=0):
    """bf16-valued float64 (rows [B * M, 512], W [n_slabs * 512, 512], bias fp32-valued [n_slabs * 512]); row 0 is zero (the bias alone),
    row 1 large, the last row small"""
    s = 100 * seed + 7 * B + M + n_slabs
    rows = _randn(B * M, 512, seed=s)
    rows[0] = 0.0
    rows[1] *= 64.0
    rows[-1] *= 2.0 ** -10
    w = _randn(n_slabs * 512, 512, seed=s + 1) / 512 ** 0.5
    return _valued(rows, torch.bfloat16), _valued(w, torch.bfloat16), _valued(_randn(n_slabs * 512, seed=s + 2) * 0.1, torch.float32)


_MODEL = {}


def neck_state_dict():
    from advancedliteratemachinery_amd.utils import synthetic as weights
    from advancedliteratemachinery_amd.utils.parser import make_args
    if 'sd' not in _MODEL:
        _MODEL['args'] = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
        _MODEL['sd'] = weights.make_state_dict(_MODEL['args'], seed=3, depths=(2, 2, 2, 2))
    return _MODEL['args'], _MODEL['sd']


def memory_weights(args, sd):
    """fp32 masters of the stacked memory projections, slabs ordered (decoder kind, layer) as Decoder stacks them: (Wk, bk, Wv, bv)"""
    from advancedliteratemachinery_amd.model.transformer import KINDS
    d = args.tfm_hidden_dim
    wk, bk, wv, bv = [], [], [], []
    for kind in KINDS:
        for l in range(args.tfm_dec_layers):
            p = 'transformer.%s_decoder.layers.%d.multihead_attn.' % (kind, l)
            w, b = sd[p + 'in_proj_weight'].detach().float(), sd[p + 'in_proj_bias'].detach().float()
            wk.append(w[d:2 * d]); bk.append(b[d:2 * d]); wv.append(w[2 * d:]); bv.append(b[2 * d:])
    return torch.cat(wk), torch.cat(bk), torch.cat(wv), torch.cat(bv)


def decoder_of(engine):
    """the Decoder of the synthetic depths = (2, 2, 2, 2) model of gpu_checks.check_kv_rows in engine precision `engine` (one model, re-packed)"""
    from tests.gpu_checks import build_model
    args, sd = neck_state_dict()
    if 'model' not in _MODEL:
        _MODEL['model'] = build_model(args, sd, (2, 2, 2, 2), torch.bfloat16)
    _MODEL['model'].set_engine_dtype(ENGINES[engine])
    return _MODEL['model'].engine()[1]


def memory_inputs(B, M, dt, call):
    """dt-valued float64 (memory, memory + pos) [B * M, 512] of project_memory call number `call`"""
    s = 1000 * call + 10 * M + B
    return _valued(_randn(B * M, 512, seed=s), dt), _valued(_randn(B * M, 512, seed=s + 5), dt)


def _sent_slab(shape, lead_rows=LEAD):
    """a bf16 slab of `shape` full of sentinels between sentinel guard rows -> (buffer [rows, 64], slab view)"""
    n = 1
    for s in shape:
        n *= s
    buf = guarded(lead_rows + n // 64, 64, torch.bfloat16, E.BF16_SENT)
    return buf, buf[lead_rows:lead_rows + n // 64].view(*shape)


def _slab_guards(buf, n_rows, probs, what):
    if not lead_kept(buf, LEAD, E.BF16_SENT):
        probs.append('%s: a row before the slab was written' % what)
    if not E.kept(buf, LEAD + n_rows, E.BF16_SENT):
        probs.append('%s: a row past the slab was written' % what)


def _sent_count(t):
    return int((_bits(t) != E.BF16_SENT).sum().item())


def gate_slabs(tally, out, tag, K, Vt, M, kref, kabs, vref, vabs, dt, split=False):
    """every element of the valid keys of the K / V^T slabs against the float64 products ([B * M, NL * 512]); -> natural-order slabs"""
    B = K.shape[1]
    kn, vn = k_natural(K.cpu(), split).double(), vt_natural(Vt.cpu(), split).double()
    for name, nat, ref, ab in (('K', kn, kref, kabs), ('V^T', vn, vref, vabs)):
        got, r = nat.sum(0)[:, :, :, :M], slab_order(ref, B, M)
        if split:
            tally.gate(out, '%s %s (hi + lo)' % (tag, name), got, r, SPLIT_TOL, 'gate %.0e absolute' % SPLIT_TOL)
        else:
            tally.gate(out, '%s %s' % (tag, name), got, r, product_gate(r, slab_order(ab, B, M), dt), 'gate 1.5 ulp + 513 u sum |a||w|')
    return kn, vn


def check_kv_rows_edges():
    from advancedliteratemachinery_amd import ops
    from advancedliteratemachinery_amd.model import packing
    out = []
    tally = Tally('kv_rows_edges')
    bf = torch.bfloat16

    def streams(w):
        wd = w.to(bf).to(DEV)
        return packing.pack_kv_rows_k(wd), packing.pack_kv_rows_v(wd)

    def project(rows, st, bias, K, Vt, B, M, Mpad, ns):
        (sk, nk), (sv, nv) = st
        ops.kv_project_rows(rows, sk, nk, bias, K, B, M, Mpad, ns, False)
        ops.kv_project_rows(rows, sv, nv, bias, Vt, B, M, Mpad, ns, True)
        torch.cuda.synchronize()

    # direct calls: one and two slabs (one slab: only the drained tail pass stores), one workgroup per image, five images, two per image
    for (ns, B, M) in KV_DIRECT:
        tag = 'kv_rows_edges[direct, slabs=%d, B=%d, M=%d]' % (ns, B, M)
        rows, w, bias = kv_inputs(B, M, ns)
        ref, ab = product64(rows, w, bias)
        st = streams(w)
        for Mpad in ((M,) + (KV_MPAD if (ns, B, M) == (2, 5, 64) else ())):
            t = tag + (', Mpad=%d' % Mpad if Mpad != M else '')
            kb, K = _sent_slab((ns, B, 8, Mpad, 64))
            vb, Vt = _sent_slab((ns, B, 8, Mpad // 32, 64, 32))
            project(rows.to(bf).to(DEV), st, bias.float().to(DEV), K, Vt, B, M, Mpad, ns)
            probs = []
            _slab_guards(kb, K.numel() // 64, probs, 'K')
            _slab_guards(vb, Vt.numel() // 64, probs, 'V^T')
            if Mpad > M:
                # keys >= M of every (slab, image, head) keep the sentinel
                out.append(rec(t + ': K keys >= M still hold the sentinel (changed elements)', _sent_count(K[:, :, :, M:]), 0))
                out.append(rec(t + ': V^T slots >= M still hold the sentinel (changed elements)', _sent_count(Vt[:, :, :, M // 32:]), 0))
            gate_slabs(tally, out, t, K, Vt, M, ref, ab, ref, ab, bf)
            guard_rec(out, t, probs)
    # argument rejection in the host check: every call raises and leaves the sentinel-filled output alone
    rows, w, bias = kv_inputs(1, 96, 1)
    (sk, nk), _ = streams(w)
    rows96, biasd = rows.to(bf).to(DEV), bias.float().to(DEV)
    for what, call in (('M = 96', lambda o: ops.kv_project_rows(rows96, sk, nk, biasd, o, 1, 96, 96, 1, False)),
                       ('wave_stride below slabs x 64 KB', lambda o: ops.kv_project_rows(rows96[:64], sk, nk - 1024, biasd, o, 1, 64, 96, 1, False)),
                       ('output pointer offset by 8 bytes', lambda o: ops.kv_project_rows(rows96[:64], sk, nk, biasd, o.reshape(-1)[4:4 + 8 * 64 * 64], 1, 64, 64, 1, False))):
        kb, K = _sent_slab((1, 1, 8, 96, 64))
        raised = False
        try:
            call(K)
        except (RuntimeError, ValueError):
            raised = True
        torch.cuda.synchronize()
        out.append(rec('kv_rows_edges[rejected: %s]: raises, output untouched (changed elements)' % what, (0 if raised else 1) + _sent_count(kb), 0))
    # the engine's path: 12 slabs of the synthetic decoder, one workgroup = one image and 3 x 192
    args, sd = neck_state_dict()
    dec = decoder_of('bf16')
    Wk, bk, Wv, bv = memory_weights(args, sd)
    same = torch.equal(dec.Wk_all.cpu(), Wk.to(bf)) and torch.equal(dec.Wv_all.cpu(), Wv.to(bf)) and torch.equal(dec.bk_all.cpu(), bk)
    out.append(rec('kv_rows_edges[engine]: the decoder stacks the weights the reference multiplies', 0 if same else 1, 0))
    for (B, M) in KV_ENGINE:
        tag = 'kv_rows_edges[engine, B=%d, M=%d]' % (B, M)
        mem, mp = memory_inputs(B, M, bf, 0)
        res = {}
        for on in (True, False):
            dec.kv_rows = on
            kv = dec.project_memory(mem.to(bf).to(DEV), mp.to(bf).to(DEV), B, M, None)
            torch.cuda.synchronize()
            res[on] = (kv['K'].clone(), kv['Vt'].clone())
            kv['K'].zero_()
            kv['Vt'].zero_()
        dec.kv_rows = True
        out.append(rec(tag + ': K slabs identical to the tiled GEMM path', 0 if torch.equal(res[True][0], res[False][0]) else 1, 0))
        out.append(rec(tag + ': V^T slabs identical to the tiled GEMM path', 0 if torch.equal(res[True][1], res[False][1]) else 1, 0))
        kref, kabs = product64(mp, _valued(Wk, bf), bk.double())
        vref, vabs = product64(mem, _valued(Wv, bf), bv.double())
        gate_slabs(tally, out, tag, res[True][0], res[True][1], M, kref, kabs, vref, vabs, bf)
    return tally.summary(out)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the cached memory slabs of Decoder.project_memory: rewritten on every call, the padded tail stays zero
# ---------------------------------------------------------------------------------------------------------------------------------------
TAIL_M = (1, 15, 16, 17, 31, 32, 33, 77)
TAIL_B = (1, 3)


def tail_key_len(B, M):
    return [max(1, M - 1 - 2 * b) for b in range(B)]


def check_memory_slab_tail(engine=None):
    out = []
    for eng in (tuple(ENGINES) if engine is None else (engine,)):
        tally = Tally('memory_slab_tail[%s]' % eng)
        args, sd = neck_state_dict()
        dec = decoder_of(eng)
        split = bool(dec.kv_split)
        dt = dec.dtype
        Wk, bk, Wv, bv = memory_weights(args, sd)
        Wk64, Wv64 = (Wk.double(), Wv.double()) if dec.x3 else (_valued(Wk, dt), _valued(Wv, dt))
        for B in TAIL_B:
            for M in TAIL_M:
                call = 0
                for key_len in (None, tail_key_len(B, M)):
                    for _ in range(2):           # the same cached (B, M) entry, other memories every time
                        mem, mp = memory_inputs(B, M, dt, call)
                        call += 1
                        kv = dec.project_memory(mem.to(dt).to(DEV), mp.to(dt).to(DEV), B, M, None, key_len=key_len)
                    torch.cuda.synchronize()
                    tag = 'memory_slab_tail[%s, B=%d, M=%d%s]' % (eng, B, M, '' if key_len is None else ', key_len=%s' % key_len)
                    kref, kabs = product64(mp, Wk64, bk.double())
                    vref, vabs = product64(mem, Wv64, bv.double())
                    kn, vn = gate_slabs(tally, out, tag, kv['K'], kv['Vt'], M, kref, kabs, vref, vabs, dt, split)
                    # the padded keys, bit for bit, in every plane
                    pad = int((_bits(k_natural(kv['K'], split)[..., M:, :].contiguous()) != 0).sum().item())
                    pad += int((_bits(vt_natural(kv['Vt'], split)[..., M:, :].contiguous()) != 0).sum().item())
                    out.append(rec(tag + ': padded keys of K and padded slots of V^T exactly zero (non-zero elements, Mpad = %d)' % kv['Mpad'], pad, 0))
                    if key_len is not None:
                        ok = kv['key_len'].cpu().tolist() == key_len and bool(torch.isfinite(kn).all().item()) and bool(torch.isfinite(vn).all().item())
                        out.append(rec(tag + ': key counts bound, rows key_len .. M - 1 projected and finite', 0 if ok else 1, 0))
        tally.summary(out)
    return out


def check_memory_slab_tail_fp32():
    return check_memory_slab_tail('fp32')


def check_memory_slab_tail_bf16():
    return check_memory_slab_tail('bf16')


def check_memory_slab_tail_bf16x3():
    return check_memory_slab_tail('bf16x3')


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. device pre-processing
# ---------------------------------------------------------------------------------------------------------------------------------------
PRE_MIN, PRE_MAX = 48, 100
# (H, W, what): under the size rule with min 48 / max 100
PRE_IMAGES = ((40, 60, 'pitched source'),                      # -> 48 x 72, a column slice of a wider image
              (48, 60, 'already at its target size'),          # h == min size: neither axis resamples
              (90, 30, 'max_size branch, portrait'),           # 48 * 3 > 100 -> 99 x 33: Hmax = 99 is no multiple of 4
              (40, 200, 'max_size branch, landscape'),         # -> 20 x 100: Wmax = 100 is no multiple of 64
              (31, 64, 'ordinary'))
# The aspect-preserving size rule never changes one axis alone (if one side already has its target the rule returns the input size), so the
# one-axis batches run the preprocessor and the reference under a size rule of their own: the kernel's need_h / need_v skips are real paths
# (utils/preprocess.py CropResizer takes them) whatever rule picks the sizes.
PRE_ONE_AXIS = ((37, 53, 37, 90), (35, 53, 61, 53), (50, 41, 50, 23), (50, 43, 19, 43), (33, 47, 33, 47))   # (H, W, oh, ow), distinct (H, W)


def pre_image(H, W, seed):
    import numpy as np
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def _pre_compare(out, tag, pre, imgs, dev_imgs, ref_fn):
    import numpy as np
    ref_t, ref_m, ref_sizes = ref_fn(imgs)
    nt, sizes = pre(dev_imgs)
    torch.cuda.synchronize()
    got_t, got_m = nt.tensors.cpu().numpy(), nt.mask.cpu().numpy()
    Hm, Wm = ref_t.shape[2:]
    out.append(rrec('%s: sizes %s (batch %d x %d)' % (tag, sizes, Hm, Wm), 0 if sizes == ref_sizes and got_t.shape == ref_t.shape else 1, 0))
    if got_t.shape != ref_t.shape:
        return
    out.append(rrec(tag + ': tensor elements whose bits differ from the reference', int((got_t.view(np.int32) != ref_t.view(np.int32)).sum()), 0,
                    '%d elements' % ref_t.size))
    out.append(rrec(tag + ': mask elements that differ', int((got_m != ref_m).sum()), 0))
    pad_bad = 0
    for b, (oh, ow) in enumerate(ref_sizes):           # the guard of a class-allocated output: exact zero padding under mask == 1
        inside = np.zeros((Hm, Wm), dtype=bool)
        inside[:oh, :ow] = True
        pad_bad += int((got_t[b][:, ~inside].view(np.int32) != 0).sum()) + int((got_m[b] != ~inside).sum())
    out.append(rec(tag + ': padding exactly zero under mask == 1, mask == 0 inside (wrong elements)', pad_bad, 0))


def check_preprocess_edges():
    from advancedliteratemachinery_amd.utils import preprocess as PP
    from oracle import preprocess_ref as P
    out = []
    imgs = [pre_image(H, W, 10 + i) for i, (H, W, _) in enumerate(PRE_IMAGES)]
    dev = [torch.from_numpy(i).to(DEV) for i in imgs]
    wide = torch.full((imgs[0].shape[0], imgs[0].shape[1] + 23, 3), 255, dtype=torch.uint8, device=DEV)
    wide[:, 7:7 + imgs[0].shape[1]] = dev[0]
    dev[0] = wide[:, 7:7 + imgs[0].shape[1]]                              # stride(0) = 3 * (W + 23) > 3 * W
    pre = PP.DevicePreprocessor(PRE_MIN, PRE_MAX, DEV)
    tag = 'preprocess_edges[size rule %d / %d]' % (PRE_MIN, PRE_MAX)
    out.append(rec(tag + ': the source is pitched and passed as it is', 0 if dev[0].stride(0) > 3 * dev[0].shape[1] and not dev[0].is_contiguous() else 1, 0))
    _pre_compare(out, tag, pre, imgs, dev, lambda im: P.preprocess_batch(im, PRE_MIN, PRE_MAX))
    # one axis alone: width only (up, down), height only (up, down), neither
    want = {(H, W): (oh, ow) for (H, W, oh, ow) in PRE_ONE_AXIS}

    class FixedSizes(PP.DevicePreprocessor):
        def output_size(self, h, w):
            return want[(h, w)]

    def ref_fixed(im):
        rule = P.get_size_with_aspect_ratio
        P.get_size_with_aspect_ratio = lambda size, mn, mx=None: want[(size[1], size[0])]
        try:
            return P.preprocess_batch(im, PRE_MIN, PRE_MAX)
        finally:
            P.get_size_with_aspect_ratio = rule
    for group, sel in (('width only', PRE_ONE_AXIS[0:1] + PRE_ONE_AXIS[2:3] + PRE_ONE_AXIS[4:]), ('height only', PRE_ONE_AXIS[1:2] + PRE_ONE_AXIS[3:4])):
        imgs = [pre_image(H, W, 30 + i) for i, (H, W, _, _) in enumerate(sel)]
        _pre_compare(out, 'preprocess_edges[%s changes]' % group, FixedSizes(PRE_MIN, PRE_MAX, DEV), imgs, [torch.from_numpy(i).to(DEV) for i in imgs], ref_fixed)
    return out


ALL_NECK_CHECKS = ('check_fpn_geometry_fp32', 'check_fpn_geometry_bf16', 'check_split_bf16_pitch', 'check_kv_rows_edges', 'check_memory_slab_tail_fp32',
                   'check_memory_slab_tail_bf16', 'check_memory_slab_tail_bf16x3', 'check_preprocess_edges')
