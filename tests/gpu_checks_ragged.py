"""GPU checks of ragged batches (OmniParser.infer(ragged=True)): per-image key counts in the cross-attention kernels
(omp_dec_cross_attn_step key_len) against fp64 softmax attention, and whole engine calls of mixed-size images against the same images
submitted alone and against the reference run on each image alone (tests/golden/spot_alone.pt, tools/gen_golden_alone.py).
Every check returns records {name, err, tol, ok, note} like tests/gpu_checks.py."""
import torch

from advancedliteratemachinery_amd import _lib, ops
from advancedliteratemachinery_amd.model.omniparser import bucket_by_size
from advancedliteratemachinery_amd.model.transformer import Decoder
from advancedliteratemachinery_amd.utils.nested_tensor import NestedTensor
from advancedliteratemachinery_amd.utils.parser import make_args
from advancedliteratemachinery_amd.utils import synthetic as weights
from oracle import gen_golden as G
from oracle import omniparser_ref as O
from tests.gpu_checks import (BF16_LOGIT_REL, DEV, ENGINES, MARGIN_K, REPORT, all_chains, build_model, golden, rec, rnd, _chain_phases)

# ---------------------------------------------------------------------------------------------------------------------------------
# op level: omp_dec_cross_attn_step with key_len
# ---------------------------------------------------------------------------------------------------------------------------------
def _slot_of_key():
    """bf16 / split V^T blocks store key kl of a 32-key block in slot _slot_of_key()[kl] (the B-operand order of the PV product)"""
    kl = torch.arange(32)
    return ((kl & 15) >> 2) * 8 + (kl >> 4) * 4 + (kl & 3)


def _vblocks(V, KB, permute):
    """[B][nH][Mpad][64] -> V^T blocks [B][nH][Mpad/KB][64][KB]"""
    B, nH, Mpad, _ = V.shape
    nat = V.reshape(B, nH, Mpad // KB, KB, 64).transpose(-1, -2)
    if not permute:
        return nat.contiguous()
    out = torch.empty(nat.shape, dtype=nat.dtype)   # contiguous: the kernel reads the dense block layout
    out[..., _slot_of_key()] = nat
    return out


def _slabs(kind, Kn, Vn):
    """natural fp32 K / V [B][nH][Mpad][64] -> (K slab, V^T slab, K values, V values): the slabs in the kernel's layout and the values
    they hold (fp64, what the reference attends over)"""
    if kind == 'fp32':
        return Kn.clone(), _vblocks(Vn, 16, False), Kn.double(), Vn.double()
    if kind == 'bf16':
        Kq, Vq = Kn.to(torch.bfloat16), Vn.to(torch.bfloat16)
        return Kq, _vblocks(Vq, 32, True), Kq.double(), Vq.double()
    # split planes: every 32-key block = [hi plane | lo plane]
    def planes(x):
        hi = x.to(torch.bfloat16)
        return hi, (x - hi.float()).to(torch.bfloat16)
    B, nH, Mpad, _ = Kn.shape
    kh, kl = planes(Kn)
    K = torch.stack([kh.reshape(B, nH, Mpad // 32, 32, 64), kl.reshape(B, nH, Mpad // 32, 32, 64)], 3)
    vh, vl = planes(Vn)
    V = torch.stack([_vblocks(vh, 32, True), _vblocks(vl, 32, True)], 3)
    return K, V, Kn.double(), Vn.double()


def _reference(qv, Kv, Vv, counts, lens, kmask):
    """fp64 softmax attention of every image's rows over ITS first lens[b] keys (minus masked ones)"""
    nH = Kv.shape[1]
    R, d = qv.shape
    ref = torch.zeros(R, d, dtype=torch.float64)
    r0 = 0
    for b, n in enumerate(counts):
        if n:
            L = lens[b]
            qh = qv[r0:r0 + n].reshape(n, nH, 64).permute(1, 0, 2) / 8.0
            att = qh @ Kv[b, :, :L].transpose(-2, -1)
            if kmask is not None:
                att = att.masked_fill(kmask[b, :L][None, None, :], float('-inf'))
            ref[r0:r0 + n] = (att.softmax(-1) @ Vv[b, :, :L]).permute(1, 0, 2).reshape(n, d)
        r0 += n
    return ref


# (B, M, key_len): lengths 1, < KB, not a multiple of KB, exactly Mpad (M = 320 is a multiple of both key blocks), and lengths short
# enough that most splits and waves of an image are empty at n_split 8 / 16
OP_CASES = ((6, 320, [1, 13, 100, 320, 45, 257]), (3, 2000, [2000, 1500, 77]))
ROWS = {1: [3, 1, 16, 5, 2, 9], 2: [20, 7, 32, 1, 30, 17], 4: [64, 33, 40, 1, 50, 64]}
RINGS = {'bf16': (1, 2, 4, 5, 6, 0), 'fp32': (1, 2, 4, 5, 6, 0), 'split': (1, 4, 5, 6, 0)}
TOL = {'bf16': 2e-2, 'fp32': 2e-5, 'split': 5e-5}


def check_cross_attn_key_len():
    out = []
    nH, d = 8, 512
    nt_knob = _lib.lib().omp_debug_cross_nt
    try:
        for kind in ('bf16', 'fp32', 'split'):
            KB = 16 if kind == 'fp32' else 32
            for B, M, lens in OP_CASES:
                Mpad = (M + KB - 1) // KB * KB
                Kn = rnd(B, nH, Mpad, 64, seed=M + 1)
                Vn = rnd(B, nH, Mpad, 64, seed=M + 2)
                Kn[:, :, M:] = 0
                Vn[:, :, M:] = 0
                K, Vt, Kv, Vv = _slabs(kind, Kn, Vn)
                # NaN wherever a key lies at or beyond key_len in K, and in every V^T block at or beyond ceil(key_len / KB) (the tail of
                # the last loaded block stays finite: a dead key's V^T enters P.V with P = 0, include/omp355.h)
                Knan, Vnan = Kn.clone(), Vn.clone()
                for b, L in enumerate(lens):
                    Knan[b, :, L:] = float('nan')
                    Vnan[b, :, (L + KB - 1) // KB * KB:] = float('nan')
                Kbad, Vbad, _, _ = _slabs(kind, Knan, Vnan)
                slabs = {'zero': (K.to(DEV), Vt.to(DEV)), 'nan': (Kbad.to(DEV), Vbad.to(DEV))}
                stride = nH * Mpad * (128 if kind == 'split' else 64)
                kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
                full = torch.full((B,), M, dtype=torch.int32, device=DEV)
                for qt, rows in ROWS.items():
                    counts = rows[:B]
                    R = sum(counts)
                    groups, qt_ = Decoder.make_tiles(counts)
                    assert qt_ == qt
                    gd = torch.tensor(groups, dtype=torch.int32, device=DEV)
                    qq = rnd(R, d, seed=qt)
                    qdt = torch.bfloat16 if kind == 'bf16' else torch.float32
                    qv = qq.to(qdt).double()
                    qd = qq.to(DEV, qdt)
                    for masked in ((False, True) if B == 6 else (False,)):
                        kmask = None
                        if masked:
                            kmask = rnd(B, M, seed=9) > 0.8
                            kmask[:, 0] = False
                        km = kmask.to(torch.uint8).to(DEV) if masked else None
                        ref = _reference(qv, Kv, Vv, counts, lens, kmask)
                        for S in (1, 2, 4, 8, 16):
                            for ring in (RINGS[kind] if qt == 4 else (1,)):
                                for nt in (1, 0):
                                    ops.cross_q4(ring)
                                    nt_knob(nt)

                                    def run(which, key_len):
                                        o = torch.full((R, d), float('nan'), device=DEV, dtype=qdt)
                                        partial = torch.full((R, nH, S, 68), float('nan'), device=DEV)
                                        ops.dec_cross_attn_step(qd, slabs[which][0], slabs[which][1], stride, Mpad, km, gd, len(groups), qt, partial,
                                                                o, M, nH, S, key_len=key_len)
                                        return o.cpu()
                                    tag = 'cross_attn_key_len[%s,B%d,M%d,qt%d,S%d,ring%d,nt%d,mask=%s]' % (kind, B, M, qt, S, ring, nt, masked)
                                    o = run('zero', kl)
                                    out.append(rec(tag, (o.double() - ref).abs().max().item(), TOL[kind]))
                                    if ring == 1:
                                        o_nan = run('nan', kl)
                                        bad = (~torch.isfinite(o_nan)).sum().item()
                                        out.append(rec(tag + ' NaN beyond key_len: finite and == zero-filled', bad + (0 if torch.equal(o_nan, o) else 1), 0,
                                                       '%d non-finite' % bad))
                                        same = torch.equal(run('zero', full), run('zero', None))
                                        out.append(rec(tag + ' key_len = [M] * B bit-identical to key_len = NULL', 0 if same else 1, 0))
    finally:
        ops.cross_q4(1)
        nt_knob(1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end: a ragged call == one call per image
# ---------------------------------------------------------------------------------------------------------------------------------
# two mixes of the SAME batch size and Mmax (stride-16 memories of 48, 140 and 80 keys -> Mmax 192) with different lengths at every
# position: the second call binds the same plans and slabs, so a replayed graph that kept the first call's key_len would show
MIX_A = [(96, 128), (160, 224), (64, 320), (96, 128)]
MIX_B = [(64, 320), (96, 128), (96, 128), (160, 224)]


def _image(hw, seed):
    h, w = hw
    return rnd(3, h, w, seed=1000 * seed + h + w).to(DEV)


def _compare(tag, got, alone, f32, out, stats):
    """one image's result of a ragged call against the same image alone: fp32-grade engines identical ids, probabilities within
    1e-5; bf16 token agreement is accumulated into stats (the near-tie rule of gpu_checks.check_batch_equivalence)"""
    if got is None or alone is None:
        ok = (got is None) == (alone is None)
        stats[0] += int(ok)
        stats[1] += 1
        if f32:
            out.append(rec(tag + ' empty result as alone', 0 if ok else 1, 0))
        return
    n_same = n_all = 0
    for x, y in zip(got[0], alone[0]):
        n = min(x.numel(), y.numel())
        n_all += max(x.numel(), y.numel())
        n_same += int((x.reshape(-1)[:n].cpu() == y.reshape(-1)[:n].cpu()).sum())
    stats[0] += n_same
    stats[1] += n_all
    if f32:
        out.append(rec(tag + ' ids identical to alone', n_all - n_same, 0))
        pa, pb = got[1][0].cpu(), alone[1][0].cpu()
        perr = (pa - pb).abs().max().item() if pa.shape == pb.shape else float('inf')
        out.append(rec(tag + ' probs vs alone', perr, 1e-5))


def check_ragged_equals_alone(dtype_name='fp32', graph=False):
    f32 = dtype_name in ('fp32', 'bf16x3')
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, pt_seq_length=10)
    depths = (2, 2, 2, 2)
    sd = weights.make_state_dict(args, seed=4, depths=depths)
    model = build_model(args, sd, depths, ENGINES[dtype_name], graph)
    seqs = O.default_prompts(args)
    st = torch.cuda.Stream() if graph else None
    out, stats, alone = [], [0, 0], {}

    def call(*a, **k):
        if st is None:
            return model.infer(*a, **k)
        with torch.cuda.stream(st):
            r = model.infer(*a, **k)
        st.synchronize()
        return r

    for mi, mix in enumerate((MIX_A, MIX_B, MIX_A)):
        imgs = [_image(hw, b) for b, hw in enumerate(mix)]
        res = call(imgs, None, seqs, ragged=True)
        _, dec = model.engine()
        kv = next(reversed(dec._kv.values()))
        want = [(hw[0] + 15) // 16 * ((hw[1] + 15) // 16) for hw in mix]
        out.append(rec('ragged[%s,graph=%s,call%d] key_len buffer holds this call\'s lengths' % (dtype_name, graph, mi),
                       0 if kv[3].tolist() == want else 1, 0, '%s vs %s' % (kv[3].tolist(), want)))
        for b, (hw, im) in enumerate(zip(mix, imgs)):
            key = (hw, b)
            if key not in alone:
                alone[key] = call(im[None], torch.zeros(1, hw[0], hw[1], dtype=torch.bool, device=DEV), seqs)[0]
            _compare('ragged[%s,graph=%s,call%d,img%d %dx%d]' % (dtype_name, graph, mi, b, hw[0], hw[1]), res[b], alone[key], f32, out, stats)
    frac = stats[0] / max(1, stats[1])
    REPORT.append(dict(name='ragged_equals_alone[%s,graph=%s]' % (dtype_name, graph), match=frac, tokens=stats[1]))
    out.append(rec('ragged_equals_alone[%s,graph=%s] token agreement' % (dtype_name, graph), 1.0 - frac, 0.0 if f32 else 0.05,
                   'agreement %.3f of %d' % (frac, stats[1])))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# against the reference: tests/golden/spot_alone.pt
# ---------------------------------------------------------------------------------------------------------------------------------
def spot_alone_inputs(case):
    """-> (args, sd, seqs, [3, h, w] images) of spot_alone's case WITHOUT the reference: spot_padded's images unpadded (same weights,
    args and draws: oracle.gen_golden.case_inputs) plus one image of extra_hw drawn from extra_seed (tools/gen_golden_alone.py)"""
    args, sd, img, mask, seqs = G.case_inputs(G.BIG_CASES[case['padded_case']])
    imgs = [t.clone() for t in NestedTensor(img, mask).unpad_tensors()]
    h, w = case['extra_hw']
    imgs.append(torch.randn(3, h, w, generator=torch.Generator().manual_seed(case['extra_seed'])))
    return args, sd, seqs, imgs


# spot_alone stores every teacher-forced logit row [.., V] as a summary, not in full (V = 1104 classes x 141 positions x 3 images would be
# 1.9 MB): the TOPK largest logits with their classes, every STRIDE-th class, and the row's logsumexp (which every class's logit moves).
# Image 0's full rows are spot_odd's, and are compared in full.
TOPK, STRIDE = 16, 16


def logit_summary(lg):
    """fp32 logits [.., V] -> dict(top_idx int16 / top_val [.., TOPK] (descending), cols [.., ceil(V / STRIDE)], lse [..])"""
    lg = lg.float()
    top = lg.topk(TOPK, dim=-1)
    return dict(top_idx=top.indices.to(torch.int16), top_val=top.values.clone(), cols=lg[..., ::STRIDE].clone(),
                lse=torch.logsumexp(lg.double(), -1).float())


def summary_error(lg, s):
    """-> (max abs error of logits lg [.., V] against a logit_summary, that summary's largest |logit|)"""
    lg = lg.float()
    err = max((lg.gather(-1, s['top_idx'].long()) - s['top_val']).abs().max().item(),
              (lg[..., ::STRIDE] - s['cols']).abs().max().item(),
              (torch.logsumexp(lg.double(), -1).float() - s['lse']).abs().max().item())
    return err, max(s['top_val'].abs().max().item(), s['cols'].abs().max().item())


def check_ragged_golden(dtype_name='fp32', chains=False):
    f32 = dtype_name in ('fp32', 'bf16x3')
    gold = golden('spot_alone')
    case = gold['case']
    args, sd, seqs, imgs = spot_alone_inputs(case)
    out = [rec('ragged_golden weight fingerprint', (G.fingerprint(sd) - gold['fingerprint']).abs().max().item(), 1e-6)]
    model = build_model(args, sd, case['depths'], ENGINES[dtype_name])
    tag = 'ragged_golden[%s%s]' % (dtype_name, ',chains' if chains else '')
    imgs = [i.to(DEV) for i in imgs]
    B = len(imgs)
    ctx = all_chains(model) if chains else None
    if ctx is not None:
        ctx.__enter__()
    try:
        res = model.infer(imgs, None, seqs, ragged=True)
        enc, dec = model.engine()
        memory, mem_pos, Mmax, key_len = model._encode_ragged(enc, imgs, bucket_by_size([tuple(i.shape[1:]) for i in imgs]))
        out.append(rec(tag + ' memory lengths', sum(abs(a - g['M']) for a, g in zip(key_len, gold['images'])), 0, str(key_len)))
        kv = dec.project_memory(memory, mem_pos, B, Mmax, None, key_len=key_len)
        npr = O.prompt_len(args)
        odd_tf = golden('spot_odd')['tf']
        for b, g in enumerate(gold['images']):
            itag = '%s img%d %dx%d' % (tag, b, g['hw'][0], g['hw'][1])
            # teacher-forced logits of this image's rows over the CALL's memory: the other images' rows are in the slabs, not in its keys
            for kind, n_prompt in (('pt', npr), ('poly', 3), ('rec', 3)):
                s_in, ref = g['tf'][kind + '_in'], g['tf'][kind + '_sum']
                counts = [0] * B
                counts[b] = s_in.shape[0]
                lg = dec.teacher_forced_logits(kind, kv, s_in, counts, n_prompt).float().cpu()
                checks = [('', *summary_error(lg, ref))]
                if b == 0:   # spot_odd holds this image's rows in full
                    full = odd_tf[kind + '_logits']
                    if not torch.equal(odd_tf[kind + '_in'], s_in):
                        out.append(rec('%s teacher-forced %s inputs are spot_odd\'s' % (itag, kind), 1, 0))
                        continue
                    checks.append((' (full rows, spot_odd)', (lg - full).abs().max().item(), full.abs().max().item()))
                for what, err, scale in checks:
                    REPORT.append(dict(name='%s teacher-forced %s logits%s' % (itag, kind, what), abs_err=err, rel_err=err / scale, ref_absmax=scale))
                    out.append(rec('%s teacher-forced %s logits%s' % (itag, kind, what), err if f32 else err / scale,
                                   1e-3 if f32 else BF16_LOGIT_REL, 'abs err %.3g' % err))
                err = max(e for _, e, _ in checks)
                top = ref['top_val'][:, n_prompt - 1:]
                clear = (top[..., 0] - top[..., 1]) > MARGIN_K * err
                agree = lg[:, n_prompt - 1:].argmax(-1) == ref['top_idx'][:, n_prompt - 1:, 0].long()
                out.append(rec('%s teacher-forced %s argmax (margin > %gx err)' % (itag, kind, MARGIN_K), float((clear & ~agree).sum()), 0))
            go, r = g['out'], res[b]
            if go is None or r is None:
                out.append(rec(itag + ' empty result as the reference', 0 if (go is None) == (r is None) else 1, 0))
                continue
            same = [t.cpu().shape == go[k].shape and bool((t.cpu() == go[k]).all()) for k, t in zip(('pt', 'poly', 'rec'), r[0])]
            REPORT.append(dict(name=itag + ' tokens identical (pt, poly, rec)', identical=same))
            if f32:
                out.append(rec(itag + ' ids identical to the reference alone', 3 - sum(same), 0))
                out.append(rec(itag + ' rec probs', (r[1][0].cpu() - go['rec_probs']).abs().max().item() if r[1][0].shape == go['rec_probs'].shape
                               else float('inf'), 1e-3))
            if b == 0 and f32:   # spot_odd is the reference on image 0 alone (the generator asserts it)
                odd = golden('spot_odd')['out']
                out.append(rec(itag + ' ids identical to spot_odd', 0 if all(bool((t.cpu() == odd[k]).all()) and t.shape == odd[k].shape
                                                                             for k, t in zip(('pt', 'poly', 'rec'), r[0])) else 1, 0))
        if chains:
            fused, ph = _chain_phases(dec)
            out.append(rec(tag + ' every decoder phase ran the row-owner chains (%d of %d)' % (len(fused), len(ph)),
                           0 if ph and len(fused) == len(ph) else 1, 0))
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# KIE: two sizes in one ragged call (kie_sroie weights)
# ---------------------------------------------------------------------------------------------------------------------------------
def check_ragged_kie(dtype_name='bf16x3'):
    case = G.CASES['kie_sroie']
    args, sd, img, _, seqs = G.case_inputs(case)
    model = build_model(args, sd, case['depths'], ENGINES[dtype_name])
    imgs = [img[0].to(DEV), rnd(3, 128, 96, seed=5).to(DEV), img[0].flip(-1).contiguous().to(DEV)]
    sizes = [torch.tensor(i.shape[1:]) for i in imgs]
    res = model.infer(imgs, None, seqs[:3] + [sizes], ragged=True)
    out = []
    for b, im in enumerate(imgs):
        h, w = im.shape[1:]
        alone = model.infer(im[None], torch.zeros(1, h, w, dtype=torch.bool, device=DEV), seqs[:3] + [torch.tensor([h, w])])[0]
        got = res[b]
        same = (got is None) == (alone is None)
        if same and got is not None:
            same = len(got) == len(alone) and all(a[0] == c[0] and a[1] == c[1] and abs(a[2] - c[2]) <= 1e-5 and
                                                  torch.allclose(torch.tensor(a[3]), torch.tensor(c[3])) for a, c in zip(got, alone))
        out.append(rec('ragged_kie[%s,img%d %dx%d] entities identical to alone' % (dtype_name, b, h, w), 0 if same else 1, 0, str(got)[:120]))
    return out
