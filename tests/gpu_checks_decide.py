"""GPU checks of the kernels that turn numbers into DECISIONS (token ids, finished flags, masks, packed payloads) at their edges.

Random logits almost never produce the inputs where these kernels can go wrong -- exact ties, -inf, a non-candidate above every candidate,
probabilities that underflow, the thresholds between kernels -- so the cases below are planted by hand.  The arbiter for ids is always the
oracle's own filter + topk (oracle/omniparser_ref.py) on the same fp32 logits, and where the expected id is known by construction (the lower
index of a tie, token 0 of an all-zero filtered row) the oracle is held to it too, so the assumption about torch's topk is tested as well.
Probabilities are compared with an fp64 softmax of those logits.  Every check returns rec() records like tests/gpu_checks.py.
"""
import torch
import torch.nn.functional as F

from advancedliteratemachinery_amd import _lib, ops
from advancedliteratemachinery_amd.utils.parser import make_args
from oracle import omniparser_ref as O
from tests.gpu_checks import DEV, rec

KIND = {'pt': _lib.DEC_PT, 'poly': _lib.DEC_POLY, 'rec': _lib.DEC_REC}
IMPL = {0: 'auto', 1: 'wave per row', 2: 'row in registers', 3: 'workgroup per row'}
STEP0 = 3                  # sequence position of the first generated token
SEQ_W = 24                 # row stride of seq / probs: wider than any position written here
SENT_TOK, SENT_PROB, SENT_LEN = -7, -3.25, 1000


def _q(t):
    """logits on a 2^-10 grid: differences of two of them are exact in fp32, so the probability gate measures the kernel's exp and sum"""
    return torch.round(t * 1024) / 1024


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _period(a):
    return 3 if a.infer_vie else 2


def _vs(a, kind, V):
    """the softmax support: the non-pt heads of a KIE model leave out the trailing vie slice"""
    return V - (a.vie_categories if (a.infer_vie and kind != 'pt') else 0)


def _candidates(a, kind, i, V, suppress):
    """bool [Vs]: the tokens the reference's filter keeps at greedy step i (transformer.py:110-123, :177-180, :275-278)"""
    Vs = _vs(a, kind, V)
    m = torch.zeros(Vs, dtype=torch.bool)
    nb, eos = a.num_bins, a.pt_eos_index
    if kind == 'pt':
        r = i % _period(a)
        if r == 2:
            m[V - a.vie_categories:] = True
        else:
            m[:nb] = True
            if r == 0 and not suppress:
                m[eos] = True
    elif kind == 'poly':
        m[:nb] = True
    else:
        m[nb:a.rec_eos_index + 1] = True
        m[a.pt_eos_index] = m[a.poly_eos_index] = False
    return m


def oracle_sample(a, kind, i, logits, suppress=0):
    """(token [R], fp32 probability [R], fp64 probability [R]) of the reference: softmax over the support, filter, top-1.  suppress_eos
    (forced-length runs) additionally zeroes pt_eos at the steps that could emit it."""
    lg = logits[:, :_vs(a, kind, logits.shape[1])]
    pr = lg.softmax(-1)
    if kind == 'pt':
        pr = O.pt_step_filter(a, pr, i)
        if suppress and i % _period(a) == 0:
            pr = pr.clone()
            pr[:, a.pt_eos_index] = 0
    elif kind == 'poly':
        pr = pr[:, :a.num_bins]
    else:
        pr = O.rec_filter(a, pr)
    p, t = pr.topk(dim=-1, k=1)
    p64 = lg.double().softmax(-1).gather(1, t)[:, 0]
    return t[:, 0], p[:, 0], p64


def _sample_cases(a, kind, i, V, suppress, seed):
    """[(name, row [V], token expected by construction or None)]: the planted cases of one (kind, step)."""
    g = _gen(seed)
    Vs = _vs(a, kind, V)
    cm = _candidates(a, kind, i, V, suppress)
    cand = cm.nonzero()[:, 0].tolist()
    cs = set(cand)
    non = [t for t in sorted({a.num_bins // 2, a.num_bins, a.num_bins + 37, a.pt_eos_index, a.poly_eos_index, a.rec_eos_index,
                              a.rec_eos_index + 1, Vs - 1, 0, V - a.vie_categories}) if 0 <= t < Vs and t not in cs]
    rows = []

    def base():
        return _q(torch.randn(V, generator=g) * 3)

    def best_cand(row):
        v = row[:Vs].masked_fill(~cm, float('-inf'))
        return int(v.argmax())

    for k in range(3):
        r = base()
        rows.append(('random %d' % k, r, best_cand(r)))
    # exact ties between two candidates: every lane distance of the shuffle reductions, the same lane in later iterations / 256-float pieces,
    # other waves of the workgroup kernel, the lowest and the highest candidate, index 0 and Vs - 1 where they are candidates
    pairs = []
    if len(cand) > 1:
        pairs.append((cand[0], cand[-1]))
        mid = cand[len(cand) // 2]
        if 0 in cs and mid != 0:
            pairs.append((0, mid))
        if Vs - 1 in cs and mid != Vs - 1:
            pairs.append((mid, Vs - 1))
    for d in (1, 2, 3, 4, 8, 16, 32, 64, 128, 192, 256, 512, 768, 1024):
        for t in cand:
            if t + d in cs and (t % 64 != 0 or d >= 64):
                pairs.append((t, t + d))
                break
    for (x, y) in pairs:
        r = base()
        r[x] = r[y] = r.max() + 1.5
        rows.append(('tie %d = %d' % (x, y), r, x))
    if non and pairs:   # the same tie under a non-candidate maximum
        x, y = pairs[-1]
        r = base()
        r[x] = r[y] = r.max() + 1.5
        r[non[0]] = r[x] + 3
        rows.append(('tie %d = %d under non-candidate %d' % (x, y, non[0]), r, x))
    if all(t in cs for t in (cand[0], cand[0] + 64, cand[0] + 256)):
        x = cand[0]
        r = base()
        r[x + 256] = r[x + 64] = r[x] = r.max() + 1
        rows.append(('three-way tie %d / %d / %d' % (x, x + 64, x + 256), r, x))
    # a non-candidate above every candidate: skipped, yet it is the softmax maximum (one row per filter branch that rejects a token here)
    for t in non:
        r = base()
        r[t] = r.max() + 20
        rows.append(('non-candidate %d above every candidate' % t, r, best_cand(r)))
    if Vs < V:   # the vie slice lies outside the support of the non-pt heads: it must not enter the softmax at all
        r = base()
        r[Vs:] = r.max() + 30
        rows.append(('vie slice above the support', r, best_cand(r)))
    # every candidate's probability underflows, or every candidate is -inf: the reference's filtered row is all zeros -> token 0, p = 0
    if non:
        r = base()
        r[non[-1]] = r.max() + 200
        rows.append(('candidates 200 below non-candidate %d' % non[-1], r, 0))
        r = base()
        r[:Vs][cm] = float('-inf')
        rows.append(('every candidate -inf', r, 0))
        r = base()
        top = r[:Vs][~cm].max()
        r[:Vs][cm] = top - 150 - _q(torch.rand(len(cand), generator=g) * 5)
        rows.append(('every candidate 150+ below the maximum', r, 0))
    # large logits and -inf elsewhere in the row (a softmax that does not subtract the maximum overflows)
    r = base()
    r[torch.randperm(V, generator=g)[:V // 8]] = float('-inf')
    r[cand[len(cand) // 3]] = 80.0
    if non:
        r[non[0]] = 79.5
        r[non[-1]] = -80.0
    r[cand[0]] = -80.0 if cand[len(cand) // 3] != cand[0] else 80.0
    rows.append(('+-80 logits, -inf entries', r, best_cand(r)))
    r = base()
    r[cand[-1]] = 100.0
    r[torch.randperm(V, generator=g)[:3]] = float('-inf')
    r[cand[-1]] = 100.0
    rows.append(('candidate at +100', r, cand[-1]))
    # pt steps that may end the sequence: EOS wins (finished / lengths bookkeeping; suppressed: never chosen)
    if kind == 'pt' and i % _period(a) == 0:
        for k in range(4):
            r = base()
            r[a.pt_eos_index] = r.max() + 2
            rows.append(('pt_eos wins %d' % k, r, None if suppress else a.pt_eos_index))
    return rows


def _fill(rows, R, V, seed):
    """the planted rows first, then random rows up to R"""
    g = _gen(seed + 7)
    out = [r for _, r, _ in rows[:R]]
    while len(out) < R:
        out.append(_q(torch.randn(V, generator=g) * 3))
    return torch.stack(out)


def _cfg(a, kind, V, suppress):
    return _lib.SampleCfg(KIND[kind], a.num_bins, a.pt_eos_index, a.poly_eos_index, a.rec_eos_index, V, a.vie_categories,
                          1 if a.infer_vie else 0, suppress, STEP0)


def _device_logits(logits, layout):
    """'pad4': rows padded to a multiple of four floats (+4) with a huge value no kernel may read as a logit; 'ld=V': dense rows;
    'offset1': a view one float into its storage (not 16-byte aligned), rows padded as in 'pad4'."""
    R, V = logits.shape
    if layout == 'ld=V':
        return logits.to(DEV)
    ldp = (V + 3) // 4 * 4 + 4
    off = 1 if layout == 'offset1' else 0
    buf = torch.full((R * ldp + 4,), 1e30, device=DEV)
    view = buf.as_strided((R, V), (ldp, 1), off)
    view.copy_(logits.to(DEV))
    return view


def _run_sample(impl, lg_dev, cfg, p, advance, fin0, len0):
    """one call of omp_head_softmax_mask_argmax with the kernel selector at `impl`; sentinel-filled outputs"""
    R = lg_dev.shape[0]
    seq = torch.full((R, SEQ_W), SENT_TOK, dtype=torch.int32, device=DEV)
    probs = torch.full((R, SEQ_W), SENT_PROB, device=DEV)
    fin, lens = fin0.to(DEV), len0.to(DEV)
    d_pos = torch.tensor([p, 0], dtype=torch.int32, device=DEV)   # (position, ticket): the workgroup kernel's advance takes the ticket
    ops.sample_impl(impl)
    try:
        ops.head_sample(lg_dev, cfg, seq, probs, fin, lens, d_pos, advance=bool(advance))
    finally:
        ops.sample_impl(0)
    torch.cuda.synchronize()
    return seq.cpu(), probs.cpu(), fin.cpu(), lens.cpu(), d_pos.cpu()


def _judge(tag, a, kind, i, logits, rows, got, p, advance, fin0, len0, suppress):
    seq, probs, fin, lens, d_pos = got
    R = logits.shape[0]
    t_ref, p_ref, p64 = oracle_sample(a, kind, i, logits, suppress)
    tok, pk = seq[:, p + 1].long(), probs[:, p + 1]
    out = []
    bad = (tok != t_ref).nonzero()[:, 0].tolist()
    names = [n for n, _, _ in rows] + ['random'] * (R - len(rows))
    out.append(rec(tag + ' ids == oracle filter + topk', len(bad), 0,
                   '; '.join('row %d (%s): %d vs %d' % (r, names[r], int(tok[r]), int(t_ref[r])) for r in bad[:4])))
    want = [(r, w) for r, (_, _, w) in enumerate(rows[:R]) if w is not None]
    ob = [(r, w) for r, w in want if int(t_ref[r]) != w]
    out.append(rec(tag + ' the oracle picks the id expected by construction (lower index of a tie, token 0 of an all-zero row)', len(ob), 0,
                   '; '.join('row %d (%s): oracle %d, expected %d' % (r, names[r], int(t_ref[r]), w) for r, w in ob[:4])))
    zero = p_ref == 0
    nz = ~zero & (p64 > 1e-30)
    rel = ((pk[nz].double() - p64[nz]).abs() / p64[nz]).max().item() if nz.any() else 0.0
    out.append(rec(tag + ' probabilities vs fp64 softmax (relative)', rel, 2e-6))
    out.append(rec(tag + ' probability exactly 0 where the oracle\'s is 0 (%d rows)' % int(zero.sum()), int((pk[zero] != 0).sum()), 0))
    out.append(rec(tag + ' never the 0x7fffffff start index', int((seq == 0x7fffffff).sum()), 0))
    keep = torch.ones(SEQ_W, dtype=torch.bool)
    keep[p + 1] = False
    untouched = int((seq[:, keep] != SENT_TOK).sum()) + int((probs[:, keep] != SENT_PROB).sum())
    out.append(rec(tag + ' seq / probs untouched outside [r, p + 1]', untouched, 0))
    if kind == 'pt':
        newly = (fin0 == 0) & (t_ref == a.pt_eos_index)
        efin = torch.where(newly, torch.ones_like(fin0), fin0)
        elen = torch.where(newly, torch.full_like(len0, p + 1), len0)
    else:
        efin, elen = fin0, len0
    out.append(rec(tag + ' finished / lengths (first EOS only; poly / rec never touch them)',
                   int((fin != efin).sum()) + int((lens != elen).sum()), 0))
    out.append(rec(tag + ' position advance %d, ticket left at 0' % advance, abs(int(d_pos[0]) - (p + advance)) + abs(int(d_pos[1])), 0))
    return out


def _fin_pattern(R):
    fin0 = (torch.arange(R) % 3 == 1).to(torch.int32)
    len0 = (SENT_LEN + torch.arange(R)).to(torch.int32)
    return fin0, len0


def check_sample_edges():
    """omp_head_softmax_mask_argmax with each sampling kernel pinned (dec_sample_kernel, dec_sample_rows_kernel, dec_sample_block_kernel +
    ticket) on one planted case table per (config, kind, step), then the auto selection at its thresholds and fallbacks."""
    out = []
    try:
        for vie in (0, 4):
            a = make_args(vie_categories=vie, infer_vie=vie > 0)
            V = a.num_classes
            runs = [('pt', i, 0) for i in range(_period(a) + 1)] + [('pt', 0, 1), ('poly', 1, 0), ('rec', 2, 0)]
            for n, (kind, i, sup) in enumerate(runs):
                rows = _sample_cases(a, kind, i, V, sup, seed=100 * vie + n)
                logits = _fill(rows, len(rows) + 5, V, seed=n)
                R = logits.shape[0]
                fin0, len0 = _fin_pattern(R)
                p = STEP0 - 1 + i
                for impl in (1, 2, 3):
                    advance = (n + impl) % 2
                    got = _run_sample(impl, _device_logits(logits, 'pad4'), _cfg(a, kind, V, sup), p, advance, fin0, len0)
                    tag = 'sample[%s,vie%d,%s,i=%d,suppress_eos=%d]' % (IMPL[impl], vie, kind, i, sup)
                    out += _judge(tag, a, kind, i, logits, rows, got, p, advance, fin0, len0, sup)
            # p + 1 < step0: nothing is written, the position still advances
            rows = _sample_cases(a, 'pt', 0, V, 0, seed=5)
            logits = _fill(rows, len(rows), V, seed=5)
            fin0, len0 = _fin_pattern(logits.shape[0])
            for impl in (1, 2, 3):
                for advance in (0, 1):
                    seq, probs, fin, lens, d_pos = _run_sample(impl, _device_logits(logits, 'pad4'), _cfg(a, 'pt', V, 0), STEP0 - 2, advance,
                                                               fin0, len0)
                    bad = int((seq != SENT_TOK).sum()) + int((probs != SENT_PROB).sum()) + int((fin != fin0).sum()) + int((lens != len0).sum())
                    out.append(rec('sample[%s,vie%d] p + 1 < step0 writes nothing' % (IMPL[impl], vie), bad, 0))
                    out.append(rec('sample[%s,vie%d] p + 1 < step0: advance %d, ticket 0' % (IMPL[impl], vie, advance),
                                   abs(int(d_pos[0]) - (STEP0 - 2 + advance)) + abs(int(d_pos[1])), 0))
        # thresholds and fallbacks of the auto selection: each must give the oracle's answer, whichever kernel it reaches
        legs = [('R=1024', dict(), 1024, 'ld=V'), ('R=1025', dict(), 1025, 'ld=V'),
                ('ld=V=1107 (V % 4 != 0)', dict(vie_categories=3, infer_vie=True), 1025, 'ld=V'),
                ('view 1 float off 16-byte alignment', dict(), 1025, 'offset1'),
                ('vocab 2104 > 2048', dict(num_bins=2000), 1025, 'pad4')]
        for name, kw, R, layout in legs:
            a = make_args(**kw)
            V = a.num_classes
            for n, (kind, i) in enumerate((('pt', 0), ('pt', 1), ('rec', 2), ('poly', 1))):
                rows = _sample_cases(a, kind, i, V, 0, seed=900 + n)
                logits = _fill(rows, R, V, seed=900 + n)
                fin0, len0 = _fin_pattern(R)
                p = STEP0 - 1 + i
                for impl in (0, 1, 2, 3):
                    refused = None
                    if impl == 2 and (V % 4 or layout == 'offset1' or V > 2048):
                        try:
                            _run_sample(2, _device_logits(logits, layout), _cfg(a, kind, V, 0), p, 1, fin0, len0)
                        except RuntimeError as e:
                            refused = str(e)
                        out.append(rec('sample[row in registers,%s] refused (OMP_ERR_UNSUPPORTED)' % name,
                                       0 if refused and '(-95)' in refused else 1, 0, refused or 'ran'))
                        continue
                    if impl in (1, 3) and (kind, i) != ('pt', 0):
                        continue
                    got = _run_sample(impl, _device_logits(logits, layout), _cfg(a, kind, V, 0), p, 1, fin0, len0)
                    out += _judge('sample[%s,%s,%s,i=%d]' % (IMPL[impl], name, kind, i), a, kind, i, logits, rows, got, p, 1, fin0, len0, 0)
    finally:
        ops.sample_impl(0)
    return out


# ---------------------------------------------------------------------------------------------
def check_row_argmax_prob_edges():
    """omp_row_argmax_prob: ids exact against torch.max on CPU (lowest index on ties), probabilities within 1e-6 relative of fp64"""
    out = []
    for V in (1, 63, 65, 1104, 50257):
        for R in (7, 4097 if V <= 1104 else 13):
            g = _gen(V + R)
            lg = _q(torch.randn(R, V, generator=g) * 3)
            want = {}
            if V > 1:
                top = lg.max() + 2
                lg[0, 0] = lg[0, V - 1] = top;                   want[0] = 0          # ties at both ends
                lg[1, V - 1] = lg[1, V // 2] = top;              want[1] = V // 2     # tie with the last column
                lg[2, :] = 0.5;                                  want[2] = 0          # the whole row tied
                for k, dd in enumerate((1, 32, 64)):                                  # across lanes and iterations
                    if 3 + k < R and 5 + dd < V:
                        lg[3 + k, 5] = lg[3 + k, 5 + dd] = top;  want[3 + k] = 5
                lg[R - 1, torch.randperm(V, generator=g)[:V // 3]] = float('-inf')   # -inf entries in an otherwise finite row
                lg[R - 1, V - 1] = 30.0;                         want[R - 1] = V - 1
            for ld in (V, V + 5):
                buf = torch.full((R, ld), 1e30)
                buf[:, :V] = lg
                dev = buf.to(DEV)[:, :V]
                ids, pr = ops.row_argmax_prob(dev)
                ids, pr = ids.cpu().long(), pr.cpu()
                ref_v, ref_i = torch.max(lg, dim=1)
                p64 = lg.double().softmax(-1).gather(1, ref_i[:, None])[:, 0]
                tag = 'row_argmax_prob[%dx%d,ld=%d]' % (R, V, ld)
                out.append(rec(tag + ' ids == torch.max', int((ids != ref_i).sum()), 0))
                out.append(rec(tag + ' torch.max and the kernel take the expected tie winner',
                               sum(int(ref_i[r] != w) + int(ids[r] != w) for r, w in want.items()), 0))
                out.append(rec(tag + ' prob (relative to fp64)', ((pr.double() - p64).abs() / p64).max().item(), 1e-6))
    return out


# ---------------------------------------------------------------------------------------------
def _pack_ref(points, poly, rec_ids, rprob, counts, N, rec_len):
    """ops.pack_spotting's docstring restated: ids[b, n] = point | polygon (32) | recognition (rec_len) of row row0[b] + n for
    n < min(counts[b], N), zeros after; probs alike (row0 = exclusive prefix sum of the uncapped counts)."""
    B = len(counts)
    ids = torch.zeros(B, N, 34 + rec_len, dtype=torch.int32)
    probs = torch.zeros(B, N, rec_len)
    r0 = 0
    for b, c in enumerate(counts):
        for n in range(min(c, N)):
            r = r0 + n
            ids[b, n] = torch.cat((points[r, :2], poly[r, :32], rec_ids[r, :rec_len]))
            probs[b, n] = rprob[r, :rec_len]
        r0 += c
    return ids, probs


def check_pack_spotting():
    """omp_pack_spotting bit-exact against the restatement: B in {1, 3, 8}, counts with 0, N and more than N (capped), rec_len 25 / 100
    (rows of 59 / 134 ids: the second wraps the 64-thread loop), strided polygon / recognition / probability rows, outputs prefilled with garbage"""
    out = []
    N = 6
    for B, counts in ((1, [4]), (1, [0]), (3, [N, 0, N + 3]), (8, [0, 1, N, N + 5, 2, 0, N - 1, 3])):
        for rec_len in (25, 100):
            Rt = max(1, sum(counts))
            g = _gen(B * 1000 + rec_len)
            ri = lambda *s: torch.randint(1, 1 << 20, s, generator=g, dtype=torch.int32)   # noqa: E731
            points = ri(Rt, 2)
            poly = ri(Rt, 40)[:, :32]
            rec_ids = ri(Rt, rec_len + 9)[:, :rec_len]
            rprob = torch.rand(Rt, rec_len + 3, generator=g)[:, :rec_len]
            ids_ref, probs_ref = _pack_ref(points, poly, rec_ids, rprob, counts, N, rec_len)
            dp = points.to(DEV)
            dpoly = torch.full((Rt, 40), -1, dtype=torch.int32, device=DEV)
            dpoly[:, :32] = poly.to(DEV)
            dpoly = dpoly[:, :32]
            drec = torch.full((Rt, rec_len + 9), -1, dtype=torch.int32, device=DEV)
            drec[:, :rec_len] = rec_ids.to(DEV)
            drec = drec[:, :rec_len]
            dprob = torch.full((Rt, rec_len + 3), -1.0, device=DEV)
            dprob[:, :rec_len] = rprob.to(DEV)
            dprob = dprob[:, :rec_len]
            c = torch.tensor(counts, dtype=torch.int32)
            row0 = (torch.cumsum(c, 0) - c).to(torch.int32).to(DEV)
            cnt = torch.minimum(c, torch.tensor(N, dtype=torch.int32)).to(DEV)
            ids = torch.full((B, N, 34 + rec_len), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
            probs = torch.full((B, N, rec_len), float('nan'), device=DEV)
            _lib.check(_lib.lib().omp_pack_spotting(ops.ptr(dp), ops.ptr(dpoly), dpoly.stride(0), ops.ptr(drec), drec.stride(0), ops.ptr(dprob),
                                                    dprob.stride(0), ops.ptr(row0), ops.ptr(cnt), B, N, rec_len, ops.ptr(ids), ops.ptr(probs),
                                                    ops.stream()), 'omp_pack_spotting')
            tag = 'pack_spotting[B%d,counts=%s,rec_len=%d]' % (B, counts, rec_len)
            out.append(rec(tag + ' ids bit-exact', 0 if torch.equal(ids.cpu(), ids_ref) else 1, 0))
            out.append(rec(tag + ' probs bit-exact', 0 if torch.equal(probs.cpu().view(torch.int32), probs_ref.view(torch.int32)) else 1, 0))
            i2, p2, n2 = ops.pack_spotting(dp, dpoly, drec, dprob, counts, N, rec_len)
            ok = torch.equal(i2.cpu(), ids_ref) and torch.equal(p2.cpu(), probs_ref) and n2.cpu().tolist() == [min(x, N) for x in counts]
            out.append(rec(tag + ' ops.pack_spotting (row offsets, caps)', 0 if ok else 1, 0))
    return out


# ---------------------------------------------------------------------------------------------
def _bf16_ulps(got, ref, floor=2e-5):
    """max |got - ref| in bf16 ulps of bf16(ref); near zero (|ref| below ~4e-3) the unit is the fp32 gate `floor` instead, since an fp32 error
    of a few 1e-7 is many ulps of a tiny value"""
    m = ref.to(torch.bfloat16).double().abs().clamp_min(2.0 ** -126)
    unit = torch.exp2(torch.floor(torch.log2(m)) - 7).clamp_min(floor)
    return ((got.double() - ref.double()).abs() / unit).max().item()


def check_dec_embed_ln():
    """omp_dec_embed_ln vs F.layer_norm(word[seq[:, p]] + pos[p]) in fp64: d with partial lanes, the first and last position, tokens 0 and
    V - 1, a seq row stride wider than needed, R of 1 / 5 / 4097; fp32 x alone, y alone, and both with y in fp32 and bf16"""
    out = []
    V, P, eps = 1108, 1024, 1e-5
    for d in (256, 260, 512, 1024):
        g = _gen(d)
        word = torch.randn(V, d, generator=g)
        pos = torch.randn(P, d, generator=g) * 0.5
        gamma = 1 + 0.1 * torch.randn(d, generator=g)
        beta = 0.1 * torch.randn(d, generator=g)
        dw, dpt, dg, db = word.to(DEV), pos.to(DEV), gamma.to(DEV), beta.to(DEV)
        for R in (1, 5, 4097):
            for p in (0, P - 1):
                seq = torch.randint(0, V, (R, P + 6), generator=g, dtype=torch.int32)
                seq[0, p] = 0
                seq[R - 1, p] = V - 1
                ref = F.layer_norm(word.double()[seq[:, p].long()] + pos.double()[p], (d,), gamma.double(), beta.double(), eps)
                dseq, dpos = seq.to(DEV), torch.tensor([p], dtype=torch.int32, device=DEV)
                tag = 'dec_embed_ln[d=%d,R=%d,p=%d]' % (d, R, p)
                x = torch.full((R, d), float('nan'), device=DEV)
                ops.dec_embed_ln(dseq, dpos, dw, dpt, dg, db, x=x, eps=eps)
                xs = x.cpu()
                out.append(rec(tag + ' x alone', (xs.double() - ref).abs().max().item(), 2e-5))
                y = torch.full((R, d), float('nan'), device=DEV)
                ops.dec_embed_ln(dseq, dpos, dw, dpt, dg, db, y=y, eps=eps)
                out.append(rec(tag + ' fp32 y alone', (y.cpu().double() - ref).abs().max().item(), 2e-5))
                x2 = torch.full((R, d), float('nan'), device=DEV)
                y2 = torch.full((R, d), float('nan'), device=DEV)
                ops.dec_embed_ln(dseq, dpos, dw, dpt, dg, db, x=x2, y=y2, eps=eps)
                out.append(rec(tag + ' x + fp32 y: both', max((x2.cpu().double() - ref).abs().max().item(), (y2.cpu().double() - ref).abs().max().item()), 2e-5))
                yb = torch.full((R, d), float('nan'), dtype=torch.bfloat16, device=DEV)
                ops.dec_embed_ln(dseq, dpos, dw, dpt, dg, db, y=yb, eps=eps)
                out.append(rec(tag + ' bf16 y alone within 1 bf16 ulp of fp64', _bf16_ulps(yb.cpu(), ref), 1.0))
                x3 = torch.full((R, d), float('nan'), device=DEV)
                yb.fill_(float('nan'))
                ops.dec_embed_ln(dseq, dpos, dw, dpt, dg, db, x=x3, y=yb, eps=eps)
                out.append(rec(tag + ' x + bf16 y: y within 1 bf16 ulp of fp64', _bf16_ulps(yb.cpu(), ref), 1.0))
                out.append(rec(tag + ' x + bf16 y: x == the fp32 result', 0 if torch.equal(x3.cpu(), xs) else 1, 0))
                out.append(rec(tag + ' x + bf16 y: y == bf16(x) (round to nearest even)', 0 if torch.equal(yb.cpu(), xs.to(torch.bfloat16)) else 1, 0))
    return out


# ---------------------------------------------------------------------------------------------
def _pad_masks(B, H, W, g):
    """every image a different padding: random, right only, bottom only, both, none, and random over a padded rectangle"""
    m = torch.zeros(B, H, W, dtype=torch.bool)
    for b in range(B):
        k = b % 6
        if k == 0:
            m[b] = torch.rand(H, W, generator=g) < 0.5
        if k in (1, 3, 5) and W > 1:
            m[b, :, W - max(1, W // (b + 3)):] = True
        if k in (2, 3, 5) and H > 1:
            m[b, H - max(1, H // (b + 2)):, :] = True
        if k == 5:
            m[b] |= torch.rand(H, W, generator=g) < 0.2
    return m


def check_mask_nearest():
    """omp_mask_nearest torch.equal to F.interpolate(mask, size=(h, w)) (mode 'nearest') on CPU: identity, exact 2x up and down,
    non-integer down (1000 -> 32, 963 -> 31, 7 -> 3), up (1 -> 5, 3 -> 7), the 1280x960 KIE input at its stride-16 level"""
    out = []
    axes = [(13, 13), (8, 16), (16, 8), (1000, 32), (963, 31), (7, 3), (1, 5), (3, 7)]
    shapes = [((H, W), (h, w)) for (H, h) in axes for (W, w) in axes] + [((960, 1280), (60, 80)), ((1280, 960), (80, 60))]
    for n, ((H, W), (h, w)) in enumerate(shapes):
        g = _gen(n)
        B = 3 if H * W > 100000 else 6
        m = _pad_masks(B, H, W, g)
        ref = F.interpolate(m[:, None].float(), size=(h, w)).bool()[:, 0]
        y = ops.mask_nearest(m.to(torch.uint8).to(DEV), h, w).cpu().bool()
        out.append(rec('mask_nearest[B%d %dx%d -> %dx%d]' % (B, H, W, h, w), int((y != ref).sum()), 0))
    return out


def check_posembed_edges():
    """omp_sine_posembed vs O.sine_position: fp32 within 2e-5, bf16 within one bf16 ulp of the fp32 oracle; padding on the right only, at
    the bottom only, both and none, in one batch; the map of the 1280x960 KIE input at the consumed stride-16 level (both orientations)"""
    out = []
    for (h, w) in ((10, 13), (60, 80), (80, 60), (1, 7), (33, 1)):
        B = 4
        m = torch.zeros(B, h, w, dtype=torch.bool)
        if w > 1:
            m[1, :, w - max(1, w // 4):] = True
            m[3, :, w - max(1, w // 3):] = True
        if h > 1:
            m[2, h - max(1, h // 5):, :] = True
            m[3, h - max(1, h // 2):, :] = True
        ref = O.sine_position(m).flatten(2).permute(0, 2, 1)
        m8 = m.to(torch.uint8).to(DEV)
        yf = ops.sine_posembed(m8, 256, torch.float32).cpu()
        out.append(rec('sine_posembed[fp32,B%d %dx%d, none / right / bottom / both]' % (B, h, w), (yf - ref).abs().max().item(), 2e-5))
        yb = ops.sine_posembed(m8, 256, torch.bfloat16).cpu()
        out.append(rec('sine_posembed[bf16,B%d %dx%d] within 1 bf16 ulp of the fp32 oracle' % (B, h, w), _bf16_ulps(yb, ref), 1.0))
        out.append(rec('sine_posembed[bf16,B%d %dx%d] == bf16(fp32 output)' % (B, h, w), 0 if torch.equal(yb, yf.to(torch.bfloat16)) else 1, 0))
    return out
