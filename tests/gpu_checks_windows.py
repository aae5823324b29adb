"""GPU checks of window prompts: omp_window_points against its numpy specification
(utils/windows.py: gather_points_cpu) on every output integer; windowed engine calls against the reference run once per window
(tests/golden/spot_windows.pt, tools/gen_golden_windows.py), against every window submitted alone through forward(samples, seqs), against
today's predict, with ragged batches, under graph replay and through the two-stage reader.  Every check returns records
{name, err, tol, ok, note} like tests/gpu_checks.py; the GPU modules are imported inside the checks so that fixture_case stays usable
without a device (tests/test_windows_host.py)."""
import numpy as np
import torch

from advancedliteratemachinery_amd.utils import windows as WN
from advancedliteratemachinery_amd.utils import synthetic as weights
from advancedliteratemachinery_amd.utils.parser import make_args

F32_GRADE = ('fp32', 'bf16x3')


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixture's inputs, rebuilt without the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def fixture_case(gold, variant):
    """-> (args, sd, img, mask, seqs) of spot_windows' `variant`: the base case's seeded weights and image draw (oracle/gen_golden.py)
    with the variant's pt_seq_length and the ONE recorded bias added to the point head's EOS logit"""
    from oracle import gen_golden as G
    c, v = gold['case'], gold['variants'][variant]
    args, sd, img, mask, seqs = G.case_inputs(dict(args=dict(c['args'], pt_seq_length=v['pt_seq_length']), hw=c['hw'], depths=c['depths']))
    assert torch.equal(G.fingerprint(sd), gold['fingerprint']), 'spot_windows was written from other weights (RNG drift)'
    sd = dict(sd)
    b = sd[c['eos_key']].clone()
    b[args.pt_eos_index] += v['eos_bias']
    sd[c['eos_key']] = b
    return args, sd, img, mask, seqs


# ---------------------------------------------------------------------------------------------------------------------------------
# op level: omp_window_points == gather_points_cpu
# ---------------------------------------------------------------------------------------------------------------------------------
OP_ROWS = (1, 2, 63, 64, 65, 257, 1023, 1024, 1025, 2500, 4096)


def _op_case(rows, mode, seed):
    """random point-phase buffers: tokens over the bins, windows of every size (some empty under the rule), EOS positions anywhere in
    the row; mode: all / none / some rows finished; some rows empty (EOS at the first step, or nothing sampled)"""
    rng = np.random.RandomState(seed)
    n_prompt = int(rng.choice([5, 7]))
    ld = int(rng.choice([n_prompt + 1, n_prompt + 2, 20, 77, 150]))
    seq = rng.randint(0, 1000, size=(rows, ld)).astype(np.int32)
    x0, y0 = rng.randint(0, 700, rows), rng.randint(0, 700, rows)
    seq[:, 0], seq[:, 1], seq[:, 2], seq[:, 3] = x0, y0, np.minimum(x0 + rng.randint(0, 600, rows), 999), np.minimum(y0 + rng.randint(0, 600, rows), 999)
    seq[rng.rand(rows) < 0.2, 0:4] = [0, 0, 999, 999]
    seq[rng.rand(rows, ld) < 0.02] = 0                       # bin 0 among the tokens
    finished = {'all': np.ones(rows), 'none': np.zeros(rows), 'some': rng.rand(rows) < 0.5}[mode].astype(np.int32)
    lengths = rng.randint(n_prompt, ld + 1, rows).astype(np.int32)
    lengths[rng.rand(rows) < 0.15] = n_prompt                # empty rows
    sampled = int(rng.randint(0, ld - n_prompt + 1))
    n_images = int(rng.randint(1, max(2, rows // 3 + 1)))
    row_image = np.sort(rng.randint(0, n_images, rows)).astype(np.int32)
    return seq, finished, lengths, n_prompt, sampled, row_image, n_images


def check_window_points_op():
    from advancedliteratemachinery_amd import ops
    from tests.gpu_checks import DEV, rec
    out = []
    for i, rows in enumerate(OP_ROWS):
        for j, mode in enumerate(('all', 'none', 'some')):
            seq, fin, lens, n_prompt, sampled, row_image, n_images = _op_case(rows, mode, 100 * i + j)
            d = [torch.from_numpy(t).to(DEV) for t in (seq, fin, lens, row_image)]
            for clip in (False, True):
                pts, owner, cnt, drop = WN.gather_points_cpu(seq, fin, lens, n_prompt, sampled, clip)
                total = int(cnt.sum())
                want = np.concatenate([cnt, drop, np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32),
                                       np.bincount(row_image, weights=cnt, minlength=n_images).astype(np.int32)])
                tag = 'window_points[rows=%d,%s,clip=%d,ld=%d,sampled=%d]' % (rows, mode, clip, seq.shape[1], sampled)
                g_pts, g_owner, g_counts = ops.window_points(d[0], d[1], d[2], d[3], n_images, n_prompt, sampled, clip=clip)
                bad = int((g_counts.cpu().numpy() != want).sum())
                out.append(rec(tag + ' row_count | dropped | row_start | image_count', bad, 0, '%d points' % total))
                bad = int((g_pts[:total].cpu().numpy() != pts).sum()) + int((g_owner[:total].cpu().numpy() != owner).sum())
                out.append(rec(tag + ' points, inst_row', bad, 0))
                # a cap below the total: the head of the same list, nothing written beyond the cap
                cap = total // 2
                g_pts, g_owner, g_counts = ops.window_points(d[0], d[1], d[2], d[3], n_images, n_prompt, sampled, clip=clip, cap=cap)
                bad = int((g_counts.cpu().numpy() != want).sum()) + int((g_pts.cpu().numpy() != pts[:cap]).sum()) \
                    + int((g_owner.cpu().numpy() != owner[:cap]).sum())
                out.append(rec(tag + ' cap=%d: the head of the list, counts in full' % cap, bad, 0))
    # rows of no image (row_image outside [0, n_images)) count for none; every other output is unchanged
    seq, fin, lens, n_prompt, sampled, row_image, n_images = _op_case(300, 'some', 7)
    row_image[::7] = -1
    row_image[3::11] = n_images
    d = [torch.from_numpy(t).to(DEV) for t in (seq, fin, lens, row_image)]
    pts, owner, cnt, drop = WN.gather_points_cpu(seq, fin, lens, n_prompt, sampled, False)
    ok = (row_image >= 0) & (row_image < n_images)
    _, _, g_counts = ops.window_points(d[0], d[1], d[2], d[3], n_images, n_prompt, sampled)
    got = ops.split_window_counts(g_counts.cpu().numpy(), 300)
    bad = int((got[3] != np.bincount(row_image[ok], weights=cnt[ok], minlength=n_images).astype(np.int32)).sum()) + int((got[0] != cnt).sum())
    out.append(rec('window_points: rows outside the image table count for no image', bad, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# against the reference: all fixture windows in ONE call
# ---------------------------------------------------------------------------------------------------------------------------------
def _by_window(res, W):
    """one image's windowed result -> per window (pt [2n], poly [n, 32], rec [n, L], probs [n, L]) or None"""
    if res is None:
        return [None] * W
    (pt, poly, rec_), (probs,), window = res
    pt, poly, rec_ = pt.reshape(-1, 2).cpu(), poly.reshape(-1, 32).cpu(), rec_[0].cpu()
    out = []
    for w in range(W):
        sel = window == w
        out.append(None if not bool(sel.any()) else (pt[sel].reshape(-1), poly[sel], rec_[sel], probs.cpu()[sel]))
    return out


def check_fixture(dtype_name, variant):
    from tests.gpu_checks import DEV, ENGINES, build_model, golden, rec
    gold = golden('spot_windows')
    var = gold['variants'][variant]
    args, sd, img, mask, seqs = fixture_case(gold, variant)
    model = build_model(args, sd, gold['case']['depths'], ENGINES[dtype_name])
    W = len(gold['windows'])
    res = model.infer(img.to(DEV), mask.to(DEV), seqs, forced_instances=var['forced_instances'], windows=gold['windows'],
                      char_windows=gold['char_windows'])[0]
    out = []
    tag0 = 'windows fixture[%s,%s]' % (dtype_name, variant)
    lens = set()
    for w, (got, ref) in enumerate(zip(_by_window(res, W), var['out'])):
        tag = '%s window %d %s' % (tag0, w, gold['prompts'][w].tolist())
        if got is None or ref is None:
            out.append(rec(tag + ' empty as the reference', 0 if (got is None) == (ref is None) else 1, 0))
            continue
        lens.add(got[0].numel())
        for name, g, r in (('pt', got[0], ref['pt'].reshape(-1)), ('poly', got[1].reshape(-1), ref['poly'].reshape(-1)),
                           ('rec', got[2].reshape(-1), ref['rec'].reshape(-1))):
            same = g.shape == r.shape and bool((g == r).all())
            out.append(rec('%s %s ids identical' % (tag, name), 0 if same else 1, 0, '%d tokens' % r.numel()))
        perr = (got[3] - ref['rec_probs']).abs().max().item() if got[3].shape == ref['rec_probs'].shape else float('inf')
        out.append(rec(tag + ' rec probs', perr, 1e-3))
    if variant == 'eos':
        out.append(rec(tag0 + ' windows end at their own lengths', 0 if len(lens) > 1 else 1, 0, 'lengths %s' % sorted(lens)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# W windows in one call == every window alone through forward(samples, seqs)
# ---------------------------------------------------------------------------------------------------------------------------------
def _small(dtype_name, graph=False, seed=4, pt_seq_length=10):
    from tests.gpu_checks import ENGINES, build_model
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, pt_seq_length=pt_seq_length)
    depths = (2, 2, 2, 2)
    sd = weights.make_state_dict(args, seed=seed, depths=depths)
    return args, build_model(args, sd, depths, ENGINES[dtype_name], graph)


def _agree(a, b, stats):
    """token agreement of two windows' results, accumulated as gpu_checks.check_batch_equivalence counts it"""
    if a is None or b is None:
        stats[1] += 1
        stats[0] += int((a is None) == (b is None))
        return
    for x, y in zip(a[:3], b[:3]):
        x, y = x.reshape(-1), y.reshape(-1)
        n = min(x.numel(), y.numel())
        stats[1] += max(x.numel(), y.numel())
        stats[0] += int((x[:n] == y[:n]).sum())


def _alone(model, args, img, mask, window, char_window=None):
    """one window through the EXISTING forward(samples, seqs): that window's prompt in seqs[0]"""
    from advancedliteratemachinery_amd.engine.inference import build_prompts
    from advancedliteratemachinery_amd.utils.nested_tensor import NestedTensor
    seqs = build_prompts(args)
    seqs[0] = WN.window_prompts(args, [window], None if char_window is None else [char_window])
    r = model(NestedTensor(img, mask), seqs)
    if r is None:
        return None
    return (r[0][0].reshape(-1).cpu(), r[0][1].reshape(-1, 32).cpu(), r[0][2][0].cpu(), r[1][0].cpu())


# Probabilities of one call against the same window alone, on the SAME engine.  The demand is on tokens; the probabilities are bounded
# by what the engine's arithmetic allows when the two runs take different kernels, which they do: a phase picks its kernels by its row
# count, and 9 windows x 2 images x 5 instances = 90 polygon / recognition rows against 5 alone.
#   fp32    both paths accumulate fp32 products in fp32, in another order: 1e-5, the bound of the ragged and batch checks.
#   bf16x3  from 65 rows on the Linear layers run as three bf16 products of split operands (a = hi + lo, the lo x lo term dropped:
#           2^-16 relative per product), below as fp32 kernels.  Neither path is the other's reference; each is held to the
#           project's gate for this engine against the fp32 reference (probabilities within 1e-3: tests/gpu_checks.py check_e2e,
#           and check_fixture above), so that gate bounds their difference too.
PROB_TOL = {'fp32': 1e-5, 'bf16x3': 1e-3}


def check_windows_equal_alone(dtype_name):
    """the same demand as check_batch_equivalence: fp32-grade engines identical tokens, bf16 within its near-tie allowance"""
    from tests.gpu_checks import DEV, REPORT, rec, rnd
    args, model = _small(dtype_name)
    imgs = rnd(2, 3, 96, 128, seed=3).to(DEV)
    mask = torch.zeros(2, 96, 128, dtype=torch.bool, device=DEV)
    from advancedliteratemachinery_amd.engine.inference import build_prompts
    seqs = build_prompts(args)
    out, stats = [], [0, 0]
    for wins, chars in ((WN.grid_windows(2, 2, args.num_bins), None), (WN.grid_windows(3, 3, args.num_bins), None),
                        ([WN.default_window(args), [100, 200, 640, 900], [0, 0, 999, 999]], [[0, 95], [0, 95], [10, 40]])):
        res = model.infer(imgs, mask, seqs, windows=wins, char_windows=chars)
        for b in range(2):
            per = _by_window(res[b], len(wins))
            for w, win in enumerate(wins):
                alone = _alone(model, args, imgs[b:b + 1], mask[b:b + 1], win, None if chars is None else chars[w])
                before = list(stats)
                _agree(per[w], alone, stats)
                if dtype_name in F32_GRADE:
                    tag = 'windows==alone[%s] %d windows, img%d window %d' % (dtype_name, len(wins), b, w)
                    out.append(rec(tag + ' tokens identical', (stats[1] - before[1]) - (stats[0] - before[0]), 0))
                    if per[w] is not None and alone is not None and per[w][3].shape == alone[3].shape:
                        out.append(rec(tag + ' rec probs', (per[w][3] - alone[3]).abs().max().item(), PROB_TOL[dtype_name]))
    frac = stats[0] / max(1, stats[1])
    REPORT.append(dict(name='windows_equal_alone[%s]' % dtype_name, match=frac, tokens=stats[1]))
    out.append(rec('windows==alone[%s] token agreement' % dtype_name, 1.0 - frac, 0.0 if dtype_name in F32_GRADE else 0.05,
                   'agreement %.3f of %d' % (frac, stats[1])))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# windows=None / the default window == today's predict
# ---------------------------------------------------------------------------------------------------------------------------------
def _strip(records, keys=('window', 'window_bins')):
    return [[{k: v for k, v in r.items() if k not in keys} for r in recs] for recs in records]


def check_default_equals_today(dtype_name):
    from advancedliteratemachinery_amd.engine.inference import build_prompts, predict
    from tests.gpu_checks import DEV, rec, rnd
    args, model = _small(dtype_name, seed=5, pt_seq_length=8)
    imgs = rnd(3, 3, 96, 128, seed=9).to(DEV)
    out = []
    today = predict(model, imgs, args)
    n = sum(len(r) for r in today)
    out.append(rec('windows default[%s]: words spotted' % dtype_name, 0 if n > 0 else 1, 0, '%d words' % n))
    same = predict(model, imgs, args, windows=None, char_windows=None, grid=None)
    out.append(rec('windows default[%s]: windows=None is today\'s predict' % dtype_name, 0 if same == today else 1, 0))
    # the default window as an explicit window: the same rows, tiles and kernels -> the same records, plus the two new keys
    got = predict(model, imgs, args, windows=[WN.default_window(args)])
    out.append(rec('windows default[%s]: windows=[default window] records minus the new keys' % dtype_name, 0 if _strip(got) == today else 1, 0))
    bad = sum(int(r.get('window') != 0 or r.get('window_bins') != WN.default_window(args)) for recs in got for r in recs)
    out.append(rec('windows default[%s]: window = 0, window_bins = the default window' % dtype_name, bad, 0))
    got = predict(model, imgs, args, grid=(1, 1))
    out.append(rec('windows default[%s]: grid=(1, 1) likewise' % dtype_name, 0 if _strip(got) == today else 1, 0))
    # infer itself: windows=None returns today's 2-tuples bit for bit
    mask = torch.zeros(3, 96, 128, dtype=torch.bool, device=DEV)
    seqs = build_prompts(args)
    a, b = model.infer(imgs, mask, seqs), model.infer(imgs, mask, seqs, windows=None)
    bad = 0
    for x, y in zip(a, b):
        if x is None or y is None:
            bad += int((x is None) != (y is None))
            continue
        bad += int(len(y) != 2) + sum(int(not torch.equal(p, q)) for p, q in zip(x[0] + x[1], y[0] + y[1]))
    out.append(rec('windows default[%s]: infer(windows=None) bit for bit' % dtype_name, bad, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# ragged batches and graph replay
# ---------------------------------------------------------------------------------------------------------------------------------
def check_ragged_windows(dtype_name):
    """two image sizes in one ragged windowed call: each image's result equals that image submitted alone (same windows)"""
    from advancedliteratemachinery_amd.engine.inference import build_prompts
    from tests.gpu_checks import DEV, REPORT, rec, rnd
    args, model = _small(dtype_name)
    seqs = build_prompts(args)
    sizes = [(96, 128), (160, 224), (96, 128)]
    imgs = [rnd(3, h, w, seed=50 + i).to(DEV) for i, (h, w) in enumerate(sizes)]
    wins = [WN.grid_windows(2, 2, args.num_bins), WN.grid_windows(3, 1, args.num_bins), WN.grid_windows(2, 2, args.num_bins)]
    res = model.infer(imgs, None, seqs, ragged=True, windows=wins)
    out, stats = [], [0, 0]
    for b, (im, (h, w)) in enumerate(zip(imgs, sizes)):
        alone = model.infer(im[None], torch.zeros(1, h, w, dtype=torch.bool, device=DEV), seqs, windows=wins[b])[0]
        before = list(stats)
        for x, y in zip(_by_window(res[b], len(wins[b])), _by_window(alone, len(wins[b]))):
            _agree(x, y, stats)
        if dtype_name in F32_GRADE:
            out.append(rec('ragged windows[%s] img%d %dx%d tokens identical to alone' % (dtype_name, b, h, w),
                           (stats[1] - before[1]) - (stats[0] - before[0]), 0))
            if res[b] is not None and alone is not None:
                same_w = res[b][2].shape == alone[2].shape and bool((res[b][2] == alone[2]).all())
                out.append(rec('ragged windows[%s] img%d window index as alone' % (dtype_name, b), 0 if same_w else 1, 0))
                if res[b][1][0].shape == alone[1][0].shape:
                    out.append(rec('ragged windows[%s] img%d rec probs' % (dtype_name, b), (res[b][1][0] - alone[1][0]).abs().max().item(), 1e-5))
    frac = stats[0] / max(1, stats[1])
    REPORT.append(dict(name='ragged_windows[%s]' % dtype_name, match=frac, tokens=stats[1]))
    out.append(rec('ragged windows[%s] token agreement' % dtype_name, 1.0 - frac, 0.0 if dtype_name in F32_GRADE else 0.05,
                   'agreement %.3f of %d' % (frac, stats[1])))
    return out


def check_graph_windows(dtype_name):
    """graph replay == eager launches on a windowed call (the second graphed call replays what the first captured)"""
    from advancedliteratemachinery_amd.engine.inference import build_prompts
    from tests.gpu_checks import DEV, rec, rnd
    imgs = rnd(2, 3, 64, 96, seed=8).to(DEV)
    mask = torch.zeros(2, 64, 96, dtype=torch.bool, device=DEV)
    st = torch.cuda.Stream()
    res = []
    for graph in (False, True):
        args, model = _small(dtype_name, graph=graph, seed=6, pt_seq_length=8)
        seqs = build_prompts(args)
        wins = WN.grid_windows(2, 2, args.num_bins)
        with torch.cuda.stream(st):
            r = model.infer(imgs, mask, seqs, forced_instances=3, windows=wins)
            r2 = model.infer(imgs, mask, seqs, forced_instances=3, windows=wins)
            r3 = model.infer(imgs, mask, seqs, windows=wins)     # EOS honoured: the polled point phase
        st.synchronize()
        res.append((r, r2, r3))
    bad = n = 0
    for b in range(2):
        for k in range(3):
            for (x, y) in ((res[0][0], res[1][0]), (res[1][0], res[1][1]), (res[0][2], res[1][2])):
                n += 1
                bad += 0 if x[b][0][k].shape == y[b][0][k].shape and bool((x[b][0][k] == y[b][0][k]).all()) else 1
        bad += 0 if bool((res[0][0][b][2] == res[1][0][b][2]).all()) else 1
    return [rec('windows graph==eager[%s]' % dtype_name, bad, 0, '%d comparisons' % n),
            rec('windows graph==eager[%s]: 4 windows x 3 forced instances per image' % dtype_name,
                sum(int(r[0][0].numel() != 24) for r in res[0][0]), 0)]


# ---------------------------------------------------------------------------------------------------------------------------------
# two-stage reader
# ---------------------------------------------------------------------------------------------------------------------------------
def check_two_stage_windows():
    from advancedliteratemachinery_amd.engine.two_stage import recognize_crops, spot_and_recognize
    from oracle import mgp_str_ref as R
    from tests.gpu_checks import DEV, build_model, rec
    from tests.gpu_checks_mgp import build
    depths = (2, 2, 2, 2)
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, pt_seq_length=6, test_min_size=64, test_max_size=112)
    sd = weights.make_state_dict(args, seed=5, depths=depths)
    omni = build_model(args, sd, depths, torch.float32)
    c = R.cfg(depth=2)
    mgp = build(c, R.make_state_dict(c, seed=17), torch.float32)
    rng = np.random.RandomState(3)
    images = [torch.from_numpy(rng.randint(0, 256, (90, 140, 3), dtype=np.uint8)), torch.from_numpy(rng.randint(0, 256, (70, 100, 3), dtype=np.uint8))]
    grid = WN.grid_windows(2, 2, args.num_bins)
    out = []
    for mode in ('box', 'polygon'):
        got, _, _ = spot_and_recognize(omni, mgp, images, args, crop=mode, grid=(2, 2))
        flat = [(b, r) for b, recs in enumerate(got) for r in recs]
        out.append(rec('two-stage windows[%s]: words spotted in several windows' % mode, 0 if len(set(r['window'] for _, r in flat)) > 1 else 1, 0,
                       '%d words' % len(flat)))
        keys = {'window', 'window_bins', 'box', 'mgp_text', 'mgp_conf', 'mgp_choice', 'mgp_ids'}
        bad = sum(int(not keys <= set(r)) + int(r['window_bins'] != grid[r['window']]) for _, r in flat)
        out.append(rec('two-stage windows[%s]: records carry window, window_bins and the mgp_* fields' % mode, bad, 0))
        bad = sum(int([r['window'] for r in recs] != sorted(r['window'] for r in recs)) for recs in got)
        out.append(rec('two-stage windows[%s]: an image\'s records are in window order' % mode, bad, 0))
        # the recogniser's reading of every record == recognize_crops on the records' own polygons / boxes
        dev_imgs = [i.to(DEV).contiguous() for i in images]
        if mode == 'polygon':
            reads, _ = recognize_crops(mgp, dev_imgs, None, polys=[(b, r['polys']) for b, r in flat])
        else:
            reads, _ = recognize_crops(mgp, dev_imgs, [(b,) + tuple(r['box']) for b, r in flat])
        bad = 0
        for (_, r), m in zip(flat, reads):
            bad += int(r['mgp_text'] != m['char_text']) + int(r['mgp_choice'] != m['choice']) + int(tuple(r['mgp_conf']) != tuple(m['conf']))
            bad += sum(int(list(r['mgp_ids'][k]) != list(m[k + '_ids'])) for k in ('char', 'bpe', 'wp'))
        out.append(rec('two-stage windows[%s]: mgp_* == recognize_crops on the same crops' % mode, bad + int(len(reads) != len(flat)), 0))
    return out
