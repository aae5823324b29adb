"""Window prompts on the host (no GPU): the grid windows against the reference's recorded partitions, the prompt rows and what they
refuse, the numpy specification of omp_window_points on hand-built and random buffers, the cross-attention tiles of windowed point
phases, how OmniParser.infer / predict route the arguments, and -- where the reference tree is present -- the oracle fed every fixture
prompt against tests/golden/spot_windows.pt.  The kernel and the end-to-end answers are tests/test_gpu_windows.py."""
import contextlib
import inspect
import json
import os

import numpy as np
import pytest
import torch

from advancedliteratemachinery_amd.engine import inference as inf
from advancedliteratemachinery_amd.engine import two_stage
from advancedliteratemachinery_amd.model import omniparser as omp
from advancedliteratemachinery_amd.model.transformer import Decoder
from advancedliteratemachinery_amd.utils import windows as WN
from advancedliteratemachinery_amd.utils.parser import make_args


# -- grid_windows ---------------------------------------------------------------------------------------------------------------------
def test_grid_windows_equal_the_reference_partitions(golden_dir):
    with open(os.path.join(golden_dir, 'window_grids.json')) as f:
        rec = json.load(f)
    assert rec['num_bins'] == 1000
    assert [(g['nx'], g['ny']) for g in rec['grids']] == list(WN.TRAINING_GRIDS) and len(rec['grids']) == 8
    for g in rec['grids']:
        assert len(g['windows']) == g['nx'] * g['ny']
        assert WN.grid_windows(g['nx'], g['ny'], rec['num_bins']) == g['windows'], (g['nx'], g['ny'])


def test_grid_windows_x_is_the_outer_loop():
    assert WN.grid_windows(2, 2, 1000) == [[0, 0, 500, 500], [0, 500, 500, 999], [500, 0, 999, 500], [500, 500, 999, 999]]
    assert WN.grid_windows(1, 1, 1000) == [[0, 0, 999, 999]]
    assert WN.grid_windows(3, 1, 1000) == [[0, 0, 333, 999], [333, 0, 666, 999], [666, 0, 999, 999]]
    with pytest.raises(ValueError):
        WN.grid_windows(0, 2, 1000)


# -- window_prompts -------------------------------------------------------------------------------------------------------------------
def _args(char=True, **kw):
    return make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=char, **kw)


def test_window_prompts_layouts_and_defaults():
    a5, a7 = _args(False), _args(True)
    nb, nc = a7.num_bins, len(a7.chars)
    assert WN.window_prompts(a5).tolist() == [[0, 0, nb - 1, nb - 1, a5.pt_sos_index]]
    assert WN.window_prompts(a7).tolist() == [[0, 0, nb - 1, nb - 1, nb, nb + nc, a7.pt_sos_index]]
    # the defaults are the plain call's prompt (engine/val.py:25-33)
    assert WN.window_prompts(a5).tolist() == inf.build_prompts(a5)[0].tolist()
    assert WN.window_prompts(a7).tolist() == inf.build_prompts(a7)[0].tolist()
    wins = [[0, 0, 500, 500], [10, 20, 30, 40]]
    p = WN.window_prompts(a5, wins)
    assert p.dtype == torch.int64 and p.tolist() == [w + [a5.pt_sos_index] for w in wins]
    p = WN.window_prompts(a7, wins, [[0, 5], [7, nc]])
    assert p.tolist() == [wins[0] + [nb, nb + 5, a7.pt_sos_index], wins[1] + [nb + 7, nb + nc, a7.pt_sos_index]]
    assert WN.window_prompts(a7, wins, [3, 9]).tolist() == [w + [nb + 3, nb + 9, a7.pt_sos_index] for w in wins]   # one pair for all
    assert WN.window_prompts(a7, wins).tolist() == [w + [nb, nb + nc, a7.pt_sos_index] for w in wins]
    assert tuple(WN.window_prompts(a7, [[0, 0, 1, 1]] * 64).shape) == (64, 7)
    assert WN.window_prompts(a7, [[5, 5, 5, 5]]).tolist()[0][:4] == [5, 5, 5, 5]   # x0 == x1 is a window (an empty one under the rule)


@pytest.mark.parametrize('wins, chars, char_cfg', [
    ([[-1, 0, 10, 10]], None, True),            # below the bins
    ([[0, 0, 1000, 10]], None, True),           # above the bins
    ([[20, 0, 10, 10]], None, True),            # x0 > x1
    ([[0, 30, 10, 10]], None, True),            # y0 > y1
    ([[0, 0, 10]], None, True),                 # not four values
    ([[0, 0, 10, 10]], [[9, 3]], True),         # c0 > c1
    ([[0, 0, 10, 10]], [[-1, 3]], True),        # below the characters
    ([[0, 0, 10, 10]], [[0, 96]], True),        # above len(chars) = 95
    ([[0, 0, 10, 10]], [[0, 3]], False),        # char_windows without use_char_window_prompt
    ([[0, 0, 10, 10]], [[0, 3], [0, 4]], True),  # two character windows for one window
    ([[0, 0, 10, 10]] * 65, None, True),        # more than 64 windows per image
    ([], None, True),
])
def test_window_prompts_refuse(wins, chars, char_cfg):
    a = _args(char_cfg)
    assert len(a.chars) == 95
    with pytest.raises(ValueError):
        WN.window_prompts(a, wins, chars)


def test_resolve_windows():
    shared = [[0, 0, 5, 5], [1, 1, 9, 9]]
    assert WN.resolve_windows(None, 3) is None
    assert WN.resolve_windows(shared, 2) == [shared, shared]
    assert WN.resolve_windows([shared, shared[:1]], 2) == [shared, shared[:1]]
    assert WN.resolve_windows(None, 2, grid=(2, 1), num_bins=1000) == [WN.grid_windows(2, 1, 1000)] * 2
    with pytest.raises(ValueError):
        WN.resolve_windows([shared], 2)                       # one list for two images
    with pytest.raises(ValueError):
        WN.resolve_windows(shared, 2, grid=(2, 2), num_bins=1000)
    per = WN.resolve_windows(shared, 2)
    assert WN.resolve_char_windows(None, per) == [None, None]
    assert WN.resolve_char_windows([0, 3], per) == [[[0, 3], [0, 3]]] * 2
    assert WN.resolve_char_windows([[0, 3], [1, 4]], per) == [[[0, 3], [1, 4]]] * 2
    assert WN.resolve_char_windows([[[0, 3], [1, 4]], [[2, 2], [5, 6]]], per) == [[[0, 3], [1, 4]], [[2, 2], [5, 6]]]


# -- gather_points_cpu ----------------------------------------------------------------------------------------------------------------
NP = 5


def _row(window, tokens, ld=16):
    r = list(window) + [1100] + list(tokens)
    return r + [0] * (ld - len(r))


def test_gather_points_hand_built():
    seq = np.array([
        _row([0, 0, 999, 999], [10, 20, 30, 40, 1099]),            # finished after two pairs (the EOS sits at position 9)
        _row([0, 0, 999, 999], []),                                 # an empty row: EOS at the first step
        _row([0, 0, 999, 999], [1, 2, 3, 4, 5]),                    # finished with an odd tail: 5 is dropped
        _row([0, 0, 999, 999], [7, 8, 9, 10, 11, 12, 13, 14]),      # unfinished: `sampled` tokens count
        _row([100, 100, 200, 200], [150, 150, 100, 150, 200, 200, 150, 201, 101, 101]),   # for the clip
        _row([0, 0, 999, 999], [0, 5, 5, 0, 5, 5]),                 # bin 0 under the default window
    ], dtype=np.int32)
    finished = np.array([1, 1, 1, 0, 0, 0], np.int32)
    lengths = np.array([NP + 4, NP, NP + 5, 0, 0, 0], np.int32)
    pts, owner, cnt, drop = WN.gather_points_cpu(seq, finished, lengths, NP, 6)
    assert cnt.tolist() == [2, 0, 2, 3, 3, 3] and drop.tolist() == [0] * 6
    assert pts.tolist() == [[10, 20], [30, 40], [1, 2], [3, 4], [7, 8], [9, 10], [11, 12], [150, 150], [100, 150], [200, 200], [0, 5], [5, 0], [5, 5]]
    assert owner.tolist() == [0, 0, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5]
    assert all(t.dtype == np.int32 for t in (pts, owner, cnt, drop)) and pts.shape == (13, 2)
    # an unfinished row with an odd number of sampled tokens drops the tail too
    assert WN.gather_points_cpu(seq, finished, lengths, NP, 7)[2].tolist() == [2, 0, 2, 3, 3, 3]
    assert WN.gather_points_cpu(seq, finished, lengths, NP, 10)[2].tolist() == [2, 0, 2, 5, 5, 5]
    # clip: x0 < x <= x1 and y0 < y <= y1 (collate_fn.py:80-81): the lower border is outside, the upper inside
    pts, owner, cnt, drop = WN.gather_points_cpu(seq, finished, lengths, NP, 10, clip=True)
    assert cnt.tolist() == [2, 0, 2, 4, 3, 1] and drop.tolist() == [0, 0, 0, 1, 2, 4]
    assert pts[owner == 4].tolist() == [[150, 150], [200, 200], [101, 101]]
    # ... so bin 0 is dropped under the default window: the reason clip is off by default
    assert pts[owner == 5].tolist() == [[5, 5]]
    assert inspect.signature(WN.gather_points_cpu).parameters['clip'].default is False
    assert inspect.signature(omp.OmniParser.infer).parameters['clip_windows'].default is False


def test_gather_points_clamps_the_token_range():
    seq = np.array([_row([0, 0, 9, 9], [1, 2, 3, 4], ld=10)], np.int32)
    for fin, ln, sampled, want in ((1, 99, 0, 2), (1, -3, 0, 0), (0, 0, 99, 2), (1, 2, 4, 0)):
        cnt = WN.gather_points_cpu(seq, np.array([fin]), np.array([ln]), NP, sampled)[2]
        assert cnt.tolist() == [want], (fin, ln, sampled)


def _loop(seq, finished, lengths, n_prompt, sampled, clip):
    pts, owner, cnt, drop = [], [], [], []
    for r in range(len(seq)):
        end = lengths[r] if finished[r] else n_prompt + sampled
        end = max(n_prompt, min(end, len(seq[r])))
        toks = list(seq[r][n_prompt:end])
        if len(toks) % 2:
            toks = toks[:-1]
        k = d = 0
        for x, y in zip(toks[0::2], toks[1::2]):
            if clip and not (x > seq[r][0] and x <= seq[r][2] and y > seq[r][1] and y <= seq[r][3]):
                d += 1
                continue
            pts.append([x, y])
            owner.append(r)
            k += 1
        cnt.append(k)
        drop.append(d)
    return pts, owner, cnt, drop


@pytest.mark.parametrize('seed', range(6))
def test_gather_points_equals_a_plain_loop(seed):
    rng = np.random.RandomState(seed)
    rows, ld, n_prompt = int(rng.randint(1, 40)), int(rng.randint(8, 60)), int(rng.choice([5, 7]))
    seq = rng.randint(0, 1000, size=(rows, ld)).astype(np.int32)
    x0, y0 = rng.randint(0, 600, rows), rng.randint(0, 600, rows)
    seq[:, 0], seq[:, 1], seq[:, 2], seq[:, 3] = x0, y0, x0 + rng.randint(0, 400, rows), y0 + rng.randint(0, 400, rows)
    finished = (rng.rand(rows) < (0.0, 1.0, 0.5)[seed % 3]).astype(np.int32)
    lengths = rng.randint(n_prompt, ld + 1, rows).astype(np.int32)
    sampled = int(rng.randint(0, ld - n_prompt + 1))
    for clip in (False, True):
        pts, owner, cnt, drop = WN.gather_points_cpu(seq, finished, lengths, n_prompt, sampled, clip)
        lp, lo, lc, ldr = _loop(seq.tolist(), finished.tolist(), lengths.tolist(), n_prompt, sampled, clip)
        assert pts.tolist() == lp and owner.tolist() == lo and cnt.tolist() == lc and drop.tolist() == ldr
        assert int(cnt.sum()) == pts.shape[0] == owner.shape[0]


# -- cross-attention tiles of windowed point phases -----------------------------------------------------------------------------------
@pytest.mark.parametrize('W, qt, per_image', [(1, 1, [1]), (9, 1, [9]), (17, 2, [17]), (64, 4, [64])])
def test_make_tiles_with_window_counts(W, qt, per_image):
    B = 3
    groups, q = Decoder.make_tiles([W] * B)
    assert q == qt
    # one group per image: all windows of an image share one pass over that image's keys
    assert groups == [(b * W, W, b) for b in range(B)]
    # mixed counts: rows stay sorted by image, every row in exactly one group of its own image
    counts = [W, 1, 9]
    groups, q = Decoder.make_tiles(counts)
    rows = [(r, img) for r0, n, img in groups for r in range(r0, r0 + n)]
    assert rows == [(r, b) for r, b in enumerate(b for b, n in enumerate(counts) for _ in range(n))]
    assert all(n <= 16 * q for _, n, _ in groups)


# -- routing: OmniParser.infer and predict with the engine stubbed out ---------------------------------------------------------------
@pytest.fixture
def model(monkeypatch):
    args = _args(True)
    m = omp.OmniParser(args, dict(depths=(2, 2, 2, 2)))
    seen = []

    class _Dec(object):
        def project_memory(self, memory, mem_pos, B, M, key_mask, key_len=None):
            return 'kv'

    def encode(enc, img, mask, no_padding=False):
        B = img.shape[0]
        return dict(memory=torch.zeros(B * 4, 8), mem_pos=torch.zeros(B * 4, 8), M=4, key_mask=torch.zeros(B, 4, dtype=torch.bool))

    def decode(dec_, kv, prompt, poly_sos, rec_sos, seq, fi, B, dev, side, packed=None):
        seen.append(prompt)
        return ['out'] * B
    monkeypatch.setattr(m, 'engine', lambda: ('enc', _Dec()))
    monkeypatch.setattr(m, '_encode_chunked', encode)
    monkeypatch.setattr(m, '_decode', decode)
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: contextlib.nullcontext())
    m.seen = seen
    return m


def test_infer_routes_windows_to_per_row_prompts(model):
    a = model.args
    seqs = inf.build_prompts(a)
    img, mask = torch.zeros(2, 3, 32, 32), torch.zeros(2, 32, 32, dtype=torch.bool)
    model.infer(img, mask, seqs)
    assert model.seen[-1] == seqs[0].reshape(-1).tolist()          # no windows: today's flat prompt list
    grid = WN.grid_windows(2, 2, a.num_bins)
    model.infer(img, mask, seqs, windows=grid, clip_windows=True)
    prompts, rows_per_image, clip = model.seen[-1]
    assert rows_per_image == [4, 4] and clip is True
    assert prompts.tolist() == WN.window_prompts(a, grid).tolist() * 2
    model.infer(img, mask, seqs, windows=[grid[:1], grid], char_windows=[[[0, 3]], [[1, 2]] * 4])
    prompts, rows_per_image, clip = model.seen[-1]
    assert rows_per_image == [1, 4] and clip is False
    assert prompts.tolist() == WN.window_prompts(a, grid[:1], [[0, 3]]).tolist() + WN.window_prompts(a, grid, [[1, 2]] * 4).tolist()
    with pytest.raises(ValueError):
        model.infer(img, mask, seqs, windows=grid, packed=4)
    with pytest.raises(ValueError):
        model.infer(img, mask, seqs, windows=[[0, 0, 2000, 5]])
    with pytest.raises(ValueError):
        model.infer(img, mask, seqs, windows=[[0, 0, 5, 5]] * 65)
    model.args.infer_vie = True
    try:
        with pytest.raises(ValueError):
            model.infer(img, mask, seqs, windows=grid)
    finally:
        model.args.infer_vie = False


class _Stub(torch.nn.Module):
    """infer() answering n instances per window, their point x = 10 * window + instance"""

    def __init__(self, rec_length):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.rec_length, self.calls = rec_length, []

    def infer(self, img, mask, seqs, has_padding=None, ragged=False, windows=None, char_windows=None, clip_windows=False):
        self.calls.append(dict(windows=windows, char_windows=char_windows, clip_windows=clip_windows))
        out = []
        for b in range(len(img)):
            W = 1 if windows is None else len(windows[b])
            win = torch.tensor([w for w in range(W) for _ in range(w % 2 + 1)])
            n = win.numel()
            pt = torch.stack([10 * win + torch.arange(n), torch.arange(n)], 1).reshape(1, -1)
            res = ([pt, torch.zeros(1, 32 * n, dtype=torch.long), torch.full((1, n, self.rec_length), 1000)], [torch.ones(n, self.rec_length)])
            out.append(res if windows is None else res + (win,))
        return out


def test_predict_records_gain_window_and_window_bins():
    a = _args(True)
    stub = _Stub(a.rec_length)
    imgs = torch.zeros(2, 3, 32, 32)
    plain = inf.predict(stub, imgs, a)
    assert stub.calls[-1] == dict(windows=None, char_windows=None, clip_windows=False)
    assert all('window' not in r and 'window_bins' not in r for recs in plain for r in recs)
    grid = WN.grid_windows(2, 2, a.num_bins)
    for kw in (dict(grid=(2, 2)), dict(windows=grid), dict(windows=[grid, grid])):
        recs = inf.predict(stub, imgs, a, clip_windows=True, **kw)
        assert stub.calls[-1]['windows'] == [grid, grid] and stub.calls[-1]['clip_windows'] is True
        for per in recs:
            assert [r['window'] for r in per] == [0, 1, 1, 2, 3, 3]
            assert [r['window_bins'] for r in per] == [grid[w] for w in (0, 1, 1, 2, 3, 3)]
            assert all(set(plain[0][0]) | {'window', 'window_bins'} == set(r) for r in per)
    with pytest.raises(ValueError):
        inf.predict(stub, imgs, a, windows=grid, grid=(2, 2))
    kie = _args(True, infer_vie=True, vie_categories=4, val_dataset=['sroie_val'])
    with pytest.raises(ValueError):
        inf.predict(stub, imgs, kie, grid=(2, 2))


def test_entry_points_take_the_window_arguments():
    for fn in (inf.predict, inf.predict_images, two_stage.spot_and_recognize):
        p = inspect.signature(fn).parameters
        assert p['windows'].default is None and p['char_windows'].default is None and p['grid'].default is None
        assert p['clip_windows'].default is False
    p = inspect.signature(omp.OmniParser.infer).parameters
    assert p['windows'].default is None and p['char_windows'].default is None


# -- the oracle against the fixture (needs the reference tree, as the fixture's generator does) -------------------------------------
def test_oracle_reproduces_spot_windows(golden_dir):
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip('the reference tree is not present')
    from oracle import omniparser_ref as O
    from tests.gpu_checks_windows import fixture_case
    torch.set_num_threads(8)
    gold = torch.load(os.path.join(golden_dir, 'spot_windows.pt'), weights_only=False)
    enc = None
    for name, var in gold['variants'].items():
        args, sd, img, mask, seqs = fixture_case(gold, name)
        assert WN.window_prompts(args, gold['windows'], gold['char_windows']).tolist() == gold['prompts'].tolist()
        with torch.no_grad():
            if enc is None:   # the variants differ in one bias of the point head: one encoder pass serves both
                enc = O.encode(sd, args, img, mask, gold['case']['depths'])
            for p, ref in zip(gold['prompts'], var['out']):
                pt, _ = O.decode_pt_seq(sd, args, p[None], enc['memory'], enc['mask'], enc['pos'], var['pt_seq_length'])
                assert torch.equal(pt, ref['pt'].reshape(-1)), (name, p.tolist())
                ids, probs = O.spot(sd, args, pt, seqs[1], seqs[2], enc['memory'], enc['mask'], enc['pos'])
                assert torch.equal(ids[1], ref['poly']) and torch.equal(ids[2], ref['rec'])
                assert (probs[0] - ref['rec_probs']).abs().max() < 1e-4


# -- the windowed decode's glue, with the device step replaced by its specification ------------------------------------------------
def test_decode_windows_assembles_per_image_results(monkeypatch):
    """_decode_windows with a stub decoder and ops.window_points standing on gather_points_cpu: the points reach the polygon /
    recognition phases compacted and in row order with per-image counts, every image's result concatenates its windows in window
    order, and `window` names the window of every instance"""
    from types import SimpleNamespace
    from advancedliteratemachinery_amd import ops
    a = _args(True)
    m = omp.OmniParser(a, dict(depths=(2, 2, 2, 2)))
    nP, L = 7, a.rec_length
    rows_per_image = [2, 3, 1]
    # rows: image 0 -> 2 + 0 points, image 1 -> 1 + 2 + 1 (the last row unfinished), image 2 -> none
    toks = [[11, 12, 13, 14], [], [21, 22], [31, 32, 33, 34, 35], [41, 42, 43], []]
    fin = [1, 1, 1, 1, 0, 1]
    seq = torch.zeros(6, 16, dtype=torch.int32)
    for r, t in enumerate(toks):
        seq[r, :4] = torch.tensor([0, 0, 999, 999])
        seq[r, nP:nP + len(t)] = torch.tensor(t, dtype=torch.int32)
    lengths = torch.tensor([nP + len(t) for t in toks], dtype=torch.int32)
    ph = SimpleNamespace(seq=seq, finished=torch.tensor(fin, dtype=torch.int32), lengths=lengths)
    seen = {}

    class _Dec(object):
        def decode_points(self, kv, prompts, forced_instances=None, rows_per_image=None):
            seen['prompts'], seen['rows_per_image'] = prompts, rows_per_image
            return dict(ph=ph, rows=6, n_prompt=nP, sampled=3, row_image=torch.tensor([0, 0, 1, 1, 1, 2], dtype=torch.int32))

        def decode_poly_and_rec(self, kv, points, counts, poly_sos, rec_sos, rec_length, streams=None):
            seen['points'], seen['counts'] = points.clone(), counts
            R = points.shape[0]
            poly = points[:, :1].repeat(1, 32)
            rec_ = points[:, 1:].repeat(1, rec_length)
            return (poly, None), (rec_, torch.ones(R, rec_length))

    def window_points(seq_, finished, lengths_, row_image, n_images, n_prompt, sampled, clip=False, cap=None):
        pts, owner, cnt, drop = WN.gather_points_cpu(seq_.numpy(), finished.numpy(), lengths_.numpy(), n_prompt, sampled, clip)
        start = np.concatenate([[0], np.cumsum(cnt)])
        per_img = np.bincount(row_image.numpy(), weights=cnt, minlength=n_images)
        counts = torch.from_numpy(np.concatenate([cnt, drop, start, per_img]).astype(np.int32))
        return torch.from_numpy(pts), torch.from_numpy(owner), counts
    monkeypatch.setattr(ops, 'window_points', window_points)
    prompts = torch.zeros(6, nP, dtype=torch.int64)
    out = m._decode_windows(_Dec(), 'kv', (prompts, rows_per_image, False), 1101, 1102, None, 3, 'cpu', False)
    assert seen['rows_per_image'] == rows_per_image and seen['prompts'] is prompts
    assert seen['counts'] == [2, 4, 0]
    assert seen['points'].tolist() == [[11, 12], [13, 14], [21, 22], [31, 32], [33, 34], [41, 42]]   # odd tails dropped, row order
    assert out[2] is None
    (pt, poly, rec_), (probs,), window = out[0]
    assert pt.tolist() == [[11, 12, 13, 14]] and window.tolist() == [0, 0] and tuple(poly.shape) == (1, 64) and tuple(rec_.shape) == (1, 2, L)
    (pt, poly, rec_), (probs,), window = out[1]
    assert pt.tolist() == [[21, 22, 31, 32, 33, 34, 41, 42]] and window.tolist() == [0, 1, 1, 2]
    assert tuple(probs.shape) == (4, L) and pt.dtype == torch.int64 and window.dtype == torch.int64
    # nothing decoded anywhere: every image answers None, and the next phases are not started
    ph.lengths = torch.full((6,), nP, dtype=torch.int32)
    ph.finished = torch.ones(6, dtype=torch.int32)
    seen.clear()
    assert m._decode_windows(_Dec(), 'kv', (prompts, rows_per_image, False), 1101, 1102, None, 3, 'cpu', False) == [None] * 3
    assert 'points' not in seen
