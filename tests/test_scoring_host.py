"""Scoring on the host (no GPU): the hand-worked cases of the protocol, the numpy specification (utils/scoring.py) against a naive
matcher in plain Python integers, quantise / bezier_polygon / levels / text_ids / metrics, the two ground-truth readers on files written
here, score_records and evaluate_spotting end to end with a stub model and the host scorer, and the C ABI's declaration.  The kernel
and the device stage are tests/test_gpu_scoring.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from advancedliteratemachinery_amd.engine import evaluate as EV
from advancedliteratemachinery_amd.utils import ground_truth as GT
from advancedliteratemachinery_amd.utils import overlap as OV
from advancedliteratemachinery_amd.utils import scoring as SC
from advancedliteratemachinery_amd.utils.nested_tensor import NestedTensor
from advancedliteratemachinery_amd.utils.parser import make_args
from tests.scoring_cases import HAND, naive_match, pages, rect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand(name, t_iou=500, t_dc=500, scores=None, thresholds=(0.0,), report=0):
    """a hand-worked case on grid 64 (a 64 x 64 image: pixels are bins) -> match_cpu's result"""
    gt, det = HAND[name]
    polys = SC.quantise([g[0] for g in gt] + [d[0] for d in det], (64, 64), 64)
    inter = OV.pair_overlap_cpu(polys, [0, len(polys)], 64)[0]
    ids_gt, ids_det = SC.text_ids([g[1] for g in gt], [d[1] for d in det])
    level = SC.levels([0.0] * len(gt) + (list(scores) if scores is not None else [1.0] * len(det)), thresholds)
    dc = [int(g[2]) for g in gt] + [0] * len(det)
    return inter, SC.match_cpu(inter, len(gt), dc, np.concatenate([ids_gt, ids_det]), level, len(thresholds), t_iou, t_dc, report)


# -- the hand-worked cases --------------------------------------------------------------------------------------------------------------
def test_rectangle_areas_are_width_times_height():
    inter, _ = hand('B')
    assert np.diag(inter).tolist() == [100, 60, 144, 400]
    assert inter[0].tolist() == [100, 60, 100, 100]


def test_case_a_greedy_takes_the_first_detection_that_passes():
    _, (counts, det_gt, gt_det) = hand('A', t_iou=500)                      # IoU of the first detection is exactly 0.5: >= passes
    assert counts.tolist() == [[1, 2, 1, 1]] and gt_det.tolist() == [0] and det_gt.tolist() == [0, -1]
    _, (counts, det_gt, gt_det) = hand('A', t_iou=501)
    assert counts.tolist() == [[1, 2, 1, 1]] and gt_det.tolist() == [1] and det_gt.tolist() == [-1, 0]


def test_case_b_dont_care_detections():
    _, (counts, det_gt, gt_det) = hand('B')                                 # 60 of 60 and 100 of 144 samples lie in the word; 100 of 400 do not
    assert counts.tolist() == [[0, 1, 0, 0]] and det_gt.tolist() == [-2, -2, -1] and gt_det.tolist() == [-2]
    _, (counts, det_gt, _) = hand('B', t_dc=250)                            # 100 of 400 is exactly a quarter
    assert counts.tolist() == [[0, 0, 0, 0]] and det_gt.tolist() == [-2, -2, -2]
    _, (counts, det_gt, _) = hand('B', t_dc=695)                            # 100 / 144 = 0.6944...
    assert counts.tolist() == [[0, 2, 0, 0]] and det_gt.tolist() == [-2, -1, -1]


def test_case_c_greedy_order_costs_a_match():
    _, (counts, det_gt, gt_det) = hand('C')
    assert counts[0, :3].tolist() == [2, 2, 1] and gt_det.tolist() == [0, -1] and det_gt.tolist() == [0, -1]
    assert counts[0, 3] == 1                                                # 'a' met 'a'


def test_threshold_levels():
    assert SC.levels([0.1, 0.5, 0.9], [0.0, 0.5, 0.95]).tolist() == [1, 2, 2]
    gt = [(rect(40, 50, 40, 50), 'q', False)]
    HAND['L'] = (gt, [(rect(0, 5, 0, 5), 'a'), (rect(10, 15, 0, 5), 'b'), (rect(20, 25, 0, 5), 'c')])
    try:
        _, (counts, det_gt, _) = hand('L', scores=[0.1, 0.5, 0.9], thresholds=(0.0, 0.5, 0.95), report=1)
    finally:
        del HAND['L']
    assert counts[:, 1].tolist() == [3, 2, 0] and det_gt.tolist() == [-3, -1, -1]
    for bad in ([], [0.5, 0.5], [0.6, 0.5], [float('nan')], list(np.linspace(0, 1, 65))):
        with pytest.raises(ValueError):
            SC.levels([0.3], bad)
    assert SC.levels([0.3], np.linspace(0, 1, 64)).tolist() == [19]      # 0.3 * 63 = 18.9: thresholds 0 .. 18


# -- the specification against a naive matcher ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid, seed', [(64, 0), (1000, 1)])
def test_match_cpu_equals_a_naive_matcher(grid, seed):
    sizes = ((0, 0), (0, 3), (3, 0), (1, 1), (9, 14), (20, 17), (12, 30))
    n_thr = 5
    case = pages(seed, sizes, grid, n_thr)
    inter = OV.pair_overlap_cpu(case['polys'], case['group_start'], grid)
    matched = dont_care = 0
    for t_iou, t_dc, report in ((500, 500, 0), (1, 1000, n_thr - 1), (1000, 1, 2), (300, 700, -1)):
        for g, (m, nd) in enumerate(sizes):
            lo, hi = int(case['group_start'][g]), int(case['group_start'][g + 1])
            args = (inter[g], m, case['gt_dc'][lo:hi], case['text'][lo:hi], case['level'][lo:hi], n_thr, t_iou, t_dc, report)
            got, want = SC.match_cpu(*args), naive_match(*args)
            for a, b in zip(got, want):
                assert a.dtype == np.int32 and a.shape == b.shape and (a == b).all(), (g, t_iou, t_dc, report)
            matched += int(got[0][:, 2].sum())
            dont_care += int((got[1] == -2).sum())
            assert (got[0][:, 3] <= got[0][:, 2]).all() and (got[0][:, 2] <= np.minimum(got[0][:, 0], got[0][:, 1])).all()
    assert matched > 50 and dont_care > 5                                  # the pages exercise both rules


def test_match_pages_cpu_is_match_cpu_per_image():
    sizes = ((2, 3), (0, 0), (5, 4), (0, 2))
    case = pages(3, sizes, 64, 3)
    mats = OV.pair_overlap_cpu(case['polys'], case['group_start'], 64)
    flat = np.concatenate([m.reshape(-1) for m in mats])
    ist = SC.inter_layout(case['group_start'])
    counts, det_gt, gt_det = SC.match_pages_cpu(flat, ist, case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], 3, 400, 600, 1)
    assert counts.shape == (4, 3, 4) and det_gt.shape == gt_det.shape == (16,)
    for g, (m, nd) in enumerate(sizes):
        lo, hi = int(case['group_start'][g]), int(case['group_start'][g + 1])
        c, dg, gd = SC.match_cpu(mats[g], m, case['gt_dc'][lo:hi], case['text'][lo:hi], case['level'][lo:hi], 3, 400, 600, 1)
        assert (counts[g] == c).all() and (det_gt[lo + m:hi] == dg).all() and (gt_det[lo:lo + m] == gd).all()
        assert (det_gt[lo:lo + m] == SC.NOT_APPLICABLE).all() and (gt_det[lo + m:hi] == SC.NOT_APPLICABLE).all()
    _, dg, gd = SC.match_pages_cpu(flat, ist, case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], 3)
    assert (dg == SC.NOT_APPLICABLE).all() and (gd == SC.NOT_APPLICABLE).all()
    host = SC.HostScorer(64).run(case['polys'], case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], 3, 400, 600, 1)
    assert (host['counts'] == counts).all() and (host['det_gt'] == det_gt).all() and (host['gt_det'] == gt_det).all()
    for bad in (dict(n_thr=0), dict(n_thr=65), dict(t_iou=0), dict(t_dc=1001), dict(report=3), dict(report=-2)):
        kw = dict(n_thr=3, t_iou=500, t_dc=500, report=-1)
        kw.update(bad)
        with pytest.raises(ValueError):
            SC.match_pages_cpu(flat, ist, case['group_start'], case['n_gt'], case['gt_dc'], case['text'], case['level'], **kw)
    with pytest.raises(ValueError):
        SC.match_pages_cpu(flat, ist, case['group_start'], [2, 0, 10, 0], case['gt_dc'], case['text'], case['level'], 3)


def test_chunk_groups():
    gs = np.concatenate([[0], np.cumsum([3, 0, 4, 2, 5, 1])])
    assert SC.chunk_groups(gs, 1 << 20) == [(0, 6)]
    assert SC.chunk_groups(gs, 25) == [(0, 3), (3, 4), (4, 5), (5, 6)]      # 9 + 0 + 16 | 4 | 25 | 1
    for cap in (25, 29, 30, 55):
        parts = SC.chunk_groups(gs, cap)
        assert parts[0][0] == 0 and parts[-1][1] == 6 and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        assert all(sum(int(s) ** 2 for s in np.diff(gs)[a:b]) <= cap for a, b in parts)
    with pytest.raises(ValueError, match='exceeds'):
        SC.chunk_groups(gs, 24)
    assert SC.chunk_groups([0]) == []


# -- quantise, bezier_polygon, text_ids, metrics ----------------------------------------------------------------------------------------
def test_quantise_clips_pads_and_refuses():
    q = SC.quantise([[[-5, 10], [199.9, 10], [200, 99.9], [400, 250]]], (100, 200), 50)
    assert q.dtype == np.int32 and q.shape == (1, 32)
    assert q[0, :8].tolist() == [0, 5, 49, 5, 49, 49, 49, 49]              # clipped on both sides; floor(199.9 * 50 / 200) = 49
    assert (q[0, 8:].reshape(-1, 2) == q[0, 6:8]).all()                     # padded with the last vertex
    assert SC.quantise([], (10, 10), 64).shape == (0, 32)
    full = [[k, 2 * k] for k in range(16)]
    assert SC.quantise([full], (64, 64), 64)[0].tolist() == [v for k in range(16) for v in (k, 2 * k)]
    for polys, size, bins in (([full + [[1, 1]]], (64, 64), 64), ([full[:2]], (64, 64), 64), ([full], (64, 64), 1), ([full], (64, 64), OV.GRID_MAX + 1),
                              ([full], (0, 64), 64), ([[[0, 0], [1, float('nan')], [2, 2]]], (64, 64), 64)):
        with pytest.raises(ValueError):
            SC.quantise(polys, size, bins)
    assert SC.quantise([full], (64, 64), OV.GRID_MAX).max() == 30 * OV.GRID_MAX // 64


def test_bezier_polygon_on_straight_lines():
    top = np.linspace([10.0, 20.0], [80.0, 41.0], 4)                        # control points on a line, equally spaced: the curve is the line
    bottom = np.linspace([80.0, 60.0], [10.0, 39.0], 4)
    p = SC.bezier_polygon(np.concatenate([top.reshape(-1), bottom.reshape(-1)]))
    assert p.shape == (16, 2) and p.dtype == np.float64
    np.testing.assert_allclose(p[:8], np.linspace([10.0, 20.0], [80.0, 41.0], 8), rtol=0, atol=1e-12)
    np.testing.assert_allclose(p[8:], np.linspace([80.0, 60.0], [10.0, 39.0], 8), rtol=0, atol=1e-12)
    curved = SC.bezier_polygon([0, 0, 0, 30, 30, 30, 30, 0] + [0] * 8)      # B(1/2) = (P0 + 3 P1 + 3 P2 + P3) / 8; 1/2 is not sampled, 3/7 is
    t = 3.0 / 7.0
    want = 3 * t * (1 - t) ** 2 * np.array([0, 30.0]) + 3 * t * t * (1 - t) * np.array([30.0, 30.0]) + t ** 3 * np.array([30.0, 0])
    np.testing.assert_allclose(curved[3], want, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        SC.bezier_polygon([0.0] * 15)


def test_text_ids():
    a, b = SC.text_ids(['Word', 'STRASSE', 'x'], ['word', 'straße', 'y', 'X'])
    assert a.dtype == b.dtype == np.int32
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[3] and b[2] not in a.tolist()       # casefold: ß == ss
    a, b = SC.text_ids(['Word'], ['word'], normalise=None)
    assert a[0] != b[0]
    a, b = SC.text_ids(['a-b'], ['ab'], normalise=lambda s: s.replace('-', ''))
    assert a[0] == b[0]


def test_metrics_zero_over_zero_and_the_tie_rule():
    m = SC.metrics([[0, 0, 0, 0], [4, 0, 0, 0], [0, 5, 0, 0], [4, 8, 2, 1], [4, 2, 2, 1], [2, 4, 2, 0]])
    assert m['det']['precision'] == [0.0, 0.0, 0.0, 0.25, 1.0, 0.5] and m['det']['recall'] == [0.0, 0.0, 0.0, 0.5, 0.5, 1.0]
    assert m['det']['hmean'][:3] == [0.0, 0.0, 0.0] and m['det']['hmean'][3] == pytest.approx(1 / 3)
    assert m['det']['hmean'][4] == m['det']['hmean'][5] == pytest.approx(2 / 3) and m['det']['best'] == 4     # the tie goes to the lower index
    assert m['e2e']['precision'][3:] == [0.125, 0.5, 0.0] and m['e2e']['best'] == 4
    assert all(isinstance(v, float) for v in m['det']['hmean'])
    assert SC.metrics([[0, 0, 0, 0]])['det']['best'] == 0


# -- the readers ------------------------------------------------------------------------------------------------------------------------
def test_load_coco_bezier(tmp_path):
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    nc = len(args.chars)

    def rec(word, unknown_at=None):
        ids = [args.chars.index(c) for c in word]
        if unknown_at is not None:
            ids.insert(unknown_at, nc)
        return ids + [nc + 1] * (args.rec_length - len(ids))
    bez = [10, 10, 20, 10, 30, 10, 40, 10, 40, 20, 30, 20, 20, 20, 10, 20]
    doc = dict(images=[dict(id=7, file_name='b.jpg', height=100, width=200), dict(id=3, file_name='a.jpg', height=50, width=60),
                       dict(id=9, file_name='empty.jpg', height=5, width=6)],
               annotations=[dict(id=1, image_id=3, bezier_pts=bez, rec=rec('Hello'), iscrowd=0),
                            dict(id=2, image_id=7, bezier_pts=bez, rec=rec('crowd'), iscrowd=1),
                            dict(id=3, image_id=7, bezier_pts=bez, rec=rec('caf', unknown_at=3), iscrowd=0),
                            dict(id=4, image_id=7, bezier_pts=bez, rec=rec('a' * args.rec_length))])
    path = tmp_path / 'anno.json'
    path.write_text(json.dumps(doc))
    images, gt = GT.load_coco_bezier(str(path), args)
    assert [im['file_name'] for im in images] == ['b.jpg', 'a.jpg', 'empty.jpg'] and (images[0]['height'], images[0]['width']) == (100, 200)
    assert [[w['text'] for w in words] for words in gt] == [['crowd', 'caf', 'a' * args.rec_length], ['Hello'], []]
    assert [[w['dc'] for w in words] for words in gt] == [[True, True, False], [False], []]
    assert gt[0][1]['dc'] and not GT.load_coco_bezier(str(path), args, dc_unknown=False)[1][0][1]['dc']
    np.testing.assert_allclose(gt[1][0]['poly'], SC.bezier_polygon(bez), rtol=0, atol=0)
    np.testing.assert_allclose(np.asarray(gt[1][0]['poly'])[[0, 7, 8, 15]], [[10, 10], [40, 10], [40, 20], [10, 20]], rtol=0, atol=1e-12)
    doc['annotations'][0]['rec'] = doc['annotations'][0]['rec'][:-1]
    path.write_text(json.dumps(doc))
    with pytest.raises(ValueError, match='rec_length'):
        GT.load_coco_bezier(str(path), args)


def test_load_icdar_txt(tmp_path):
    path = tmp_path / 'gt_img_1.txt'
    path.write_text('\ufeff10,10,50,10,50,30,10,30,Hello\n'
                    '1,2,3,4,5,6,7,8,###\n'
                    '\n'
                    '1,2,3,4,5,6,7,8,1,000\n'
                    '1,2,3,4,5,6,7,8,2019\n'
                    '0,0,9.5,0,9.5,9,5,12,0,9,five, with a comma\n', encoding='utf-8')
    words = GT.load_icdar_txt(str(path))
    assert [w['text'] for w in words] == ['Hello', '###', '1,000', '2019', 'five, with a comma']
    assert [w['dc'] for w in words] == [False, True, False, False, False]
    assert words[0]['poly'] == [[10.0, 10.0], [50.0, 10.0], [50.0, 30.0], [10.0, 30.0]] and len(words[4]['poly']) == 5
    assert [w['text'] for w in GT.load_icdar_txt(str(path), points=4)[:4]] == ['Hello', '###', '1,000', '2019']
    assert GT.load_icdar_dir(str(tmp_path), ['some/dir/img_1.jpg'])[0] == words
    with pytest.raises(FileNotFoundError):
        GT.load_icdar_dir(str(tmp_path), ['img_2.jpg'])
    bad = tmp_path / 'bad.txt'
    bad.write_text('1,2,3,4,word\n')
    with pytest.raises(ValueError, match='bad.txt:1'):
        GT.load_icdar_txt(str(bad))


# -- score_records and evaluate_spotting with a stub model and the host scorer ----------------------------------------------------------
class _Stub(torch.nn.Module):
    """infer() answering n words per image on a loose grid of the page, in bins; score and text vary with the word"""

    def __init__(self, args, n=7):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.args, self.n, self.calls = args, n, []

    def infer(self, img, mask, seqs, has_padding=None, ragged=False, windows=None, char_windows=None, clip_windows=False):
        a, n = self.args, self.n
        self.calls.append(len(img))
        out = []
        for b in range(len(img)):
            polys, pts = [], []
            for k in range(n):
                x0, y0 = 60 + 300 * (k % 3), 80 + 250 * (k // 3)
                top = np.linspace(x0, x0 + 210, 8)
                polys.append([v for x in top for v in (x, y0)] + [v for x in top[::-1] for v in (x, y0 + 60)])
                pts += [x0 + 100, y0 + 30]
            rec = torch.full((1, n, a.rec_length), a.recog_pad_index)
            for k in range(n):
                rec[0, k, :3] = torch.tensor([a.num_bins + a.chars.index('a') + (k + j) % 20 for j in range(3)])
                rec[0, k, 3] = a.rec_eos_index
            probs = torch.tensor([0.3 + 0.1 * (k % 7) for k in range(n)])[:, None].repeat(1, a.rec_length)
            out.append(([torch.tensor(pts).reshape(1, -1), torch.tensor(polys, dtype=torch.float64).round().long().reshape(1, -1), rec], [probs]))
        return out


class _Pre(object):
    def __call__(self, images):
        return NestedTensor(torch.zeros(len(images), 3, 32, 32), torch.zeros(len(images), 32, 32, dtype=torch.bool)), None


SIZES_HW = ((100, 200), (90, 64), (300, 300), (50, 70), (64, 64))


@pytest.fixture
def engine():
    a = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    rng = np.random.RandomState(1)
    return a, _Stub(a), [torch.from_numpy(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in SIZES_HW]


def _truth(records, drop=None):
    return [[dict(poly=r['polys'], text=r['rec'].upper(), dc=False) for k, r in enumerate(recs) if drop is None or k % drop != drop - 1] for recs in records]


def test_score_records_perfect_and_with_dropped_ground_truth(engine):
    from advancedliteratemachinery_amd.engine import inference as inf
    a, model, images = engine
    records, _ = inf.predict_images(model, images, a, preprocessor=_Pre())
    assert [len(r) for r in records] == [7] * 5 and len(records[0][0]['polys']) == 16
    host = SC.HostScorer(a.num_bins)
    res = EV.score_records(records, _truth(records), SIZES_HW, a.num_bins, scorer=host, report=0)
    assert res['counts'].shape == (5, 1, 4) and res['total'].tolist() == [[35, 35, 35, 35]]
    for kind in ('det', 'e2e'):
        assert res[kind]['precision'] == res[kind]['recall'] == res[kind]['hmean'] == [1.0]
    assert res['best'] == dict(det=0, e2e=0) and res['thresholds'] == [0.0]
    assert res['matches'] == [list(range(7))] * 5
    assert all(r['gt'] == k and r['gt_text'] == r['rec'].upper() for recs in records for k, r in enumerate(recs))
    # every third ground-truth word dropped: recall stays, precision falls
    res = EV.score_records(records, _truth(records, drop=3), SIZES_HW, a.num_bins, scorer=host)
    assert res['total'].tolist() == [[25, 35, 25, 25]] and res['matches'] is None
    assert res['det']['recall'] == [1.0] and res['det']['precision'] == [25 / 35] and res['e2e']['hmean'] == [pytest.approx(2 * 25 / 60)]
    # case matters without casefold; another text costs end-to-end matches only
    res = EV.score_records(records, _truth(records), SIZES_HW, a.num_bins, scorer=host, normalise=None)
    assert res['total'].tolist() == [[35, 35, 35, 0]]
    # a sweep: scores are 0.3 .. 0.9 in steps of 0.1, one word each per image
    res = EV.score_records(records, _truth(records), SIZES_HW, a.num_bins, scorer=host, thresholds=(0.0, 0.55, 0.95))
    assert res['total'][:, 1].tolist() == [35, 20, 0] and res['total'][:, 2].tolist() == [35, 20, 0] and res['best']['det'] == 0
    assert res['det']['hmean'][2] == 0.0
    # min_len, don't-care flags, the lexicon key with its fallback
    truth = _truth(records)
    truth[0][0]['text'] = 'ab'
    truth[1][1]['dc'] = True
    res = EV.score_records(records, truth, SIZES_HW, a.num_bins, scorer=host, min_len=3, report=0)
    assert res['total'].tolist() == [[33, 33, 33, 33]] and records[0][0]['gt'] == -2 and records[1][1]['gt'] == -2 and res['matches'][0][0] == -2
    for recs in records:
        for k, r in enumerate(recs):
            r['lex'] = None if k % 2 else 'zzz'
    res = EV.score_records(records, _truth(records), SIZES_HW, a.num_bins, scorer=host, text_key='lex')
    assert res['total'].tolist() == [[35, 35, 35, 15]]                        # None falls back to `rec`
    with pytest.raises(ValueError, match='text_key'):
        EV.score_records(records, truth, SIZES_HW, a.num_bins, scorer=host, text_key='nope')
    with pytest.raises(KeyError):
        EV.score_records(records, truth, SIZES_HW, a.num_bins, scorer=host, text_key='mgp_text')
    for bad in (dict(iou=0.0), dict(dc_overlap=1.5), dict(report=1), dict(thresholds=(0.5, 0.4))):
        with pytest.raises(ValueError):
            EV.score_records(records, truth, SIZES_HW, a.num_bins, scorer=host, **bad)
    with pytest.raises(ValueError, match='per image'):
        EV.score_records(records[:2], truth, SIZES_HW, a.num_bins, scorer=host)
    with pytest.raises(RuntimeError, match='MI355X'):
        SC.SpottingScorer('cpu', a.num_bins)                                  # there is no CPU stage
    empty = EV.score_records([[], []], [[], truth[0]], SIZES_HW[:2], a.num_bins, scorer=host, report=0)
    assert empty['total'].tolist() == [[7, 0, 0, 0]] and empty['det']['hmean'] == [0.0] and empty['matches'] == [[], [-1] * 7]


def test_evaluate_spotting_runs_in_batches_and_sums_the_counts(engine):
    from advancedliteratemachinery_amd.engine import inference as inf
    a, model, images = engine
    records, _ = inf.predict_images(model, images, a, preprocessor=_Pre())
    truth = _truth(records, drop=3)
    model.calls = []
    host = SC.HostScorer(a.num_bins)
    res = EV.evaluate_spotting(model, images, truth, a, batch=2, preprocessor=_Pre(), scorer=host, thresholds=(0.0, 0.55), report=1)
    assert model.calls == [2, 2, 1]
    whole = EV.score_records(records, truth, SIZES_HW, a.num_bins, scorer=host, thresholds=(0.0, 0.55), report=1)
    assert (res['counts'] == whole['counts']).all() and (res['total'] == whole['total']).all() and res['best'] == whole['best']
    assert res['matches'] == whole['matches'] and res['det'] == whole['det'] and res['e2e'] == whole['e2e']
    assert res['records'] == records and all('gt' in r for recs in res['records'] for r in recs)
    assert res['total'][0].tolist() == [25, 35, 25, 25] and res['total'][1, 1] == 20
    # stage arguments reach the engine call
    seen = {}
    real = inf.predict_images

    def spy(model, imgs, args, **kw):
        seen.update(kw)
        return real(model, imgs, args, **{k: v for k, v in kw.items() if k in ('preprocessor', 'ragged', 'file_names')})
    inf.predict_images, keep = spy, inf.predict_images
    try:
        EV.evaluate_spotting(model, images[:1], truth[:1], a, preprocessor=_Pre(), scorer=host, ragged=True, suppress=0.5, grid=(2, 2), lexicon=['a'])
    finally:
        inf.predict_images = keep
    assert seen['ragged'] is True and seen['suppress'] == 0.5 and seen['grid'] == (2, 2) and seen['lexicon'] == ['a'] and 'scorer' not in seen
    kie = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    kie.infer_vie = True
    with pytest.raises(ValueError, match='infer_vie'):
        EV.evaluate_spotting(model, images, truth, kie, scorer=host)
    with pytest.raises(ValueError, match='mgp='):
        EV.evaluate_spotting(model, images, truth, a, scorer=host, text_key='mgp_text')
    with pytest.raises(ValueError):
        EV.evaluate_spotting(model, images[:2], truth, a, scorer=host)


# -- the command line ---------------------------------------------------------------------------------------------------------------
def test_eval_spotting_scores_a_results_file(tmp_path, capsys, engine):
    import sys
    from advancedliteratemachinery_amd.engine import inference as inf
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import eval_spotting
    assert eval_spotting.parse_thresholds('0:0') == [0.0] and eval_spotting.parse_thresholds('0.5') == [0.5]
    assert eval_spotting.parse_thresholds('0.1:0.9:0.2') == [0.1, 0.3, 0.5, 0.7, 0.9] and len(eval_spotting.parse_thresholds('0:1:0.05')) == 21
    a, model, images = engine
    names = ['img_%d.jpg' % k for k in range(len(images))]
    records, _ = inf.predict_images(model, images, a, file_names=names, preprocessor=_Pre())
    (tmp_path / 'results.json').write_text(json.dumps([r for recs in records for r in recs], indent=4))      # as validate writes it
    nc = len(a.chars)
    anno = dict(images=[dict(id=k, file_name=n, height=h, width=w) for k, (n, (h, w)) in enumerate(zip(names, SIZES_HW))], annotations=[])
    for k, recs in enumerate(records):
        for j, r in enumerate(recs):
            if j % 3 == 2:
                continue
            p = np.asarray(r['polys'])
            ctrl = np.concatenate([np.linspace(p[0], p[7], 4), np.linspace(p[8], p[15], 4)]).reshape(-1)
            ids = [a.chars.index(c) for c in r['rec']]
            anno['annotations'].append(dict(id=len(anno['annotations']), image_id=k, bezier_pts=ctrl.tolist(), iscrowd=int(j == 0),
                                            rec=ids + [nc + 1] * (a.rec_length - len(ids))))
    (tmp_path / 'anno.json').write_text(json.dumps(anno))
    doc = eval_spotting.main(['--results', str(tmp_path / 'results.json'), '--anno', str(tmp_path / 'anno.json'), '--thresholds', '0:0.9:0.3',
                              '--tfm_pre_norm', '--use_fpn', '--use_char_window_prompt'], scorer=SC.HostScorer(a.num_bins))
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(doc))
    assert doc['thresholds'] == [0.0, 0.3, 0.6, 0.9] and doc['images'] == 5 and doc['records'] == 35 and doc['bins'] == a.num_bins
    assert doc['total'][0] == [20, 30, 20, 20]                              # 5 words per image, the first don't-care and so is its detection
    assert doc['det']['recall'][0] == 1.0 and doc['det']['precision'][0] == pytest.approx(2 / 3) and doc['best']['det'] == 0
    assert doc['best_threshold']['det'] == 0.0 and doc['best_hmean']['e2e'] == pytest.approx(0.8)
    assert 'not been checked' in doc['note']


# -- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_entry_point_matches_the_header():
    from advancedliteratemachinery_amd import _lib, build, ops
    text = open(os.path.join(ROOT, 'include', 'omp355.h')).read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24   # the library only gains an entry point
    m = re.search(r'int omp_spotting_match\((.*?)\);', text, re.S)
    want = []
    for p in (' '.join(p.split()) for p in m.group(1).split(',')):
        if '*' in p or p.startswith('omp_stream_t'):
            want.append(ctypes.c_void_p)
        else:
            assert p.startswith('int '), p
            want.append(ctypes.c_int)
    res, args = _lib._SIGS['omp_spotting_match']
    assert res is ctypes.c_int and args == want and len(want) == 17 and 'omp_spotting_match' in _lib.EXPORTS
    assert 'score.hip' in build.SOURCES and callable(ops.spotting_match) and callable(ops.split_match_ints)
    src = open(os.path.join(ROOT, 'advancedliteratemachinery_amd', 'csrc', 'score.hip')).read()
    assert 'extern "C" int omp_spotting_match(' in src
    assert 'SC_MAX_GROUP = %d' % SC.GROUP_MAX in src and 'SC_MAX_THR = %d' % SC.T_MAX in src and SC.GROUP_MAX == OV.GROUP_MAX
    assert 'SC_NA = %d' % SC.NOT_APPLICABLE in src
    assert 'row_thresholds' not in src and 'sort16' not in src             # the intersections are omp_polygon_overlap's, not a copy
