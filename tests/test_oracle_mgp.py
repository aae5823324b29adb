"""MGP-STR oracle (oracle/mgp_str_ref.py) pinned to the reference: golden fixture and what the reference's own code computed
on a fresh case (tests/golden/reference_pins_mgp.pt); host-side pieces of the MGP-STR engine that need no GPU."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import gen_golden_mgp as G
from oracle import mgp_str_ref as R
from oracle import gen_golden_pins as P


def _close(a, b, tol):
    return (a - b).abs().max().item() <= tol


def test_oracle_matches_reference_fixture(golden_dir):
    fix = torch.load(os.path.join(golden_dir, 'mgp_str_base.pt'), weights_only=False)
    c, ref = fix['cfg'], fix['ref']
    sd = R.make_state_dict(c, seed=fix['seed_w'])
    with torch.no_grad():
        x = R.encoder(sd, c, fix['img'])
        attens, (ch, bp, wp) = R.heads(sd, c, x)
    got = G.reduce_outputs(x, attens, ch, bp, wp)
    assert _close(got['enc_proj'], ref['enc_proj'], 2e-4)
    for a, b in zip(got['attens'], ref['attens']):
        assert _close(a, b, 1e-5)
    assert _close(got['char'], ref['char'], 1e-3)
    assert _close(got['bpe_sub'], ref['bpe_sub'], 1e-3) and _close(got['wp_sub'], ref['wp_sub'], 1e-3)
    for name in ('char', 'bpe', 'wp'):
        assert torch.equal(got[name + '_ids'], ref[name + '_ids'])
        assert _close(got[name + '_prob'], ref[name + '_prob'], 1e-4)


def test_fresh_case_against_reference_code(golden_dir):
    """different depth / seed than the fixture, against what the reference's MGPSTR.forward and the REAL TokenLearner computed on
    the same inputs (tests/golden/reference_pins_mgp.pt, oracle/gen_golden_pins.py); both sides in float64, so that the gates
    measure the restatement and not the host's fp32 rounding"""
    c, sd, img, x = P.mgp_fresh_case()
    ref = {k: ([t.double() for t in v] if isinstance(v, list) else v.double())
           for k, v in torch.load(os.path.join(golden_dir, 'reference_pins_mgp.pt'), weights_only=False)['mgp_fresh'].items()}
    # the wide heads are the reference's nn.Linear on the inputs it recorded (their logits are too large to store)
    ref_out = [ref['attens'], ref['char']] + [F.linear(ref[n + '_head_in'], sd['mgp_str.%s_head.weight' % n], sd['mgp_str.%s_head.bias' % n])
                                             for n in ('bpe', 'wp')]
    with torch.no_grad():
        mine = R.forward(sd, c, img)
        # the A^3 restatement against the reference class alone, on an arbitrary token tensor
        sel, out = R.token_learner(sd, c, x, 'bpe')
    assert len(ref_out[0]) == len(mine[0]) == 3 and ref_out[1].shape[0] == img.shape[0] and mine[1].dtype == torch.float64
    for a, b in zip(ref_out[0], mine[0]):
        assert _close(a, b, 1e-6)
    for a, b in zip(ref_out[1:], mine[1:]):
        assert a.shape == b.shape and _close(a, b, 1e-4)
    assert _close(sel, ref['sel'], 1e-6) and _close(out, ref['tl_out'], 1e-5)


def _crafted_logits(ids_rows, V, hi=9.0):
    """logits whose greedy ids are `ids_rows` ([B, 27]) with a clear margin"""
    B, S = len(ids_rows), len(ids_rows[0])
    lg = torch.randn(B, S, V, generator=torch.Generator().manual_seed(V)) * 0.3
    for b in range(B):
        for s in range(S):
            lg[b, s, ids_rows[b][s]] = hi - 0.1 * s
    return lg


def test_decode_confidence_and_fusion():
    """test_final.py:172-240 restated: EOS handling of each granularity, empty-prefix -> 0.0, strict-> fusion order"""
    S = 27
    # sample 0: char 'ab' then [s]; bpe EOS (2) at position 3; wp has no EOS (102)
    # sample 1: char has no [s] at all; bpe EOS first; wp EOS at position 1
    char = [[0] + [12, 13, 1] + [5] * (S - 4), [0] + [7] * (S - 1)]
    bpe = [[0] + [500, 600, 2] + [9] * (S - 4), [0] + [2] + [9] * (S - 2)]
    wp = [[0] + [300] * (S - 1), [0] + [102] + [8] * (S - 2)]
    ch, bp, wp_l = _crafted_logits(char, 38), _crafted_logits(bpe, 700), _crafted_logits(wp, 400)
    res = R.decode(ch, bp, wp_l)
    pc = F.softmax(ch, dim=2).max(dim=2)[0][:, 1:]
    pb = F.softmax(bp, dim=2).max(dim=2)[0][:, 1:]
    pw = F.softmax(wp_l, dim=2).max(dim=2)[0][:, 1:]
    assert res[0]['char_text'] == 'ab'
    assert abs(res[0]['conf'][0] - float(pc[0, :3].prod())) < 1e-6
    assert abs(res[0]['conf'][1] - float(pb[0, :3].prod())) < 1e-6
    assert res[0]['conf'][2] == 0.0
    assert res[0]['choice'] == (0 if res[0]['conf'][0] >= res[0]['conf'][1] else 1)
    assert res[1]['conf'][0] == 0.0 and res[1]['char_text'] == (R.CHAR_TABLE[7] * 26)[:-1]   # no [s]: s[:-1], test_final.py:178
    assert abs(res[1]['conf'][1] - float(pb[1, 0])) < 1e-6
    assert abs(res[1]['conf'][2] - float(pw[1, 0])) < 1e-6
    assert res[1]['choice'] in (1, 2)
    # the engine's host-side decode (model/mgp_str.py) is the same function of (ids, probs)
    from advancedliteratemachinery_amd.model import mgp_str as M
    ids = [lg.argmax(-1)[:, 1:] for lg in (ch, bp, wp_l)]
    probs = [pc, pb, pw]
    mine = M.decode_ids(ids, probs)
    for a, b in zip(mine, res):
        assert a['char_ids'] == b['char_ids'] and a['bpe_ids'] == b['bpe_ids'] and a['wp_ids'] == b['wp_ids']
        assert a['char_text'] == b['char_text'] and a['choice'] == b['choice']
        assert max(abs(x - y) for x, y in zip(a['conf'], b['conf'])) < 1e-6


def test_state_dict_layout_and_grouped_conv_expansion():
    from advancedliteratemachinery_amd.model import mgp_str as M
    c = R.cfg(depth=2)
    sd = R.make_state_dict(c, seed=3)
    spec = M.expected_state_dict(dict(M.BASE_CFG, depth=2))
    assert set(spec) == set(sd)
    for k, shape in spec.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    model = M.MGPSTR(dict(depth=2), engine_dtype='fp32')
    model.load_reference_state_dict({'module.' + k: v for k, v in sd.items()})
    back = model.state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    # grouped 1x1 conv == dense GEMM with the block-diagonal expansion
    w = sd['mgp_str.char_tokenLearner.feat.weight']
    x = torch.randn(5, 768, generator=torch.Generator().manual_seed(1))
    ref = F.conv2d(x.t().reshape(1, 768, 5, 1), w, groups=8).reshape(768, 5).t()
    assert _close(x @ M._grouped_to_dense(w).t(), ref, 1e-5)
    # no CPU fallback
    with pytest.raises(RuntimeError):
        model(torch.zeros(1, 3, 32, 128))
