"""TEST INFRASTRUCTURE -- generate tests/golden/spot_alone.pt from the REAL reference (ragged batches).

Run where the reference tree exists:  python tools/gen_golden_alone.py
The fixture pins what a ragged engine call (OmniParser.infer(ragged=True)) must answer: the reference run on every image ALONE,
unpadded, at batch 1 on CPU fp32 (engine/val.py:22 asserts batch 1).  The images are spot_padded's two (same weights and args:
oracle.gen_golden.case_inputs, then unpad_tensors()) plus one portrait image drawn from ALONE_SEED.  spot_odd is the reference on
image 0 alone (same weights, args, seed and input draws), so its outputs must come out again here: the script asserts that.
Per image the fixture stores the greedy result `out` (ids, probs), the teacher-forced inputs with a summary of their logit rows
(tests/gpu_checks_ragged.py: logit_summary -- the full rows would make the file 1.9 MB) in `tf`, and the memory length M.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402
from oracle import ref_import  # noqa: E402
from tests.gpu_checks_ragged import logit_summary, spot_alone_inputs  # noqa: E402  (the tests rebuild the images the same way)

ALONE_SEED = 7
PORTRAIT = (203, 150)


def case():
    """spot_padded's images (its weights WEIGHT_SEED, args and image draws IMG_SEED of oracle/gen_golden.py) + one portrait image"""
    return dict(padded_case='spot_padded', weight_seed=G.WEIGHT_SEED, img_seed=G.IMG_SEED, extra_hw=PORTRAIT, extra_seed=ALONE_SEED)


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)
    return a == b


def main():
    torch.set_num_threads(8)
    c = case()
    pc = G.BIG_CASES[c['padded_case']]
    args, sd, seqs, imgs = spot_alone_inputs(c)
    model = ref_import.build_reference_model(args, sd, depths=pc['depths'], **pc.get('swin', {}))
    per = []
    for im in imgs:
        _, h, w = im.shape
        g = G._run_one(model, args, sd, pc, im[None], torch.zeros(1, h, w, dtype=torch.bool), seqs)
        per.append(dict(hw=(h, w), M=int(g['key_mask'].numel()), out=g['out'], tf=g['tf']))   # tf in full until spot_odd is checked
        print('image %dx%d  M=%d  pt=%s' % (h, w, per[-1]['M'], None if g['out'] is None else g['out']['pt'].tolist()))
    odd = torch.load(os.path.join(G.GOLDEN_DIR, 'spot_odd.pt'), weights_only=False)
    assert torch.equal(odd['fingerprint'], G.fingerprint(sd)), 'spot_odd has other weights'
    assert _same(per[0]['out'], odd['out']) and _same(per[0]['tf'], odd['tf']), 'image 0 alone differs from spot_odd'
    for im in per:   # the logit rows as summaries (tests/gpu_checks_ragged.py: logit_summary); image 0's full rows are spot_odd's
        im['tf'] = dict({k: v for k, v in im['tf'].items() if k.endswith('_in')},
                        **{k[:-len('_logits')] + '_sum': logit_summary(v) for k, v in im['tf'].items() if k.endswith('_logits')})
    gold = dict(name='spot_alone', case=dict(c, args=pc['args'], depths=pc['depths']), fingerprint=G.fingerprint(sd), images=per)
    path = os.path.join(G.GOLDEN_DIR, 'spot_alone.pt')
    torch.save(gold, path)
    print('spot_alone %.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
