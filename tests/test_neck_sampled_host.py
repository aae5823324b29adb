"""Host logic of the sampled encoder neck (model/backbone.py Encoder.neck_sampled, the two entry points' bindings): no GPU."""
import ctypes
import os
import re
import types

import torch

from advancedliteratemachinery_amd import _lib
from advancedliteratemachinery_amd.model.backbone import Encoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def level_chain(H, W):
    """the four level sizes of an H x W image: the 4x4 patch embedding, then PatchMerging halves with ceil"""
    s = [(-(-H // 4), -(-W // 4))]
    for _ in range(3):
        s.append((-(-s[-1][0] // 2), -(-s[-1][1] // 2)))
    return s


def _enc(**kw):
    return types.SimpleNamespace(**dict(dict(use_fpn=True, dtype=torch.bfloat16, x3=False), **kw))


def test_neck_sampled_is_the_regular_geometry():
    """sampled exactly where h2 == 2 h3 == 4 h4 and the widths alike; then the stride-2 grid is the stage-2 grid"""
    n = 0
    for H in range(1, 200):
        for W in (H, 1, 64, 75, 160, 333):
            (h2, w2), (h3, w3), (h4, w4), _ = level_chain(H, W)
            regular = h2 == 2 * h3 == 4 * h4 and w2 == 2 * w3 == 4 * w4
            assert Encoder.neck_sampled(_enc(), H, W) == regular, (H, W)
            if regular:
                assert (-(-h3 // 2), -(-w3 // 2)) == (h4, w4)
                n += 1
    assert n > 0
    for side in (32, 640, 1024):
        assert Encoder.neck_sampled(_enc(), side, side)
    assert Encoder.neck_sampled(_enc(), 960, 1280) and not Encoder.neck_sampled(_enc(), 72, 104)


def test_neck_sampled_engines():
    """the bf16 engine with the FPN only"""
    assert not Encoder.neck_sampled(_enc(use_fpn=False), 64, 64)
    assert not Encoder.neck_sampled(_enc(dtype=torch.float32), 64, 64)
    assert not Encoder.neck_sampled(_enc(dtype=torch.float32, x3=True), 64, 64)


def test_bindings_and_abi():
    with open(os.path.join(ROOT, 'include', 'omp355.h')) as f:
        text = f.read()
    assert int(re.search(r'#define OMP_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 24   # the library only gains entry points
    p, i, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = {'omp_layernorm_sampled': [p, i, p, p, p, i, i, i, i, i, i, i, fl, p],
            'omp_fpn_fuse_sampled': [p, p, p, p, p] + [i] * 10 + [p]}
    for name, args in want.items():
        res, got = _lib._SIGS[name]
        assert res is ctypes.c_int and got == args and name in _lib.EXPORTS
        proto = re.search(r'int %s\(([^;]*)\);' % name, text).group(1)
        assert len(proto.split(',')) == len(args), name
