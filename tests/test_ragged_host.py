"""Ragged batches on the host (no GPU): the extent of every image of a padded batch, the size buckets, the ragged memory layout, how
OmniParser.infer(ragged=True) routes and places each image's memory rows, and validate(ragged=True) handing the model unpadded images.
The kernels and the end-to-end answers are tests/test_gpu_ragged.py."""
import contextlib
import json
import os

import pytest
import torch

from advancedliteratemachinery_amd.engine import inference as inf
from advancedliteratemachinery_amd.model import omniparser as omp
from advancedliteratemachinery_amd.utils.nested_tensor import nested_tensor_from_tensor_list
from advancedliteratemachinery_amd.utils.parser import make_args

SIZES = [(32, 48), (48, 32), (32, 48), (40, 40), (48, 32)]


def _images(sizes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(3, h, w, generator=g) for h, w in sizes]


def test_mask_extents_of_a_collated_batch():
    nt = nested_tensor_from_tensor_list(_images(SIZES))
    assert omp.mask_extents(nt.mask) == SIZES
    assert omp.mask_extents(torch.zeros(2, 5, 7, dtype=torch.bool)) == [(5, 7), (5, 7)]


def test_mask_extents_refuses_what_it_cannot_read():
    m = nested_tensor_from_tensor_list(_images(SIZES[:2])).mask.clone()
    m[0, 3, 4] = True                         # a hole inside the image
    with pytest.raises(ValueError):
        omp.mask_extents(m)
    m = torch.ones(1, 4, 4, dtype=torch.bool)
    m[0, 2:, 2:] = False                      # image at the bottom right
    with pytest.raises(ValueError):
        omp.mask_extents(m)
    with pytest.raises(ValueError):
        omp.mask_extents(torch.ones(1, 4, 4, dtype=torch.bool))   # no image at all


def test_bucket_by_size():
    assert omp.bucket_by_size(SIZES) == [((32, 48), [0, 2]), ((48, 32), [1, 4]), ((40, 40), [3])]
    assert omp.bucket_by_size([(8, 8)] * 3) == [((8, 8), [0, 1, 2])]


def test_ragged_layout():
    Mmax, key_len, row0 = omp.ragged_layout([2700, 2700, 1300, 64, 1])
    assert Mmax == 2752 and Mmax % 64 == 0
    assert key_len == [2700, 2700, 1300, 64, 1]
    assert row0 == [0, 2752, 5504, 8256, 11008]
    assert omp.ragged_layout([64, 128])[0] == 128


# -- OmniParser.infer routing, with the engine stubbed out -------------------------------------------------------------------------
D = 8


def _m_of(h, w):
    return (h // 8) * (w // 8)


class _Dec(object):
    def __init__(self):
        self.calls = []

    def project_memory(self, memory, mem_pos, B, M, key_mask, key_len=None):
        self.calls.append(dict(memory=memory.clone(), mem_pos=mem_pos.clone(), B=B, M=M, key_mask=key_mask, key_len=key_len))
        return 'kv'


@pytest.fixture
def model(monkeypatch):
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    m = omp.OmniParser(args, dict(depths=(2, 2, 2, 2)))
    dec = _Dec()
    enc_calls = []

    def encode(enc, img, mask, no_padding=False):
        enc_calls.append(dict(shape=tuple(img.shape), padded=bool(mask.any()), no_padding=no_padding))
        B, _, h, w = img.shape
        M = _m_of(h, w)
        # memory row of image b, key k = (image content, k): placement errors show up as wrong values
        key = img.reshape(B, -1).sum(1)
        mem = key[:, None, None] + torch.arange(M, dtype=torch.float32)[None, :, None] * 1000 + torch.zeros(1, 1, D)
        return dict(memory=mem.reshape(B * M, D), mem_pos=-mem.reshape(B * M, D), M=M, key_mask=mask[:, :1, :M].reshape(B, -1))

    monkeypatch.setattr(m, 'engine', lambda: ('enc', dec))
    monkeypatch.setattr(m, '_encode_chunked', encode)
    monkeypatch.setattr(m, '_decode', lambda dec_, kv, prompt, poly_sos, rec_sos, seq, fi, B, dev, side, packed=None: ['out'] * B)
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: contextlib.nullcontext())
    m.enc_calls, m.dec = enc_calls, dec
    return m


SEQS = [torch.tensor([[0, 0, 999, 999, 1000, 1095, 1100]]), torch.tensor([[1101]]), torch.tensor([[1102]])]


def test_one_size_takes_the_padding_free_path(model):
    imgs = _images([(32, 48)] * 3)
    assert model.infer(imgs, None, SEQS, ragged=True) == ['out'] * 3
    assert model.enc_calls == [dict(shape=(3, 3, 32, 48), padded=False, no_padding=True)]
    (c,) = model.dec.calls
    assert c['B'] == 3 and c['M'] == _m_of(32, 48) and c['key_mask'] is None and c['key_len'] is None
    # a padded batch whose images all have one (smaller) extent: cropped, then the same path
    model.enc_calls.clear()
    model.dec.calls.clear()
    nt = nested_tensor_from_tensor_list(imgs)
    big = torch.zeros(3, 3, 40, 56)
    big[:, :, :32, :48] = nt.tensors
    mask = torch.ones(3, 40, 56, dtype=torch.bool)
    mask[:, :32, :48] = False
    model.infer(big, mask, SEQS, ragged=True)
    assert model.enc_calls == [dict(shape=(3, 3, 32, 48), padded=False, no_padding=True)]
    assert model.dec.calls[0]['key_len'] is None and model.dec.calls[0]['key_mask'] is None


def test_mixed_sizes_bucket_encode_and_place_rows(model):
    imgs = _images(SIZES, seed=3)
    for inp, mask in ((imgs, None), (nested_tensor_from_tensor_list(imgs).tensors, nested_tensor_from_tensor_list(imgs).mask)):
        model.enc_calls.clear()
        model.dec.calls.clear()
        assert model.infer(inp, mask, SEQS, ragged=True) == ['out'] * len(SIZES)
        assert model.enc_calls == [dict(shape=(2, 3, 32, 48), padded=False, no_padding=True), dict(shape=(2, 3, 48, 32), padded=False, no_padding=True),
                                   dict(shape=(1, 3, 40, 40), padded=False, no_padding=True)]
        (c,) = model.dec.calls
        keys = [_m_of(h, w) for h, w in SIZES]
        Mmax = (max(keys) + 63) // 64 * 64
        assert c['B'] == len(SIZES) and c['M'] == Mmax and c['key_len'] == keys and c['key_mask'] is None
        mem = c['memory'].reshape(len(SIZES), Mmax, D)
        for b, im in enumerate(imgs):
            want = im.sum() + torch.arange(keys[b], dtype=torch.float32) * 1000
            assert torch.allclose(mem[b, :keys[b], 0], want) and torch.allclose(c['mem_pos'].reshape(len(SIZES), Mmax, D)[b, :keys[b], 0], -want)
            assert not mem[b, keys[b]:].any(), 'rows beyond M_b must be zero'


def test_packed_is_padded_only(model):
    with pytest.raises(ValueError):
        model.infer(_images(SIZES), None, SEQS, ragged=True, packed=8)


# -- validate(ragged=True) with a stub model ------------------------------------------------------------------------------------
REC = 25


def _fake(img):
    key = int(img.abs().sum().item() * 10) % 997
    n = key % 3
    if n == 0:
        return None
    g = torch.Generator().manual_seed(key)
    return ([torch.randint(0, 1000, (1, 2 * n), generator=g), torch.randint(0, 1000, (1, 32 * n), generator=g),
             torch.randint(1000, 1096, (1, n, REC), generator=g)], [torch.rand(n, REC, generator=g)])


class RaggedStub(torch.nn.Module):
    """answers per UNPADDED image content; records what it was handed"""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def infer(self, img, mask, seqs, has_padding=None, ragged=False, **kw):
        if ragged:
            assert mask is None and isinstance(img, list)
            self.calls.append(('ragged', [tuple(i.shape) for i in img]))
            return [_fake(i) for i in img]
        assert img.shape[0] == 1 and not bool(mask.any()) and not has_padding
        self.calls.append(('padded', [tuple(img.shape[1:])]))
        return [_fake(img[0])]


def _loader(n):
    items = []
    for i in range(n):
        h, w = 32 + 8 * (i % 3), 40 + 8 * (i % 2)
        img = torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(70 + i))
        items.append((nested_tensor_from_tensor_list([img[0]]), [{'file_name': 'img_%02d.jpg' % i, 'orig_size': torch.tensor([h * 2, w * 2]),
                                                                  'dataset_name': 'unit_val'}]))
    return items


def test_validate_ragged_hands_over_unpadded_images(tmp_path):
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    n = 9
    texts = {}
    for tag, bs, rg in (('single', 1, False), ('ragged', 4, True)):
        args.output_folder = str(tmp_path / tag)
        stub = RaggedStub()
        inf.validate(stub, _loader(n), 0, args, batch_size=bs, ragged=rg)
        with open(os.path.join(args.output_folder, 'results', 'ep000', 'unit_val.json')) as f:
            texts[tag] = f.read()
        if rg:
            assert [k for k, _ in stub.calls] == ['ragged'] * 3
            assert [len(s) for _, s in stub.calls] == [4, 4, 1]
            want = [(3, 32 + 8 * (i % 3), 40 + 8 * (i % 2)) for i in range(n)]
            assert [s for _, ss in stub.calls for s in ss] == want   # every image at its own size: nothing padded
    assert json.loads(texts['ragged']) and texts['ragged'] == texts['single']


def test_predict_ragged_orig_size_is_each_images_own():
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    imgs = _images([(32, 40), (48, 40), (40, 48)], seed=11)
    stub = RaggedStub()
    got = inf.predict(stub, imgs, args, ragged=True)
    for im, recs in zip(imgs, got):
        raw = _fake(im)
        want = [] if raw is None else inf.decode_pred_seq([t[0] for t in raw[0]], raw[1][0],
                                                           {'file_name': '', 'orig_size': tuple(im.shape[1:])}, args)
        assert [r['pts'] for r in recs] == [r['pts'] for r in want]
