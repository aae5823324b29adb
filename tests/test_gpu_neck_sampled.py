"""GPU tests of the sampled encoder neck: on the regular geometry (h2 == 2 h3 == 4 h4) Encoder.encode normalises and projects only the
pixels of c2 / c3 that the stride-2 FPN fuse reads (omp_layernorm_sampled, the lateral products on compact rows, omp_fpn_fuse_sampled).
It is the same arithmetic on fewer rows, so every gate here is bit equality (torch.equal on the raw bits), and every pixel the sampled path
must not read holds NaN:

  * the encoder output of the sampled path against the full path (want_intermediates=True runs it), fallback sizes included;
  * omp_layernorm_sampled against omp_layernorm of the gathered rows, between NaN guard rows, into a sentinel-filled output;
  * omp_fpn_fuse_sampled against omp_fpn_fuse fed full laterals whose unsampled pixels are NaN;
  * a lateral product on the compact rows against the sampled rows of the product on all rows, across every kernel the dispatch table of
    csrc/gemm.hip can pick for N = 256 without an epilogue (row streaming, 64x64 rings of 8 and 4 stages, 128x128 and 256x256 tiles).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FC = 256
LEAD = 8                                        # guard rows in front of a buffer
H4W4 = ((1, 1), (3, 5), (4, 4))                 # stage-2 grids (h4, w4) of the kernel tests
NECK = {128: (4, 2), 256: (2, 1)}               # stage width -> (step, group) of the rows / columns the neck reads (c2, c3)


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from advancedliteratemachinery_amd import _lib, ops
    from tests import gpu_checks_encoder as E
    return type('Gpu', (), dict(ops=ops, lib=_lib, E=E))


@pytest.fixture(scope='module')
def encoder(gpu):
    """the bf16 engine's encoder on the seeded synthetic checkpoint (Swin-B widths, two blocks per stage)"""
    from advancedliteratemachinery_amd.utils import synthetic as weights
    from advancedliteratemachinery_amd.utils.parser import make_args
    from tests.gpu_checks import build_model
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    sd = weights.make_state_dict(args, seed=5, depths=(2, 2, 2, 2))
    model = build_model(args, sd, (2, 2, 2, 2), torch.bfloat16)
    return model.engine()[0]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def sampled_index(B, H, W, step, group):
    """rows of a token-major [B*H*W, C] map that the neck reads, in the order of the compact map: rows / columns q * step + r, r < group"""
    ys = torch.tensor([q * step + r for q in range(H // step) for r in range(group)])
    xs = torch.tensor([q * step + r for q in range(W // step) for r in range(group)])
    img = (ys[:, None] * W + xs[None, :]).reshape(-1)
    return (torch.arange(B)[:, None] * (H * W) + img[None, :]).reshape(-1)


def randn(*shape, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV).to(dtype)


def guarded(E, rows, width, dt, guard_bits, fill=None):
    """[LEAD + rows + GUARD, width] buffer of guard_bits -> (buffer, view of the rows in between, = fill where given)"""
    buf = E.guarded(LEAD + rows, width, dt, guard_bits)
    view = buf[LEAD:LEAD + rows]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guards_kept(E, buf, rows, guard_bits):
    return bool((bits(buf)[:LEAD] == guard_bits).all().item()) and E.kept(buf, LEAD + rows, guard_bits)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the encoder: sampled path == full path, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
def spy_sampled(gpu, monkeypatch):
    calls = []
    real = gpu.ops.fpn_fuse_sampled

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(gpu.ops, 'fpn_fuse_sampled', spy)
    return calls


def images(B, H, W, seed):
    return randn(B, 3, H, W, seed=seed), torch.zeros(B, H, W, dtype=torch.bool, device=DEV)


@pytest.mark.parametrize('B,H,W,sampled', [(2, 64, 64, True), (1, 96, 160, True), (1, 72, 104, False)])
def test_encode_sampled_equals_full(gpu, encoder, monkeypatch, B, H, W, sampled):
    """72x104 is not regular (h2 = 18): it must take today's path, and still equal it"""
    calls = spy_sampled(gpu, monkeypatch)
    img, mask = images(B, H, W, seed=H + W)
    fast = encoder.encode(img, mask)
    assert encoder.neck_sampled(H, W) == sampled and len(calls) == (1 if sampled else 0)
    full = encoder.encode(img, mask, want_intermediates=True)
    assert len(calls) == (1 if sampled else 0), 'want_intermediates=True must run the full neck'
    assert full['feats'][0][0].shape[0] == B * full['feats'][0][1] * full['feats'][0][2]   # the full c2 map
    assert bool(torch.isfinite(fast['memory'].float()).all().item())
    for k in ('memory', 'mem_pos'):
        assert same_bits(fast[k], full[k]), k


def test_encode_sampled_padded_batch(gpu, encoder, monkeypatch):
    """two image sizes in one padded batch, the padding masked"""
    calls = spy_sampled(gpu, monkeypatch)
    img, mask = images(2, 96, 128, seed=3)
    img[1, :, 64:, :] = 0
    img[1, :, :, 96:] = 0
    mask[1, 64:, :] = True
    mask[1, :, 96:] = True
    fast = encoder.encode(img, mask)
    full = encoder.encode(img, mask, want_intermediates=True)
    assert len(calls) == 1
    for k in ('memory', 'mem_pos'):
        assert same_bits(fast[k], full[k]), k
    assert torch.equal(fast['key_mask'], full['key_mask'])
    assert bool(full['key_mask'][1].any().item()) and not bool(full['key_mask'][0].any().item())


@pytest.mark.parametrize('B,H,W', [(2, 64, 64), (2, 96, 160)])     # 32 rows: the small-M products; 120 rows: one product, two destinations
def test_encode_sampled_out_views(gpu, encoder, monkeypatch, B, H, W):
    """the output written through `out=` views of a larger tensor, as OmniParser._encode_chunked passes them"""
    calls = spy_sampled(gpu, monkeypatch)
    img, mask = images(B, H, W, seed=11)
    full = encoder.encode(img, mask, want_intermediates=True)
    R, d = full['memory'].shape
    sent = gpu.E.sent_bits(torch.bfloat16)
    big = [torch.empty((3 * R, d), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    for t in big:
        bits(t).fill_(sent)
    fast = encoder.encode(img, mask, no_padding=True, out=(big[0][R:2 * R], big[1][R:2 * R]))
    torch.cuda.synchronize()
    assert len(calls) == 1
    for t, k in zip(big, ('memory', 'mem_pos')):
        assert fast[k].data_ptr() == t[R:2 * R].data_ptr()
        assert same_bits(t[R:2 * R], full[k]), k
        assert bool((bits(t)[:R] == sent).all().item()) and bool((bits(t)[2 * R:] == sent).all().item()), k + ': rows outside the view written'


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. omp_layernorm_sampled
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [128, 256])
def test_layernorm_sampled(gpu, C):
    """fp32 in, bf16 out; every unsampled input row and the guard rows are NaN, the output lies between sentinel rows"""
    E, ops = gpu.E, gpu.ops
    g, b = randn(C, seed=1) * 0.1 + 1, randn(C, seed=2) * 0.1
    nanb, sentb = E.nan_bits(torch.float32), E.sent_bits(torch.bfloat16)
    for step, group in NECK.values():
        for h4, w4 in H4W4:
            for B in (1, 3):
                H, W = step * h4, step * w4
                idx = sampled_index(B, H, W, step, group).to(DEV)
                rows = randn(idx.numel(), C, seed=C + H + W + B) * 2 + 0.3
                xbuf, x = guarded(E, B * H * W, C, torch.float32, nanb)
                x[idx] = rows
                n = idx.numel()
                ybuf, y = guarded(E, n, C, torch.bfloat16, sentb)
                rc = gpu.lib.lib().omp_layernorm_sampled(ops.ptr(x), ops.dt(x), ops.ptr(g), ops.ptr(b), ops.ptr(y), ops.dt(y), B, H, W, C, step, group,
                                                         1e-5, ops.stream())
                gpu.lib.check(rc, 'omp_layernorm_sampled')
                ref = ops.layernorm(rows, g, b, out_dtype=torch.bfloat16, eps=1e-5)
                torch.cuda.synchronize()
                tag = 'C=%d step=%d group=%d %dx%d B=%d' % (C, step, group, h4, w4, B)
                assert guards_kept(E, ybuf, n, sentb), tag + ': a row outside the compact map was written'
                assert guards_kept(E, xbuf, B * H * W, nanb), tag + ': input guard rows changed'
                assert bool(torch.isfinite(y.float()).all().item()), tag + ': NaN in the output (an unsampled row was read)'
                assert same_bits(y, ref), tag
                y2, hq, wq = ops.layernorm_sampled(x, g, b, B, H, W, step, group, out_dtype=torch.bfloat16)
                assert (hq, wq) == (group * h4, group * w4) and same_bits(y2, ref), tag + ' (ops.layernorm_sampled)'


def test_layernorm_sampled_refuses_irregular(gpu):
    ops = gpu.ops
    x, g, b = randn(6 * 8, 128, seed=1), randn(128, seed=2), randn(128, seed=3)
    with pytest.raises(RuntimeError):
        ops.layernorm_sampled(x, g, b, 1, 6, 8, 4, 2)      # H = 6 is no multiple of the step
    with pytest.raises(RuntimeError):
        ops.layernorm_sampled(x, g, b, 1, 6, 8, 2, 3)      # group > step


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. omp_fpn_fuse_sampled
# ---------------------------------------------------------------------------------------------------------------------------------------
def level_sizes(h4, w4):
    return ((4 * h4, 4 * w4), (2 * h4, 2 * w4), (h4, w4), ((h4 + 1) // 2, (w4 + 1) // 2))


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
def test_fpn_fuse_sampled(gpu, dt):
    E, ops = gpu.E, gpu.ops
    nanb, sentb = E.nan_bits(dt), E.sent_bits(dt)
    for h4, w4 in H4W4:
        for B in (1, 3):
            sizes = level_sizes(h4, w4)
            lat = [randn(B * h * w, FC, seed=100 * i + h4 + w4 + B, dtype=dt) for i, (h, w) in enumerate(sizes)]
            full, comp = [], []
            for i, (step, group) in enumerate(NECK.values()):      # l2, l3: NaN in every pixel the compact maps omit
                idx = sampled_index(B, sizes[i][0], sizes[i][1], step, group).to(DEV)
                planted = torch.empty_like(lat[i])
                bits(planted).fill_(nanb)
                planted[idx] = lat[i][idx]
                full.append(planted)
                comp.append(guarded(E, idx.numel(), FC, dt, nanb, lat[i][idx])[1])
            ref, ho, wo = ops.fpn_fuse(full[0], full[1], lat[2], lat[3], B, sizes, 2)
            assert (ho, wo) == (h4, w4)
            R = B * h4 * w4
            obuf, y = guarded(E, R, 4 * FC, dt, sentb)
            (h2, w2), (h3, w3), _, (h5, w5) = sizes
            rc = gpu.lib.lib().omp_fpn_fuse_sampled(ops.ptr(comp[0]), ops.ptr(comp[1]), ops.ptr(lat[2]), ops.ptr(lat[3]), ops.ptr(y), ops.dt(dt), B,
                                                    h2, w2, h3, w3, h4, w4, h5, w5, ops.stream())
            gpu.lib.check(rc, 'omp_fpn_fuse_sampled')
            torch.cuda.synchronize()
            tag = '%dx%d B=%d' % (h4, w4, B)
            assert bool(torch.isfinite(ref.float()).all().item()), tag + ': omp_fpn_fuse at stride 2 read a pixel outside the sampled set'
            assert guards_kept(E, obuf, R, sentb), tag + ': a row outside the output was written'
            assert same_bits(y, ref), tag
            assert same_bits(ops.fpn_fuse_sampled(comp[0].contiguous(), comp[1].contiguous(), lat[2], lat[3], B, sizes)[0], ref), tag + ' (ops)'


def test_fpn_fuse_sampled_refuses_irregular(gpu):
    ops = gpu.ops
    sizes = ((18, 26), (9, 13), (5, 7), (3, 4))       # a 72 x 104 image
    z = torch.zeros((4 * 5 * 7, FC), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        ops.fpn_fuse_sampled(z, z[:5 * 7], z, z, 1, sizes)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the lateral products: a row's bits do not depend on how many rows the launch has, nor on the kernel that takes it
# ---------------------------------------------------------------------------------------------------------------------------------------
# (K, B, H, W) of the full map; the kernel tests' sizes, the engine-class launches scaled down to 4096 / 1024 rows, and sizes that put the
# full and the compact launch on either side of every boundary of gemm_auto_select (N = 256, bf16, no epilogue): 3 row streaming (M <= 64),
# 6 64x64 rings (8 stages up to 8192 rows, 4 above), 5 128x128 tiles (M > 16256), 9 256x256 tiles (M >= 49152)
LATERAL_CASES = ([(K, B, NECK[K][0] * h4, NECK[K][0] * w4) for K in NECK for h4, w4 in H4W4 for B in (1, 3)] +
                 [(128, 1, 64, 64), (256, 1, 32, 32), (256, 1, 64, 64), (128, 1, 32, 32),
                  (128, 1, 128, 160), (256, 1, 128, 160), (128, 1, 192, 256), (256, 1, 192, 256), (128, 1, 384, 512), (256, 1, 384, 512)])


def test_lateral_gemm_rows_independent_of_m(gpu):
    ops = gpu.ops
    seen = set()
    for K, B, H, W in LATERAL_CASES:
        step, group = NECK[K]
        Wt = randn(FC, K, seed=K, dtype=torch.bfloat16) * 0.1
        A = randn(B * H * W, K, seed=K + H + W + B, dtype=torch.bfloat16)
        idx = sampled_index(B, H, W, step, group).to(DEV)
        full = ops.gemm(A, Wt)
        comp = ops.gemm(A[idx].contiguous(), Wt)
        sel = (ops.gemm_choice(A.shape[0], FC, K, bias=False), ops.gemm_choice(idx.numel(), FC, K, bias=False))
        seen.update(sel)
        assert same_bits(comp, full[idx]), 'K=%d B=%d %dx%d: selectors %s (full, compact)' % (K, B, H, W, sel)
    assert seen == {3, 6, 5, 9}, 'kernels covered: %s' % sorted(seen)
