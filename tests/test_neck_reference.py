"""The restatements and helpers of tests/gpu_checks_neck.py, proven on the CPU before any kernel is held to them: the float64 FPN against
the oracle (oracle/omniparser_ref.py fpn), the one-level inputs, the slab readers against the slab writers of tests/fake_ops.py, the split
reference, and the derived product gate against a float32 CPU product of the checks' own inputs.  CPU only."""
import torch

from tests import fake_ops
from tests import gpu_checks_neck as N

f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16


def test_fpn_restatement_equals_oracle_on_every_chain():
    for start in N.FPN_STARTS:
        sizes = N.level_chain(*start)
        lat = N.fpn_inputs(sizes, 'random', f32)
        r = N.ref_fpn(lat, False)
        assert r.shape == (2, 4 * N.FC, sizes[1][0], sizes[1][1])
        scale = r.abs().max().item()
        assert (r - N.fpn_oracle(lat, f64)).abs().max().item() <= 1e-13 * scale, start
        # float32: three sums and a four-tap bilinear, a few roundings of values no larger than `scale`; and the source coordinate
        # scale * (dst + 0.5) - 0.5 of either axis, computed in float32: three roundings of a number below the map's size, which move the
        # weight between two taps that differ by 2 * scale at most
        assert (r - N.fpn_oracle(lat, f32)).abs().max().item() <= (16 + 6 * (start[0] + start[1])) * 2.0 ** -24 * scale, start
        # the bf16 restatement differs from the exact one by its four roundings (three sums, the output), half an ulp each at most
        lb = N.fpn_inputs(sizes, 'random', bf16)
        rb, re = N.ref_fpn(lb, True), N.ref_fpn(lb, False)
        assert torch.equal(rb, rb.to(bf16).double())
        assert (rb - re).abs().max().item() <= 4 * 2.0 ** -9 * 2 * re.abs().max().item(), start


def test_level_chain_is_the_backbone_s():
    assert N.level_chain(38, 51) == ((38, 51), (19, 26), (10, 13), (5, 7))
    assert N.level_chain(1, 40) == ((1, 40), (1, 20), (1, 10), (1, 5))
    assert N.level_chain(65, 3) == ((65, 3), (33, 2), (17, 1), (9, 1))


def test_one_level_inputs_light_the_expected_slices():
    for start in N.FPN_STARTS:
        sizes = N.level_chain(*start)
        for k, kind in enumerate(N.FPN_INPUTS[1:]):
            lat = N.fpn_inputs(sizes, kind, f32)
            assert [bool((t != 0).any()) for t in lat] == [i == k for i in range(4)]
            for stride in (1, 2):
                # (the restatement is pinned to the oracle above; the oracle itself on the small chains)
                for ref in ((N.ref_fpn(lat, False),) + ((N.fpn_oracle(lat, f64),) if start[0] * start[1] <= 100 and stride == 1 else ())):
                    y = N.token_major(ref, stride).reshape(-1, 4 * N.FC)
                    ok, nz = N.level_slices_ok(y, kind)
                    assert ok, (start, kind, nz)
                    # a level that is fed reaches EVERY token of its own and of every finer slice
                    assert bool((y[:, :(k + 1) * N.FC] != 0).all()), (start, kind)


def test_token_major_takes_the_strided_grid():
    t = torch.arange(2 * 3 * 5 * 7, dtype=f64).reshape(2, 3, 5, 7)
    y = N.token_major(t, 2)
    assert y.shape == (2, 3 * 4, 3)
    assert torch.equal(y[1, 1 * 4 + 2], t[1, :, 2, 4])


def test_slab_helpers_invert_the_fake_writers():
    nH, d = 8, 512
    for (B, T, KB, NL) in ((2, 37, 32, 2), (3, 20, 16, 1), (1, 64, 32, 3)):
        Mpad = -(-T // KB) * KB
        a = torch.randn(B * T, d, generator=torch.Generator().manual_seed(T))
        w = torch.randn(NL * d, d, generator=torch.Generator().manual_seed(T + 1)) / d ** 0.5
        bias = torch.randn(NL * d, generator=torch.Generator().manual_seed(T + 2))
        y = a @ w.t() + bias
        K = torch.zeros(NL, B, nH, Mpad, 64)
        Vt = torch.zeros(NL, B, nH, Mpad // KB, 64, KB)
        fake_ops.gemm(a, w, bias, out=K, store_mode=fake_ops.STORE_KBLK, kv=(B, T, Mpad, nH, KB))
        fake_ops.gemm(w, a, bias, out=Vt, store_mode=fake_ops.STORE_VBLK, kv=(B, T, Mpad, nH, KB), bias_along_m=True)
        want = N.slab_order(y, B, T)
        kn, vn = N.k_natural(K), N.vt_natural(Vt)
        assert kn.shape == vn.shape == (1, NL, B, nH, Mpad, 64)
        assert torch.equal(kn[0][:, :, :, :T], want)
        assert torch.allclose(vn[0][:, :, :, :T], want, rtol=0, atol=1e-5)       # (the fake V product sums in another order)
        assert not kn[0][:, :, :, T:].any() and not vn[0][:, :, :, T:].any()
        # the split-plane slabs: [block][plane][32 x 64] and [block][plane][64 x 32]
        if KB == 32:
            Ks = torch.stack([K.reshape(NL, B, nH, Mpad // 32, 32, 64), 2 * K.reshape(NL, B, nH, Mpad // 32, 32, 64)], 4)
            Vs = torch.stack([Vt, 2 * Vt], 4)
            ks, vs = N.k_natural(Ks, True), N.vt_natural(Vs, True)
            assert torch.equal(ks[0], kn[0]) and torch.equal(ks[1], 2 * kn[0])
            assert torch.equal(vs[0], vn[0]) and torch.equal(vs[1], 2 * vn[0])
    k = torch.arange(32)
    assert torch.equal(N.vt_slot(k), fake_ops._slot(k)) and sorted(N.vt_slot(k).tolist()) == list(range(32))


def test_split_reference_round_trips():
    tiny = torch.finfo(f32).tiny
    for C in N.SPLIT_C:
        x = N.split_inputs(C)
        assert x.shape == (333, C) and torch.equal(x, x.float().double())
        hi, lo = N.split_ref(x)
        for t in (x, hi.double(), lo.double()):
            assert bool(torch.isfinite(t).all()) and not bool(((t != 0) & (t.abs() < tiny)).any())
        # hi + lo restores x to 16 significant bits, and lo is what is left of x after hi: at most half an ulp of hi
        assert bool(((hi.double() + lo.double() - x).abs() <= 2.0 ** -16 * x.abs()).all())
        assert bool((lo.double().abs() <= 0.5 * N.ulp_of(hi.double(), bf16) * (1 + 2.0 ** -8)).all())
        # the planted kinds, also in row 0 alone: hi rounded away from zero, both zeros with their signs, the magnitude range
        for rows in (x[:1], x):
            h, l = N.split_ref(rows)
            assert bool(((h.double().abs() > rows.abs()) & (l.double() * rows < 0)).any()) or C < 3
            z = rows == 0
            assert bool((z & torch.signbit(rows)).any()) and (bool((z & ~torch.signbit(rows)).any()) or C < 6)
            assert torch.equal(h.view(torch.int16)[z & torch.signbit(rows)].unique(), torch.tensor([-32768], dtype=torch.int16))
            assert not bool(l.view(torch.int16)[z].any())
        assert x.abs().max().item() > 2.0 ** 99 and x[x != 0].abs().min().item() < 2.0 ** -99
        for triple in (False, True):
            y = N.split_expected(x, triple)
            assert y.shape == (333, (3 if triple else 2) * C)
            assert torch.equal(y[:, :C], hi) and torch.equal(y[:, -C:], lo) and torch.equal(y[:, C:2 * C], hi if triple else lo)


def test_ulp_of():
    r = torch.tensor([0.0, 1.0, -1.0, 1.5, 2.0, 0.99, 3e-5], dtype=f64)
    assert N.ulp_of(r, bf16).tolist() == [0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -23]
    assert N.ulp_of(r, f32)[1:3].tolist() == [2.0 ** -23, 2.0 ** -23]
    for dt in (bf16, f32):        # the next number of the format is one ulp away
        v = torch.tensor([1.0, 1.75, 100.0, 3e-5], dtype=f64).to(dt)
        nxt = torch.nextafter(v.float(), torch.tensor(float('inf'))) if dt == f32 else (v.view(torch.int16) + 1).view(bf16)
        assert torch.equal(nxt.double() - v.double(), N.ulp_of(v.double(), dt))


def _f32_product_inside_gate(a, w, bias, dt):
    """the float32 CPU product of the same operands, rounded to dt, against the float64 product: elements outside the derived gate"""
    ref, ab = N.product64(a, w, bias)
    got = (a.float() @ w.float().t() + bias.float()).to(dt)
    bad, worst, n = N.outside(got, ref, N.product_gate(ref, ab, dt))
    assert bad == 0 and 0 < worst < 1, (bad, worst)
    return worst


def test_product_gate_holds_for_a_float32_product_of_the_checks_inputs():
    for (ns, B, M) in N.KV_DIRECT:
        rows, w, bias = N.kv_inputs(B, M, ns)
        assert torch.equal(rows, rows.to(bf16).double()) and torch.equal(w, w.to(bf16).double()) and not rows[0].any()
        _f32_product_inside_gate(rows, w, bias, bf16)
    args, sd = N.neck_state_dict()
    Wk, bk, Wv, bv = N.memory_weights(args, sd)
    assert Wk.shape == Wv.shape == (12 * 512, 512) and bk.shape == bv.shape == (12 * 512,)
    for dt in (bf16, f32):
        for (B, M) in ((3, 1), (1, 33), (3, 77)):
            mem, mp = N.memory_inputs(B, M, dt, 1)
            assert not torch.equal(mem, N.memory_inputs(B, M, dt, 2)[0])
            _f32_product_inside_gate(mp, Wk.to(dt).double(), bk.double(), dt)
            _f32_product_inside_gate(mem, Wv.to(dt).double(), bv.double(), dt)
    # the split engine's absolute gate: even a plain float32 product of the fp32 masters stays far inside it
    mem, mp = N.memory_inputs(3, 77, f32, 1)
    ref, _ = N.product64(mp, Wk.double(), bk.double())
    assert (mp.float() @ Wk.t() + bk - ref).abs().max().item() < N.SPLIT_TOL / 4


def test_outside_counts_and_ratios():
    ref = torch.tensor([1.0, 2.0, 0.0, 4.0], dtype=f64)
    assert N.outside(torch.tensor([1.0, 2.5, 0.0, 4.0]), ref, 1.0) == (0, 0.5, 4)
    assert N.outside(torch.tensor([1.0, 2.5, 0.0, float('nan')]), ref, 1.0)[0] == 1
    bad, worst, _ = N.outside(torch.tensor([1.0, 2.0, 1e-9, 4.0]), ref, torch.tensor([1.0, 1.0, 0.0, 1.0], dtype=f64))
    assert bad == 1 and worst == float('inf')
    assert N.outside(ref.float(), ref, 0.0)[:2] == (0, 0.0)


def test_size_rule_never_changes_one_axis_alone():
    """why check_preprocess_edges gives its one-axis batches a size rule of their own"""
    from oracle import preprocess_ref as P
    for h in range(1, 130):
        for w in range(1, 130):
            oh, ow = P.get_size_with_aspect_ratio((w, h), N.PRE_MIN, N.PRE_MAX)
            assert (oh == h) == (ow == w), (h, w, oh, ow)
    sizes = [P.get_size_with_aspect_ratio((W, H), N.PRE_MIN, N.PRE_MAX) for (H, W, _) in N.PRE_IMAGES]
    assert sizes == [(48, 72), (48, 60), (99, 33), (20, 100), (48, 99)]
    assert max(s[0] for s in sizes) % 4 and max(s[1] for s in sizes) % 64
    assert [(oh != H, ow != W) for (H, W, oh, ow) in N.PRE_ONE_AXIS] == [(False, True), (True, False), (False, True), (True, False), (False, False)]
    assert len({(H, W) for (H, W, _, _) in N.PRE_ONE_AXIS}) == len(N.PRE_ONE_AXIS)      # the fixed size rule is keyed by the source size
    assert [ow > W for (H, W, oh, ow) in N.PRE_ONE_AXIS[0::2][:2]] == [True, False] and [oh > H for (H, W, oh, ow) in N.PRE_ONE_AXIS[1::2]] == [True, False]
