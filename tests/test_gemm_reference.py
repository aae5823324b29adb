"""The float64 restatements of omp_gemm_bias_act (tests/gpu_checks_gemm.py: ref_gemm, ref_ln_gemm) against plain torch (F.linear, F.gelu,
F.layer_norm) and against tests/fake_ops.gemm, and the checker of the GPU tests (run_case) against a fake launch built on fake_ops.gemm
with ONE seeded defect at a time: each defect must yield a failing record of the kind that is there to catch it, and the clean fake none
-- a checker that cannot fail proves nothing about the kernels.  The bias table's per-row form (bias 'table': bias_row_mod / bias_row_off)
has its own pins and its own four seeded defects, each of which must fail the float64 gate AND the bit gate against the one-row form.
CPU only."""
import pytest
import torch
import torch.nn.functional as F

from tests import fake_ops
from tests import gpu_checks_gemm as G

TOL = 1e-12   # float64 against float64: only the summation order differs


def _r(*shape, seed, s=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * s


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize('act', [G.ACT_NONE, G.ACT_GELU, G.ACT_RELU])
@pytest.mark.parametrize('mode', ['n', 'm', 'row'])
def test_ref_gemm_is_linear_activation_residual(mode, act):
    M, N, K = 37, 29, 96
    A, W, res = _r(M, K, seed=1), _r(N, K, seed=2, s=K ** -0.5), _r(M, N, seed=3)
    bias = {'n': _r(N, seed=4), 'm': _r(M, seed=4), 'row': _r(5, N, seed=4)}[mode]
    got = G.ref_gemm(A, W, bias, mode, act, res, row=3)
    if mode == 'm':
        y = F.linear(A, W) + bias[:, None]
    else:
        y = F.linear(A, W, bias[3] if mode == 'row' else bias)
    y = F.gelu(y) if act == G.ACT_GELU else (F.relu(y) if act == G.ACT_RELU else y)
    assert _rel(got, y + res) < TOL
    assert _rel(G.ref_gemm(A, W, None, mode, act, None), F.gelu(F.linear(A, W)) if act == G.ACT_GELU else
                (F.relu(F.linear(A, W)) if act == G.ACT_RELU else F.linear(A, W))) < TOL


def test_ref_gemm_rounds_once():
    A, W, b = _r(19, 64, seed=5), _r(24, 64, seed=6, s=0.125), _r(24, seed=7)
    y = G.ref_gemm(A, W, b)
    assert torch.equal(G.ref_gemm(A, W, b, out='bf16'), y.to(torch.bfloat16).double())
    hi, lo = G.ref_gemm(A, W, b, out='split')
    assert torch.equal(hi, y.to(torch.bfloat16).double())
    assert torch.equal(lo, (y - hi).to(torch.bfloat16).double())
    assert _rel(hi + lo, y) < 2.0 ** -15      # a pair resolves 16 mantissa bits


@pytest.mark.parametrize('dtn', ['bf16', 'fp32'])
@pytest.mark.parametrize('mode', ['n', 'm'])
def test_ref_gemm_against_fake_ops(mode, dtn):
    """fake_ops.gemm (the fp32 test double of the host-flow tests) on the same rounded operands"""
    dt = G.DT[dtn]
    M, N, K = 33, 40, 128
    A, W = _r(M, K, seed=1).to(dt), _r(N, K, seed=2, s=K ** -0.5).to(dt)
    bias, res = _r(M if mode == 'm' else N, seed=3).float(), _r(M, N, seed=4).to(dt)
    for act in (G.ACT_NONE, G.ACT_GELU, G.ACT_RELU):
        fake = fake_ops.gemm(A, W, bias, residual=res, act=act, bias_along_m=mode == 'm', out_dtype=torch.float32)
        assert _rel(fake.double(), G.ref_gemm(A, W, bias, mode, act, res)) < 2e-6   # fp32 summation of the double
    assert torch.equal(G.wrap_a(A, 192, 128), torch.cat([A, A[:, :64]], 1))


@pytest.mark.parametrize('eps', [1e-5, 1e-3])
@pytest.mark.parametrize('dtn', ['bf16', 'fp32'])
def test_ref_ln_gemm_is_layer_norm_then_linear(dtn, eps):
    dt = G.DT[dtn]
    M, N, K = 21, 32, 384
    X, g, b = _r(M, K, seed=1, s=1.5).float() + 0.2, _r(K, seed=2, s=0.1).float() + 1, _r(K, seed=3, s=0.1).float()
    W, bias = _r(N, K, seed=4, s=K ** -0.5).to(dt), _r(N, seed=5).float()
    y = F.layer_norm(X.double(), (K,), g.double(), b.double(), eps).to(dt).double()
    want = F.relu(F.linear(y, W.double(), bias.double()))
    assert _rel(G.ref_ln_gemm(X, g, b, eps, W, dt, bias=bias, act=G.ACT_RELU), want) < TOL
    # a constant row normalises to beta exactly; the planted rows sit where the checks look for them
    Xp = G.plant_ln(X, M)
    rc, ro = G.ln_plant_rows(M)
    assert (rc, ro) == (0, M - 1) and G.ln_plant_rows(1) == (None, None) and G.ln_plant_rows(2) == (0, None)
    n = F.layer_norm(Xp.double(), (K,), g.double(), b.double(), eps)
    assert torch.equal(n[rc], b.double())
    lo = G.ln_low_row(M)
    assert lo == 1 and G.ln_low_row(1) == 0 and G.ln_low_row(2) == 1 and lo not in (rc, ro)
    assert 0.5 * G.LN_LOW ** 2 < Xp[lo].var().item() < 2 * G.LN_LOW ** 2 < 2 * max(G.LN_EPS) * 1.01   # of the order of the larger eps
    two = [F.layer_norm(Xp[lo].double(), (K,), None, None, e) for e in G.LN_EPS]
    assert _rel(two[0], two[1]) > 0.2                             # the two eps values move this row by a third
    assert abs(Xp[ro].mean().item() - G.LN_OFFSET) < 0.5 and 0.5 < Xp[ro].std().item() < 1.5


# ---------------------------------------------------------------------------------------------------------------------------------------
# the checker against seeded defects
# ---------------------------------------------------------------------------------------------------------------------------------------
def _beyond(v, rows, cols):
    """the storage around a view: [rows, cols] from the view's origin with the view's pitch"""
    return torch.as_strided(v, (rows, cols), v.stride(), v.storage_offset())


def fake_launch(defect=None):
    """omp_gemm_bias_act on CPU views, built on fake_ops.gemm; defect: the one thing it does wrong"""
    def launch(c):
        M, N, K = c['M'], c['N'], c['K']
        A, W = c['A'], c['W']
        if defect == 'reads row M':              # the last row comes from the row behind the view
            A = A.clone()
            A[M - 1] = _beyond(c['A'], M + 1, A.shape[1])[M]
        if defect == 'row M-1 from row M-2':
            A = A.clone()
            A[M - 1] = A[M - 2]
        if c['ln'] is not None:
            A = F.layer_norm(A.double(), (K,), c['ln'][0].double(), c['ln'][1].double(), c['ln_eps']).to(W.dtype)
        A = G.wrap_a(A, K, c['a_wrap'])
        if defect == 'last K tile skipped':
            kt = 128 // W.element_size()
            A, W = A[:, :K - kt], W[:, :K - kt]
        bias = c['bias']
        if bias is not None and c['bias_mode'] == 'row':
            bias = bias[int(c['bias_row'].item())]
        if defect == 'bias_along_m dropped' and c['bias_mode'] == 'm':
            bias = None
        mod, off = c['bias_row_mod'], c['bias_row_off']
        if bias is not None and c['bias_mode'] == 'table' and mod == 0:     # the one-row form on the per-row cases' table
            bias = bias[int(c['bias_row'].item())]
        if mod > 0 and defect in TABLE_DEFECTS:
            rows = {'table: off dropped': torch.arange(M) % mod, 'table: every row takes row off': torch.full((M,), off % mod),
                    'table: shifted by one': (off + torch.arange(M) + 1) % mod, 'table: ragged N keeps the column bias': (off + torch.arange(M)) % mod}[defect]
            bias = bias[rows].clone()
            if defect == 'table: ragged N keeps the column bias':          # the 16-byte chunk that straddles N: bias[n], which is table row 0
                ch = 16 // c['out'].element_size()
                bias[:, N // ch * ch:] = c['bias'][0, N // ch * ch:]
            mod, off = M, 0
        y = fake_ops.gemm(A, W, bias, act=c['act'], bias_along_m=c['bias_mode'] == 'm', out_dtype=torch.float32, bias_row_mod=mod, bias_row_off=off)
        if c['out2'] is not None:
            c['out2'].copy_(y.to(c['out2'].dtype))
        if c['residual'] is not None:
            y = y + c['residual'].float()
        out = c['out']
        if c['split']:
            hi = y.to(torch.bfloat16)
            out[:, :N] = hi
            out[:, N:] = (y - hi.float()).to(torch.bfloat16)
        elif c['trans_rows']:
            tr = c['trans_rows']
            out.copy_(y.reshape(M // tr, tr, N).permute(0, 2, 1).reshape(-1, tr).to(out.dtype))
        else:
            out.copy_(y.to(out.dtype))
        if defect == 'gap column':
            _beyond(out, out.shape[0], out.shape[1] + 1)[0, out.shape[1]] = 1.0
        if defect == 'guard row':
            _beyond(out, out.shape[0] + 1, out.shape[1])[out.shape[0], 0] = 1.0
    return launch


CASES = [
    G.case(5, 'bf16', 'bf16', 129, 136, 128, bias='m'),
    G.case(5, 'bf16', 'fp32', 129, 136, 128, bias='m', res=True, pitch='scalar'),
    G.case(6, 'fp32', 'fp32', 65, 67, 96, act=G.ACT_GELU, res=True, pitch='ldr_odd'),
    G.case(6, 'bf16', 'split', 65, 72, 128, act=G.ACT_GELU),
    G.case(5, 'bf16', 'bf16', 129, 136, 128, res=True, c2=True),
    G.case(5, 'bf16', 'bf16', 129, 72, 128, trans=43),
    G.case(3, 'bf16', 'fp32', 17, 67, 384, a_wrap=256, res=True, tail=64),
    G.case(4, 'bf16', 'fp32', 49, 67, 512, inplace=True, rows=64, tail=64),
    G.case(4, 'fp32', 'fp32', 17, 20, 384, bias='row', act=G.ACT_RELU, ln=1e-3, rows=64, plant=True, tail=64),
]
# defect -> the kind of record that must fail
DEFECTS = {'bias_along_m dropped': 'value', 'last K tile skipped': 'value', 'gap column': 'guards', 'guard row': 'guards',
           'reads row M': 'nan', 'row M-1 from row M-2': 'value'}
# the per-row bias table: defect -> what it does; each must fail the float64 gate of run_case AND the bit gate against the one-row form
TABLE_DEFECTS = ('table: off dropped', 'table: every row takes row off', 'table: shifted by one', 'table: ragged N keeps the column bias')
TABLE_CASES = [
    G.case(6, 'bf16', 'bf16', 65, 67, 128, bias='table', mod=6, off=4),
    G.case(6, 'bf16', 'fp32', 129, 67, 128, bias='table', mod=7, off=10, inplace=True, pitch='scalar'),
    G.case(5, 'bf16', 'split', 129, 136, 128, bias='table', mod=6, off=4, act=G.ACT_GELU),
    G.case(5, 'fp32', 'fp32', 129, 131, 64, bias='table', mod=2, off=5, res=True),
    G.case(5, 'bf16', 'bf16', 257, 136, 128, bias='table', mod=7, off=10, res=True, c2=True),
    G.case(4, 'bf16', 'fp32', 17, 20, 128, bias='table', mod=6, off=4, rows=64, tail=64, hint=True),
    G.case(4, 'fp32', 'fp32', 49, 20, 64, bias='table', mod=7, off=10, ln=1e-5, rows=64, tail=64, hint=True),
]
# what the fp32 test double itself is off by, relative to a row's max |ref|, per destination: its float summation (K <= 512), one bf16
# rounding of the result (2^-8 of the element, twice where a rounding flips), the 16 mantissa bits of a pair row
FAKE_REL = {'fp32': 1e-5, 'bf16': 2.0 ** -7, 'split': 2.0 ** -15}


def _value_fails(records, c):
    """a failing value record: beyond the absolute gate of the existing checks, or (a measured gate may not exist on this machine's
    table) a relative error far beyond what the clean double shows"""
    return [r for r in records if r['kind'] in ('value', 'cap') and not r['ok']]


@pytest.mark.parametrize('c', CASES, ids=G.tag)
def test_clean_fake_passes(c):
    records, outs = G.run_case(c, fake_launch(), 'cpu', report=False)
    assert outs
    bad = [r for r in records if not r['ok'] and r['kind'] in ('guards', 'nan', 'launch', 'cap')]
    assert not bad, bad
    key = G.tol_key(c)
    assert G.WORST[key] >= 0
    rel = [float(r['note'].split('rel ')[1]) for r in records if 'rel ' in r['note']]
    assert rel and max(rel) <= FAKE_REL[c['out']], rel


@pytest.mark.parametrize('defect', sorted(DEFECTS))
def test_seeded_defect_yields_a_failing_record(defect):
    hit = 0
    for c in CASES:
        if defect == 'bias_along_m dropped' and c['bias'] != 'm':
            continue
        if defect == 'row M-1 from row M-2' and c['plant']:
            continue
        records, _ = G.run_case(c, fake_launch(defect), 'cpu', report=False)
        kinds = {r['kind'] for r in records if not r['ok']}
        want = DEFECTS[defect]
        assert (want in kinds) or (want == 'value' and 'cap' in kinds), (G.tag(c), defect, [r for r in records if not r['ok']])
        if want == 'guards':
            assert 'nan' not in kinds and 'cap' not in kinds, (G.tag(c), kinds)   # only the sentinel record notices a stray write
        hit += 1
    assert hit >= 2


def test_in_place_and_bit_records():
    c = G.case(4, 'bf16', 'fp32', 33, 67, 512, res=True, act=G.ACT_RELU, rows=64, tail=64)
    _, a = G.run_case(c, fake_launch(), 'cpu', report=False)
    _, b = G.run_case(dict(c, inplace=True), fake_launch(), 'cpu', report=False)
    out = []
    G.same_bits(out, 'in place', b['C'], a['C'])
    assert out[0]['ok']
    b['C'][32, 66] += 1e-3
    G.same_bits(out, 'in place, one element off', b['C'], a['C'])
    assert not out[1]['ok'] and out[1]['err'] == 1


def test_constant_row_record():
    """ln_constant_row: exact on the clean double, failing when the LayerNorm launch got its constant row from another row"""
    M, N, K = 17, 67, 384
    c = G.case(4, 'bf16', 'bf16', M, N, K, ln=1e-5, rows=64, seed=K + N, plant=True, tail=64)
    _, o = G.run_case(c, fake_launch(), 'cpu', report=False)
    assert all(r['ok'] for r in G.ln_constant_row('bf16', M, N, K, o['C'], fake_launch(), 'cpu'))
    wrong = o['C'].clone()
    wrong[0] = wrong[1]
    assert not all(r['ok'] for r in G.ln_constant_row('bf16', M, N, K, wrong, fake_launch(), 'cpu'))


def test_refusal_record():
    c = G.case(9, 'bf16', 'bf16', 257, 264, 256, bias='m')

    def refuse(call):
        raise RuntimeError('omp_gemm_bias_act failed (-95): does not take this product')
    assert all(r['ok'] for r in G.run_case(c, refuse, 'cpu', expect=G.ERR_UNSUPPORTED)[0])
    assert not all(r['ok'] for r in G.run_case(c, fake_launch(), 'cpu', expect=G.ERR_UNSUPPORTED)[0])   # it ran instead
    assert not G.accepts(c) and G.accepts(dict(c, sel=5)) and not G.accepts(dict(c, bias='n', sel=16, K=320))


def test_shapes_follow_the_kernels():
    """the sweeps hold the sizes they claim: every MF boundary, the partial fetch rounds, the partial LayerNorm passes"""
    assert {16, 17, 32, 33, 48, 49, 64} <= set(G.EDGE_M)
    assert 1152 // 4 // 32 == 9 and 128 // 4 // 32 == 1           # bf16 k-steps per wave: one partial second round of PF = 8, one step
    assert 1152 // 4 // 4 == 72 and 2048 // 4 // 4 == 128 and 64 // 4 // 4 == 4   # fp32: partial ninth round, full rounds, half a round
    assert [k // 4 for k in G.LN_K['bf16']] == [32, 96, 128, 256] and G.LN_K['fp32'][0] == 64
    for sel, T in G.TILE.items():
        assert all(G.accepts(G.case(sel, 'bf16', 'bf16', 2 * T, 2 * T, nt * 64)) for nt in G.K_TILES[sel]), sel


# ---------------------------------------------------------------------------------------------------------------------------------------
# the bias table's per-row form
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [G.ACT_NONE, G.ACT_GELU, G.ACT_RELU])
@pytest.mark.parametrize('mod,off', [(1, 4), (2, 5), (6, 4), (7, 10), (7, 0)])
def test_ref_gemm_table_is_linear_plus_the_row_of_the_table(mod, off, act):
    M, N, K = 37, 29, 96
    A, W, res, tab = _r(M, K, seed=1), _r(N, K, seed=2, s=K ** -0.5), _r(M, N, seed=3), _r(mod, N, seed=4)
    y = torch.stack([F.linear(A[m], W, tab[(off + m) % mod]) for m in range(M)])
    y = F.gelu(y) if act == G.ACT_GELU else (F.relu(y) if act == G.ACT_RELU else y)
    assert _rel(G.ref_gemm(A, W, tab, 'table', act, res, mod=mod, off=off), y + res) < TOL
    # and fake_ops.gemm states the same
    fake = fake_ops.gemm(A.float(), W.float(), tab.float(), residual=res.float(), act=act, bias_row_mod=mod, bias_row_off=off, out_dtype=torch.float32)
    assert _rel(fake.double(), y + res) < 2e-6


def test_table_offsets_tell_the_formulas_apart():
    """off is no multiple of mod and M >= 2 mod + 1 in the cases the checks run: the four formulas of TABLE_DEFECTS give other rows"""
    for mod in G.TABLE_MODS[1:]:
        assert G.table_offs(mod)[0] == 0 and G.table_offs(mod)[1] == 4 and G.table_offs(mod)[2] % mod   # mod + 3: never a multiple
    for (mod, off) in G.TABLE_TILE_MODS:
        assert mod == 1 or off % mod
        assert all(M >= 2 * mod + 1 for sel in (5, 6) for M in G.TABLE_TILE_SHAPES[sel][0])
    assert G.PTABLE_ROWS == max(G.TABLE_MODS)


@pytest.mark.parametrize('c', TABLE_CASES, ids=G.tag)
def test_clean_fake_passes_both_table_gates(c):
    records = G.run_table(c, fake_launch(), 'cpu')
    bad = [r for r in records if not r['ok'] and r['kind'] in ('guards', 'nan', 'launch', 'cap', 'bits')]
    assert not bad, bad
    assert sum(r['kind'] == 'bits' for r in records) == (2 if c['c2'] else 1)
    rel = [float(r['note'].split('rel ')[1]) for r in records if 'rel ' in r['note']]
    assert rel and max(rel) <= FAKE_REL[c['out']], rel


@pytest.mark.parametrize('defect', TABLE_DEFECTS)
def test_seeded_table_defect_fails_both_gates(defect):
    hit = 0
    for c in TABLE_CASES:
        if 'ragged' in defect and (c['sel'] == 4 or c['N'] % 8 == 0):   # the 4-value path of the tile kernels at a ragged N edge
            continue
        records = G.run_table(c, fake_launch(defect), 'cpu')
        kinds = {r['kind'] for r in records if not r['ok']}
        assert 'bits' in kinds and ({'value', 'cap'} & kinds), (G.tag(c), defect, [r for r in records if not r['ok']])
        assert 'guards' not in kinds and 'nan' not in kinds, (G.tag(c), kinds)
        hit += 1
    assert hit >= 3


def test_table_guard_rows_are_nan():
    """a launch that reads the row behind the table (mod taken one too large) is seen by value: the NaN record fails"""
    c = TABLE_CASES[0]

    def launch(call):
        tab = _beyond(call['bias'], c['mod'] + 1, c['N'])
        fake_launch()(dict(call, bias=tab, bias_row_mod=c['mod'] + 1))
    kinds = {r['kind'] for r in G.run_case(c, launch, 'cpu', report=False)[0] if not r['ok']}
    assert 'nan' in kinds


def test_ln_inputs_stay_clear_of_bf16_ties():
    """ln_resolvable: a normalised element on a bf16 rounding tie (to fp32 resolution) is seen where its flip matters, next to the tie
    not, nor where the flip is negligible against the row's largest output; the seeds the per-row table sweep draws its LayerNorm rows from exist, pass, and
    seed 16 -- one element 3e-8 from a tie -- is passed over"""
    K = 128
    lo = torch.tensor(1.5, dtype=torch.bfloat16)
    hi = (lo.view(torch.int16) + 1).view(torch.bfloat16)
    tie = ((lo.double() + hi.double()) / 2).item()
    W = _r(16, K, seed=3, s=K ** -0.5)
    X = torch.ones(1, K)                       # a constant row normalises to beta exactly
    for delta, ok in ((0.0, False), (3e-8, False), (-5e-7, False), (1e-5, True), (-1e-5, True)):
        assert G.ln_resolvable(X, torch.ones(K), torch.full((K,), tie * (1 + delta), dtype=torch.float64), 1e-5, W) == ok, delta
    Wbig = torch.cat([W, torch.full((1, K), 40.0, dtype=torch.float64)])           # a row max the flip cannot move: it does not count
    assert G.ln_resolvable(X, torch.ones(K), torch.full((K,), tie, dtype=torch.float64), 1e-5, Wbig * torch.cat([torch.full((16, 1), 1e-3, dtype=torch.float64), torch.ones(1, 1, dtype=torch.float64)]))
    for N in (16, 20, 512):
        seed = G.ln_seed('bf16', N, K, 1e-5, N)
        assert seed % 1000 == N and G.ln_seed('fp32', N, 64, 1e-5, N) == N
        h = G.host('bf16', 64, N, K, 0, seed, True)
        assert G.ln_resolvable(h['A'], h['g'], h['b'], 1e-5, h['W'])
    h = G.host('bf16', 64, 16, K, 0, 16, True)
    assert not G.ln_resolvable(h['A'], h['g'], h['b'], 1e-5, h['W']) and G.ln_seed('bf16', 16, K, 1e-5, 16) != 16
