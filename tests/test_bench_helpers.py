"""bench.py's host-side helpers (no GPU): percentile, the committed PMC records it reads for `roofline.traffic`, argument
defaults the docs quote."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_module', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_percentile_interpolates():
    b = _bench()
    assert b.pct([3.0, 1.0, 2.0], 0.5) == 2.0
    assert abs(b.pct([1.0, 2.0], 0.9) - 1.9) < 1e-12
    assert b.pct([], 0.5) is None


def test_committed_pmc_records_feed_the_roofline_traffic():
    """profiles/pmc_cross_attn.json (keyed by images per launch) and profiles/pmc_gemm.json: measured HBM bytes within a few
    per cent of (cross-attention) / a small factor above (GEMM class, re-reads through L2) the algorithmic bytes"""
    b = _bench()
    for images in (160, 256, 512):      # 160 = the driver's `--steps 20` engine call (round 3)
        t = b.pmc_traffic(images)
        alg = images * 2 * 4096 * 512 * 2
        assert t is not None and 1.0 <= t / alg < 1.03, (images, t, alg)
    assert b.pmc_traffic(77) is None          # no pass at that size -> null in the bench line, never a guess
    g = b.pmc_gemm_traffic(1024, 'bf16')
    assert g is not None and g[0] > 1e8 and 1.0 <= g[1] < 1.5
    assert b.pmc_gemm_traffic(640, 'bf16') is None and b.pmc_gemm_traffic(1024, 'fp32') is None
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'pmc_gemm.json')))['summary']
    assert abs(rec['gemm_measured_bytes'] / rec['gemm_alg_bytes'] - rec['gemm_measured_over_alg']) < 1e-9


def test_defaults_are_the_documented_ones(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py'])
    for k in ('OMP355_LANES', 'OMP355_COALESCE', 'OMP355_GRAPH'):
        monkeypatch.delenv(k, raising=False)
    b = _bench()
    a = b.parse()
    assert (a.gpus, a.steps, a.warmup, a.lanes, a.coalesce, a.workload, a.dtype) == (1, 192, 32, 1, 64, 'spotting', 'bf16')
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '20', '--warmup', '5'])
    a = b.parse()
    assert max(1, min(a.coalesce, -(-a.steps // max(1, a.lanes)))) == 20   # one engine call of 160 images per repetition


def test_round3_flags_and_host_pinning(monkeypatch):
    """the legs the default line carries can be switched off one by one; pin_host_threads gives every rank its own slice of the
    cores the process may use and leaves a single rank alone"""
    b = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--no-parity-leg', '--no-config-legs', '--dtype', 'bf16x3', '--cross-nt', '2'])
    a = b.parse()
    assert a.no_parity_leg and a.no_config_legs and a.dtype == 'bf16x3' and a.cross_nt == 2
    monkeypatch.setattr(sys, 'argv', ['bench.py'])
    a = b.parse()
    assert not a.no_parity_leg and not a.no_config_legs and a.cross_nt == 1
    before = os.sched_getaffinity(0)
    try:
        assert b.pin_host_threads(0, 1) is None and os.sched_getaffinity(0) == before
        if len(before) >= 2:
            mine = b.pin_host_threads(1, 2)
            assert mine is not None and set(mine) == os.sched_getaffinity(0) and len(mine) == len(before) // 2
            assert set(mine).isdisjoint(sorted(before)[:len(before) // 2])
    finally:
        os.sched_setaffinity(0, before)


def test_split_plane_pmc_record_and_payload_round_trip():
    """round 4: the parity engine's cross-attention kernels have their own PMC record (`x3_<images>`: 4 bytes per (key, dim) element);
    the per-call all-gather payload (ids + probability bit patterns + counts in ONE int32 tensor) round-trips exactly."""
    import torch
    b = _bench()
    t = b.pmc_traffic(160, 'x3_')
    alg = 160 * 2 * 4096 * 512 * 4
    assert t is not None and 1.0 <= t / alg < 1.03, (t, alg)
    from advancedliteratemachinery_amd.utils import dist as D
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 1104, (3, 5, 59), generator=g, dtype=torch.int32)
    pr = torch.rand(3, 5, 25, generator=g)
    n = torch.tensor([5, 0, 3], dtype=torch.int32)
    buf = D.pack_payload(ids, pr, n)
    assert buf.dtype == torch.int32 and buf.shape == (3, 5 * 59 + 5 * 25 + 1)
    i2, p2, n2 = D.unpack_payload(torch.cat([buf, buf]), ids.shape[1:], pr.shape[1:])
    assert torch.equal(i2[:3], ids) and torch.equal(p2[3:], pr) and torch.equal(n2[:3], n)
    i3, p3, n3 = D.unpack_payload(D.pack_payload(ids, pr), ids.shape[1:], pr.shape[1:], with_n=False)
    assert n3 is None and torch.equal(i3, ids) and torch.equal(p3, pr)


def test_gemm4w_register_audit_catches_a_compiler_touch():
    """advancedliteratemachinery_amd/audit.py (run by build.py on the device assembly): a compiler-generated v_accvgpr_* / scratch access outside an asm
    block, a spill count or a short AGPR allocation in a gemm_4w kernel fails the build; the clean form passes."""
    from advancedliteratemachinery_amd import audit as audit_gemm4w
    import tempfile
    clean = ('_ZN1x7gemm_4wIfEEv: ; @k\n\ts_nop 0\n\t;;#ASMSTART\n\tv_accvgpr_write_b32 a[0], 0\n\t;;#ASMEND\n\tv_mov_b32 v0, v1\n\ts_endpgm\n'
             '  - .name:           _ZN1x7gemm_4wIfEEv\n    .agpr_count:     256\n    .private_segment_fixed_size: 0\n    .vgpr_spill_count: 0\n    .wavefront_size: 64\n')
    for text, n_bad in ((clean, 0), (clean.replace('\tv_mov_b32 v0, v1', '\tv_accvgpr_read_b32 v0, a3'), 1),
                        (clean.replace('.vgpr_spill_count: 0', '.vgpr_spill_count: 12'), 1), (clean.replace('.agpr_count:     256', '.agpr_count:     128'), 1)):
        with tempfile.NamedTemporaryFile('w', suffix='.s', delete=False) as f:
            f.write(text)
        try:
            seen, bad, checked = audit_gemm4w.audit(f.name)
        finally:
            os.unlink(f.name)
        assert seen == 1 and len(bad) == n_bad and checked == 0, (seen, bad, checked)   # gemm_4w itself has no asm-loaded fragments: no stage-loop check


def test_gemm4w_audit_refuses_a_register_copy_in_the_stage_loop():
    """gemm_4w_r / gemm_4w_p load their fragments with asm statements and count the waits by hand: a compiler-inserted vector-register copy
    inside the stage loop could read a fragment before it lands.  advancedliteratemachinery_amd/audit.py demands that the innermost loop of those two
    kernels holds all 512 MFMAs of its four stages and no such copy (scalar-source moves are fine)."""
    from advancedliteratemachinery_amd import audit as audit_gemm4w
    import tempfile
    body = '\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]\n' * 512
    def kernel(extra):
        return ('_ZN1x9gemm_4w_pIfLb0ELi0EEEvNS_5GemmPE: ; @k\n\ts_nop 0\n.LBB1_2: ; %loop\n ; =>This Inner Loop Header: Depth=1\n' + body + extra +
                '\ts_cbranch_scc1 .LBB1_2\n; %bb.3:\n\tv_mov_b32_e32 v9, v8\n\ts_endpgm\n'
                '  - .name:           _ZN1x9gemm_4w_pIfLb0ELi0EEEvNS_5GemmPE\n    .agpr_count:     256\n    .private_segment_fixed_size: 0\n    .vgpr_spill_count: 0\n    .wavefront_size: 64\n')
    for extra, n_bad in (('', 0), ('\tv_mov_b32_e32 v1, s3\n', 0), ('\tv_mov_b32_e32 v1, v2\n', 1), ('\tv_mov_b64_e32 v[2:3], v[4:5]\n', 1)):
        with tempfile.NamedTemporaryFile('w', suffix='.s', delete=False) as f:
            f.write(kernel(extra))
        try:
            seen, bad, checked = audit_gemm4w.audit(f.name)
        finally:
            os.unlink(f.name)
        assert seen == 1 and len(bad) == n_bad and checked == 1, (extra, seen, bad, checked)


def _gemm4w_unit(names, extra=''):
    """synthetic device assembly of a unit: one kernel per mangled name, each with a 512-MFMA innermost loop (+ extra inside it)"""
    body = '\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]\n' * 512
    text = ''
    for i, name in enumerate(names):
        text += ('%s: ; @k\n\ts_nop 0\n.LBB%d_2: ; %%loop\n ; =>This Inner Loop Header: Depth=1\n' % (name, i) + body + extra +
                 '\ts_cbranch_scc1 .LBB%d_2\n; %%bb.3:\n\ts_endpgm\n' % i)
    for name in names:
        text += '  - .name:           %s\n    .agpr_count:     256\n    .private_segment_fixed_size: 0\n    .vgpr_spill_count: 0\n    .wavefront_size: 64\n' % name
    return text


def test_gemm4w_audit_recognises_production_kernels_of_the_split_units():
    """csrc/gemm4wp.hip is a unit of its own and the parameter block lives in the named namespace omp_gemm: the production instantiations of
    gemm_4w_p as hipcc mangles them there (kernel in the unit's anonymous namespace; GemmP as a substitution, or spelled out as it would be from
    outside omp_gemm) are recognised and go through the stage-loop check, the ablation (ABL = 5) does not; a register copy in the loop of a
    production kernel is still refused."""
    from advancedliteratemachinery_amd import audit
    import tempfile
    prod = ['_ZN8omp_gemm12_GLOBAL__N_19gemm_4w_pIfLb0ELi0ELb0EEEvNS_5GemmPE', '_ZN8omp_gemm12_GLOBAL__N_19gemm_4w_pIDF16bLb1ELi0ELb1EEEvNS_5GemmPE',
            '_ZN12_GLOBAL__N_19gemm_4w_pIDF16bLb0ELi0ELb0EEEvN8omp_gemm5GemmPE']
    abl = ['_ZN8omp_gemm12_GLOBAL__N_19gemm_4w_pIfLb0ELi5ELb0EEEvNS_5GemmPE']
    for extra, n_bad in (('', 0), ('\tv_mov_b32_e32 v1, v2\n', len(prod))):
        with tempfile.NamedTemporaryFile('w', suffix='.s', delete=False) as f:
            f.write(_gemm4w_unit(prod + abl, extra))
        try:
            seen, bad, checked = audit.audit_unit(f.name)
        finally:
            os.unlink(f.name)
        assert seen == len(prod) + 1 and checked == len(prod) and len(bad) == n_bad, (extra, seen, checked, bad)


def test_build_refuses_a_gemm4w_unit_whose_stage_loops_went_unchecked(tmp_path, monkeypatch):
    """The audit finds the production kernels by their mangled names and skips what it does not recognise.  A unit of gemm_4w_r / gemm_4w_p
    kernels of which NONE was recognised (here: the parameter block renamed) must not pass for want of anything to check: build.py's audit
    step refuses it and leaves no audit stamp; the same unit under the names the audit knows passes and is stamped."""
    import pytest
    from advancedliteratemachinery_amd import build as B
    monkeypatch.setattr(B, 'OBJ', str(tmp_path))
    good = ['_ZN8omp_gemm12_GLOBAL__N_19gemm_4w_rIfLb0ELi0EEEvNS_5GemmPE', '_ZN8omp_gemm12_GLOBAL__N_19gemm_4w_rIDF16bLb1ELi0EEEvNS_5GemmPE']
    open(B._asm_of('gemm4wr.hip'), 'w').write(_gemm4w_unit([n.replace('5GemmPE', '6GemmP2E') for n in good]))
    with pytest.raises(RuntimeError, match='stage loop went unchecked'):
        B._audit({'gemm4wr.hip': 'digest'})
    assert not os.path.exists(str(tmp_path / 'gemm4wr.o.audit.stamp'))
    open(B._asm_of('gemm4wr.hip'), 'w').write(_gemm4w_unit(good))
    B._audit({'gemm4wr.hip': 'digest'})
    assert open(str(tmp_path / 'gemm4wr.o.audit.stamp')).read() == 'digest'


def test_rocpd_rate_bins_dispatches_per_window(tmp_path, capsys):
    """tools/rocpd_rate.py (round 6: what bounds the 8-image calls on four lanes) on a synthetic rocpd database: two windows of 20 ms, the first
    with 4 kernels of 5 ms on two queues side by side (concurrency 1.0), the second with one marker kernel."""
    import sqlite3
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import rocpd_rate
    db = str(tmp_path / 'x.db')
    con = sqlite3.connect(db)
    con.execute('create table rocpd_info_kernel_symbol (id integer, display_name text)')
    con.execute('create table rocpd_kernel_dispatch (start integer, end integer, kernel_id integer, queue_id integer)')
    con.executemany('insert into rocpd_info_kernel_symbol values (?, ?)', [(1, 'gemm_small<x>'), (2, 'dec_fused_self_attn_kernel<true, 4>')])
    ms = 1000000
    con.executemany('insert into rocpd_kernel_dispatch values (?, ?, ?, ?)',
                    [(0, 5 * ms, 1, 7), (0, 5 * ms, 1, 8), (10 * ms, 15 * ms, 1, 7), (10 * ms, 15 * ms, 1, 8), (25 * ms, 26 * ms, 2, 7)])
    con.commit()
    con.close()
    argv = sys.argv
    sys.argv = ['rocpd_rate.py', db, '20']
    try:
        rocpd_rate.main()
    finally:
        sys.argv = argv
    lines = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()]
    assert lines[0] == ['t_ms', 'dispatches', 'kernels/ms', 'concurrency', 'queues', 'marker']
    assert lines[1] == ['0', '4', '0.2', '1.00', '2', '0']
    assert lines[2] == ['20', '1', '0.1', '0.05', '1', '1']


def test_plain_run_is_lean_and_full_is_opt_in(monkeypatch):
    """a plain line times exactly --steps steps once and writes no outputs; --full and --dump-outputs are opt-in"""
    b = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '20', '--warmup', '5'])
    a = b.parse()
    assert not a.full and a.dump_outputs is None and a.min_seconds is None
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'out', '--min-seconds', '5'])
    a = b.parse()
    assert a.full and a.dump_outputs == 'out' and a.min_seconds == 5.0


def test_dump_outputs_writes_float32_npy(tmp_path):
    import numpy as np
    import torch
    b = _bench()
    ids = torch.arange(24, dtype=torch.int32).view(2, 3, 4)
    probs = torch.rand(2, 3, 5)
    b.dump_outputs(str(tmp_path / 'd'), dict(ids=ids, probs=probs))
    x, p = np.load(str(tmp_path / 'd' / 'ids.npy')), np.load(str(tmp_path / 'd' / 'probs.npy'))
    assert x.dtype == np.float32 and x.shape == (2, 3, 4) and np.array_equal(x, ids.numpy().astype(np.float32))
    assert p.dtype == np.float32 and np.array_equal(p, probs.numpy())
