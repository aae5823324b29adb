#!/usr/bin/env python
"""OmniParser text-spotting throughput on MI355X (BASELINE.json config 2).

  python bench.py --gpus N --steps K --warmup W
  (N > 1: one rank per GPU over RCCL -- under torch.distributed.run when RANK / WORLD_SIZE are set, otherwise bench.py
   re-launches itself under torch.distributed.run with N ranks; it refuses to run if RCCL does not see exactly N)

Workload ("step" = one batch through the whole hot path): Swin-B -> FPN -> input_proj ->
memory K/V projection -> point decoder -> polygon decoder -> recognition decoder on a batch of
`--batch` synthetic 1024x1024 images per rank, bf16 engine, seeded procedural weights in the
reference's state-dict layout.  Random weights never emit a sensible EOS, so decoding is FORCED to
`--instances` text instances per image: 2*64+6 point steps, 32+2 polygon steps and
25+2 recognition steps, every step a full 4-layer decoder pass for every row.  Nothing is skipped
or cached across steps; images are resident in HBM before the timed region.

Engine scheduling (all inside the timed region): `--coalesce` consecutive steps (default 64) are merged into one engine
call (dynamic batching: the decoder steps then advance coalesce*batch images per launch, the encoder runs them 32 at a
time) and `--lanes` such groups are in flight at once on separate HIP streams (engine/pipeline.py; default 1: with every
phase throughput-bound, one call of 512 images beats two of 256 in flight at the same latency, profiles/r02ze).

Scaling is weak: every rank processes its own `--batch` images per step; ranks exchange one all-gather
of the decoded (padded) sequences per engine call, as a real image-sharded deployment would.

Timing: W warm-up steps, then EXACTLY K steps between barrier + synchronize pairs, MAX over ranks; `ms_per_step` is that
region's time over K.  With --min-seconds S the K-step region is REPEATED (each repetition bracketed the same way) until S
seconds have been measured; `value` then comes from the MEDIAN repetition and the spread is reported (`timing`).  Every
engine call is also bracketed with HIP events on its lane stream (`engine_call_ms`: median / p10 / p90).  Steps use
DISTINCT images (a resident pool of `coalesce` batches).

A plain run measures the headline alone: set-up, warm-up, the K timed steps, the outputs (--dump-outputs DIR: the last
timed step's decoded ids and probabilities as DIR/<name>.npy, float32) and one JSON line on rank 0: images/s (whole job),
chars/s, ms per step.  --full adds everything else: the measured legs on rank 0 -- `batch8` = the same steps with coalesce
1 (every 8-image batch its own engine call: BASELINE config 2's literal batch), `eos_run` = EOS honoured instead of forced
instance counts, the parity engine and BASELINE configs 3 / 4 / 5 -- `roofline` = the dominant kernel class by GPU time
(large-M GEMMs against the 2.5 PFLOP/s bf16 matrix-core peak, or the decoder cross-attention against 8 TB/s), the other
classes under `roofline_other`, all timed live with HIP events on their launch streams, and the CPU baseline (the oracle
= reference algorithm restated on CPU, timed on a bounded sample of the same workload, scaled as its `sample` says).
The --no-* switches turn single parts of --full off.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from advancedliteratemachinery_amd.utils.dist import pack_payload, unpack_payload  # noqa: E402

HBM_PEAK_GBS = 8000.0    # MI355X_MICROARCH.md: HBM3E 8 TB/s peak
MFMA_PEAK_TFS = 2500.0   # MI355X_MICROARCH.md: dense bf16 matrix-core peak


def parse():
    p = argparse.ArgumentParser()
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--rccl-selftest', action='store_true',
                   help='run the N > 1 protocol (RCCL rendezvous, device check, one all-gather per engine call, barriers, max over ranks) with however many ranks there '
                        'are -- ONE on a 1-GPU box: launch under torch.distributed.run exactly as the driver launches N > 1')
    p.add_argument('--steps', type=int, default=192)
    p.add_argument('--warmup', type=int, default=32)
    p.add_argument('--full', action='store_true',
                   help='also run everything beyond the headline: the batch8 / eos_run / parity / config legs, the rooflines and the CPU baseline')
    p.add_argument('--dump-outputs', metavar='DIR', default=None,
                   help='after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32)')
    p.add_argument('--min-seconds', type=float, default=None,
                   help='repeat the K-step timed region until this much time is measured (default: one region; the --full legs: 5)')
    p.add_argument('--no-batch8', action='store_true', help='skip the coalesce-1 (true batch-8 engine calls) leg')
    p.add_argument('--no-eos-run', action='store_true', help='skip the EOS-honouring leg')
    p.add_argument('--eos-pt-len', type=int, default=130, help='pt_seq_length of the EOS-honouring leg (<= 64 instances per image)')
    p.add_argument('--workload', default='spotting', choices=['spotting', 'kie', 'mgp_str'],
                   help="spotting = BASELINE config 2 (the bench line the driver records); kie = config 3 (--infer_vie, batch 32 @ "
                        "960x1280 per GPU); mgp_str = config 5 (MGP-STR ViT-B, batch 512 words).  The side workloads print the same "
                        "JSON line format for their own metric")
    p.add_argument('--batch', type=int, default=None, help='images per GPU per step (default: 8 spotting, 32 kie, 512 mgp_str)')
    p.add_argument('--size', type=int, default=1024)
    p.add_argument('--instances', type=int, default=64, help='forced text instances per image')
    p.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32', 'bf16x3'],
                   help='engine precision: bf16 (BASELINE config 2), fp32, or bf16x3 = the parity engine (fp32 storage, split-bf16 products)')
    p.add_argument('--mgp-logits', type=int, default=0, help='MGP-STR workload: 1 = materialise the fp32 logits of every head, then arg-max (the step of rounds 1-5)')
    p.add_argument('--no-parity-leg', action='store_true', help='skip the parity_engine leg (bf16x3 engine on the same workload)')
    p.add_argument('--no-config-legs', action='store_true', help='skip the summary legs of BASELINE configs 3 / 4 / 5 (kie, long_pt, mgp_str)')
    p.add_argument('--graph', type=int, default=int(os.environ.get('OMP355_GRAPH', '1')))
    p.add_argument('--no-cpu-baseline', action='store_true')
    p.add_argument('--no-roofline', action='store_true')
    p.add_argument('--phase-times', action='store_true', help='also print a per-phase time breakdown (stderr)')
    p.add_argument('--overlap', type=int, default=1, help='polygon || recognition decoders on two streams')
    p.add_argument('--q4-mode', type=int, default=1, help='A/B: omp_debug_cross_q4 selector (1 default, 2 = one 32-key block per step, 4 = chunks with temporal loads)')
    p.add_argument('--dec-fused', type=int, default=0, help='A/B: omp_debug_dec_fused (0 default: fused few-row decoder kernels where they apply, 1 = one launch per op everywhere)')
    p.add_argument('--rows-tile', type=int, default=0, help='A/B: omp_debug_rows_tile (0 = by row count, 2..5 = 16-row tiles per workgroup of every decoder chain launch)')
    p.add_argument('--cross-nt', type=int, default=1, help='A/B: omp_debug_cross_nt selector (1 = non-temporal K / V^T loads always (default), 2 = only from 32 images per launch, 0 = never)')
    p.add_argument('--lanes', type=int, default=int(os.environ.get('OMP355_LANES', '1')),
                   help='step groups in flight per GPU (engine/pipeline.py): they overlap on separate HIP streams')
    p.add_argument('--lane-side', type=int, default=int(os.environ.get('OMP355_LANE_SIDE', '0')),
                   help='1 = every pipeline lane gets two side streams (polygon || recognition); 0 = ONE HIP stream per lane: streams that '
                        'share a hardware queue serialise and with three streams per lane the collisions make small-call pipelines swing '
                        '95-208 img/s (profiles/r03j_lane_sweep_*)')
    p.add_argument('--batch8-lanes', type=int, default=4, help='lanes of the batch8 leg (one 8-image engine call each)')
    p.add_argument('--coalesce', type=int, default=int(os.environ.get('OMP355_COALESCE', '64')),
                   help='consecutive steps (batches of --batch images) merged into one engine call: the decoders then '
                        'advance coalesce*batch images per launch (dynamic batching across steps); 1 = every step alone; '
                        'capped at ceil(steps / lanes) so that every lane gets work')
    return p.parse_args()


def build_model(dtype, graph, device):
    from advancedliteratemachinery_amd.model import OmniParser
    from advancedliteratemachinery_amd.utils.parser import make_args
    from advancedliteratemachinery_amd.utils import synthetic as weights   # seeded procedural checkpoint (data only)
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    sd = weights.make_state_dict(args, seed=0)
    model = OmniParser(args, engine_dtype=dtype)
    model.load_state_dict(sd)
    model = model.to(device)
    model.use_graph = bool(graph)
    return model, args, sd


def phase_breakdown(model, one_step, stream):
    model.phase_events = []
    with torch.cuda.stream(stream):
        one_step()
        torch.cuda.synchronize()
    ev = model.phase_events
    model.phase_events = None
    return {ev[i][0]: ev[i - 1][1].elapsed_time(ev[i][1]) for i in range(1, len(ev))}


def prompts(args):
    nb = args.num_bins
    pt = torch.tensor([[0, 0, nb - 1, nb - 1, nb, nb + len(args.chars), args.pt_sos_index]], dtype=torch.long)
    return [pt, torch.full((1, 1), args.poly_sos_index, dtype=torch.long), torch.full((1, 1), args.rec_sos_index, dtype=torch.long)]


def pin_host_threads(local_rank, ranks_on_node):
    """One rank per GPU on a shared host: give every rank its own slice of the cores it may use, so that N Python launch threads
    (and their lane threads) do not migrate over each other.  Returns the cores this rank was pinned to (or None)."""
    try:
        cores = sorted(os.sched_getaffinity(0))
        if ranks_on_node <= 1 or len(cores) < ranks_on_node:
            return None
        per = len(cores) // ranks_on_node
        mine = cores[local_rank * per:(local_rank + 1) * per]
        os.sched_setaffinity(0, mine)
        return mine
    except (AttributeError, OSError):
        return None


def pmc_traffic(images_per_launch, prefix=''):
    """HBM bytes per cross-attention launch from the rocprofv3 PMC passes (separate runs; tools/pmc_cross_json.py
    turns their summaries into profiles/pmc_cross_attn.json, one record per images-per-launch).  FETCH_SIZE is in KiB
    and counts 16-byte/lane streaming reads at half their size on gfx950 (MI355X_MICROARCH.md, HBM) -> x2;
    WRITE_SIZE is in KiB."""
    path = os.environ.get('OMP355_PMC_JSON', os.path.join(ROOT, 'profiles', 'pmc_cross_attn.json'))
    try:
        with open(path) as f:
            rec = json.load(f)
        if 'images_per_launch' in rec:          # single record (round-1 format)
            rec = {str(rec['images_per_launch']): rec}
        r = rec.get(prefix + str(int(images_per_launch)))   # prefix 'x3_': the split-plane kernels of the parity engine (tools/cross_pmc.py <images> split)
        if r is None:
            return None
        return float(r['fetch_kib_mean']) * 1024.0 * 2.0 + float(r['write_kib_mean']) * 1024.0
    except (OSError, ValueError, KeyError):
        return None


def pmc_gemm_traffic(size, dtype):
    """Measured HBM bytes of the large GEMMs from the rocprofv3 PMC passes over one encoder chunk + its K / V^T projection
    (tools/encode_pmc.py run / summarise -> profiles/pmc_gemm.json): (bytes per launch, measured / algorithmic)."""
    if size != 1024 or dtype != 'bf16':
        return None
    try:
        with open(os.environ.get('OMP355_PMC_GEMM_JSON', os.path.join(ROOT, 'profiles', 'pmc_gemm.json'))) as f:
            s_ = json.load(f)['summary']
        return float(s_['gemm_measured_bytes_per_launch']), float(s_['gemm_measured_over_alg'])
    except (OSError, ValueError, KeyError, TypeError):
        return None


def pmc_mlp_chain_traffic(size, dtype):
    """Measured HBM bytes of the fused MLP + Swin stage-2 chain class from the same passes (profiles/pmc_gemm.json, round 6):
    (bytes per launch, measured / algorithmic)."""
    if size != 1024 or dtype != 'bf16':
        return None
    try:
        with open(os.environ.get('OMP355_PMC_GEMM_JSON', os.path.join(ROOT, 'profiles', 'pmc_gemm.json'))) as f:
            s_ = json.load(f)['summary']
        return float(s_['mlp_chain_measured_bytes_per_launch']), float(s_['mlp_chain_measured_over_alg'])
    except (OSError, ValueError, KeyError, TypeError):
        return None


def pmc_rows_traffic():
    """Measured HBM bytes per launch of the row-owner chain kernels from the rocprofv3 PMC passes over the polygon / recognition phase of a
    160-image engine call (tools/dec_rows_pmc.py -> profiles/pmc_dec_rows.json): (bytes per launch, measured / algorithmic, scope)."""
    try:
        with open(os.environ.get('OMP355_PMC_ROWS_JSON', os.path.join(ROOT, 'profiles', 'pmc_dec_rows.json'))) as f:
            s_ = json.load(f)['summary']
        return float(s_['measured_bytes_per_launch']), float(s_['measured_over_alg']), s_.get('scope', '')
    except (OSError, ValueError, KeyError):
        return None


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: re-run this script under torch.distributed.run, one rank per GPU."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def pct(xs, f):
    xs = sorted(xs)
    if not xs:
        return None
    i = f * (len(xs) - 1)
    lo, hi = int(i), min(int(i) + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (i - lo)


def host_cores():
    """Cores this process may really use: affinity mask, capped by the cgroup CPU quota."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ('/sys/fs/cgroup/cpu.max', '/sys/fs/cgroup/cpu/cpu.cfs_quota_us'):
        try:
            txt = open(path).read().split()
            if path.endswith('cpu.max'):
                if txt[0] != 'max':
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
                    n = min(n, max(1, int(q / per + 0.5)))
        except (OSError, ValueError, IndexError):
            pass
    return max(1, n)


def cpu_baseline(args, sd, size, instances, pt_steps, budget_s=32.0):
    """Reference algorithm (oracle restatement: no KV cache, full prefix re-decoded every step, memory broadcast per instance) on the
    host cores -- `kind: port`: the oracle is pinned to the reference's own classes (tests/test_oracle_vs_reference.py) but it is
    the oracle, not /root/reference, that is timed: the reference does not exist on the GPU box.
      * `value`: ONE complete run of the path at the benchmark's image size with 8 instances per image (pt_seq_length 16: 8 points,
        8 x 32 polygon and 8 x rec_length recognition steps, every step the full reference recomputation), extrapolated x8 to the
        benchmark's 64 instances: t = t_encode + (t_total - t_encode) x (instances / 8)   (the reference's decode cost
        is linear in the instance count -- memory is replicated per instance -- and its point sequence grows with it);
      * `measured_c1`: BASELINE config 1 run COMPLETE (one 640x640 image, Swin-T widths, 16 instances).
    Hosts with fewer than 8 usable cores run the 8-instance leg at half the image size (and say so)."""
    import copy
    from oracle import omniparser_ref as O
    cores = host_cores()
    torch.set_num_threads(min(cores, 64))
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    log = lambda m: print('[cpu_baseline] ' + m, file=sys.stderr, flush=True)  # noqa: E731
    # -- BASELINE config 1 COMPLETE (Swin-T widths, one 640x640 image, pt_seq_length 32 -> 16 instances with their 32-token polygons and
    #    25-token transcriptions; the case of tools/cpu_full_c1.py): ~10 s on 16 threads, skipped on small hosts
    measured_c1 = None
    if cores >= 8:
        from oracle import gen_golden as G_
        case = dict(args=dict(tfm_pre_norm=True, use_fpn=False, use_char_window_prompt=True, pt_seq_length=32),
                    hw=(640, 640), depths=(2, 2, 6, 2), swin=dict(embed_dim=96, num_heads=(3, 6, 12, 24)))
        a1, sd1, img1, mask1_, seqs1 = G_.case_inputs(case)
        with torch.no_grad():
            t0 = time.time()
            out1 = O.forward(sd1, a1, img1, mask1_, seqs1, depths=case['depths'], num_heads=case['swin']['num_heads'])
            t_c1 = time.time() - t0
        n1 = 0 if out1 is None else int(out1[0][0].numel()) // 2
        measured_c1 = dict(value=1.0 / t_c1, unit='images/s', seconds=t_c1, image_size=640, instances=n1, chars_per_sec=n1 * a1.rec_length / t_c1,
                           sample='BASELINE config 1 run COMPLETE, not extrapolated: oracle.forward on one 640x640 image, Swin-T widths (embed 96, depths 2-2-6-2, '
                                  'no FPN), pt_seq_length 32 (%d instances), %d threads' % (n1, min(cores, 64)))
        log('config 1 complete: 640x640, %d instances: %.2fs' % (n1, t_c1))
        del sd1, img1
    # -- the benchmark's own configuration, 8 instances, complete
    n_s = 8
    side = size if cores >= 8 else max(64, size // 2)
    small = copy.copy(args)
    small.pt_seq_length = 2 * n_s
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        img = torch.randn(1, 3, side, side, generator=g)
        msk = torch.zeros(1, side, side, dtype=torch.bool)
        t0 = time.time()
        O.encode(sd, args, img, msk)
        t_enc = time.time() - t0
        log('encode %dx%d: %.2fs (cores=%d)' % (side, side, t_enc, cores))
        t0 = time.time()
        out_s = O.forward(sd, small, img, msk, O.default_prompts(small))
        t_all = time.time() - t0
    n_got = 0 if out_s is None else int(out_s[0][0].numel()) // 2
    log('complete run %dx%d, %d instances: %.2fs' % (side, side, n_got, t_all))
    if n_got <= 0:
        raise RuntimeError('cpu_baseline: the oracle decoded no instance')
    px = (size / float(side)) ** 2            # 1.0 unless the host is small
    t_dec = max(t_all - t_enc, 0.0)
    t_total = t_enc * px + t_dec * (instances / float(n_got)) * px   # the decoders' memory has (side/16)^2 tokens: linear in pixels too
    measured = dict(value=1.0 / t_all, unit='images/s', seconds=t_all, encode_seconds=t_enc, image_size=side, instances=n_got,
                    chars_per_sec=n_got * args.rec_length / t_all)
    return dict(value=1.0 / t_total, unit='images/s', cores=cores, kind='port', estimated=True, measured_n8=measured, measured_c1=measured_c1,
                sample=('oracle (CPU restatement of the reference path, pinned to the reference classes; fp32, %d threads): ONE COMPLETE run of the path on a '
                        '%dx%d image with %d instances (pt_seq_length %d: %d point tokens, %d x 32 polygon and %d x %d recognition steps) measured '
                        '%.1fs (encode %.2fs of it); `value` extrapolates the decode part x%.1f to the benchmark\'s %d instances%s: %.1fs per image'
                        % (min(cores, 64), side, side, n_got, small.pt_seq_length, 2 * n_got, n_got, n_got, args.rec_length, t_all, t_enc,
                           instances / float(n_got), instances, (' and everything x%.0f to %dx%d pixels (fewer than 8 host cores)' % (px, size, size)) if px != 1.0 else '',
                           t_total)),
                chars_per_sec=instances * args.rec_length / t_total)


# ---------------------------------------------------------------------------------------------------------------------
# side workloads (BASELINE configs 3 and 5): same timing protocol, their own metric
# ---------------------------------------------------------------------------------------------------------------------
def _timed_loop(a, world, device, step):
    """W warm-up steps, then exactly K steps between barrier + synchronize pairs (max over ranks), repeated until
    --min-seconds are measured; -> (median seconds per K steps, all repetitions)."""
    def barrier():
        if world > 1:
            dist.barrier()
    for i in range(a.warmup):
        step(i)
    reps = []
    while True:
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(i)
        torch.cuda.synchronize()
        barrier()
        el = time.perf_counter() - t0
        stop = 0.0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        reps.append(el)
        stop = 1.0 if (sum(reps) >= (a.min_seconds or 0.0) or len(reps) >= 64) else 0.0
        if world > 1:
            t = torch.tensor([stop], device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            stop = float(t.item())
        if stop > 0:
            return pct(reps, 0.5), reps


def _class_roofline(lib, cls, eager_steps, kernel_name, peak, unit, scale):
    """hipEvent-bracketed launches of one kernel class over `eager_steps()` -> roofline record (work / time vs peak)."""
    lib.omp_prof_enable(1 << cls)
    eager_steps()
    torch.cuda.synchronize()
    ms, cnt, work = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    lib.omp_prof_read_class(cls, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(work))
    lib.omp_prof_enable(0)
    if cnt.value == 0 or ms.value <= 0:
        return None
    ach = work.value / (ms.value * 1e-3) / scale
    return dict(bound='mfma' if unit == 'TFLOP/s' else 'hbm', kernel=kernel_name, achieved=ach, peak=peak, unit=unit, frac=ach / peak,
                traffic=None, launches=int(cnt.value), avg_us=ms.value * 1e3 / cnt.value,
                note='hipEvent-bracketed eager launches on their launch stream; no PMC pass for this workload (traffic null)')


def run_mgp_str(a, device, world, rank):
    """BASELINE config 5: MGP-STR (ViT-B patch 4, 32x128), batch 512 cropped words per GPU, bf16; step = one forward
    (encoder, three A^3 modules + heads) + greedy ids / probabilities of the three granularities on the device."""
    from advancedliteratemachinery_amd import _lib, ops
    from advancedliteratemachinery_amd.model.mgp_str import MGPSTR
    from advancedliteratemachinery_amd.utils import synthetic as W
    B = a.batch or 512
    c = W.mgp_cfg()
    sd = W.make_mgp_state_dict(c, seed=0)
    model = MGPSTR(engine_dtype=a.dtype)
    model.load_reference_state_dict({'module.' + k: v for k, v in sd.items()})
    model = model.to(device)
    g = torch.Generator().manual_seed(99 + rank)
    pool = [(torch.rand(B, 3, 32, 128, generator=g) * 2 - 1).to(device) for _ in range(2)]
    stream = torch.cuda.Stream(device=device)
    last = {}

    def step(i):
        # recognition as MGPSTR.recognize runs it: encoder, three A^3 modules, heads, greedy ids + probabilities on the device.  Since round 6 the wide
        # heads decode from the head product's row statistics (no 2.8 / 1.7 GB logits tensors: `--mgp-logits 1` times the logits + arg-max pass)
        if a.mgp_logits:
            outs = model(pool[i % 2])
            last['ids'] = [ops.row_argmax_prob(lg.reshape(B * lg.shape[1], -1)) for lg in outs]
        else:
            last['ids'] = model.greedy(pool[i % 2])
    with torch.cuda.stream(stream):
        el, reps = _timed_loop(a, world, device, step)
        if a.dump_outputs and rank == 0:
            torch.cuda.synchronize()
            names = ('char', 'bpe', 'wp')
            dump_outputs(a.dump_outputs, dict([(n + '_ids', i) for n, (i, _) in zip(names, last['ids'])] +
                                              [(n + '_prob', p_) for n, (_, p_) in zip(names, last['ids'])]))
        roof = _class_roofline(_lib.lib(), 1, lambda: [step(i) for i in range(2)],
                               'gemm_256 / gemm_dma (ViT-B q / k / v / proj / fc1 / fc2, A^3 modules, vocabulary heads)', MFMA_PEAK_TFS, 'TFLOP/s', 1e12) if not a.no_roofline else None
    wps = world * B * a.steps / el
    res = dict(metric='words/sec, MGP-STR recogniser (ViT-B patch4 32x128)', value=wps, unit='words/s', n_gpus=world, steps=a.steps, warmup=a.warmup,
               ms_per_step=el / a.steps * 1e3, higher_is_better=True, scaling='weak', vs_baseline=None, dtype=a.dtype, data='synthetic',
               timing=dict(repeats=len(reps), seconds_measured=sum(reps), ms_per_step_p10=pct(reps, 0.1) / a.steps * 1e3, ms_per_step_p90=pct(reps, 0.9) / a.steps * 1e3),
               config=dict(workload='MGP-STR (BASELINE config 5), ViT-B patch4 32x128, batch %d words/GPU, %s, three granularities decoded greedily on the device%s' % (B, a.dtype, ' (logits materialised)' if a.mgp_logits else ' (wide heads from row statistics, no logits tensor)'),
                           global_batch=world * B, parallelism='word-sharded dp%d' % world, tflops_model=49.8e9 * wps / 1e12),
               roofline=roof)
    if rank == 0 and not a.no_cpu_baseline:
        from oracle import mgp_str_ref as R
        torch.set_num_threads(min(host_cores(), 64))
        sdf = {k: v.float() for k, v in sd.items()}
        img = pool[0][:2].float().cpu()
        with torch.no_grad():
            R.forward(sdf, c, img)
            t0 = time.time()
            n = 0
            while time.time() - t0 < 10.0:
                R.forward(sdf, c, img)
                n += 1
        dtc = (time.time() - t0) / n
        res['cpu_baseline'] = dict(value=2.0 / dtc, unit='words/s', cores=min(host_cores(), 64), kind='port',
                                   sample='oracle/mgp_str_ref.py forward (fp32) on 2 words, %d repetitions in %.1f s' % (n, time.time() - t0))
    return res


def run_kie(a, device, world, rank):
    """BASELINE config 3: OmniParser KIE (--infer_vie, SROIE-style classes), Swin-B, batch 32 @ 1280x960 per GPU, bf16.
    Random weights: decoding is forced to --instances point-sequence items per image (3 tokens each with --infer_vie);
    the entity walk (transformer.py:143-217) then decodes polygon + recognition for every word it finds."""
    from advancedliteratemachinery_amd import _lib
    from advancedliteratemachinery_amd.model import OmniParser
    from advancedliteratemachinery_amd.utils.parser import make_args
    from advancedliteratemachinery_amd.utils import synthetic as weights
    B, N = a.batch or 32, a.instances
    H, Wd = 960, 1280
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True, infer_vie=True, vie_categories=4, val_dataset=['sroie_val'])
    sd = weights.make_state_dict(args, seed=0)
    model = OmniParser(args, engine_dtype=a.dtype)
    model.load_state_dict(sd)
    model = model.to(device)
    model.use_graph = bool(a.graph)
    model.overlap_decoders = bool(a.overlap)
    seqs = prompts(args) + [torch.tensor([H, Wd])]
    g = torch.Generator().manual_seed(77 + rank)
    pool = [torch.randn(B, 3, H, Wd, generator=g).to(device) for _ in range(2)]
    mask = torch.zeros(B, H, Wd, dtype=torch.bool, device=device)
    stream = torch.cuda.Stream(device=device)
    stats = dict(entities=0, words=0, images=0)

    def step(i):
        res = model.infer(pool[i % 2], mask, seqs, forced_instances=N, has_padding=False)
        for r in res:
            stats['images'] += 1
            if r:
                stats['entities'] += len(r)
                stats['words'] += sum(len(t[3]) for t in r)
    with torch.cuda.stream(stream):
        el, reps = _timed_loop(a, world, device, step)
        roof = None
        if not a.no_roofline:
            model.use_graph = False
            roof = _class_roofline(_lib.lib(), 1, lambda: step(0), 'gemm_256 / gemm_dma (Swin-B, FPN, input_proj, K-V projection, large-row decoder GEMMs)',
                                   MFMA_PEAK_TFS, 'TFLOP/s', 1e12)
    ips = world * B * a.steps / el
    return dict(metric='images/sec (1280x960), OmniParser KIE (--infer_vie)', value=ips, unit='images/s', n_gpus=world, steps=a.steps, warmup=a.warmup,
                ms_per_step=el / a.steps * 1e3, higher_is_better=True, scaling='weak', vs_baseline=None, dtype=a.dtype, data='synthetic',
                timing=dict(repeats=len(reps), seconds_measured=sum(reps), ms_per_step_p10=pct(reps, 0.1) / a.steps * 1e3, ms_per_step_p90=pct(reps, 0.9) / a.steps * 1e3),
                config=dict(workload='OmniParser KIE (BASELINE config 3), Swin-B, batch %d/GPU @ 1280x960, forced %d point-sequence items/image, %s' % (B, N, a.dtype),
                            global_batch=world * B, image_size=[H, Wd], parallelism='image-sharded dp%d' % world,
                            words_per_image=stats['words'] / max(1, stats['images']), entities_per_image=stats['entities'] / max(1, stats['images'])),
                roofline=roof)


class StepLoop(object):
    """The part of the bench line that must be right on N GPUs, as an object (tests/test_bench_loop.py drives it over world-2 gloo with a stub
    engine): K steps in groups of `group` consecutive steps per engine call, ONE all-gather of the packed payload per engine call issued in
    step order from the calling thread, a barrier + synchronize pair on both sides of EXACTLY K steps, the MAX over ranks of the elapsed
    time, the stop decision of the repetition loop all-reduced so that every rank takes the same one, every rank's own ms per step gathered.
    run_group(first_step, n_steps, lane, forced) -> (ids int32 [b, N, T], probs fp32 [b, N, L]) is the engine call; on a CPU device
    (the tests) the stream / event calls are skipped, the protocol is the same."""

    def __init__(self, run_group, world, rank, device, group, pools=None, collectives=None):
        self.run_group, self.world, self.rank, self.device, self.G = run_group, world, rank, device, group
        # collectives: run the N > 1 protocol (default: world > 1; --rccl-selftest turns it on for ONE rank, the only RCCL run a 1-GPU box allows)
        self.coll = (world > 1) if collectives is None else bool(collectives)
        self.cuda = device.type == 'cuda'
        self.pools = pools if pools is not None else {'active': None}
        self.gather_ev = []   # (start, end) events around every all-gather of the timed region (cuda)
        self.local_s = []     # this rank's own time of every repetition (before the max over ranks)
        self.n_gathers = 0

    def sync(self):
        if self.cuda:
            torch.cuda.synchronize()

    def barrier(self):
        if self.coll:
            dist.barrier()

    def exchange(self, ids, probs):
        if not self.coll:
            return ids, probs
        e0 = e1 = None
        if self.cuda:
            # results were produced on a lane stream and are consumed by RCCL on this one: tell the caching allocator
            ids.record_stream(torch.cuda.current_stream())
            probs.record_stream(torch.cuda.current_stream())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        # ONE collective per engine call: ids and probability bit patterns in one int32 payload (utils/dist.py::pack_payload)
        payload = pack_payload(ids, probs)
        buf = torch.empty(self.world * payload.shape[0], payload.shape[1], dtype=torch.int32, device=self.device)
        dist.all_gather_into_tensor(buf, payload)
        all_ids, all_pr, _ = unpack_payload(buf, ids.shape[1:], probs.shape[1:], with_n=False)
        self.n_gathers += 1
        if self.cuda:
            e1.record()
            self.gather_ev.append((e0, e1))
        return all_ids, all_pr

    def run_steps(self, k, group=None, forced=None):
        """k steps = k batches through the whole hot path, in groups of `group` consecutive steps per engine call.
        With lanes > 1 consecutive groups are in flight on different HIP streams (lane threads enqueue them); the
        all-gather of the decoded sequences (one per group) is issued from THIS thread in step order, after the
        lane's completion event, so every rank calls the collectives in the same order."""
        group = group or self.G
        sizes = [group] * (k // group) + ([k % group] if k % group else [])
        firsts = [sum(sizes[:i]) for i in range(len(sizes))]
        out = None
        pl = self.pools['active']
        if pl is None:
            for f0, g_ in zip(firsts, sizes):
                ids, probs = self.run_group(f0, g_, None, forced)
                out = self.exchange(ids, probs)
            return out
        futs = [pl.submit(lambda lane, f0=f0, g_=g_: self.run_group(f0, g_, lane, forced)) for f0, g_ in zip(firsts, sizes)]
        for f in futs:
            (ids, probs), ev = f.result()
            ev.wait()   # LaneEvent: inside the capture gate (engine/pipeline.py)
            out = self.exchange(ids, probs)
        return out

    def timed(self, k, group=None, forced=None):
        """EXACTLY k steps between barrier + synchronize pairs; MAX over ranks."""
        self.sync()
        self.barrier()
        t0 = time.perf_counter()
        out = self.run_steps(k, group, forced)
        self.sync()
        self.barrier()
        el = time.perf_counter() - t0
        self.local_s.append(el)
        if self.coll:
            t = torch.tensor([el], dtype=torch.float64, device=self.device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, out

    def repeat(self, k, min_seconds, max_reps=64, group=None, forced=None):
        """timed(k) until min_seconds are measured (or max_reps): every rank takes the SAME stop decision (all-reduced).  -> (reps, last out)"""
        reps, out = [], None
        while True:
            el, out = self.timed(k, group, forced)
            reps.append(el)
            stop = sum(reps) >= min_seconds or len(reps) >= max_reps
            if self.coll:
                t = torch.tensor([1.0 if stop else 0.0], device=self.device)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                stop = bool(t.item() > 0)
            if stop:
                return reps, out

    def per_rank_ms(self, steps):
        """every rank's own median ms per step (before the max over ranks), gathered on all ranks"""
        if not self.coll:
            return None
        mine = torch.tensor([pct(self.local_s, 0.5) / steps * 1e3], dtype=torch.float64, device=self.device)
        allr = torch.empty(self.world, dtype=torch.float64, device=self.device)
        dist.all_gather_into_tensor(allr, mine)
        return [float(v) for v in allr.tolist()]


def dump_outputs(dirname, arrays):
    """--dump-outputs: every array as DIR/<name>.npy in float32 (the ids are exact: they are far below 2^24)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    host = {k: v.detach().float().cpu().contiguous().numpy() for k, v in arrays.items()}
    total = sum(v.nbytes for v in host.values())
    if total > 64 << 20:
        raise SystemExit('--dump-outputs: %d bytes of outputs, more than 64 MB' % total)
    for k, v in host.items():
        np.save(os.path.join(dirname, k + '.npy'), v)


def main():
    a = parse()
    if not a.full:
        # a plain run measures the headline alone; the --no-* switches below only matter under --full
        a.no_batch8 = a.no_eos_run = a.no_parity_leg = a.no_config_legs = a.no_roofline = a.no_cpu_baseline = True
    if a.dump_outputs and a.workload == 'kie':
        raise SystemExit('--dump-outputs: the spotting and mgp_str workloads (kie returns per-image entity records, not arrays)')
    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(spawn_ranks(a.gpus))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if a.gpus != world:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d' % (a.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X (no CPU fallback for the hot path)')
    if torch.cuda.device_count() < world:
        raise SystemExit('--gpus %d but only %d GPUs are visible' % (world, torch.cuda.device_count()))
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    dist_on = world > 1 or a.rccl_selftest   # (--rccl-selftest: the N > 1 protocol over RCCL with ONE rank, as torch.distributed.run launches it)
    if dist_on:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', init_method='env://', device_id=device)
        # RCCL must see exactly N ranks on N distinct devices
        seen = torch.zeros(world, dtype=torch.int32, device=device)
        seen[rank] = 1 + local
        dist.all_reduce(seen)
        if dist.get_world_size() != a.gpus or int((seen > 0).sum()) != a.gpus or len(set(seen.tolist())) != a.gpus:
            raise SystemExit('RCCL sees %d ranks / devices %s, expected %d distinct' % (dist.get_world_size(), seen.tolist(), a.gpus))

    pinned = pin_host_threads(local, world)
    rank_diag = None
    if dist_on:
        # what RCCL actually sees: every rank's (rank, device index, device name, pinned cores) -- the first SCALE run is self-diagnosing
        info = dict(rank=rank, local_rank=local, device=torch.cuda.current_device(), name=torch.cuda.get_device_name(local),
                    pinned_cores=len(pinned) if pinned else None)
        gathered = [None] * world
        dist.all_gather_object(gathered, info)
        rank_diag = gathered
    if a.workload != 'spotting':
        res = (run_mgp_str if a.workload == 'mgp_str' else run_kie)(a, device, world, rank)
        if rank == 0:
            print(json.dumps(res), flush=True)
        if dist_on:
            dist.destroy_process_group()
        return
    a.batch = a.batch or 8

    from advancedliteratemachinery_amd import _lib
    if a.q4_mode != 1:
        _lib.check(_lib.lib().omp_debug_cross_q4(a.q4_mode), 'omp_debug_cross_q4')
    if a.cross_nt != 1:
        _lib.check(_lib.lib().omp_debug_cross_nt(a.cross_nt), 'omp_debug_cross_nt')
    if a.dec_fused != 0:
        _lib.check(_lib.lib().omp_debug_dec_fused(a.dec_fused), 'omp_debug_dec_fused')
    if a.rows_tile != 0:
        _lib.check(_lib.lib().omp_debug_rows_tile(a.rows_tile), 'omp_debug_rows_tile')
    model, args, sd = build_model(a.dtype, a.graph, device)
    model.overlap_decoders = bool(a.overlap)
    model.engine()   # pack the weights once, before any lane thread asks for them
    B, N = a.batch, a.instances
    seqs = prompts(args)
    stream = torch.cuda.Stream(device=device)

    from advancedliteratemachinery_amd.engine.pipeline import LanePool
    lanes = max(1, a.lanes)
    pool = LanePool(device, lanes, side_streams=bool(a.lane_side)) if lanes > 1 else None
    pools = {'active': pool, 'b8': None}   # the batch-8 leg pipelines its small engine calls over two lanes of its own

    # steps per engine call: `coalesce`, but never so many that a lane would stay idle in a short run
    G = max(1, min(a.coalesce, -(-a.steps // lanes)))
    # resident pool of DISTINCT batches (step s uses batch s % POOL); in HBM before the timed region starts
    POOL = max(G, 1)
    g = torch.Generator(device='cpu').manual_seed(1234 + rank)
    batches = [torch.randn(B, 3, a.size, a.size, generator=g).to(device) for _ in range(POOL)]
    mask1 = torch.zeros(B, a.size, a.size, dtype=torch.bool, device=device)
    calls = []   # (start event, end event, images) of every engine call, recorded on its lane stream

    def run_group(first_step, g_, lane=None, forced=N, model=model):   # StepLoop's engine call
        """steps first_step .. first_step+g_-1 as ONE engine call: their batches arrive as separate tensors and are
        concatenated here, inside the timed region, as a serving engine would have to."""
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        if g_ == 1:
            gi, gm = batches[first_step % POOL], mask1
        else:
            gi = torch.cat([batches[(first_step + i) % POOL] for i in range(g_)], 0)
            gm = mask1.expand(g_, B, a.size, a.size).reshape(g_ * B, a.size, a.size)
        # packed: the padded all-gather payload comes out of ONE device kernel (ops.pack_spotting), no per-image host work
        ids_, probs_, n_ = model.infer(gi, gm, seqs, forced_instances=forced, has_padding=False, lane=lane, packed=N)
        inst_log.append(n_)      # instances per image (device int32): read by the EOS leg after its timed region
        if len(inst_log) > 4096:
            del inst_log[:2048]
        out = (ids_, probs_)
        ev1.record()
        calls.append((ev0, ev1, B * g_))
        return out

    inst_log = []
    loop = StepLoop(lambda f0, g_, lane, forced: run_group(f0, g_, lane, N if forced == 'N' else forced), world, rank, device, G, pools, collectives=dist_on)
    # (forced: 'N' = the benchmark's forced instance count, None = EOS honoured)
    run_steps = lambda k, group=None, forced='N': loop.run_steps(k, group, forced)     # noqa: E731
    timed = lambda k, group=None, forced='N': loop.timed(k, group, forced)             # noqa: E731
    gather_ev, local_s = loop.gather_ev, loop.local_s

    with torch.cuda.stream(stream):
        # untimed set-up: every lane (or the model itself) allocates its buffers and captures its graphs for
        # both group sizes the timed region will use (full groups and the remainder group)
        for g_ in sorted({G, a.steps % G, a.warmup % G} - {0}):
            for _ in range(lanes):
                run_steps(g_)
        run_steps(a.warmup)
        torch.cuda.synchronize()
        del calls[:]
        del gather_ev[:]
        del local_s[:]
        reps, out = loop.repeat(a.steps, a.min_seconds or 0.0, 64, forced='N')
        torch.cuda.synchronize()
        if a.dump_outputs and rank == 0:
            # the last timed step = the last `B` images of every rank's share of the last engine call's all-gathered result
            last_g = a.steps % G or G
            ids_, probs_ = out
            dump_outputs(a.dump_outputs, dict(ids=ids_.reshape(world, last_g * B, *ids_.shape[1:])[:, -B:].reshape(world * B, *ids_.shape[1:]),
                                              probs=probs_.reshape(world, last_g * B, *probs_.shape[1:])[:, -B:].reshape(world * B, *probs_.shape[1:])))
        call_ms = [e0.elapsed_time(e1) for e0, e1, _ in calls]
        call_imgs = calls[0][2] if calls else B * G
    elapsed = pct(reps, 0.5)
    per_rank_ms = loop.per_rank_ms(a.steps)
    gather_ms = [e0.elapsed_time(e1) for e0, e1 in gather_ev] if dist_on else None
    total_images = world * B * a.steps
    ips = total_images / elapsed
    # sanity: the forced workload really produced N instances x rec_length chars per image
    ids, _ = out
    last_g = a.steps % G or G
    assert ids.shape[0] == world * B * last_g and int((ids[:, :, 34:] >= args.num_bins).all()), 'decode output malformed'

    extra = {}
    leg_seconds = 5.0 if a.min_seconds is None else a.min_seconds   # the batch8 / eos_run legs' own repetition budget (--full)
    def leg(name, fn):
        try:
            extra[name] = fn()
        except Exception as e:  # noqa: BLE001 -- a failed side leg is reported, it must not lose the headline
            extra[name] = dict(error='%s: %s' % (type(e).__name__, e))

    def batch8_leg():
        # BASELINE config 2 literally: every batch of 8 images its own engine call (no cross-step coalescing)
        lanes8 = max(lanes, a.batch8_lanes)
        if pools['active'] is None:
            pools['b8'] = LanePool(device, lanes8, side_streams=bool(a.lane_side))
            pools['active'] = pools['b8']
        with torch.cuda.stream(stream):
            for _ in range(2):
                run_steps(lanes8, group=1)    # every lane allocates its buffers and captures its graphs
            k8 = max(min(a.steps, 32), 4 * lanes8)
            r8 = []
            # two lanes of 8-image calls interleave differently from run to run (96 .. 139 img/s over four 128-step runs,
            # profiles/r02zb): several short repetitions, median and spread reported
            while (sum(r8) < min(leg_seconds, 6.0) or len(r8) < 4) and len(r8) < 12:
                r8.append(timed(k8, group=1)[0])
        e8 = pct(r8, 0.5)
        pools['active'] = pool
        return dict(images_per_sec=B * k8 / e8, ms_per_step=e8 / k8 * 1e3, steps=k8, repeats=len(r8),
                    ms_per_step_p10=pct(r8, 0.1) / k8 * 1e3, ms_per_step_p90=pct(r8, 0.9) / k8 * 1e3,
                    note='coalesce 1: one engine call per 8-image batch, %d lanes, %s' % (lanes8, 'two side streams per lane' if a.lane_side else 'one HIP stream per lane'))
    def eos_leg():
        # EOS honoured (no forced instance count) on the sharpened synthetic checkpoint; the point sequence is
        # capped at --eos-pt-len tokens so that an image yields at most 64 instances, as in the forced workload
        keep = args.pt_seq_length
        args.pt_seq_length = a.eos_pt_len
        try:
            # the same pipeline as the batch8 leg (every lane polls the EOS flags of its own call: the polls block that lane only)
            lanes8 = max(lanes, a.batch8_lanes)
            if pools['active'] is None:
                if pools['b8'] is None:
                    pools['b8'] = LanePool(device, lanes8, side_streams=bool(a.lane_side))
                pools['active'] = pools['b8']
            with torch.cuda.stream(stream):
                ke = max(min(a.steps, 32), 4 * lanes8)
                for _ in range(2):
                    run_steps(lanes8, group=1, forced=None)
                torch.cuda.synchronize()
                del inst_log[:]
                re_ = []
                while (sum(re_) < min(leg_seconds, 4.0) or len(re_) < 3) and len(re_) < 10:
                    re_.append(timed(ke, group=1, forced=None)[0])
                n_inst = torch.cat(inst_log).tolist()
            ee = pct(re_, 0.5)
            per_img = sum(n_inst) / max(1, len(n_inst))
            return dict(images_per_sec=B * ke / ee, steps=ke, repeats=len(re_), ms_per_step_p10=pct(re_, 0.1) / ke * 1e3,
                        ms_per_step_p90=pct(re_, 0.9) / ke * 1e3, mean_instances_per_image=per_img,
                        chars_per_sec=B * ke * per_img * args.rec_length / ee,
                        note='EOS honoured, pt_seq_length %d, one engine call per 8-image batch, %d single-stream lanes' % (a.eos_pt_len, lanes8))
        finally:
            args.pt_seq_length = keep
            pools['active'] = pool

    def measure_rooflines(mdl, dtype_name, n_groups):
        """Kernel classes of engine `mdl` timed with HIP events over `n_groups` eager engine calls -> (dominant class, other classes)."""
        # Kernel classes timed with HIP events on their launch streams over the same engine calls as the timed region,
        # launched eagerly on one stream (events cannot bracket kernels inside a graph replay; one lane so that a
        # kernel's duration is its own): large-M GEMMs and the fused MLP (matrix-core bound, flops counted by the
        # library per launch) and the decoder cross-attention (HBM bound: streams K and V^T of every image once per
        # launch, shared by all query rows).
        was = mdl.use_graph
        mdl.use_graph = False
        h = _lib.lib()
        with torch.cuda.stream(stream):
            run_group(0, G, model=mdl)
            torch.cuda.synchronize()
            h.omp_prof_enable(31)
            for i in range(n_groups):
                run_group(i * G, G, model=mdl)
            torch.cuda.synchronize()

        def read(cls):
            tot, cnt, work = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0)
            h.omp_prof_read_class(cls, ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(work))
            return tot.value, cnt.value, work.value
        def read_roof(cls):
            by, rs = ctypes.c_double(0), ctypes.c_double(0)
            h.omp_prof_read_roofline(cls, ctypes.byref(by), ctypes.byref(rs))
            return by.value, rs.value
        t_cross, n_cross, _ = read(0)
        t_gemm, n_gemm, f_gemm = read(1)
        t_mlp, n_mlp, f_mlp = read(2)
        t_gd, n_gd, f_gd = read(3)   # the same GEMM kernels on decoder-phase rows (M < 32768: the 10240-row polygon / recognition products)
        t_rw, n_rw, f_rw = read(4)   # round 5: the decoders' many-row Linear layers as row-owner chains (csrc/dec_rows.hip)
        (b_gemm, r_gemm), (b_mlp, r_mlp), (b_gd, r_gd), (b_rw, r_rw) = read_roof(1), read_roof(2), read_roof(3), read_roof(4)
        h.omp_prof_enable(0)
        mdl.use_graph = was
        M = (a.size // 16) ** 2
        esz = 2 if dtype_name == 'bf16' else 4   # bytes per (key, dim) of the K / V^T slabs: bf16; fp32, or split-bf16 planes [hi | lo] (bf16x3)
        BI = B * G   # images per launch
        recs = []
        if n_gemm:
            tf = f_gemm / (t_gemm / 1e3) / 1e12
            gt = pmc_gemm_traffic(a.size, dtype_name)
            grec = dict(bound='mfma', kernel='gemm_256 + gemm_dma<128,128,2> + gemm_4w + gemm_4w_p at M >= 32768 rows (Swin qkv / proj / fc1 / fc2 / merge, FPN, input_proj, K-V projection)',
                        achieved=tf, peak=MFMA_PEAK_TFS, unit='TFLOP/s', frac=tf / MFMA_PEAK_TFS, traffic=gt[0] if gt else None,
                        launches=int(n_gemm), avg_us=t_gemm / n_gemm * 1e3, flops_per_launch=f_gemm / n_gemm,
                        gpu_ms_per_image=t_gemm / (n_groups * BI))
            # the class mixes matrix-core-bound (stage 2 / 3) and HBM-bound products (K = 128 / 256, fp32 decoder outputs): the time
            # its launches would take on their OWN rooflines, max(flops / 2.5 PF, algorithmic bytes / 8 TB/s) each, over the measured time
            grec['alg_bytes_per_launch'] = b_gemm / n_gemm
            grec['frac_of_launch_rooflines'] = r_gemm / (t_gemm / 1e3)
            if gt:
                grec['traffic_over_algorithmic'] = gt[1]
                grec['traffic_scope'] = 'HBM bytes per tile-GEMM launch of one 80-image encoder chunk (profiles/pmc_gemm.json, tools/encode_pmc.py)'
            recs.append((t_gemm, grec))
        if n_gd:
            tf = f_gd / (t_gd / 1e3) / 1e12
            recs.append((t_gd, dict(bound='mfma', kernel='gemm_256 / gemm_dma<128,128,2> on decoder-phase rows (M < 32768: the many-row polygon / recognition steps; '
                                                        'on the unbracketed 64x64 kernel until round 4)',
                                    achieved=tf, peak=MFMA_PEAK_TFS, unit='TFLOP/s', frac=tf / MFMA_PEAK_TFS, traffic=None, launches=int(n_gd),
                                    avg_us=t_gd / n_gd * 1e3, flops_per_launch=f_gd / n_gd, alg_bytes_per_launch=b_gd / n_gd,
                                    frac_of_launch_rooflines=r_gd / (t_gd / 1e3), gpu_ms_per_image=t_gd / (n_groups * BI))))
        if n_rw:
            tf = f_rw / (t_rw / 1e3) / 1e12
            rt_ = pmc_rows_traffic()
            recs.append((t_rw, dict(bound='mfma', kernel='dec_rows_mid_kernel / dec_rows_ffn_kernel (row-owner chains: the Linear layers of the many-row polygon / recognition '
                                                        'steps, two launches per decoder layer; on gemm_256 / gemm_dma launches until round 5)',
                                    achieved=tf, peak=MFMA_PEAK_TFS, unit='TFLOP/s', frac=tf / MFMA_PEAK_TFS, traffic=rt_[0] if rt_ else None, launches=int(n_rw),
                                    avg_us=t_rw / n_rw * 1e3, flops_per_launch=f_rw / n_rw, alg_bytes_per_launch=b_rw / n_rw,
                                    frac_of_launch_rooflines=r_rw / (t_rw / 1e3), gpu_ms_per_image=t_rw / (n_groups * BI),
                                    **(dict(traffic_over_algorithmic=rt_[1], traffic_scope=rt_[2]) if rt_ else {}))))
        if n_mlp:
            tf = f_mlp / (t_mlp / 1e3) / 1e12
            mt_ = pmc_mlp_chain_traffic(a.size, dtype_name)
            recs.append((t_mlp, dict(bound='mfma', kernel='mlp_fused_kernel (Swin stages 0/1: LayerNorm + fc1 + GELU + fc2 + residual) + dec_rows_ffn_kernel on Swin stage 2 (round 5: a block minus its window attention as one row-owner chain)',
                                     achieved=tf, peak=MFMA_PEAK_TFS, unit='TFLOP/s', frac=tf / MFMA_PEAK_TFS, traffic=mt_[0] if mt_ else None,
                                     launches=int(n_mlp), avg_us=t_mlp / n_mlp * 1e3, flops_per_launch=f_mlp / n_mlp,
                                     alg_bytes_per_launch=b_mlp / n_mlp, frac_of_launch_rooflines=r_mlp / (t_mlp / 1e3),
                                     gpu_ms_per_image=t_mlp / (n_groups * BI),
                                     **(dict(traffic_over_algorithmic=mt_[1], traffic_scope='HBM bytes per launch of the class over one 80-image encoder chunk '
                                                                                            '(profiles/pmc_gemm.json, tools/encode_pmc.py)') if mt_ else {}))))
        if n_cross:
            # algorithmic bytes per launch: K + V^T of the images in the call (d = 512) + q in / o out of the
            # rows (launch-weighted: 1 row/image in the point phase, N rows/image in polygon / recognition)
            rows_avg = BI * (1 * (2 * N + 6) + N * (34 + 27)) / float((2 * N + 6) + 34 + 27)
            alg = BI * 2 * M * 512 * esz + rows_avg * 2 * 512 * esz
            avg_s = (t_cross / 1e3) / n_cross
            ach = alg / avg_s / 1e9
            recs.append((t_cross, dict(bound='hbm', kernel='dec_cross_attn_kernel / dec_cross_attn_q4_kernel' + (' <split-bf16 planes>' if dtype_name == 'bf16x3' else ''), achieved=ach, peak=HBM_PEAK_GBS,
                                       unit='GB/s', frac=ach / HBM_PEAK_GBS, traffic=pmc_traffic(BI, 'x3_' if dtype_name == 'bf16x3' else ''), launches=int(n_cross),
                                       avg_us=avg_s * 1e6, alg_bytes_per_launch=alg, images_per_launch=BI,
                                       gpu_ms_per_image=t_cross / (n_groups * BI))))
        # FAMILIES: everything that runs on the matrix cores is one family -- the encoder-sized GEMMs, the same kernels on
        # decoder-phase rows, the fused MLPs and the row-owner chains -- so that `roofline` names the family that bounds the engine, with its
        # classes beneath it; the HBM-bound cross-attention kernels are the other family.
        note = ('hipEvent-bracketed eager launches of %d engine calls of %d images on one stream (graph replay cannot be bracketed); families ordered '
                'by GPU time, their classes beneath them; traffic = rocprofv3 FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE per launch from the committed '
                'PMC passes (profiles/pmc_cross_attn.json, pmc_gemm.json, pmc_dec_rows.json), null for classes / sizes without a pass' % (n_groups, BI))
        mm = sorted([r for r in recs if r[1]['bound'] == 'mfma'], key=lambda r: -r[0])
        fams = []
        if mm:
            t_f = sum(t for t, _ in mm)
            fl_f = sum(r['flops_per_launch'] * r['launches'] for _, r in mm)
            roof_f = sum(r['frac_of_launch_rooflines'] * t for t, r in mm)
            tf = fl_f / (t_f / 1e3) / 1e12
            fams.append((t_f, dict(bound='mfma', kernel='matrix-core family: ' + ' | '.join(r['kernel'].split(' (')[0].split(' at M')[0] for _, r in mm),
                                   achieved=tf, peak=MFMA_PEAK_TFS, unit='TFLOP/s', frac=tf / MFMA_PEAK_TFS, traffic=None,
                                   launches=sum(r['launches'] for _, r in mm), avg_us=t_f / sum(r['launches'] for _, r in mm) * 1e3,
                                   frac_of_launch_rooflines=roof_f / t_f, gpu_ms_per_image=t_f / (n_groups * BI), classes=[r for _, r in mm],
                                   traffic_note='per-launch HBM traffic is a per-class figure: see `classes`')))
        for t, r in recs:
            if r['bound'] == 'hbm':
                fams.append((t, r))
        fams.sort(key=lambda r: -r[0])
        if fams:
            return dict(fams[0][1], note=note), [r for _, r in fams[1:]]
        return None, []


    def parity_leg():
        # The engine that MEETS the parity contract (tests/test_gpu_e2e.py::test_parity_engine_bf16x3: logits within 1e-3 of the
        # reference, ids identical on every fixture) on the same workload and the same engine-call size, one lane
        m2, _, _ = build_model('bf16x3', a.graph, device)
        m2.overlap_decoders = bool(a.overlap)
        m2.engine()
        kp = min(a.steps, G)
        with torch.cuda.stream(stream):
            run_group(0, kp, model=m2)
            torch.cuda.synchronize()
            rp = []
            while sum(rp) < 3.0 and len(rp) < 6:
                t0 = time.perf_counter()
                run_group(0, kp, model=m2)
                torch.cuda.synchronize()
                rp.append(time.perf_counter() - t0)
        ep = pct(rp, 0.5)
        proof, pother = (None, []) if (a.no_roofline or kp < G) else measure_rooflines(m2, 'bf16x3', 1)
        del m2
        torch.cuda.empty_cache()
        return dict(engine='bf16x3', roofline=proof, roofline_other=pother, images_per_sec=B * kp / ep, chars_per_sec=B * kp / ep * N * args.rec_length, ms_per_step=ep / kp * 1e3,
                    images_per_engine_call=B * kp, repeats=len(rp),
                    note='cheapest engine precision that passes the fp32 parity gates (logits <= 1e-3, decoded ids identical, '
                         'tests/test_gpu_e2e.py::test_parity_engine_bf16x3): fp32 storage, large products as 3 bf16 matrix-core products '
                         'of split operands; same workload, one lane')

    def side_args(**kw):
        b_ = argparse.Namespace(**vars(a))
        b_.steps, b_.warmup, b_.min_seconds, b_.no_roofline, b_.no_cpu_baseline, b_.batch = 3, 1, 1.5, True, True, None
        b_.dump_outputs = None
        for k_, v_ in kw.items():
            setattr(b_, k_, v_)
        return b_

    def kie_leg():      # BASELINE config 3 (per GPU: batch 32 @ 960x1280, --infer_vie); full line: bench.py --workload kie
        r_ = run_kie(side_args(), device, 1, 0)
        return dict(images_per_sec=r_['value'], ms_per_step=r_['ms_per_step'], workload=r_['config']['workload'],
                    words_per_image=r_['config']['words_per_image'], entities_per_image=r_['config']['entities_per_image'])

    def mgp_leg():      # BASELINE config 5 (MGP-STR ViT-B, batch 512 words); full line: bench.py --workload mgp_str
        r_ = run_mgp_str(side_args(steps=6, warmup=2), device, 1, 0)
        return dict(words_per_sec=r_['value'], ms_per_step=r_['ms_per_step'], workload=r_['config']['workload'],
                    model_tflops=r_['config']['tflops_model'])

    def kie_parity_leg():   # the same config-3 leg on the engine that meets the parity gates (bf16x3)
        r_ = run_kie(side_args(dtype='bf16x3'), device, 1, 0)
        return dict(engine='bf16x3', images_per_sec=r_['value'], ms_per_step=r_['ms_per_step'], workload=r_['config']['workload'],
                    words_per_image=r_['config']['words_per_image'], entities_per_image=r_['config']['entities_per_image'],
                    note='tests/test_gpu_e2e.py: kie fixtures identical to the reference on this engine')

    def mgp_parity_leg():   # config 5 on MGP-STR's parity engine (round 5: split-bf16 products, split-plane attention; logits <= 1.6e-4 at batch 512)
        r_ = run_mgp_str(side_args(steps=4, warmup=1, dtype='bf16x3'), device, 1, 0)
        return dict(engine='bf16x3', words_per_sec=r_['value'], ms_per_step=r_['ms_per_step'], workload=r_['config']['workload'],
                    note='tests/test_gpu_mgp.py::test_mgp_golden_parity_engine / test_mgp_batch512_config5[bf16x3]: fp32 gates')

    def long_pt_leg():
        # BASELINE config 4 as far as the reference allows: the released code has no table-recognition head and its
        # position tables hold 1024 entries (transformer.py:475), so the long structured-sequence decode is the point decoder at
        # its maximum: N = 508 forced instances -> 1016 + 6 point steps, then 508 polygon / recognition rows per image
        Nl = 508

        def run_long(Bl):
            imgs = batches[0][:Bl]
            with torch.cuda.stream(stream):
                model.infer(imgs, mask1[:Bl], seqs, forced_instances=Nl, has_padding=False, packed=Nl)
                torch.cuda.synchronize()
                rl = []
                while sum(rl) < 2.0 and len(rl) < 4:
                    t0 = time.perf_counter()
                    ids_l, _, n_l = model.infer(imgs, mask1[:Bl], seqs, forced_instances=Nl, has_padding=False, packed=Nl)
                    torch.cuda.synchronize()
                    rl.append(time.perf_counter() - t0)
            assert int(n_l.min()) == Nl, 'long decode produced %d instances' % int(n_l.min())
            return pct(rl, 0.5)
        Bl = 2
        el_ = run_long(Bl)
        toks = Bl * (2 * Nl + Nl * (32 + args.rec_length))
        out_ = dict(images_per_sec=Bl / el_, tokens_per_sec=toks / el_, ms_per_call=el_ * 1e3, images_per_call=Bl, point_sequence_tokens=2 * Nl,
                    instances_per_image=Nl, note='table-recognition stand-in: point sequence at the 1024-entry position-table limit '
                                                 '(2 x 508 tokens + 6 prompt), then 508 polygon + recognition rows per image; %s engine' % a.dtype)
        # config 4's literal per-GPU batch (16 images over 4 GPUs): the 1022 sequential point steps are latency-bound, so their cost is shared by the images of a call
        B4 = min(4, B)
        e4_ = run_long(B4)
        out_['batch4'] = dict(images_per_sec=B4 / e4_, tokens_per_sec=toks / Bl * B4 / e4_, ms_per_call=e4_ * 1e3, images_per_call=B4)
        return out_

    # the two legs on the main model first (same thermal / cache state as the headline they are compared with), then the legs
    # that build other models (r03e / r03i: batch8 measured after the config legs read 118-121 img/s, 152-155 straight after
    # the headline on the same code)
    if rank == 0 and world == 1 and not a.no_batch8:
        leg('batch8', batch8_leg)
    if rank == 0 and world == 1 and not a.no_eos_run:
        leg('eos_run', eos_leg)
    if rank == 0 and world == 1 and not a.no_parity_leg and a.dtype == 'bf16':
        leg('parity_engine', parity_leg)
    if rank == 0 and world == 1 and not a.no_config_legs:
        leg('kie', kie_leg)
        leg('mgp_str', mgp_leg)
        leg('long_pt', long_pt_leg)
        if not a.no_parity_leg and a.dtype == 'bf16':
            leg('kie_parity', kie_parity_leg)
            leg('mgp_str_parity', mgp_parity_leg)

    if a.phase_times and rank == 0:
        def one_step():
            return model.infer(batches[0], mask1, seqs, forced_instances=N, has_padding=False, packed=N)
        print('phase ms: %s' % json.dumps(phase_breakdown(model, one_step, stream)), file=sys.stderr, flush=True)

        def one_call():
            gi = torch.cat([batches[i % POOL] for i in range(G)], 0)
            gm = mask1.expand(G, B, a.size, a.size).reshape(G * B, a.size, a.size)
            return model.infer(gi, gm, seqs, forced_instances=N, has_padding=False)
        print('phase ms (one synchronous engine call of %d images): %s' % (B * G, json.dumps(phase_breakdown(model, one_call, stream))),
              file=sys.stderr, flush=True)

    roof, roof_other = None, []
    if rank == 0 and not a.no_roofline:
        roof, roof_other = measure_rooflines(model, a.dtype, max(1, min(4, (a.steps + G - 1) // G)))

    if rank == 0:
        rec = dict(metric='images/sec (1024x1024) + chars/sec decoded, OmniParser text-spotting', value=ips, unit='images/s',
                   n_gpus=world, steps=a.steps, warmup=a.warmup, ms_per_step=elapsed / a.steps * 1e3,
                   higher_is_better=True, scaling='weak', vs_baseline=None, dtype=a.dtype, data='synthetic',
                   chars_per_sec=ips * N * args.rec_length,
                   timing=dict(repeats=len(reps), seconds_measured=sum(reps), ms_per_step_median=elapsed / a.steps * 1e3,
                               ms_per_step_p10=pct(reps, 0.1) / a.steps * 1e3, ms_per_step_p90=pct(reps, 0.9) / a.steps * 1e3,
                               note='each repetition = exactly %d steps between barrier+synchronize pairs, max over ranks; value from the median' % a.steps),
                   engine_call_ms=dict(images_per_call=call_imgs, calls=len(call_ms), median=pct(call_ms, 0.5), p10=pct(call_ms, 0.1),
                                       p90=pct(call_ms, 0.9), note='HIP events on the lane stream around every engine call of the timed region (latency, lanes overlap)'),
                   config=dict(workload='OmniParser text-spotting, Swin-B, batch %d/GPU per step @ %dx%d, %d steps coalesced per engine call = %d '
                                        'images per engine call, forced %d instances/image (%d pt + 34 poly + 27 rec decoder steps), %s'
                                        % (B, a.size, a.size, G, B * G, N, 2 * N + 6, a.dtype),
                               global_batch=world * B, image_size=a.size, instances_per_image=N, parallelism='image-sharded dp%d' % world,
                               hip_graph=bool(a.graph), lanes=lanes, coalesce=G, images_per_engine_call=B * G, distinct_batches=POOL))
        rec.update(extra)
        # the driver's record keeps `config`, `roofline` and `cpu_baseline` whole and only the NAMES of other extra keys: the
        # figures that qualify the headline -- BASELINE config 2's literal batch, the engine with parity credit, EOS honoured, configs 3 / 4 / 5 --
        # ride inside `config` as value + unit each
        def _leg(name, key, unit):
            v = extra.get(name)
            if not isinstance(v, dict):
                return None
            if 'error' in v:
                return dict(error=v['error'])
            return dict(value=v.get(key), unit=unit, **({'engine': v['engine']} if 'engine' in v else {}))
        legs = dict(batch8=_leg('batch8', 'images_per_sec', 'images/s'), eos_run=_leg('eos_run', 'images_per_sec', 'images/s'),
                    parity_engine=_leg('parity_engine', 'images_per_sec', 'images/s'), kie=_leg('kie', 'images_per_sec', 'images/s'),
                    kie_parity=_leg('kie_parity', 'images_per_sec', 'images/s'), mgp_str=_leg('mgp_str', 'words_per_sec', 'words/s'),
                    mgp_str_parity=_leg('mgp_str_parity', 'words_per_sec', 'words/s'), long_pt=_leg('long_pt', 'tokens_per_sec', 'tokens/s'))
        lp = extra.get('long_pt')
        if isinstance(lp, dict) and isinstance(lp.get('batch4'), dict):
            legs['long_pt_batch4'] = dict(value=lp['batch4']['tokens_per_sec'], unit='tokens/s')
        rec['config']['legs'] = {k: v for k, v in legs.items() if v is not None}
        rec['config']['legs_note'] = ('batch8 = one engine call per 8-image batch (config 2 literally); parity_engine / kie_parity / mgp_str_parity = the bf16x3 engines that '
                                      'pass the fp32 gates (logits <= 1e-3, ids identical); eos_run = EOS honoured; kie = config 3; mgp_str = config 5; long_pt = config 4 stand-in')
        # the literal BASELINE config-2 batch (one engine call per 8 images) next to the coalesced headline, at top level
        rec['images_per_sec_coalesced'] = ips
        rec['images_per_sec_batch8'] = extra.get('batch8', {}).get('images_per_sec') if isinstance(extra.get('batch8'), dict) else None
        # the engine that meets north_star's parity gate (logits <= 1e-3, ids identical) on the same workload, at top level beside the bf16 figure
        rec['images_per_sec_parity_engine'] = extra.get('parity_engine', {}).get('images_per_sec') if isinstance(extra.get('parity_engine'), dict) else None
        if dist_on:
            rec['ranks'] = rank_diag
            rec['backend'] = dist.get_backend()
            rec['per_rank_ms_per_step'] = per_rank_ms
            rec['all_gather_ms'] = dict(calls=len(gather_ms), median=pct(gather_ms, 0.5), p90=pct(gather_ms, 0.9),
                                        note='ONE all_gather_into_tensor per engine call (ids + probability bit patterns in one int32 payload), packing included, HIP events on rank 0')
        if roof is not None:
            rec['roofline'] = roof
            rec['roofline_other'] = roof_other
            pe = extra.get('parity_engine')
            if isinstance(pe, dict) and pe.get('roofline'):
                # the parity engine's own dominant family next to the bf16 one, inside the object the driver keeps whole
                pr = pe['roofline']
                rec['roofline']['parity_engine'] = dict({k: pr.get(k) for k in ('bound', 'kernel', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'launches', 'avg_us',
                                                                                'frac_of_launch_rooflines', 'gpu_ms_per_image', 'alg_bytes_per_launch') if k in pr},
                                                        images_per_sec=pe.get('images_per_sec'),
                                                        other=[dict({k: o.get(k) for k in ('bound', 'kernel', 'achieved', 'unit', 'frac', 'traffic', 'gpu_ms_per_image') if k in o})
                                                               for o in (pe.get('roofline_other') or [])])
        if not a.no_cpu_baseline and world == 1:
            rec['cpu_baseline'] = cpu_baseline(args, sd, a.size, N, 2 * N + 1)
        print(json.dumps(rec), flush=True)
    for pl in (pool, pools['b8']):
        if pl is not None:
            pl.close()
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
