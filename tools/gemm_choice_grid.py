"""Record / replay the GEMM dispatch table (csrc/gemm.hip: launch_gemm) over a grid that covers every rule and every refusal.

    python tools/gemm_choice_grid.py --write tests/golden/gemm_choice_grid.json      # record
    python tools/gemm_choice_grid.py --check tests/golden/gemm_choice_grid.json      # replay, list the blocks that differ
    python tools/gemm_choice_grid.py --print f4/F32-F32/ROWSTAT                      # one block, cell by cell

omp_debug_gemm_choice touches no device: the answer of a cell is the selector the call would run, or its negative error code (argument
checks of omp_gemm_bias_act included).  The grid is cut into blocks, one per (forced selector, dtype pair, store mode); the recorded file
holds per block the SHA-256 of its answer vector (one int8 per cell, in the order cells() yields them) and the histogram of its answers.
tests/test_host_logic.py::test_gemm_choice_grid_matches_the_record replays it.

Pointers are synthetic as in ops.gemm_choice (the library tests them for null and alignment only); `bias_off` moves the bias pointer alone.
"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.append(ROOT)

FORCED = (0, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22, 7)   # 7: no such selector
F32, BF16, BF16X2 = 0, 1, 2
DTYPES = (('F32-F32', F32, F32), ('BF16-BF16', BF16, BF16), ('BF16-F32', BF16, F32), ('BF16-BF16X2', BF16, BF16X2))
PLAIN, KBLK, VBLK, ROWSTAT = 0, 2, 3, 4
# one legal geometry per blocked store that lands on the grid: K slabs of a 32-image chunk of 4096 tokens, 8 heads (M = 131072, N % 512 == 0);
# V^T slabs of 3 images x 512 tokens, one head, bias along M (N = 1536, M % 64 == 0); (images, tokens, mpad, heads, key block)
STORES = (('PLAIN', PLAIN, None, 0), ('KBLK', KBLK, (32, 4096, 4096, 8, 32), 0), ('VBLK', VBLK, (3, 512, 512, 1, 32), 1), ('ROWSTAT', ROWSTAT, None, 0))
MS = (8, 64, 65, 160, 300, 10240, 131000, 131072, 524288)
NS = (128, 256, 384, 512, 768, 1104, 1536)
KS = (64, 128, 256, 512, 768, 1024, 1536)
ACTS = (0, 1)                      # none, GELU
DESTS = (0, 1, 2)                  # no residual, residual, residual + second destination
BASE = 1 << 20


def blocks():
    for f in FORCED:
        for dname, dt, odt in DTYPES:
            for sname, sm, kv, bias_m in STORES:
                yield 'f%d/%s/%s' % (f, dname, sname), f, dt, odt, sm, kv, bias_m


def cells():
    """The cells of one block, in recorded order: (M, N, K, a_wrap, act, dest, small_m, ln, bias_off)."""
    for M in MS:
        for N in NS:
            for K in KS:
                for aw in ((0, 2 * K // 3) if (2 * K) % 3 == 0 and (2 * K // 3) % 64 == 0 else (0,)):
                    for act in ACTS:
                        for dest in DESTS:
                            for small_m in (0, 1):
                                for ln in (0, 1):
                                    for boff in (0, 4):
                                        yield M, N, K, aw, act, dest, small_m, ln, boff


def run_block(lib, forced, dt, odt, sm, kv, bias_m, show=None):
    """-> answers of the block (list of int).  show: a callable taking (cell, answer)."""
    from advancedliteratemachinery_amd import _lib
    a = _lib.GemmArgs()
    ref = ctypes.byref(a)
    choice = lib.omp_debug_gemm_choice
    a.W, a.C = BASE + (1 << 30), BASE + (4 << 30)
    a.A, a.dtype, a.out_dtype, a.store_mode, a.bias_along_m, a.ln_eps = BASE, dt, odt, sm, bias_m, 1e-5
    if kv is not None:
        a.kv_images, a.kv_tokens, a.kv_mpad, a.kv_heads, a.kv_key_block = kv
    out = []
    lib.omp_debug_force_gemm_kernel(forced)
    try:
        for cell in cells():
            M, N, K, aw, act, dest, small_m, ln, boff = cell
            a.M, a.N, a.K, a.a_wrap, a.act, a.small_m_splitk = M, N, K, aw, act, small_m
            a.lda, a.ldw, a.ldc = (aw if aw else K), K, (2 * N if odt == BF16X2 else N)
            a.bias = BASE + (2 << 30) + boff
            a.residual, a.ldr = (BASE + (3 << 30), N) if dest else (None, 0)
            a.C2, a.ldc2 = (BASE + (7 << 30), N) if dest == 2 else (None, 0)
            a.ln_gamma, a.ln_beta = (BASE + (5 << 30), BASE + (6 << 30)) if ln else (None, None)
            rc = choice(ref)
            out.append(rc)
            if show is not None:
                show(cell, rc)
    finally:
        lib.omp_debug_force_gemm_kernel(0)
    return out


def summarize(answers):
    hist = {}
    for v in answers:
        hist[v] = hist.get(v, 0) + 1
    dg = hashlib.sha256(bytes(v & 0xFF for v in answers)).hexdigest()
    return {'sha256': dg, 'hist': {str(k): hist[k] for k in sorted(hist)}}


def record(only=None):
    from advancedliteratemachinery_amd import _lib
    lib = _lib.lib()
    rec = {}
    for key, f, dt, odt, sm, kv, bias_m in blocks():
        if only is None or key in only:
            rec[key] = summarize(run_block(lib, f, dt, odt, sm, kv, bias_m))
    return rec


def main(argv):
    if len(argv) == 2 and argv[0] == '--write':
        rec = record()
        n = sum(sum(b['hist'].values()) for b in rec.values())
        with open(argv[1], 'w') as f:
            json.dump({'cells': n, 'blocks': rec}, f, indent=0, sort_keys=True)
            f.write('\n')
        print('%d cells in %d blocks -> %s' % (n, len(rec), argv[1]))
    elif len(argv) == 2 and argv[0] == '--check':
        with open(argv[1]) as f:
            want = json.load(f)['blocks']
        got = record()
        bad = [k for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]
        for k in bad:
            print(k, 'recorded', want.get(k, {}).get('hist'), 'now', got.get(k, {}).get('hist'))
        print('%d of %d blocks differ' % (len(bad), len(got)))
        return 1 if bad else 0
    elif len(argv) == 2 and argv[0] == '--print':
        from advancedliteratemachinery_amd import _lib
        for key, f, dt, odt, sm, kv, bias_m in blocks():
            if key == argv[1]:
                print('# M N K a_wrap act dest small_m ln bias_off -> answer')
                run_block(_lib.lib(), f, dt, odt, sm, kv, bias_m, show=lambda c, rc: print(*c, '->', rc))
                return 0
        print('no such block:', argv[1])
        return 1
    else:
        print(__doc__)
        return 2
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
