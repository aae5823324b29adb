"""The decoder cross-attention kernels of csrc/decoder.hip (dec_cross_attn_kernel: every wave streams a private key slice through a register
ring of PD blocks; dec_cross_attn_q4_kernel: a workgroup streams its split through an LDS ring of NS stages consumed in chunks of CH blocks;
dec_cross_merge_kernel) through ops.dec_cross_attn_step with PLANTED keys at every key count where their loops change shape.

A launch holds one image per length of LENGTHS in slabs of M = Mpad = 640 keys (the lengths go through key_len), nH = 8, d = 512; the rows per
image (ROWS) rotate over the images from phase to phase.  Kinds: bf16, fp32 and split (split-plane slabs, fp32 q / out); variants: every ring
omp_debug_cross_q4 builds for the kind at q_tiles 4 (RINGS of tests/gpu_checks_ragged.py, 0 = the register-streaming kernel), omp_debug_cross_nt
0 / 1, n_split 1 .. 16.  config() restates launch_cross: KB, slices per n_split, PD or NS / CH; tests/test_crossattn_reference.py asserts that
LENGTHS gives every configuration an empty slice and slices of 1, depth - 1, depth, depth + 1 and 2 depth + 1 blocks (chunks), proves the
stated outputs in float64 and that a lost, shifted, stale, unpermuted or leaked key breaks the gates.

Planted inputs (all values exact in bf16 unless said otherwise; H = the 64 x 64 Sylvester Hadamard matrix, row r of an image has q = H[r % 64]
in every head, and H[:, 0] = 1):

  * loud dead keys: every dead key of a loaded block -- a padded key M .. Mpad, a masked key, a key at or beyond key_len -- holds K = 512 e0
    (score 64 against every row) and V^T = -256; blocks at or beyond ceil(key_len / KB) are never loaded and hold NaN in K and V^T.  One leaked
    dead key drags every output to -256, more than 13 times the largest stated value (7, or 17 / n_live).
  * peaked walk: V[j] = v_pat(j) (+-1 .. 7 with a sign code); the target key of (row r, head h) holds 4 H[r] -- a key that several rows aim at
    holds the sum of their codes (at most 256, a multiple of 4) -- so a row scores 32 on its own target and exactly 0 on every other key: the
    output is V[target] up to e^-32 n_keys.  Targets differ by head (slot = 8 code + head of the phase's window over the LIVE keys) and always
    include the first and the last live key; phases advance the window until every live key of every length has been a target.
  * uniform walk: every live key is 0, V is 0 except one target per (image, head) holding u_pat: the output is u / n_live; a dropped target
    gives 0, a doubled one twice the value.
  split slabs: V and u carry a lo plane, 2^-10 (1 .. 7): exact as hi + lo, not as one bf16, 140 times the walk gate.
  * score ramps along e0 (which every q shares) rising / falling to RAMP_TOP: the running maximum changes at every block, chunk, wave slice
    and split, or never; V random.
  * plane ramps (split): K[j, 0] = 256 + t_j with t_j = k / 128 < 1 (all of it in K's lo plane) against q0 = 64: scores 2048 + 8 t_j; and
    q0 = 1 + 2^-10, q1 = -1 against K[j, 0] = K[j, 1] = 1024 k: scores k / 8 that live in K_hi q_lo alone.  Without either cross term the
    weights are uniform.
  * random base: randn x 1.5 in q, K and V.
Masks: none; a 2-D padding mask per image (live columns w of W, live rows h of H, flattened: whole blocks, wave slices and trailing splits are
dead); a dead run of 70 leading keys plus every 7th key (m stays -inf through the first blocks).  No image is fully masked.

Every launch: q is a column window of a wider NaN-filled buffer, out a column window of a wider NaN-filled buffer with guard rows, partial is
NaN-filled with guard rows; afterwards everything outside out's window, the guard rows and both slabs are bit-identical and every output is
finite.

Gates.  Walks, per (row, head) relative to that head's largest stated value: WALK_GATE of tests/gpu_checks_selfattn.py -- bf16 2^-8 (one
output rounding, below 2^-9), fp32 and split 1e-6 (exact terms, one reciprocal and one multiply).  Ramps and random data against ref_cross,
a float64 restatement over the bytes of the slabs (natural() undoes the slab layout), on the device: the project's absolute gates fp32 2e-5,
bf16 2e-2, split 5e-5 (check_cross_attn, check_cross_attn_split, TOL of the ragged checks).  The ramps' V is randn x RAMP_V: a bf16 output
in [4, 8) is rounded by up to 2^-6 = 1.6e-2 whatever the scores are, which no lower ramp top could bring under half of the bf16 gate; with
|V| < 2 the rounding stays below 2^-8 and the rounding of P to bf16 below 2^-9 |V|.  RAMP_TOP is 80 for every kind: the scores c_j / 8 are
single exact products, and so are their differences to the running maximum wherever the weight matters; no top had to be lowered (MEASURED:
every ramp stays below half of its gate).

What these checks found: the random base on SPLIT slabs missed its gate of 5e-5 with 5.1e-5 .. 7.7e-5, the same figure from every kernel,
ring, n_split and nt on the same data -- no layout error, but the kernels' arithmetic: q / 8 and P entered the products as hi + lo of two bf16
(2^-17 relative) and K_lo q_lo was dropped; with scores of standard deviation 2.25 over 1 .. 65 keys a few weights compete for values 10
apart (the same three products formed in float64 without any fp32 rounding gave 3.4e-5 .. 5.1e-5 on these inputs; check_cross_attn_split
runs unit-variance data over 77 keys and more).  The kernels now split q / 8 and P into three planes (exact) and add K_lo q_lo, K_hi q_lo2,
V_lo p_lo and V_hi p_lo2: 6.1e-6 on the same data, the fp32 slabs' level; the split ramps fell from 1.2e-5 to 1.4e-6."""
import contextlib

import torch

from tests.gpu_checks import DEV, rec, rrec
from tests.gpu_checks_ragged import RINGS, TOL, _slabs, _slot_of_key, _vblocks
from tests.gpu_checks_selfattn import WALK_GATE, _filled, _is_nan_fill, _refused, _same_bits, head_rel, u_pat, v_pat

NH, HD, D = 8, 64, 512
M_SLAB = 640
PAD, GUARD = 8, 4                    # columns beside the q / out windows (16 bytes at least: the kernels' vector loads and stores), guard rows
LOUD_K, LOUD_V = 512.0, -256.0
KINDS = ('bf16', 'fp32', 'split')
S_ALL = (1, 2, 4, 8, 16)
MASKS = ('none', 'pad2d', 'lead')
ROWS = {1: (1, 2, 15, 16), 2: (1, 17, 31, 32), 4: (1, 16, 17, 33, 47, 48, 49, 63, 64)}
LENGTHS = sorted({1, 2, 639, 640} | {m + e for m in range(16, 65, 16) for e in (-1, 0, 1)}
                 | {m + e for m in (96, 128, 192, 256, 320, 384, 512) for e in (-1, 0, 1)})
RAGGED_M = (77, 129, 640)            # key_len = None, M itself ragged: Mpad is rounded up per kind
LONG_M = 2081                        # 66 blocks of 32 / 131 of 16 keys: eight wraps of the eight-stage ring at n_split 1
RAMP_TOP = {'fp32': 80.0, 'bf16': 80.0, 'split': 80.0}
RAMP_V = {'fp32': 1.5, 'bf16': 0.35, 'split': 1.5}
# measured worst on an MI355X over every variant (the parity report holds every figure per kind and variant) -- gate
MEASURED = {'peaked walk': {'bf16': 0.0, 'fp32': 0.0, 'split': 0.0},                                    # 2^-8, 1e-6, 1e-6
            'uniform walk': {'bf16': 3.3e-3, 'fp32': 1.1e-7, 'split': 1.1e-7},
            'ramp rising': {'bf16': 3.9e-3, 'fp32': 7.6e-7, 'split': 1.2e-6},                          # 2e-2, 2e-5, 5e-5
            'ramp falling': {'bf16': 3.9e-3, 'fp32': 1.3e-6, 'split': 1.4e-6},
            'plane ramp klo': {'split': 6.1e-7}, 'plane ramp qlo': {'split': 8.9e-7},
            'random': {'bf16': 1.57e-2, 'fp32': 6.4e-6, 'split': 6.1e-6}}      # bf16: the 2^-6 rounding of outputs in [4, 8)


def walk_gate(kind):
    return WALK_GATE[torch.bfloat16 if kind == 'bf16' else torch.float32]


def key_block(kind):
    return 16 if kind == 'fp32' else 32


def round_up(n, m):
    return (n + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------------------------------
# the built configurations (csrc/decoder.hip launch_cross)
# ---------------------------------------------------------------------------------------------------------------------------------------
_PD = {('fp32', 1): 4, ('fp32', 2): 2, ('fp32', 4): 2, ('bf16', 1): 4, ('bf16', 2): 2, ('bf16', 4): 2, ('split', 1): 2, ('split', 2): 2, ('split', 4): 1}
_RING = {'split': {1: (2, 1), 4: (8, 2), 5: (4, 1), 6: (3, 1)},
         'fp32': {1: (8, 2), 2: (8, 1), 4: (8, 2), 5: (6, 2), 6: (4, 1)},
         'bf16': {1: (6, 2), 2: (8, 1), 4: (8, 2), 5: (8, 2), 6: (4, 1)}}


def config(kind, qt, ring, nt):
    """-> dict(KB, mult = key slices per n_split, depth, CH): the register-streaming kernel (4 waves cut a split again, PD blocks in flight:
    depth = PD blocks) or the ring kernel (depth = NS / CH chunk slots of CH blocks)"""
    KB = key_block(kind)
    if qt == 4 and ring != 0:
        NS, CH = _RING[kind][ring]
        if kind == 'bf16' and ring == 1 and not nt:
            NS, CH = 8, 2
        return dict(KB=KB, mult=1, NS=NS, CH=CH, depth=NS // CH, ring=True)
    return dict(KB=KB, mult=4, PD=_PD[kind, qt], CH=1, depth=_PD[kind, qt], ring=False)


def variants(kind, qt, rings=None):
    rs = RINGS[kind] if qt == 4 else (1,)
    return [(r, nt) for r in rs if rings is None or r in rings for nt in (1, 0)]


def slice_blocks(L, S, cfg):
    """key blocks of every slice of an image of L keys at n_split S (image_keys: kpw = round_up(ceil(L / slices), KB))"""
    n, KB = S * cfg['mult'], cfg['KB']
    kpw = round_up((L + n - 1) // n, KB)
    return [max(0, (min((i + 1) * kpw, L) - i * kpw + KB - 1) // KB) for i in range(n)]


@contextlib.contextmanager
def variant(ring, nt):
    from advancedliteratemachinery_amd import _lib, ops
    try:
        ops.cross_q4(ring)
        _lib.lib().omp_debug_cross_nt(nt)
        yield
    finally:
        ops.cross_q4(1)
        _lib.lib().omp_debug_cross_nt(1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# slabs <-> natural order, float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def slabs(kind, Kn, Vn):
    """_slabs of the ragged checks on the device its operands are on"""
    with torch.device(Kn.device):
        K, Vt, _, _ = _slabs(kind, Kn, Vn)
    return K.contiguous(), Vt.contiguous()


def _unblock(vb, permute):
    """V^T blocks [B][nH][nb][64][KB] -> [B][nH][nb * KB][64]"""
    if permute:
        vb = vb[..., _slot_of_key().to(vb.device)]
    return vb.transpose(-1, -2).reshape(vb.shape[0], vb.shape[1], -1, 64)


def natural(kind, K, Vt, planes=False):
    """the values a slab pair holds, float64 in natural order [B][nH][Mpad][64] -> (K, V); planes (split): ((K_hi, K_lo), (V_hi, V_lo))"""
    if kind != 'split':
        return K.double(), _unblock(Vt, kind == 'bf16').double()
    B, nH = K.shape[:2]
    k = [K[:, :, :, i].double().reshape(B, nH, -1, 64) for i in (0, 1)]
    v = [_unblock(Vt[:, :, :, i], True).double() for i in (0, 1)]
    return ((k[0], k[1]), (v[0], v[1])) if planes else (k[0] + k[1], v[0] + v[1])


def split_q(q):
    """the kernels' split of a query row: q / 8 -> (hi, lo) bf16 planes, float64"""
    x = (q * 0.125).float()
    hi = x.to(torch.bfloat16).float()
    return hi.double(), (x - hi).to(torch.bfloat16).double()


def ref_cross(q, Kv, Vv, counts, live, ksrc=None, vsrc=None, weight=None, kplanes=None, drop=None):
    """softmax(q K^T / 8) V per head of every image's rows over ITS live keys.  q [R, d] float64, Kv / Vv [B][nH][Mpad][64] float64 (what
    natural() returns: NaN where nothing is loaded), counts = rows per image (rows sorted by image), live [B][Mpad] bool -> [R, d].
    The mutants of tests/test_crossattn_reference.py: ksrc / vsrc [B][Mpad] = the key whose K / V row position j reads; weight [R][nH][Mpad]
    = how often a key counts; kplanes = (K_hi, K_lo) with drop = None / 'klo_qhi' / 'khi_qlo': the score from the three leading products
    of the split kernels, K_hi q_hi + K_lo q_hi + K_hi q_lo (q / 8 as two planes), without the dropped term."""
    R, d = q.shape
    nH = Kv.shape[1]
    out = torch.zeros(R, d, dtype=torch.float64, device=q.device)
    r0 = 0
    for b, n in enumerate(counts):
        if n:
            lv = live[b]
            gk = (lambda t: t[b]) if ksrc is None else (lambda t: t[b][:, ksrc[b]])
            qr = q[r0:r0 + n].reshape(n, nH, HD)
            dead0 = lambda t: torch.where(lv[None, :, None], t, torch.zeros_like(t))
            if kplanes is None:
                s = torch.einsum('rhd,hkd->rhk', qr * 0.125, dead0(gk(Kv)))
            else:
                qh, ql = split_q(qr)
                kh, kl = dead0(gk(kplanes[0])), dead0(gk(kplanes[1]))
                s = torch.einsum('rhd,hkd->rhk', qh, kh)
                if drop != 'klo_qhi':
                    s = s + torch.einsum('rhd,hkd->rhk', qh, kl)
                if drop != 'khi_qlo':
                    s = s + torch.einsum('rhd,hkd->rhk', ql, kh)
            s = s.masked_fill(~lv[None, None, :], float('-inf'))
            p = torch.exp(s - s.amax(-1, keepdim=True))
            if weight is not None:
                p = p * weight[r0:r0 + n]
            v = dead0(Vv[b] if vsrc is None else Vv[b][:, vsrc[b]])
            out[r0:r0 + n] = (torch.einsum('rhk,hkd->rhd', p, v) / p.sum(-1, keepdim=True)).reshape(n, d)
        r0 += n
    return out


def ref_cross_merged(q, Kv, Vv, counts, live, lens, S, cfg, inf_weight=0.0):
    """ref_cross the way a launch with n_split S forms it: every key slice of an image gives a partial (m, l, o) -- m = -inf, l = 0, o = 0
    when it has no live key -- and the partials merge with weights exp(m - max m); a -inf partial enters with `inf_weight`."""
    R, d = q.shape
    nH = Kv.shape[1]
    out = torch.zeros(R, d, dtype=torch.float64, device=q.device)
    n_sl, KB = S * cfg['mult'], cfg['KB']
    r0 = 0
    for b, n in enumerate(counts):
        kpw = round_up((lens[b] + n_sl - 1) // n_sl, KB)
        qr = q[r0:r0 + n].reshape(n, nH, HD) * 0.125
        ms, ls, os_ = [], [], []
        for i in range(n_sl):
            lv = live[b].clone()
            lv[:i * kpw] = False
            lv[(i + 1) * kpw:] = False
            k = torch.where(lv[None, :, None], Kv[b], torch.zeros_like(Kv[b]))
            v = torch.where(lv[None, :, None], Vv[b], torch.zeros_like(Vv[b]))
            s = torch.einsum('rhd,hkd->rhk', qr, k).masked_fill(~lv[None, None, :], float('-inf'))
            m = s.amax(-1)
            p = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m)[..., None])      # the kernels' mref
            ms.append(m)
            ls.append(p.sum(-1))
            os_.append(torch.einsum('rhk,hkd->rhd', p, v))
        m, l, o = torch.stack(ms), torch.stack(ls), torch.stack(os_)
        w = torch.where(torch.isinf(m), torch.full_like(m, inf_weight), torch.exp(m - m.amax(0, keepdim=True)))
        out[r0:r0 + n] = ((o * w[..., None]).sum(0) / (l * w).sum(0)[..., None]).reshape(n, d)
        r0 += n
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# layouts: images, rows, groups, masks, targets
# ---------------------------------------------------------------------------------------------------------------------------------------
def hadamard(dev='cpu'):
    i = torch.arange(64, device=dev)
    x = i[:, None] & i[None, :]
    par = torch.zeros_like(x)
    for b in range(6):
        par ^= (x >> b) & 1
    return (1 - 2 * par).double()


def make_mask(name, lens, M):
    """-> None or bool [B][M], True = dead.  pad2d: image b is a W x H grid (W ~ sqrt(L)) whose last third of columns and of rows is padding;
    lead: min(70, L - 1) leading keys and every key j % 7 == 3 behind them are dead.  Key positions at or beyond L are marked dead."""
    if name == 'none':
        return None
    m = torch.ones(len(lens), M, dtype=torch.bool)
    j = torch.arange(M)
    for b, L in enumerate(lens):
        if name == 'pad2d':
            W = max(1, int(round(L ** 0.5)))
            Hn = -(-L // W)
            dead = (j % W >= max(1, W - W // 3)) | (j // W >= max(1, Hn - Hn // 3))
        else:
            lead = min(70, L - 1)
            dead = (j < lead) | ((j > lead) & (j % 7 == 3))
        m[b, :L] = dead[:L]
    return m


class Layout:
    """one launch's geometry (CPU tensors): image b has lens[b] keys (through key_len, or = M with key_len = None) in slabs of M keys padded to
    Mpad, counts[b] rows in groups of <= 16 qt; live / loud / never [B][Mpad]: attended keys, dead keys of loaded blocks, blocks never loaded"""

    def __init__(self, kind, lens, counts, M, qt, mask='none', key_len=True):
        self.kind, self.M, self.qt, self.B, self.mask_name, self.key_len = kind, M, qt, len(counts), mask, key_len
        self.KB = key_block(kind)
        self.Mpad = round_up(M, self.KB)
        self.lens = list(lens) if key_len else [M] * self.B
        self.counts = list(counts)
        assert len(self.lens) == self.B and all(1 <= L <= M for L in self.lens)
        self.mask = make_mask(mask, self.lens, M)
        j = torch.arange(self.Mpad)[None, :]
        L = torch.tensor(self.lens)[:, None]
        live = j < L
        if self.mask is not None:
            live[:, :M] &= ~self.mask
        loaded = j < (L + self.KB - 1) // self.KB * self.KB
        self.live, self.loud, self.never = live, loaded & ~live, ~loaded
        self.n_live = live.sum(1)
        assert bool((self.n_live > 0).all()), 'a fully masked image: the reference gives NaN'
        self.R = sum(self.counts)
        self.row_img = torch.repeat_interleave(torch.arange(self.B), torch.tensor(self.counts))
        self.row0 = [sum(self.counts[:b]) for b in range(self.B)]
        self.row_code = torch.cat([torch.arange(n) % 64 for n in self.counts])
        self.ncode = [min(n, 64) for n in self.counts]
        self.pair0 = [sum(self.ncode[:b]) for b in range(self.B)]
        self.P = sum(self.ncode)
        self.pair_img = torch.repeat_interleave(torch.arange(self.B), torch.tensor(self.ncode))
        self.pair_code = torch.cat([torch.arange(n) for n in self.ncode])
        self.row_pair = torch.tensor(self.pair0)[self.row_img] + self.row_code
        g = 16 * qt
        self.groups = [(self.row0[b] + o, min(g, n - o), b) for b, n in enumerate(self.counts) for o in range(0, n, g)]

    def targets(self, bases):
        """-> int64 [P][nH]: the target key of (image, code, head).  Slot t = 8 code + head of image b's window aims at live key
        (bases[b] + t - 1) % n_live; slot 0 at the first, the last slot at the last live key."""
        tg = torch.empty(self.P, NH, dtype=torch.int64)
        for b in range(self.B):
            idx = torch.nonzero(self.live[b])[:, 0]
            T = self.ncode[b] * NH
            key = idx[(bases[b] + torch.arange(T) - 1) % idx.numel()]
            key[0], key[T - 1] = idx[0], idx[-1]
            tg[self.pair0[b]:self.pair0[b] + self.ncode[b]] = key.reshape(self.ncode[b], NH)
        return tg

    def advance(self, bases):
        return [a + max(self.ncode[b] * NH - 2, 1) for b, a in enumerate(bases)]


def rows_of_phase(qt, phase, B):
    return [ROWS[qt][(b + phase) % len(ROWS[qt])] for b in range(B)]


def sweep(kind, qt, mask, lens=None, M=M_SLAB, key_len=True):
    """the phases [(Layout, bases)] after which every live key of every image has been a target; the row counts rotate over the images"""
    lens = LENGTHS if lens is None else lens
    out, bases = [], [0] * len(lens)
    while True:
        lay = Layout(kind, lens, rows_of_phase(qt, len(out), len(lens)), M, qt, mask, key_len)
        out.append((lay, bases))
        bases = lay.advance(bases)
        if all(a >= int(n) for a, n in zip(bases, lay.n_live)):
            return out


def edge_phases(lay):
    """the first and the last window of a layout: targets at both ends of the live keys only"""
    return [(lay, [0] * lay.B), (lay, [max(0, int(n) - (lay.ncode[b] * NH - 2)) for b, n in enumerate(lay.n_live)])]


# ---------------------------------------------------------------------------------------------------------------------------------------
# planted inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def to_kind(kind, x):
    """fp32 values exact in the slab format of `kind`: fp32, one bf16, or hi + lo of two bf16"""
    x = x.float()
    if kind == 'fp32':
        return x
    hi = x.to(torch.bfloat16).float()
    return hi if kind == 'bf16' else hi + (x - hi).to(torch.bfloat16).float()


def lo_pat(rows, d, dev='cpu'):
    """[len(rows), d] of 2^-10 (1 .. 7): the lo plane of the split walks' values"""
    r = torch.as_tensor(rows, dtype=torch.int64, device=dev)[:, None]
    c = torch.arange(d, device=dev)[None, :]
    return (1 + (3 * r + c) % 7).double() * 2.0 ** -10


class Plant:
    """q [R, d] float64 (exact in the query dtype), Kn / Vn natural fp32 [B][nH][Mpad][64] with the loud dead keys and the NaN blocks in place,
    want [R, d] float64 or None"""

    def __init__(self, lay, name, dev):
        self.lay, self.name, self.dev = lay, name, dev
        self.Kn = torch.zeros(lay.B, NH, lay.Mpad, HD, device=dev)
        self.Vn = torch.zeros(lay.B, NH, lay.Mpad, HD, device=dev)
        self.q = hadamard(dev)[lay.row_code.to(dev)].repeat(1, NH)
        self.want = None
        self.tgt = None

    def finish(self):
        lay, dev = self.lay, self.dev
        loud, never = lay.loud.to(dev)[:, None, :, None], lay.never.to(dev)[:, None, :, None]
        e0 = torch.zeros(HD, device=dev)
        e0[0] = LOUD_K
        self.Kn = torch.where(never, torch.full_like(self.Kn, float('nan')), torch.where(loud, e0.expand_as(self.Kn), self.Kn))
        self.Vn = torch.where(never, torch.full_like(self.Vn, float('nan')), torch.where(loud, torch.full_like(self.Vn, LOUD_V), self.Vn))
        return self


def _heads(t):
    """[n, 512] -> [nH, n, 64]"""
    return t.reshape(t.shape[0], NH, HD).transpose(0, 1)


def plant_peaked(lay, bases, dev='cpu'):
    p = Plant(lay, 'peaked', dev)
    tg = lay.targets(bases).to(dev)
    hi = torch.arange(NH, device=dev)[None, :].expand(lay.P, NH)
    code = 4.0 * hadamard(dev)[lay.pair_code.to(dev)].float()
    p.Kn.index_put_((lay.pair_img.to(dev)[:, None].expand(lay.P, NH), hi, tg), code[:, None, :].expand(lay.P, NH, HD), accumulate=True)
    keys = list(range(lay.Mpad))
    V = v_pat(keys, D, dev) + (lo_pat(keys, D, dev) if lay.kind == 'split' else 0)
    p.Vn[:] = _heads(V).float()
    p.tgt = tg[lay.row_pair.to(dev)]                                        # [R, nH]
    p.want = _heads(V)[hi[:1].expand_as(p.tgt), p.tgt].reshape(lay.R, D)
    return p.finish()


def plant_uniform(lay, bases, pick=0, dev='cpu'):
    p = Plant(lay, 'uniform', dev)
    tg = lay.targets(bases)
    ut = torch.stack([tg[lay.pair0[b] + pick % lay.ncode[b]] for b in range(lay.B)]).to(dev)      # [B, nH]
    imgs = list(range(lay.B))
    u = u_pat(imgs, D, dev) + (lo_pat(imgs, D, dev) if lay.kind == 'split' else 0)
    bi = torch.arange(lay.B, device=dev)[:, None].expand(lay.B, NH)
    hi = torch.arange(NH, device=dev)[None, :].expand(lay.B, NH)
    p.Vn[bi, hi, ut] = u.reshape(lay.B, NH, HD).float()
    p.tgt = ut[lay.row_img.to(dev)]
    p.want = (u / lay.n_live.to(dev)[:, None])[lay.row_img.to(dev)]
    return p.finish()


def _randn(shape, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=dev)


def _ramp(lay, rising, dev):
    """[B][Mpad] in [0, 1]: j / (L - 1) or (L - 1 - j) / (L - 1) below L"""
    j = torch.arange(lay.Mpad, dtype=torch.float64)[None, :]
    L1 = (torch.tensor(lay.lens, dtype=torch.float64)[:, None] - 1).clamp_min(1)
    return ((j if rising else L1 - j) / L1).clamp(0, 1).to(dev)


def plant_ramp(lay, rising, dev='cpu', seed=0):
    """K[j] = c_j e0 with c_j / 8 rising (falling) from 0 to RAMP_TOP over the image's keys; V = randn x RAMP_V"""
    p = Plant(lay, 'ramp %s' % ('rising' if rising else 'falling'), dev)
    p.Kn[..., 0] = to_kind(lay.kind, 8.0 * RAMP_TOP[lay.kind] * _ramp(lay, rising, dev))[:, None, :]
    p.Vn[:] = to_kind(lay.kind, _randn(p.Vn.shape, 11 + seed, dev) * RAMP_V[lay.kind])
    return p.finish()


def plant_random(lay, dev='cpu', seed=0):
    p = Plant(lay, 'random', dev)
    qk = 'bf16' if lay.kind == 'bf16' else 'fp32'
    p.q = to_kind(qk, _randn((lay.R, D), 21 + seed, dev) * 1.5).double()
    p.Kn[:] = to_kind(lay.kind, _randn(p.Kn.shape, 22 + seed, dev) * 1.5)
    p.Vn[:] = to_kind(lay.kind, _randn(p.Vn.shape, 23 + seed, dev) * 1.5)
    return p.finish()


def plant_plane_ramp(lay, which, dev='cpu', seed=0):
    """split slabs.  'klo': K[j, 0] = 256 + k_j / 128 (hi plane 256, the ramp in the lo plane), q0 = 64: scores 2048 + k_j / 16, rising.
    'qlo': q0 = 1 + 2^-10, q1 = -1 (q / 8: hi planes +-1 / 8, lo plane 2^-13), K[j, 0] = K[j, 1] = 1024 k_j: scores k_j / 8, falling.  k_j = 0 .. 127"""
    assert lay.kind == 'split'
    p = Plant(lay, 'plane ramp ' + which, dev)
    k = torch.floor(127.0 * _ramp(lay, which == 'klo', dev)).float()[:, None, :]
    q = p.q.reshape(lay.R, NH, HD)
    if which == 'klo':
        q[..., 0] = 64.0
        p.Kn[..., 0] = 256.0 + k / 128.0
    else:
        q[..., 0], q[..., 1] = 1.0 + 2.0 ** -10, -1.0
        p.Kn[..., 0] = 1024.0 * k
        p.Kn[..., 1] = 1024.0 * k
    p.q = q.reshape(lay.R, D)
    p.Vn[:] = to_kind('split', _randn(p.Vn.shape, 31 + seed, dev) * 1.5)
    return p.finish()


# ---------------------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------------------
class Prepared:
    """a plant on the device: slabs (and their pristine copies), q as a column window of a wider buffer, mask, key_len, groups"""

    def __init__(self, plant):
        lay = self.lay = plant.lay
        self.name, self.kind, self.want, self.tgt = plant.name, lay.kind, plant.want, plant.tgt
        self.K, self.Vt = slabs(lay.kind, plant.Kn.to(DEV), plant.Vn.to(DEV))
        self.K0, self.Vt0 = self.K.clone(), self.Vt.clone()
        self.qdt = torch.bfloat16 if lay.kind == 'bf16' else torch.float32
        qbuf = _filled((lay.R, D + 2 * PAD), self.qdt)
        qbuf[:, PAD:PAD + D] = plant.q.to(DEV, self.qdt)
        self.q = qbuf[:, PAD:PAD + D]
        self.qv = self.q.double()
        self.km = None if lay.mask is None else lay.mask.to(torch.uint8).to(DEV).contiguous()
        self.kl = torch.tensor(lay.lens, dtype=torch.int32, device=DEV) if lay.key_len else None
        self.gd = torch.tensor(lay.groups, dtype=torch.int32, device=DEV)
        self.stride = NH * lay.Mpad * (128 if lay.kind == 'split' else 64)
        self.live = lay.live.to(DEV)
        self._ref = None

    def ref(self):
        """float64 over the bytes of the slabs, computed once per plant"""
        if self._ref is None:
            Kv, Vv = natural(self.kind, self.K0, self.Vt0)
            self._ref = ref_cross(self.qv, Kv, Vv, self.lay.counts, self.live)
        return self._ref


def launch(pp, S, out, tag, pairs=False):
    """one launch; appends the memory-discipline record -> the output rows [R, d] (pairs: (hi rows, lo rows) bf16)"""
    from advancedliteratemachinery_amd import ops
    lay = pp.lay
    R = lay.R
    partial = _filled((R + GUARD, NH, S, 68), torch.float32) if S > 1 else None
    args = (pp.q, pp.K, pp.Vt, pp.stride, lay.Mpad, pp.km, pp.gd, len(lay.groups), lay.qt, None if partial is None else partial[:R])
    if pairs:
        lo_off = D + PAD
        obuf = _filled((R + GUARD, 2 * D + 3 * PAD), torch.bfloat16)
        ops.cross_attn_pairs(*args, obuf[:R, PAD:], lo_off, lay.M, NH, S, key_len=pp.kl)
        wins = [(PAD, PAD + D), (PAD + lo_off, PAD + lo_off + D)]
    else:
        obuf = _filled((R + GUARD, D + 2 * PAD), pp.qdt)
        ops.dec_cross_attn_step(*args, obuf[:R, PAD:PAD + D], lay.M, NH, S, key_len=pp.kl)
        wins = [(PAD, PAD + D)]
    torch.cuda.synchronize()
    probs = []
    edges = [0] + [c for w in wins for c in w] + [obuf.shape[1]]
    if not all(_is_nan_fill(obuf[:R, a:b]) for a, b in zip(edges[0::2], edges[1::2])):
        probs.append('out written outside its column window')
    if not _is_nan_fill(obuf[R:]):
        probs.append('out guard rows written')
    if partial is not None and not _is_nan_fill(partial[R:]):
        probs.append('partial guard rows written')
    if not (_same_bits(pp.K, pp.K0) and _same_bits(pp.Vt, pp.Vt0)):
        probs.append('a slab changed')
    got = [obuf[:R, a:b] for a, b in wins]
    if not all(bool(torch.isfinite(g).all().item()) for g in got):
        probs.append('NaN / inf in an output row')
    out.append(rec(tag + ': slabs bit-identical, nothing written beside the output rows, outputs finite%s' % ('' if not probs else ' -- ' + '; '.join(probs)),
                   len(probs), 0))
    return got if pairs else got[0]


def _tag(pp, S, ring, nt, extra=''):
    lay = pp.lay
    return 'cross_attn %s[%s qt%d ring%d nt%d S%d M%d%s mask=%s%s]' % (pp.name, pp.kind, lay.qt, ring, nt, S, lay.M, '' if lay.key_len else ' no key_len',
                                                                       lay.mask_name, extra)


class Worst:
    """the worst error per (case, ring, nt) of one check -> rrec records"""

    def __init__(self):
        self.w = {}

    def add(self, key, err, where):
        if key not in self.w or not err <= self.w[key][0]:
            self.w[key] = (err, where)

    def records(self, kind, qt, gate_of):
        return [rrec('cross_attn %s[%s qt%d ring%d nt%d] worst' % (case, kind, qt, ring, nt), e, gate_of(case), 'worst at ' + where)
                for (case, ring, nt), (e, where) in sorted(self.w.items())]


def _walk_launch(out, worst, pp, S, ring, nt, extra=''):
    tag = _tag(pp, S, ring, nt, extra)
    got = launch(pp, S, out, tag)
    e = head_rel(got, pp.want, NH)
    i = int(e.reshape(-1).argmax())
    err = e.reshape(-1)[i].item()
    note = 'worst at row %d (image %d, %d keys) head %d target %d' % (i // NH, int(pp.lay.row_img[i // NH]), pp.lay.lens[int(pp.lay.row_img[i // NH])], i % NH,
                                                                      int(pp.tgt[i // NH, i % NH]))
    out.append(rec(tag + ' vs the stated output per (row, head)', err, walk_gate(pp.kind), note))
    worst.add((pp.name + ' walk', ring, nt), err, tag)


def _walk_plants(lay, bases, pick):
    yield Prepared(plant_peaked(lay, bases, DEV))
    yield Prepared(plant_uniform(lay, bases, pick, DEV))


def check_walks(kind, qt, rings=None):
    """both walks over LENGTHS under every mask: the default variant (ring 1, nt 1) at n_split 1 and 2 in every phase of the sweep; every
    variant at every n_split in the first and the last phase"""
    out, worst = [], Worst()
    var = variants(kind, qt, rings)
    for mask in MASKS:
        phases = sweep(kind, qt, mask)
        for pi, (lay, bases) in enumerate(phases):
            edge = pi in (0, len(phases) - 1)
            if not edge and (1, 1) not in var:
                continue
            for pp in _walk_plants(lay, bases, pi):
                for ring, nt in var:
                    if not edge and (ring, nt) != (1, 1):
                        continue
                    with variant(ring, nt):
                        for S in (S_ALL if edge else (1, 2)):
                            _walk_launch(out, worst, pp, S, ring, nt, ' phase %d/%d' % (pi, len(phases)))
    return out + worst.records(kind, qt, lambda case: walk_gate(kind))


def check_walks_ragged_m(kind, qt, rings=None):
    """key_len = None and M itself ragged (77, 129, 640; Mpad rounded up per kind: the padded keys are loud), and the long case M = 2081"""
    out, worst = [], Worst()
    for M in RAGGED_M + (LONG_M,):
        for mask in (('none',) if M == LONG_M else ('none', 'lead')):
            B = 2 if M == LONG_M else 4
            counts = sorted(rows_of_phase(qt, len(ROWS[qt]) - 2, B), reverse=True)
            lay = Layout(kind, [M] * B, counts, M, qt, mask, key_len=False)
            for pi, (_, bases) in enumerate(edge_phases(lay)):
                for pp in _walk_plants(lay, bases, pi):
                    for ring, nt in variants(kind, qt, rings):
                        with variant(ring, nt):
                            for S in S_ALL:
                                _walk_launch(out, worst, pp, S, ring, nt, ' edge %d' % pi)
    return out + worst.records(kind, qt, lambda case: walk_gate(kind))


def _f64_launch(out, worst, pp, S, ring, nt):
    tag = _tag(pp, S, ring, nt)
    got = launch(pp, S, out, tag)
    err = (got.double() - pp.ref()).abs().max().item()
    out.append(rec(tag + ' vs float64', err, TOL[pp.kind]))
    worst.add((pp.name, ring, nt), err, tag)


def _f64_check(kind, qt, rings, plants):
    out, worst = [], Worst()
    for plant in plants:
        pp = Prepared(plant)
        for ring, nt in variants(kind, qt, rings):
            with variant(ring, nt):
                for S in S_ALL:
                    _f64_launch(out, worst, pp, S, ring, nt)
    return out + worst.records(kind, qt, lambda case: TOL[kind])


def _lengths_layout(kind, qt, mask, phase=0):
    return Layout(kind, LENGTHS, rows_of_phase(qt, phase, len(LENGTHS)), M_SLAB, qt, mask)


def _long_layout(kind, qt):
    return Layout(kind, [LONG_M] * 2, sorted(rows_of_phase(qt, len(ROWS[qt]) - 2, 2), reverse=True), LONG_M, qt, 'none', key_len=False)


def check_ramps(kind, qt, rings=None):
    """rising and falling score ramps over LENGTHS (no mask / the 2-D padding mask) and over the long case"""
    def plants():
        for rising in (True, False):
            for mi, mask in enumerate(('none', 'pad2d')):
                yield plant_ramp(_lengths_layout(kind, qt, mask, mi + 1), rising, DEV)
            yield plant_ramp(_long_layout(kind, qt), rising, DEV)
    return _f64_check(kind, qt, rings, plants())


def check_plane_ramps(qt, rings=None):
    def plants():
        for which in ('klo', 'qlo'):
            for mi, mask in enumerate(('none', 'lead')):
                yield plant_plane_ramp(_lengths_layout('split', qt, mask, mi + 2), which, DEV)
    return _f64_check('split', qt, rings, plants())


def check_random(kind, qt, rings=None):
    def plants():
        for mi, mask in enumerate(('none', 'lead')):
            yield plant_random(_lengths_layout(kind, qt, mask, mi + 3), DEV)
        yield plant_random(_long_layout(kind, qt), DEV)
    return _f64_check(kind, qt, rings, plants())


def groups_layout(kind, qt, mask='none'):
    """several groups per image, as Decoder.make_prefill_tiles cuts them: two or three groups of 16 qt rows plus a remainder; the second
    image's row0 is no multiple of 16.  Rows 64 apart share a code and a target."""
    g = 16 * qt
    return Layout(kind, [640, 385, 33, 129], [2 * g + 5, 3 * g + 1, 7, 3 * g - 1], M_SLAB, qt, mask)


def check_groups(kind, qt, rings=None):
    out, worst = [], Worst()
    lay = groups_layout(kind, qt)
    assert any(r0 % 16 for r0, _, _ in lay.groups) and max(sum(1 for g in lay.groups if g[2] == b) for b in range(lay.B)) >= 4
    plants = [Prepared(plant_peaked(lay, edge_phases(lay)[1][1], DEV)), Prepared(plant_uniform(lay, [0] * lay.B, 1, DEV)),
              Prepared(plant_ramp(groups_layout(kind, qt, 'pad2d'), True, DEV))]
    for pp in plants:
        for ring, nt in variants(kind, qt, rings):
            with variant(ring, nt):
                for S in S_ALL:
                    if pp.want is None:
                        _f64_launch(out, worst, pp, S, ring, nt)
                    else:
                        _walk_launch(out, worst, pp, S, ring, nt, ' groups')
    return out + worst.records(kind, qt, lambda case: walk_gate(kind) if case.endswith('walk') else TOL[kind])


# ---------------------------------------------------------------------------------------------------------------------------------------
# split-pair output rows (CrossP.lo_off > 0, omp_debug_cross_attn_pairs): what step_launch_x3 runs over split-plane slabs
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_pairs(qt, rings=None):
    """the pair rows against the fp32 rows of the same launch configuration: hi == bf16(val), lo == bf16(val - hi), bit for bit; n_split 1 on
    both kernels and n_split > 1 (the merge kernel)"""
    out = []
    lay = _lengths_layout('split', qt, 'lead', 1)
    plants = [Prepared(plant_random(lay, DEV, seed=7)), Prepared(plant_peaked(lay, [0] * lay.B, DEV)), Prepared(plant_random(groups_layout('split', qt), DEV, seed=8))]
    for pp in plants:
        for ring, nt in variants('split', qt, rings):
            with variant(ring, nt):
                for S in (1, 2, 16):
                    tag = _tag(pp, S, ring, nt, ' pairs')
                    val = launch(pp, S, out, tag + ' (fp32 rows)')
                    hi, lo = launch(pp, S, out, tag, pairs=True)
                    want_hi = val.to(torch.bfloat16)
                    want_lo = (val - want_hi.float()).to(torch.bfloat16)
                    out.append(rec(tag + ': hi == bf16(val) and lo == bf16(val - hi), bit for bit',
                                   int((hi.view(torch.int16) != want_hi.view(torch.int16)).sum()) + int((lo.view(torch.int16) != want_lo.view(torch.int16)).sum()), 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_refusals():
    """every refusal is a host-side check before any launch: OMP_ERR_INVALID, the error text set, out and partial untouched"""
    from advancedliteratemachinery_amd import _lib, ops
    h = _lib.lib()
    out = []
    R, M, S = 4, 64, 2
    groups = torch.tensor([[0, R, 0]], dtype=torch.int32, device=DEV)
    for kind in KINDS:
        KB = key_block(kind)
        qdt = torch.bfloat16 if kind == 'bf16' else torch.float32
        K, Vt = slabs(kind, torch.zeros(1, NH, M, HD, device=DEV), torch.zeros(1, NH, M, HD, device=DEV))
        qbuf = torch.zeros(R, D + 8, dtype=qdt, device=DEV)
        o, partial = _filled((R, D), qdt), _filled((R, NH, 16, 68), torch.float32)
        bufs = (o, partial)
        code = ops.OMP_BF16X2 if kind == 'split' else ops.dt(qdt)
        stride = NH * M * (128 if kind == 'split' else 64)

        def step(q=qbuf[:, :D], ldq=D + 8, Mpad=M, n_groups=1, q_tiles=1, R=R, partial=partial, out=o, ldo=D, dtype=code, M=M, n_split=S):
            return h.omp_dec_cross_attn_step(ops.ptr(q), ldq, ops.ptr(K), ops.ptr(Vt), stride, Mpad, None, None, ops.ptr(groups), n_groups, q_tiles, R,
                                             ops.ptr(partial), ops.ptr(out), ldo, dtype, M, NH, n_split, ops.stream())
        t = 'omp_dec_cross_attn_step [%s]' % kind
        for bad in (0, 3, 32):
            _refused(out, t + ' n_split %d' % bad, lambda: step(n_split=bad), bufs)
        _refused(out, t + ' q_tiles 3', lambda: step(q_tiles=3), bufs)
        _refused(out, t + ' n_split 2 without a partial buffer', lambda: step(partial=None), bufs)
        _refused(out, t + ' Mpad no multiple of %d' % KB, lambda: step(Mpad=M + KB // 2, M=M), bufs)
        _refused(out, t + ' Mpad < M', lambda: step(Mpad=M - KB, M=M), bufs)
        _refused(out, t + ' R = 0', lambda: step(R=0), bufs)
        _refused(out, t + ' M = 0', lambda: step(M=0), bufs)
        if kind == 'split':
            _refused(out, t + ' ldq % 4 != 0', lambda: step(ldq=D + 6), bufs)
            _refused(out, t + ' q not 16-byte aligned', lambda: step(q=qbuf[:, 2:D + 2]), bufs)
            po = _filled((R, 2 * D + 8), torch.bfloat16)
            pb = (po, partial)

            def pairs(out=po, ldo=2 * D + 8, lo_off=D, dtype=code, n_split=S, partial=partial, q=qbuf[:, :D], ldq=D + 8):
                return h.omp_debug_cross_attn_pairs(ops.ptr(q), ldq, ops.ptr(K), ops.ptr(Vt), stride, M, None, None, ops.ptr(groups), 1, 1, R, ops.ptr(partial),
                                                    ops.ptr(out), ldo, lo_off, dtype, M, NH, n_split, ops.stream())
            t = 'omp_debug_cross_attn_pairs'
            _refused(out, t + ' fp32 slabs', lambda: pairs(dtype=ops.dt(torch.float32)), pb)
            _refused(out, t + ' bf16 slabs', lambda: pairs(dtype=ops.dt(torch.bfloat16)), pb)
            _refused(out, t + ' lo_off 0', lambda: pairs(lo_off=0), pb)
            _refused(out, t + ' lo_off % 4 != 0', lambda: pairs(lo_off=D + 2), pb)
            _refused(out, t + ' ldo % 4 != 0', lambda: pairs(ldo=2 * D + 6), pb)
            _refused(out, t + ' out not 8-byte aligned', lambda: pairs(out=po[:, 2:]), pb)
            _refused(out, t + ' ldq % 4 != 0', lambda: pairs(ldq=D + 6), pb)
            _refused(out, 'omp_dec_cross_attn_step through the pairs entry: n_split 3', lambda: pairs(n_split=3), pb)
            _refused(out, 'omp_dec_cross_attn_step through the pairs entry: n_split 2 without a partial buffer', lambda: pairs(partial=None), pb)
    return out
