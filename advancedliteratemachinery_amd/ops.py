"""Thin tensor -> pointer wrappers over the C ABI (include/omp355.h).

PyTorch is used for device memory and streams only; every computation below happens inside
libomp355.so.  All wrappers launch on torch's CURRENT stream and never synchronise.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, ACT_RELU, OMP_BF16, OMP_BF16X2, OMP_F32  # noqa: F401

_DT = {torch.float32: OMP_F32, torch.bfloat16: OMP_BF16}
SPLIT = 'bf16x2'   # out_dtype of producers that write split-bf16 pair rows [hi | lo] (OMP_BF16X2): a bf16 tensor [rows, 2C]


def dt(t):
    try:
        return _DT[t if isinstance(t, torch.dtype) else t.dtype]
    except KeyError:
        raise TypeError('libomp355 supports float32/bfloat16 tensors only, got %s' % (t,))


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('libomp355 ops need device tensors (got a CPU tensor); there is no CPU fallback')
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _c(t, name):
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)
    return t


def layernorm(x, gamma, beta, out_dtype=None, out=None, out_f32=None, eps=1e-5, want_out=True):
    """x [rows, C] -> LN in `out_dtype` (default x.dtype) and/or fp32 copy."""
    _c(x, 'x')
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    out_dtype = out_dtype or x.dtype
    split = out_dtype == SPLIT
    if out is None and want_out:
        out = (torch.empty((rows, 2 * C), dtype=torch.bfloat16, device=x.device) if split
               else torch.empty(x.shape, dtype=out_dtype, device=x.device))
    rc = _lib.lib().omp_layernorm(ptr(x), dt(x), ptr(gamma), ptr(beta), ptr(out),
                                  OMP_BF16X2 if split else (dt(out) if out is not None else OMP_F32), ptr(out_f32), rows, C,
                                  float(eps), stream())
    _lib.check(rc, 'omp_layernorm')
    return out


def layernorm_sampled(x, gamma, beta, B, H, W, step, group, out_dtype=None, eps=1e-5):
    """x [B*H*W, C] -> LN of the rows and columns q * step + r (r < group) only, as a compact [B * hq * wq, C] map in `out_dtype`
    (default x.dtype); -> (map, hq, wq).  omp_layernorm_sampled: the other pixels are never read."""
    _c(x, 'x')
    C = x.shape[-1]
    if x.numel() != B * H * W * C:
        raise ValueError('layernorm_sampled: x must hold B * H * W rows')
    hq, wq = H // step * group, W // step * group
    out = torch.empty((B * hq * wq, C), dtype=out_dtype or x.dtype, device=x.device)
    rc = _lib.lib().omp_layernorm_sampled(ptr(x), dt(x), ptr(gamma), ptr(beta), ptr(out), dt(out), B, H, W, C, step, group, float(eps), stream())
    _lib.check(rc, 'omp_layernorm_sampled')
    return out, hq, wq


def gemm(A, W, bias=None, residual=None, act=ACT_NONE, out=None, out_dtype=None, M=None, lda=None,
         ldw=None, ldc=None, N=None, K=None, bias_row=None, bias_row_stride=0, trans_rows=0, trans_ld=0,
         ln=None, ln_eps=1e-5, small_m=False, store_mode=0, kv=None, bias_along_m=False, out_noresidual=None, a_wrap=0,
         bias_row_mod=0, bias_row_off=0):
    """out[M,N] = act(A[M,K] @ W[N,K]^T + bias) + residual.  A/W may be strided row views (lda/ldw).
    bias_row_mod > 0: bias is a table of bias_row_stride-pitched rows and row m takes table row (bias_row_off + m) % bias_row_mod.
    out_noresidual (optional, with a residual): also receives act(A W^T + bias) without the residual.
    a_wrap > 0: bf16x3 product -- A is a split-bf16 pair tensor [M, a_wrap] = [hi | lo], W the [N, K] = [hi | hi | lo] image of an
    fp32 weight (split_weight3), K = 3/2 a_wrap.  out_dtype=SPLIT: the result is written as split pairs [M, 2N]."""
    K = K or (W.shape[-1] if a_wrap else A.shape[-1])
    N = N or W.shape[0]
    M = M or A.numel() // A.shape[-1]
    lda = lda or A.stride(-2) if A.dim() > 1 else K
    ldw = ldw or W.stride(0)
    out_dtype = out_dtype or W.dtype
    split = out_dtype == SPLIT
    if out is None:
        if trans_rows:
            raise ValueError('trans_out needs a preallocated (zeroed) output')
        out = torch.empty((M, 2 * N if split else N), dtype=torch.bfloat16 if split else out_dtype, device=A.device)
    ldc = ldc or (out.stride(-2) if out.dim() > 1 and not store_mode else N)
    a = _lib.GemmArgs()
    a.A, a.lda, a.W, a.ldw = ptr(A), lda, ptr(W), ldw
    a.bias, a.bias_row, a.bias_row_stride = ptr(bias), ptr(bias_row), bias_row_stride
    a.bias_row_mod, a.bias_row_off = int(bias_row_mod), int(bias_row_off)
    a.residual, a.ldr = ptr(residual), (residual.stride(-2) if residual is not None else 0)
    a.C, a.ldc = ptr(out), ldc
    a.M, a.N, a.K = M, N, K
    a.dtype, a.out_dtype, a.act = dt(W), (OMP_BF16X2 if split else dt(out)), act
    a.a_wrap = int(a_wrap)
    if ln is not None:
        a.ln_gamma, a.ln_beta, a.ln_eps = ptr(ln[0]), ptr(ln[1]), float(ln_eps)
    a.small_m_splitk = 1 if small_m else 0
    a.store_mode, a.bias_along_m = store_mode, 1 if bias_along_m else 0
    if kv is not None:  # (images, tokens per image, padded tokens, heads, key block) of the blocked K / V^T slabs
        a.kv_images, a.kv_tokens, a.kv_mpad, a.kv_heads, a.kv_key_block = kv
    a.trans_out, a.trans_rows, a.trans_ld = (1 if trans_rows else 0), trans_rows, trans_ld
    if out_noresidual is not None:
        a.C2, a.ldc2 = ptr(out_noresidual), out_noresidual.stride(-2)
    rc = _lib.lib().omp_gemm_bias_act(ctypes.byref(a), stream())
    _lib.check(rc, 'omp_gemm_bias_act')
    return out


def gemm_choice(M, N, K, dtype=OMP_BF16, out_dtype=None, act=ACT_NONE, residual=False, bias=True, a_wrap=0, store_mode=0, kv=None,
                lda=None, ldw=None, ldc=None, two_destinations=False, ln=False, small_m=False, base=1 << 20):
    """Host logic only (no device, no launch): the kernel selector omp_gemm_bias_act would take for a product of this shape -- the
    dispatch table of csrc/gemm.hip as a function (tests/test_host_logic.py pins it).  Pointers are synthetic, 4 KB-aligned addresses:
    the library only tests them for null and alignment.  Returns the selector (a row of
    csrc/gemm.hip: GEMM_SELECTORS) or raises on an argument error."""
    out_dtype = dtype if out_dtype is None else out_dtype
    a = _lib.GemmArgs()
    split = out_dtype == OMP_BF16X2
    ka = a_wrap if a_wrap else K
    a.A, a.lda, a.W, a.ldw = base, lda or ka, base + (1 << 30), ldw or K
    a.bias = base + (2 << 30) if bias else None
    a.residual, a.ldr = (base + (3 << 30), N) if residual else (None, 0)
    a.C, a.ldc = base + (4 << 30), ldc or (2 * N if split else N)
    a.M, a.N, a.K = M, N, K
    a.dtype, a.out_dtype, a.act, a.a_wrap = dtype, out_dtype, act, int(a_wrap)
    if ln:
        a.ln_gamma, a.ln_beta, a.ln_eps = base + (5 << 30), base + (6 << 30), 1e-5
    a.small_m_splitk = 1 if small_m else 0
    a.store_mode = store_mode
    if kv is not None:
        a.kv_images, a.kv_tokens, a.kv_mpad, a.kv_heads, a.kv_key_block = kv
    if two_destinations:
        a.C2, a.ldc2 = base + (7 << 30), N
    rc = _lib.lib().omp_debug_gemm_choice(ctypes.byref(a))
    if rc < 0:
        _lib.check(rc, 'omp_debug_gemm_choice')
    return rc


def swin_mlp_fused(x, ln_g, ln_b, wpack, b2, out=None, eps=1e-5):
    """x [M, C] bf16 or fp32 (fp32 residual stream) -> x + fc2(GELU(fc1(LN(x)))) in one launch, same type; wpack from
    model.packing.pack_mlp (bf16 matrix-core operands either way).  out may be x."""
    _c(x, 'x')
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError('swin_mlp_fused takes a bf16 or fp32 residual stream')
    M, C = x.numel() // x.shape[-1], x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    rc = _lib.lib().omp_swin_mlp_fused2(ptr(x), dt(x), C, ptr(ln_g), ptr(ln_b), float(eps), ptr(wpack), ptr(b2), ptr(out), C, M, C,
                                        wpack.shape[0] * 32, stream())
    _lib.check(rc, 'omp_swin_mlp_fused')
    return out


def patch_embed_ln(img, w, b, gamma, beta, out_dtype, eps=1e-5):
    _c(img, 'img')
    B, _, H, W = img.shape
    E = w.shape[0]
    Hp, Wp = (H + 3) // 4, (W + 3) // 4
    out = torch.empty((B, Hp * Wp, E), dtype=out_dtype, device=img.device)
    rc = _lib.lib().omp_patch_embed_ln(ptr(img), ptr(w), ptr(b), ptr(gamma), ptr(beta), ptr(out), dt(out),
                                       B, H, W, E, float(eps), stream())
    _lib.check(rc, 'omp_patch_embed_ln')
    return out, Hp, Wp


def swin_expand_bias(table):
    """relative_position_bias_table fp32 [169, nH] -> fp32 [nH, 64, 64] (bias / scale, -inf on padding keys), once per checkpoint."""
    nH = table.shape[1]
    out = torch.empty((nH, 64, 64), dtype=torch.float32, device=table.device)
    _lib.check(_lib.lib().omp_swin_expand_bias(ptr(_c(table, 'table')), nH, ptr(out), stream()), 'omp_swin_expand_bias')
    return out


def swin_window_attn(qkv, qkv_bias, table, B, H, W, C, nH, shift, out=None, window=7, bias_expanded=None, out_split=False):
    """out_split (fp32 qkv only): out is [B*H*W, 2C] bf16 split pairs [hi | lo] for the bf16x3 proj GEMM."""
    _c(qkv, 'qkv')
    if out is None:
        out = (torch.empty((B * H * W, 2 * C), dtype=torch.bfloat16, device=qkv.device) if out_split
               else torch.empty((B * H * W, C), dtype=qkv.dtype, device=qkv.device))
    rc = _lib.lib().omp_swin_window_attn2(ptr(qkv), ptr(qkv_bias), ptr(table), ptr(bias_expanded), ptr(out), dt(qkv),
                                          OMP_BF16X2 if out_split else dt(qkv), B, H, W, C, nH, window, shift, stream())
    _lib.check(rc, 'omp_swin_window_attn')
    return out


def swin_attn_block(x, ln_g, ln_b, qkv_w, qkv_b, bias_expanded, proj_w, proj_b, B, H, W, C, nH, shift, out=None, window=7, eps=1e-5):
    """x (fp32 [B*H*W, C]) -> x + proj(window attention(qkv(LayerNorm(x)))) in one launch (omp_swin_attn_block: C = 128, 4 heads);
    out defaults to x (in place)."""
    _c(x, 'x')
    _c(qkv_w, 'qkv_w')
    _c(proj_w, 'proj_w')
    if x.dtype != torch.float32 or qkv_w.dtype != torch.bfloat16 or proj_w.dtype != torch.bfloat16:
        raise TypeError('swin_attn_block: fp32 residual stream with bf16 weights')
    if x.numel() != B * H * W * C or tuple(qkv_w.shape) != (3 * C, C) or tuple(proj_w.shape) != (C, C) or bias_expanded.numel() != nH * 4096:
        raise ValueError('swin_attn_block: x [B*H*W, C], qkv_w [3C, C], proj_w [C, C], bias_expanded [nH, 64, 64] expected')
    out = x if out is None else _c(out, 'out')
    if out.dtype != torch.float32 or out.numel() != x.numel():
        raise ValueError('swin_attn_block: out must be fp32 with the shape of x')
    rc = _lib.lib().omp_swin_attn_block(ptr(x), ptr(out), ptr(ln_g), ptr(ln_b), float(eps), ptr(qkv_w), ptr(qkv_b), ptr(bias_expanded),
                                        ptr(proj_w), ptr(proj_b), B, H, W, C, nH, window, shift, stream())
    _lib.check(rc, 'omp_swin_attn_block')
    return out


def swin_attn_block_packed(x, ln_g, ln_b, wpack, qkv_b, bias_expanded, proj_b, B, H, W, C, nH, shift, out=None, window=7, eps=1e-5):
    """swin_attn_block for C = 256 with 8 heads: wpack = model.packing.pack_attn_block(qkv.weight, proj.weight, nH) (omp_swin_attn_block_packed)."""
    _c(x, 'x')
    if x.dtype != torch.float32 or wpack.dtype != torch.bfloat16:
        raise TypeError('swin_attn_block_packed: fp32 residual stream with a bf16 weight image')
    out = x if out is None else out
    rc = _lib.lib().omp_swin_attn_block_packed(ptr(x), ptr(out), ptr(ln_g), ptr(ln_b), float(eps), ptr(wpack), ptr(qkv_b), ptr(bias_expanded),
                                               ptr(proj_b), B, H, W, C, nH, window, shift, stream())
    _lib.check(rc, 'omp_swin_attn_block_packed')
    return out


def patch_merge_gather_ln(x, gamma, beta, B, H, W, C, eps=1e-5, out_dtype=None):
    """out_dtype: x.dtype (default), torch.bfloat16 for an fp32 x, or SPLIT (split pairs [rows, 8C])."""
    _c(x, 'x')
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    out_dtype = out_dtype or x.dtype
    split = out_dtype == SPLIT
    out = torch.empty((B * H2 * W2, (8 if split else 4) * C), dtype=torch.bfloat16 if split else out_dtype, device=x.device)
    rc = _lib.lib().omp_patch_merge_gather_ln2(ptr(x), dt(x), ptr(gamma), ptr(beta), ptr(out), OMP_BF16X2 if split else dt(out),
                                               B, H, W, C, float(eps), stream())
    _lib.check(rc, 'omp_patch_merge_gather_ln')
    return out, H2, W2


def split_bf16(x, triple=False, out=None):
    """fp32 [rows, C] -> bf16 split pairs [rows, 2C] = [hi | lo] (triple: [rows, 3C] = [hi | hi | lo]); omp_split_bf16."""
    if x.dtype != torch.float32:
        raise TypeError('split_bf16 takes fp32 rows')
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    n = 3 if triple else 2
    if out is None:
        out = torch.empty((rows, n * C), dtype=torch.bfloat16, device=x.device)
    rc = _lib.lib().omp_split_bf16(ptr(x), x.stride(-2) if x.dim() > 1 else C, ptr(out), out.stride(-2), rows, C, 1 if triple else 0, stream())
    _lib.check(rc, 'omp_split_bf16')
    return out


def split_weight3(w):
    """fp32 weight [N, K] -> bf16 [N, 3K] = [w_hi | w_hi | w_lo]: the W-side image of a bf16x3 product (once per checkpoint)."""
    w = w.detach().float()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, hi, lo], dim=1).contiguous()


def split_weight2(w):
    """fp32 weight [N, K] -> bf16 [N, 2K] = [w_hi | w_lo]: the A-side operand of a bf16x3 product with swapped operands."""
    w = w.detach().float()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=1).contiguous()


def fpn_fuse(l2, l3, l4, l5, B, sizes, stride):
    (h2, w2), (h3, w3), (h4, w4), (h5, w5) = sizes
    ho, wo = (h3 + stride - 1) // stride, (w3 + stride - 1) // stride
    out = torch.empty((B * ho * wo, 1024), dtype=l2.dtype, device=l2.device)
    rc = _lib.lib().omp_fpn_fuse(ptr(l2), ptr(l3), ptr(l4), ptr(l5), ptr(out), dt(l2), B, h2, w2, h3, w3,
                                 h4, w4, h5, w5, stride, stream())
    _lib.check(rc, 'omp_fpn_fuse')
    return out, ho, wo


def fpn_fuse_sampled(l2s, l3s, l4, l5, B, sizes):
    """fpn_fuse(..., stride=2) from the sampled laterals (omp_fpn_fuse_sampled): l3s [B*h4*w4, 256] holds l3's pixels (2ty, 2tx), l2s
    [B*2h4*2w4, 256] l2's rows / columns {4t, 4t+1}; `sizes` are the FULL level sizes, which must be regular (h2 == 2 h3 == 4 h4)."""
    (h2, w2), (h3, w3), (h4, w4), (h5, w5) = sizes
    if l3s.shape[0] != B * h4 * w4 or l2s.shape[0] != 4 * B * h4 * w4:
        raise ValueError('fpn_fuse_sampled: l3s must hold B * h4 * w4 rows and l2s four times as many')
    out = torch.empty((B * h4 * w4, 1024), dtype=l2s.dtype, device=l2s.device)
    rc = _lib.lib().omp_fpn_fuse_sampled(ptr(_c(l2s, 'l2s')), ptr(_c(l3s, 'l3s')), ptr(l4), ptr(l5), ptr(out), dt(l2s), B, h2, w2, h3, w3,
                                         h4, w4, h5, w5, stream())
    _lib.check(rc, 'omp_fpn_fuse_sampled')
    return out, h4, w4


def mask_nearest(mask_u8, h, w):
    """uint8 [B,H,W] -> uint8 [B,h,w]: F.interpolate(..., mode='nearest') of the reference (swin_transformer.py:621)."""
    _c(mask_u8, 'mask')
    B, H, W = mask_u8.shape
    out = torch.empty((B, h, w), dtype=torch.uint8, device=mask_u8.device)
    rc = _lib.lib().omp_mask_nearest(ptr(mask_u8), ptr(out), B, H, W, h, w, stream())
    _lib.check(rc, 'omp_mask_nearest')
    return out


def sine_posembed(mask_u8, npf, out_dtype, temperature=10000.0):
    _c(mask_u8, 'mask')
    B, h, w = mask_u8.shape
    out = torch.empty((B, h * w, 2 * npf), dtype=out_dtype, device=mask_u8.device)
    rc = _lib.lib().omp_sine_posembed(ptr(mask_u8), ptr(out), dt(out), B, h, w, npf, float(temperature),
                                      stream())
    _lib.check(rc, 'omp_sine_posembed')
    return out


def dec_embed_ln(seq, d_pos, word, postab, gamma, beta, x=None, y=None, eps=1e-5):
    R, d = seq.shape[0], word.shape[1]
    rc = _lib.lib().omp_dec_embed_ln(ptr(seq), seq.stride(0), ptr(d_pos), ptr(word), ptr(postab), ptr(gamma),
                                     ptr(beta), ptr(x), ptr(y), dt(y) if y is not None else OMP_F32, R, d,
                                     float(eps), stream())
    _lib.check(rc, 'omp_dec_embed_ln')


def dec_self_attn_step(qkv, kcache, vcache, out, d_pos, nH):
    R, d3 = qkv.shape
    d = d3 // 3
    rc = _lib.lib().omp_dec_self_attn_step(ptr(qkv), ptr(kcache), ptr(vcache), ptr(out), ptr(d_pos), dt(qkv),
                                           R, nH, d, kcache.shape[1], stream())
    _lib.check(rc, 'omp_dec_self_attn_step')


def dec_cross_attn_step(q, K, Vt, img_stride, Mpad, key_mask, groups, n_groups, q_tiles, partial, out, M, nH, n_split, key_len=None):
    """K / Vt in q's dtype: the bf16 / fp32 slabs; fp32 q with bf16 K / Vt: SPLIT-PLANE slabs (OMP_BF16X2: 32-key blocks of
    [hi plane | lo plane], img_stride = nH * Mpad * 128 bf16 elements; fp32 out).
    key_len: None, or device int32 [B] with 1 <= key_len[b] <= M -- image b attends over its first key_len[b] keys only (ragged batches)."""
    if key_len is not None and (key_len.dtype != torch.int32 or not key_len.is_contiguous()):
        raise TypeError('dec_cross_attn_step: key_len is a contiguous int32 device tensor')
    R = q.shape[0]
    split = q.dtype == torch.float32 and K.dtype == torch.bfloat16
    if split and (Vt.dtype != torch.bfloat16 or out.dtype != torch.float32):
        raise TypeError('split-plane slabs: bf16 K and V^T planes, fp32 q and out')
    if not split and (K.dtype != q.dtype or Vt.dtype != q.dtype or out.dtype != q.dtype):
        raise TypeError('dec_cross_attn_step: q, K, V^T and out share one dtype (or fp32 q / out over split-plane bf16 slabs)')
    rc = _lib.lib().omp_dec_cross_attn_step(ptr(q), q.stride(0), ptr(K), ptr(Vt), img_stride, Mpad, ptr(key_mask),
                                            ptr(key_len), ptr(groups), n_groups, q_tiles, R, ptr(partial), ptr(out), out.stride(0),
                                            OMP_BF16X2 if split else dt(q), M, nH, n_split, stream())
    _lib.check(rc, 'omp_dec_cross_attn_step')


def cross_attn_pairs(q, K, Vt, img_stride, Mpad, key_mask, groups, n_groups, q_tiles, partial, out, lo_off, M, nH, n_split, key_len=None):
    """debug/testing: dec_cross_attn_step over SPLIT-PLANE slabs (fp32 q, bf16 K / V^T planes) whose output rows are split-bf16 pairs, as
    the bf16x3 engine launches it: out [R, >= lo_off + 64 nH] bf16, hi = bf16(value) in columns [0, 64 nH), lo = bf16(value - hi) lo_off
    columns further (omp_debug_cross_attn_pairs)."""
    if q.dtype != torch.float32 or K.dtype != torch.bfloat16 or Vt.dtype != torch.bfloat16 or out.dtype != torch.bfloat16:
        raise TypeError('cross_attn_pairs: fp32 q, bf16 K and V^T planes, bf16 pair rows')
    if key_len is not None and (key_len.dtype != torch.int32 or not key_len.is_contiguous()):
        raise TypeError('cross_attn_pairs: key_len is a contiguous int32 device tensor')
    rc = _lib.lib().omp_debug_cross_attn_pairs(ptr(q), q.stride(0), ptr(K), ptr(Vt), img_stride, Mpad, ptr(key_mask), ptr(key_len),
                                               ptr(groups), n_groups, q_tiles, q.shape[0], ptr(partial), ptr(out), out.stride(0),
                                               int(lo_off), OMP_BF16X2, M, nH, n_split, stream())
    _lib.check(rc, 'omp_debug_cross_attn_pairs')


def head_sample(logits, cfg, seq, probs, finished, lengths, d_pos, advance=True):
    R = logits.shape[0]
    rc = _lib.lib().omp_head_softmax_mask_argmax(ptr(logits), logits.stride(0), R, ctypes.byref(cfg), ptr(seq),
                                                 ptr(probs), seq.stride(0), ptr(finished), ptr(lengths),
                                                 ptr(d_pos), 1 if advance else 0, stream())
    _lib.check(rc, 'omp_head_softmax_mask_argmax')


def pack_spotting(points, poly, rec, rprob, counts, N, rec_len):
    """Decoded rows (device int32 [R,2] / [R,>=32] / [R,>=rec_len], fp32 [R,>=rec_len]; rows sorted by image, counts per image)
    -> (ids int32 [B, N, 34 + rec_len], probs fp32 [B, N, rec_len], n_inst int32 [B]) in ONE launch (omp_pack_spotting)."""
    dev = points.device
    B = len(counts)
    c = torch.tensor(counts, dtype=torch.int32)
    row0 = (torch.cumsum(c, 0) - c).to(torch.int32)
    cd, r0 = torch.minimum(c, torch.tensor(N, dtype=torch.int32)).to(dev, non_blocking=True), row0.to(dev, non_blocking=True)
    ids = torch.empty((B, N, 34 + rec_len), dtype=torch.int32, device=dev)
    probs = torch.empty((B, N, rec_len), dtype=torch.float32, device=dev)
    for t in (points, poly, rec, rprob):
        if t.stride(-1) != 1:
            raise ValueError('pack_spotting: rows must be contiguous along the last dimension')
    rc = _lib.lib().omp_pack_spotting(ptr(points), ptr(poly), poly.stride(0), ptr(rec), rec.stride(0), ptr(rprob), rprob.stride(0),
                                      ptr(r0), ptr(cd), B, N, rec_len, ptr(ids), ptr(probs), stream())
    _lib.check(rc, 'omp_pack_spotting')
    return ids, probs, cd


def vit_patch_embed(img, w, bias, cls, pos, out_dtype):
    """img [B,3,H,W] fp32 -> tokens [B, T, E] with T = (H/4)*(W/4) + 1 (token 0 = cls), pos_embed added."""
    _c(img, 'img')
    B, _, H, W = img.shape
    E = w.shape[0]
    T = (H // 4) * (W // 4) + 1
    out = torch.empty((B, T, E), dtype=out_dtype, device=img.device)
    rc = _lib.lib().omp_vit_patch_embed(ptr(img), ptr(w), ptr(bias), ptr(cls), ptr(pos), ptr(out), dt(out), B, H, W, E, stream())
    _lib.check(rc, 'omp_vit_patch_embed')
    return out


def vit_attn(q, K, Vt, out, B, T, nH, Mpad):
    """bf16 ViT self-attention on one layer's blocked slabs: q [B*T, nH*64], K [B, nH, Mpad, 64], Vt [B, nH, Mpad/32, 64, 32]
    -> out [B*T, nH*64] (all heads, all images, one launch).
    Slab contract: keys at and beyond T are padding.  Their K rows may hold anything (NaN included): the kernel masks their scores
    before the softmax.  Their V^T slots must be ZERO, as the model's slabs are (allocated zeroed, the projections write keys < T
    only): they are multiplied by a weight of exactly 0, and 0 * NaN would reach the output."""
    rc = _lib.lib().omp_vit_attn(ptr(q), q.stride(0), ptr(K), ptr(Vt), Mpad, ptr(out), out.stride(0), dt(q), B, T, nH, stream())
    _lib.check(rc, 'omp_vit_attn')
    return out


def vit_attn_qkv(qkv, out, B, T, nH):
    """bf16 ViT self-attention on the token-major fused projection qkv [B*T, 3*nH*64] = [q | k | v] -> out [B*T, nH*64]: one workgroup per
    (image, head), keys by strided DMA, the blocked V^T image built in LDS by the kernel (omp_vit_attn_qkv)."""
    rc = _lib.lib().omp_vit_attn_qkv(ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), dt(qkv), B, T, nH, stream())
    _lib.check(rc, 'omp_vit_attn_qkv')
    return out


def a3_pool(sel, feat, B, T, S, want_attn=True):
    """sel fp32 [B*T, >=S], feat [B*T, C] -> (pooled fp32 [B*S, C], maps fp32 [B, S, T] or None)."""
    C = feat.shape[-1]
    pooled = torch.empty((B * S, C), dtype=torch.float32, device=feat.device)
    attn = torch.empty((B, S, T), dtype=torch.float32, device=feat.device) if want_attn else None
    rc = _lib.lib().omp_a3_pool(ptr(sel), sel.stride(0), ptr(feat), dt(feat), ptr(pooled), ptr(attn), B, T, S, C, stream())
    _lib.check(rc, 'omp_a3_pool')
    return pooled, attn


def row_argmax_prob(logits):
    """logits fp32 [R, V] -> (ids int32 [R], prob fp32 [R]): greedy id and its softmax probability."""
    R, V = logits.shape
    ids = torch.empty(R, dtype=torch.int32, device=logits.device)
    prob = torch.empty(R, dtype=torch.float32, device=logits.device)
    rc = _lib.lib().omp_row_argmax_prob(ptr(logits), logits.stride(0), R, V, ptr(ids), ptr(prob), stream())
    _lib.check(rc, 'omp_row_argmax_prob')
    return ids, prob


def row_argmax_prob_2d(logits, B, S):
    """row_argmax_prob of logits [B * S, V] as ([B, S] ids, [B, S] prob)"""
    i, p = row_argmax_prob(logits.reshape(B * S, -1))
    return i.view(B, S), p.view(B, S)


def gemm_row_argmax_prob(A, W, bias=None, a_wrap=0):
    """(ids int32 [M], prob fp32 [M]) of the rows of A W^T + bias WITHOUT materialising the [M, N] logits: the product stores per
    (row, 128-column tile) its maximum, arg-max and sum of exponentials (omp_gemm_bias_act, OMP_STORE_ROWSTAT), omp_row_stat_merge folds
    the tiles.  The same values as row_argmax_prob(gemm(A, W, bias, out_dtype=float32)) (identical product bits; the probability within
    the rounding of a different summation order).  a_wrap: a split-pair A against the [hi | hi | lo] image of an fp32 weight (bf16x3)."""
    M = A.numel() // A.shape[-1]
    N = W.shape[0]
    nt = 2 * ((N + 127) // 128)        # one record per 64-column half of a 128-column tile
    stats = torch.empty((M, nt, 4), dtype=torch.float32, device=A.device)
    gemm(A, W, bias, out=stats, out_dtype=torch.float32, store_mode=_lib.STORE_ROWSTAT, ldc=N, a_wrap=a_wrap)
    ids = torch.empty(M, dtype=torch.int32, device=A.device)
    prob = torch.empty(M, dtype=torch.float32, device=A.device)
    _lib.check(_lib.lib().omp_row_stat_merge(ptr(stats), M, nt, ptr(ids), ptr(prob), stream()), 'omp_row_stat_merge')
    return ids, prob


class Context(object):
    """An omp_ctx: independent kernel selectors, captured decoder graphs and measurement brackets (include/omp355.h).
    `with ctx:` makes it current for the calling thread and restores the previous one; pipeline lane threads inherit the
    context that was current where their LanePool was created."""

    def __init__(self):
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().omp_ctx_create(ctypes.byref(h)), 'omp_ctx_create')
        self.handle = h.value
        self._prev = []
        from .model.transformer import _GraphSlots
        _GraphSlots._dead_ctx.discard(self.handle)   # the allocator may hand a destroyed context's address out again

    def make_current(self):
        _lib.check(_lib.lib().omp_ctx_make_current(ctypes.c_void_p(self.handle)), 'omp_ctx_make_current')

    def __enter__(self):
        self._prev.append(current_context_handle())
        self.make_current()
        return self

    def __exit__(self, *exc):
        _lib.check(_lib.lib().omp_ctx_make_current(ctypes.c_void_p(self._prev.pop())), 'omp_ctx_make_current')
        return False

    def destroy(self):
        if self.handle:
            from .model.transformer import _GraphSlots
            _GraphSlots._dead_ctx.add(self.handle)   # graphs captured in it die with it: never reset them through it again
            _lib.check(_lib.lib().omp_ctx_destroy(ctypes.c_void_p(self.handle)), 'omp_ctx_destroy')
            self.handle = None


def current_context_handle():
    """raw omp_ctx* of the calling thread (the process default context unless one was made current)"""
    return _lib.lib().omp_ctx_current()


def make_context_current(handle):
    _lib.check(_lib.lib().omp_ctx_make_current(ctypes.c_void_p(handle)), 'omp_ctx_make_current')


class capture_gate(object):
    """`with ops.capture_gate():` -- bracket for NON-BLOCKING event calls on a stream another host thread drives through omp_decoder_run
    (omp_capture_gate_enter / _leave, include/omp355.h: no graph capture begins or is in progress inside the bracket)."""

    def __enter__(self):
        _lib.lib().omp_capture_gate_enter()
        return self

    def __exit__(self, *exc):
        _lib.lib().omp_capture_gate_leave()
        return False


def cu_mask_words(n_per_xcd, total_cus=256, n_xcd=8, complement=False):
    """CU mask with `n_per_xcd` compute units on every XCD: bit i is set iff (i mod 32) < n_per_xcd ... balanced under both
    numberings a runtime may use for the mask (XCD-major: xcd = i / 32; interleaved: xcd = i mod 8) when n_per_xcd is a
    multiple of 8.  complement=True returns the other CUs."""
    per = total_cus // n_xcd
    words = [0] * ((total_cus + 31) // 32)
    for i in range(total_cus):
        inside = (i % per) < n_per_xcd
        if inside != complement:
            words[i // 32] |= 1 << (i % 32)
    return words


def masked_stream(words, device=None):
    """torch.cuda.ExternalStream on the CUs of `words` (omp_stream_create_cu_mask); the HIP stream lives as long as
    the process (a handful per lane)."""
    arr = (ctypes.c_uint32 * len(words))(*words)
    out = ctypes.c_void_p()
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        rc = _lib.lib().omp_stream_create_cu_mask(ctypes.cast(arr, ctypes.c_void_p), len(words), ctypes.byref(out))
        _lib.check(rc, 'omp_stream_create_cu_mask')
        return torch.cuda.ExternalStream(out.value, device=device)


def where_probe(n_workgroups):
    """(xcc_id, hw_id) int32 [n_workgroups, 2] of a short probe grid on the current stream."""
    out = torch.zeros((n_workgroups, 2), dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().omp_debug_where(ptr(out), n_workgroups, stream()), 'omp_debug_where')
    return out


def force_gemm_kernel(which):
    """debug/testing: 0 auto, 3 row-streaming, 4 split-K small-M, 5 DMA 128x128 (2 stages), 6 DMA 64x64 ring, 9 gemm_256 (256x256 tiles,
    eight waves), 10 gemm_4w (four waves), 16 gemm_4w_r (four waves, weights streamed into registers), 20 gemm_4w_p (16 made persistent,
    register-only epilogue); the ablation / trace selectors are listed in csrc/omp355_debug.h."""
    _lib.check(_lib.lib().omp_debug_force_gemm_kernel(which), 'omp_debug_force_gemm_kernel')


def cross_q4(on):
    """debug/testing: 1 = LDS-ring cross-attention kernel for 33..64 rows per image (default: 64-key chunks on bf16 / fp32 slabs, three
    one-block stages on split-plane slabs), 2 = the ring consumed one 32-key block per step, 4 = chunks with temporal loads (split
    planes: eight stages in 64-key chunks), 5 / 6 = split planes with four / two stages, 0 = register-streaming kernel."""
    _lib.check(_lib.lib().omp_debug_cross_q4(int(on)), 'omp_debug_cross_q4')


def rows_tile_choice(R, mid=False):
    """host logic (no launch, no device): rows per workgroup a decoder row-owner chain launch of R rows takes (csrc/dec_rows.hip rows_rtt)."""
    rc = _lib.lib().omp_debug_rows_tile_choice(int(R), 1 if mid else 0)
    if rc < 0:
        _lib.check(rc, 'omp_debug_rows_tile_choice')
    return rc


def rows_tile(rtt):
    """debug/testing: rows per workgroup of the decoder row-owner chains (bf16 engine) = 16 x rtt; 0 = chosen from the launch's row count
    (csrc/dec_rows.hip rows_rtt), 2..5 forced."""
    _lib.check(_lib.lib().omp_debug_rows_tile(int(rtt)), 'omp_debug_rows_tile')


def dec_fused(mode):
    """debug/testing: 0 = fused few-row decoder step kernels where they apply (default), 1 = one launch per op everywhere."""
    _lib.check(_lib.lib().omp_debug_dec_fused(int(mode)), 'omp_debug_dec_fused')


def self_attn_impl(which):
    """debug/testing: kernel of dec_self_attn_step: 0 = by row count (default), 1 = one wave per (row, head), 2 = one wave per row."""
    _lib.check(_lib.lib().omp_debug_self_attn_impl(int(which)), 'omp_debug_self_attn_impl')


def fused_self_attn(x, ln_g, ln_b, W, bias_tab, kcache, vcache, out, d_pos, eps=1e-5, embed=None):
    """debug/testing: the fused few-row self-attention step of the point decoder on its own (omp_debug_fused_self_attn, d = 512, 8 heads).
    x [R, 512] fp32 (None with embed), W [1536, 512] bf16, bias_tab [Pmax, 1536] fp32, caches [R, Lmax, 512] bf16, out [R, 512] bf16.
    embed: None, or (seq int32 [R, >= pos + 1], word_emb, pos_tab, emb_g, emb_b, x_out [R, 512] fp32) -- layer 0."""
    R, Lmax = out.shape[0], kcache.shape[1]
    seq, word, pos_tab, emb_g, emb_b, x_out = embed if embed is not None else (None,) * 6
    rc = _lib.lib().omp_debug_fused_self_attn(ptr(x), ptr(ln_g), ptr(ln_b), float(eps), ptr(W), ptr(bias_tab), ptr(kcache), ptr(vcache),
                                              ptr(out), ptr(d_pos), R, Lmax, ptr(seq), seq.stride(0) if seq is not None else 0, ptr(word),
                                              ptr(pos_tab), ptr(emb_g), ptr(emb_b), ptr(x_out), 0 if embed is None else 1, stream())
    _lib.check(rc, 'omp_debug_fused_self_attn')


def sample_impl(which):
    """debug/testing: kernel of head_sample (omp_head_softmax_mask_argmax): 0 = auto (default), 1 = wave per row, 2 = the row in registers
    (refused unless the row stride is a multiple of 4, the rows are 16-byte aligned and vocab <= 2048), 3 = workgroup per row; with 3 and
    advance, d_pos holds (position, ticket = 0) and the kernel's last workgroup advances the position."""
    _lib.check(_lib.lib().omp_debug_sample_impl(int(which)), 'omp_debug_sample_impl')


def swin_attn_impl(which):
    """debug/testing: 0 = matrix-core window attention (default), 1 = scalar cross-check kernel, 2 = matrix cores with table lookups,
    3 = fp32 matrix cores also for split-pair output (the parity engine's call otherwise runs three bf16 products of split operands),
    4 = that split-product kernel also for fp32 output."""
    _lib.check(_lib.lib().omp_debug_swin_attn_impl(which), 'omp_debug_swin_attn_impl')


def swin_mlp_variant(v):
    """debug/testing: alternative (rows per wave, waves per workgroup, ring depth) instantiations of the fused MLP kernel."""
    _lib.check(_lib.lib().omp_debug_swin_mlp_variant(int(v)), 'omp_debug_swin_mlp_variant')


def kv_project_rows(rows, wstream, wave_stride, bias, out, B, M, Mpad, n_slabs, vt):
    """omp_kv_project_rows: the cross-attention memory projection of all (decoder, layer) slabs in one row-owner launch (csrc/kv_rows.hip).
    rows [B * M, 512] bf16; wstream / wave_stride from model/packing.py::pack_kv_rows_k / _v; out: the K (vt False) or V^T (vt True) slab tensor."""
    _c(rows, "rows"); _c(bias, "bias"); _c(out, "out")
    if rows.dtype != torch.bfloat16 or out.dtype != torch.bfloat16 or rows.shape != (B * M, 512) or not rows.is_contiguous():
        raise ValueError('kv_project_rows: [B * M, 512] contiguous bf16 rows and bf16 slabs')
    _lib.check(_lib.lib().omp_kv_project_rows(ptr(rows), ptr(wstream), int(wave_stride), ptr(bias), ptr(out), int(B), int(M), int(Mpad), int(n_slabs),
                                              1 if vt else 0, stream()), 'omp_kv_project_rows')
    return out


def dec_rows_mid(att, x, wstream, wave_stride, out_b, ln_g, ln_b, qbias_tab, d_pos, q=None, eps=1e-5, x3=False, xcd_mask=0, pos_mod=0):
    """x += att Wo^T + bo;  q = bf16(LayerNorm(x) Wq^T + qbias_tab[*d_pos])  -- one launch, a workgroup owns 80 rows (include/omp355.h).
    pos_mod > 0 (bf16 chains): row r takes qbias_tab[r % pos_mod] and d_pos is not read.
    x3: the parity engine's chain -- att as split pairs bf16 [R, 1024], q fp32, split weight stream, 48 rows per workgroup."""
    R = x.shape[0]
    if q is None:
        q = torch.empty((R, 512), dtype=torch.float32 if x3 else torch.bfloat16, device=x.device)
    a = _lib.DecRowsArgs()
    a.x3, a.xcd_mask, a.pos_mod = 1 if x3 else 0, int(xcd_mask), int(pos_mod)
    a.R, a.eps, a.d_pos, a.x, a.att = R, float(eps), ptr(d_pos), ptr(_c(x, 'x')), ptr(_c(att, 'att'))
    a.wstream, a.wave_stride = ptr(wstream), int(wave_stride)
    a.out_b, a.ln_g, a.ln_b, a.qbias_tab, a.q = ptr(out_b), ptr(ln_g), ptr(ln_b), ptr(qbias_tab), ptr(q)
    _lib.check(_lib.lib().omp_dec_rows_mid(ctypes.byref(a), stream()), 'omp_dec_rows_mid')
    return q


def dec_rows_ffn(x, wstream, wave_stride, d_pos, lnt_g, lnt_b, att=None, out_b=None, ln_g=None, ln_b=None, ff1_b=None, ff2_b=None,
                 embed=None, bias_tab=None, qkv=None, head_b=None, logits=None, vocab=0, eps=1e-5, x3=False, xcd_mask=0):
    """The chain behind the cross-attention (or, embed=(seq, word_emb, pos_tab, emb_g, emb_b), the embedding of layer 0) and its tail:
    bias_tab given -> the next layer's q | k | v (bf16 [R, 1536]); head_b=(b0, b1, b2) -> the prediction head's logits (fp32 [R, vocab])."""
    R = x.shape[0]
    a = _lib.DecRowsArgs()
    a.x3, a.xcd_mask = 1 if x3 else 0, int(xcd_mask)
    a.R, a.eps, a.d_pos, a.x = R, float(eps), ptr(d_pos), ptr(_c(x, 'x'))
    a.wstream, a.wave_stride = ptr(wstream), int(wave_stride)
    a.lnt_g, a.lnt_b = ptr(lnt_g), ptr(lnt_b)
    if embed is not None:
        seq, word, pos_tab, eg, eb = embed
        a.prologue, a.seq, a.seq_ld, a.word_emb, a.pos_tab, a.emb_g, a.emb_b = 1, ptr(seq), seq.stride(0), ptr(word), ptr(pos_tab), ptr(eg), ptr(eb)
    else:
        a.prologue, a.att = 0, ptr(_c(att, 'att'))
        a.out_b, a.ln_g, a.ln_b, a.ff1_b, a.ff2_b = ptr(out_b), ptr(ln_g), ptr(ln_b), ptr(ff1_b), ptr(ff2_b)
    if head_b is None:
        if qkv is None:
            qkv = torch.empty((R, 1536), dtype=torch.float32 if x3 else torch.bfloat16, device=x.device)
        a.tail, a.bias_tab, a.qkv = 0, ptr(bias_tab), ptr(qkv)
        out = qkv
    else:
        if logits is None:
            logits = torch.empty((R, vocab), dtype=torch.float32, device=x.device)
        a.tail, a.h0_b, a.h1_b, a.h2_b, a.logits, a.vocab = 1, ptr(head_b[0]), ptr(head_b[1]), ptr(head_b[2]), ptr(logits), int(vocab)
        out = logits
    _lib.check(_lib.lib().omp_dec_rows_ffn(ctypes.byref(a), stream()), 'omp_dec_rows_ffn')
    return out


def swin_rows_qkv(x, n1, qkv_b, wstream, wave_stride, qkv=None, eps=1e-5, x3=False):
    """qkv = bf16(LayerNorm(x; n1) Wqkv^T + bqkv) for x [M, 512] fp32 (Swin-B stage 2, the stage's first block): omp_swin_rows_block mode 0.
    x3: the parity engine's chain (fp32 qkv)."""
    M = x.numel() // 512
    if qkv is None:
        qkv = torch.empty((M, 1536), dtype=torch.float32 if x3 else torch.bfloat16, device=x.device)
    a = _lib.SwinRowsArgs()
    a.x3 = 1 if x3 else 0
    a.M, a.eps, a.mode, a.x, a.qkv = M, float(eps), 0, ptr(_c(x, 'x')), ptr(qkv)
    a.wstream, a.wave_stride = ptr(wstream), int(wave_stride)
    a.n1_g, a.n1_b, a.qkv_b = ptr(n1[0]), ptr(n1[1]), ptr(qkv_b)
    _lib.check(_lib.lib().omp_swin_rows_block(ctypes.byref(a), stream()), 'omp_swin_rows_block')
    return qkv


def swin_rows_block(x, att, wstream, wave_stride, proj_b, n2, fc1_b, fc2_b, next_n1=None, next_qkv_b=None, qkv=None, eps=1e-5, x3=False):
    """x += att Wproj^T + bproj; x += fc2(GELU(fc1(LN(x; n2)))) in place on the fp32 residual stream [M, 512]; with next_n1 / next_qkv_b also
    the next block's qkv = bf16(LN(x; next_n1) Wqkv'^T + b') -> returned (else None).  omp_swin_rows_block mode 1."""
    if x.dtype != torch.float32 or x.shape[-1] != 512:
        raise TypeError('swin_rows_block takes the fp32 residual stream [M, 512]')
    M = x.numel() // 512
    a = _lib.SwinRowsArgs()
    a.x3 = 1 if x3 else 0
    a.M, a.eps, a.mode, a.x, a.att = M, float(eps), 1, ptr(_c(x, 'x')), ptr(_c(att, 'att'))
    a.wstream, a.wave_stride = ptr(wstream), int(wave_stride)
    a.proj_b, a.n2_g, a.n2_b, a.fc1_b, a.fc2_b = ptr(proj_b), ptr(n2[0]), ptr(n2[1]), ptr(fc1_b), ptr(fc2_b)
    if next_n1 is not None:
        if qkv is None:
            qkv = torch.empty((M, 1536), dtype=torch.float32 if x3 else torch.bfloat16, device=x.device)
        a.n1_g, a.n1_b, a.qkv_b, a.qkv = ptr(next_n1[0]), ptr(next_n1[1]), ptr(next_qkv_b), ptr(qkv)
    else:
        qkv = None
    _lib.check(_lib.lib().omp_swin_rows_block(ctypes.byref(a), stream()), 'omp_swin_rows_block')
    return qkv


def lexicon_nearest(q_codes, q_len, q_lo, q_hi, pool, pool_bytes, offsets, L, best=None, range_hint=0):
    """omp_lexicon_nearest (csrc/lexicon.hip; operands as utils/lexicon.py packs them): q_codes uint8 [N, 64], q_len / q_lo /
    q_hi int32 [N] (q_lo and q_hi both None: the whole lexicon), pool uint8 with pool_bytes valid bytes, offsets int32 [L + 1]
    -> best int64 [N] holding the uint64 keys (dist << 32) | idx, all ones = no word."""
    N = q_len.numel()
    for name, t, dtype, numel in (('q_codes', q_codes, torch.uint8, N * 64), ('q_len', q_len, torch.int32, N), ('q_lo', q_lo, torch.int32, N),
                                  ('q_hi', q_hi, torch.int32, N), ('pool', pool, torch.uint8, pool_bytes), ('offsets', offsets, torch.int32, L + 1)):
        if t is None:
            continue
        _c(t, name)
        if t.dtype != dtype or t.numel() < numel:
            raise ValueError('%s must be %s with at least %d elements, got %s x %d' % (name, dtype, numel, t.dtype, t.numel()))
    if best is None:
        best = torch.empty(N, dtype=torch.int64, device=q_len.device)
    elif best.dtype != torch.int64 or best.numel() < N or not best.is_contiguous():
        raise ValueError('best must be a contiguous int64 tensor with at least %d elements' % N)
    rc = _lib.lib().omp_lexicon_nearest(ptr(q_codes), ptr(q_len), ptr(q_lo), ptr(q_hi), N, ptr(pool), pool_bytes, ptr(offsets), L,
                                        int(range_hint), ptr(best), stream())
    _lib.check(rc, 'omp_lexicon_nearest')
    return best


def logprob_costs(logits, costs=None, greedy=None, n=None):
    """omp_logprob_costs (csrc/lexicon_post.hip; utils/lexicon_post.py: costs_cpu / greedy_cpu are the specification): the character
    head's logits fp32 [N, 27, 38] -> (costs int32 [N, 26, 38], greedy int32 [N, 2])."""
    if logits is not None:
        _c(logits, 'logits')
        if logits.dtype != torch.float32 or logits.dim() != 3 or tuple(logits.shape[1:]) != (27, 38):
            raise ValueError('logits must be fp32 [N, 27, 38], got %s %s' % (logits.dtype, tuple(logits.shape)))
    N = int(logits.shape[0]) if n is None else int(n)
    if costs is None:
        costs = torch.empty((max(N, 0), 26, 38), dtype=torch.int32, device=logits.device)
    if greedy is None:
        greedy = torch.empty((max(N, 0), 2), dtype=torch.int32, device=logits.device)
    for name, t, numel in (('costs', costs, N * 26 * 38), ('greedy', greedy, N * 2)):
        if t.dtype != torch.int32 or t.numel() < numel or not t.is_contiguous():
            raise ValueError('%s must be a contiguous int32 tensor with at least %d elements' % (name, numel))
    rc = _lib.lib().omp_logprob_costs(ptr(logits), N, ptr(costs), ptr(greedy), stream())
    _lib.check(rc, 'omp_logprob_costs')
    return costs, greedy


LEXICON_POST_WORK_SLICES = 4096   # omp_lexicon_posterior: work holds 2 * (n + 4096) uint64 (include/omp355.h)


def lexicon_posterior(costs, q_lo, q_hi, pool, pool_bytes, offsets, L, class_table, range_hint=0, best=None, work=None, n=None):
    """omp_lexicon_posterior (csrc/lexicon_post.hip; utils/lexicon_post.py: score_cpu is the specification): costs int32 [N, 26, 38],
    q_lo / q_hi int32 [N] (both None: the whole lexicon), pool uint8 with pool_bytes valid bytes, offsets int32 [L + 1], class_table
    uint8 [256] -> best int64 [N, 2] holding the uint64 keys (score << 32) | idx of the best word and of the runner-up, all ones =
    none.  work: int64 scratch of at least 2 * (N + 4096) elements (allocated here when None)."""
    N = int(costs.shape[0]) if n is None else int(n)
    for name, t, dtype, numel in (('costs', costs, torch.int32, N * 26 * 38), ('q_lo', q_lo, torch.int32, N), ('q_hi', q_hi, torch.int32, N),
                                  ('pool', pool, torch.uint8, pool_bytes), ('offsets', offsets, torch.int32, L + 1),
                                  ('class_table', class_table, torch.uint8, 256)):
        if t is None:
            continue
        _c(t, name)
        if t.dtype != dtype or t.numel() < numel:
            raise ValueError('%s must be %s with at least %d elements, got %s x %d' % (name, dtype, numel, t.dtype, t.numel()))
    if best is None:
        best = torch.empty((max(N, 0), 2), dtype=torch.int64, device=costs.device)
    elif best.dtype != torch.int64 or best.numel() < 2 * N or not best.is_contiguous():
        raise ValueError('best must be a contiguous int64 tensor with at least %d elements' % (2 * N))
    if work is None:
        work = torch.empty(2 * (max(N, 0) + LEXICON_POST_WORK_SLICES), dtype=torch.int64, device=best.device)
    elif work.dtype != torch.int64 or work.numel() < 2 * (N + LEXICON_POST_WORK_SLICES) or not work.is_contiguous():
        raise ValueError('work must be a contiguous int64 tensor with at least %d elements' % (2 * (N + LEXICON_POST_WORK_SLICES)))
    rc = _lib.lib().omp_lexicon_posterior(ptr(costs), N, ptr(q_lo), ptr(q_hi), ptr(pool), pool_bytes, ptr(offsets), L, ptr(class_table),
                                          int(range_hint), ptr(best), ptr(work), stream())
    _lib.check(rc, 'omp_lexicon_posterior')
    return best


def window_points(seq, finished, lengths, row_image, n_images, n_prompt, sampled, clip=False, cap=None):
    """omp_window_points (csrc/window_points.hip; utils/windows.py: gather_points_cpu is the specification): the buffers of a finished
    point phase -- seq int32 [rows, seq_ld], finished / lengths int32 [rows] -- and the row -> image table
    -> (points int32 [cap, 2], inst_row int32 [cap], counts): counts is ONE int32 tensor [3 * rows + 1 + n_images] =
    row_count | dropped | row_start (rows + 1 entries, the last one the total) | image_count, so that a caller fetches everything that
    sizes the next phases in one copy (split_window_counts).  cap defaults to rows * (pairs a row can hold)."""
    if seq.dim() != 2 or not (0 <= int(n_prompt) <= seq.shape[1]):
        raise ValueError('seq must be [rows, seq_ld] with n_prompt inside a row')
    rows, seq_ld = int(seq.shape[0]), int(seq.shape[1])
    for name, t in (('seq', seq), ('finished', finished), ('lengths', lengths), ('row_image', row_image)):
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.shape[0] != rows:
            raise ValueError('%s must be a contiguous device int32 tensor with %d rows' % (name, rows))
    if cap is None:
        cap = rows * ((int(seq.shape[1]) - int(n_prompt)) // 2)
    dev = seq.device
    points = torch.empty(max(cap, 1), 2, dtype=torch.int32, device=dev)
    inst_row = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    counts = torch.empty(3 * rows + 1 + int(n_images), dtype=torch.int32, device=dev)
    row_count, dropped, row_start, image_count = counts[:rows], counts[rows:2 * rows], counts[2 * rows:3 * rows + 1], counts[3 * rows + 1:]
    rc = _lib.lib().omp_window_points(ptr(seq), seq_ld, ptr(finished), ptr(lengths), ptr(row_image), rows, int(n_images), int(n_prompt),
                                      int(sampled), 1 if clip else 0, ptr(points), ptr(inst_row), int(cap),
                                      ptr(row_count), ptr(dropped), ptr(row_start), ptr(image_count), stream())
    _lib.check(rc, 'omp_window_points')
    return points[:cap], inst_row[:cap], counts


def split_window_counts(counts, rows):
    """the counts tensor of window_points (on either side of the copy) -> (row_count, dropped, row_start, image_count)"""
    return counts[:rows], counts[rows:2 * rows], counts[2 * rows:3 * rows + 1], counts[3 * rows + 1:]


def polygon_overlap(polys, group_start, order, mask_start, mask_words, grid, t, measure, inter_start=None, inter_total=0, out=None):
    """omp_polygon_overlap (csrc/overlap.hip; utils/overlap.py holds the specification and packs the tables): polys int32 [N, 32],
    group_start int32 [G + 1], order int32 [N], mask_start int64 [G + 1] (utils.overlap.mask_layout; mask_words = its last entry),
    measure 0 = IoU / 1 = intersection over the smaller area, t in permille; inter_start int64 [G + 1] with inter_total asks for the
    dense intersection matrices too.
    -> dict(ints: ONE int32 tensor [6 N + G] = bbox [N, 4] | area [N] | owner [N] | kept [G] (the last two are polygon_keep's, so that a
    caller fetches everything in one copy: split_overlap_ints), bbox, area: views of it, mask: int64 [mask_words] holding the uint64
    words, inter: int32 [inter_total] or None)."""
    N, G = int(polys.shape[0]), int(group_start.numel()) - 1
    for name, tt, dtype, numel in (('polys', polys, torch.int32, 32 * N), ('group_start', group_start, torch.int32, G + 1), ('order', order, torch.int32, N),
                                   ('mask_start', mask_start, torch.int64, G + 1), ('inter_start', inter_start, torch.int64, G + 1)):
        if tt is None:
            continue
        if not tt.is_cuda or tt.dtype != dtype or not tt.is_contiguous() or tt.numel() != numel:
            raise ValueError('%s must be a contiguous device %s tensor with %d elements' % (name, dtype, numel))
    if polys.dim() != 2 or polys.shape[1] != 32 or N < 1 or G < 1 or int(mask_words) < 1:
        raise ValueError('polys must be [N, 32] with at least one polygon and one group')
    dev = polys.device
    if out is None:
        out = torch.empty(6 * N + G, dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or out.numel() != 6 * N + G or not out.is_contiguous():
        raise ValueError('out must be a contiguous int32 tensor with %d elements' % (6 * N + G))
    bbox, area = out[:4 * N], out[4 * N:5 * N]
    mask = torch.empty(int(mask_words), dtype=torch.int64, device=dev)
    inter = torch.empty(int(inter_total), dtype=torch.int32, device=dev) if inter_start is not None else None
    rc = _lib.lib().omp_polygon_overlap(ptr(polys), N, ptr(group_start), G, ptr(order), ptr(mask_start), int(mask_words), int(grid), int(t),
                                        int(measure), ptr(area), ptr(bbox), ptr(mask), ptr(inter), ptr(inter_start),
                                        int(inter_total) if inter is not None else 0, stream())
    _lib.check(rc, 'omp_polygon_overlap')
    return dict(ints=out, bbox=bbox.view(N, 4), area=area, mask=mask, inter=inter)


def polygon_keep(mask, mask_start, group_start, order, n, out=None):
    """omp_polygon_keep: the greedy pass over polygon_overlap's mask, in the priority order the mask was built for.
    -> the int32 tensor [6 n + G] of polygon_overlap (`out`, or a new one whose first 5 n entries are not written) with owner at
    [5 n, 6 n) and kept at [6 n, 6 n + G): split_overlap_ints."""
    G = int(group_start.numel()) - 1
    for name, tt, dtype, numel in (('mask', mask, torch.int64, int(mask.numel())), ('mask_start', mask_start, torch.int64, G + 1),
                                   ('group_start', group_start, torch.int32, G + 1), ('order', order, torch.int32, int(n))):
        if not tt.is_cuda or tt.dtype != dtype or not tt.is_contiguous() or tt.numel() != numel:
            raise ValueError('%s must be a contiguous device %s tensor with %d elements' % (name, dtype, numel))
    n = int(n)
    if out is None:
        out = torch.empty(6 * n + G, dtype=torch.int32, device=mask.device)
    elif out.dtype != torch.int32 or out.numel() != 6 * n + G or not out.is_contiguous():
        raise ValueError('out must be a contiguous int32 tensor with %d elements' % (6 * n + G))
    rc = _lib.lib().omp_polygon_keep(ptr(mask), ptr(mask_start), int(mask.numel()), ptr(group_start), G, n, ptr(order), ptr(out[5 * n:6 * n]),
                                     ptr(out[6 * n:]), stream())
    _lib.check(rc, 'omp_polygon_keep')
    return out


def split_overlap_ints(ints, n):
    """the int32 tensor of polygon_overlap / polygon_keep (on either side of the copy) -> (bbox [n, 4], area, owner, kept)"""
    return ints[:4 * n].reshape(n, 4), ints[4 * n:5 * n], ints[5 * n:6 * n], ints[6 * n:]


def spotting_match(inter, inter_start, group_start, n_gt, gt_dc, text, level, n_thr, t_iou, t_dc, report=-1, out=None):
    """omp_spotting_match (csrc/score.hip; utils/scoring.py holds the specification): inter int32, polygon_overlap's dense matrices (None
    when there is no polygon), inter_start int64 [G + 1], group_start int32 [G + 1], n_gt int32 [G], gt_dc / text / level int32 [n] with
    n = the number of polygons, ground truth first inside every group; t_iou, t_dc in permille; report -1 or a threshold index.
    -> ONE int32 tensor [4 G n_thr + 2 n] = counts [G, n_thr, 4] | det_gt [n] | gt_det [n] (split_match_ints), so that a caller fetches
    everything in one copy."""
    G, n = int(group_start.numel()) - 1, int(level.numel())
    if G < 1:
        raise ValueError('group_start must hold at least one group')
    for name, tt, dtype, numel in (('inter', inter, torch.int32, None), ('inter_start', inter_start, torch.int64, G + 1),
                                   ('group_start', group_start, torch.int32, G + 1), ('n_gt', n_gt, torch.int32, G), ('gt_dc', gt_dc, torch.int32, n),
                                   ('text', text, torch.int32, n), ('level', level, torch.int32, n)):
        if tt is None:
            if name == 'inter' and n == 0:
                continue
            raise ValueError('%s is missing' % name)
        if not tt.is_cuda or tt.dtype != dtype or not tt.is_contiguous() or (numel is not None and tt.numel() != numel):
            raise ValueError('%s must be a contiguous device %s tensor%s' % (name, dtype, '' if numel is None else ' with %d elements' % numel))
    n_thr = int(n_thr)
    size = 4 * G * max(n_thr, 0) + 2 * n
    dev = group_start.device
    if out is None:
        out = torch.empty(max(size, 1), dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or out.numel() != max(size, 1) or not out.is_contiguous():
        raise ValueError('out must be a contiguous int32 tensor with %d elements' % max(size, 1))
    c = 4 * G * max(n_thr, 0)
    rc = _lib.lib().omp_spotting_match(ptr(inter), ptr(inter_start), ptr(group_start), ptr(n_gt), ptr(gt_dc) if n else None, ptr(text) if n else None,
                                       ptr(level) if n else None, n, G, n_thr, int(t_iou), int(t_dc), int(report), ptr(out),
                                       ptr(out[c:c + n]) if n else None, ptr(out[c + n:c + 2 * n]) if n else None, stream())
    _lib.check(rc, 'omp_spotting_match')
    return out[:size]


def split_match_ints(ints, n, n_groups, n_thr):
    """the int32 tensor of spotting_match (on either side of the copy) -> (counts [G, n_thr, 4], det_gt [n], gt_det [n])"""
    c = 4 * n_groups * n_thr
    return ints[:c].reshape(n_groups, n_thr, 4), ints[c:c + n], ints[c + n:c + 2 * n]


PAGE_TEXT_SLICE_BYTES = 32768   # omp_page_edit_distance: scratch per pair (csrc/myers.h: PT_SLICE_BYTES)


def page_scratch_bytes(n_pairs):
    """the scratch omp_page_edit_distance needs for n_pairs pairs: two carry buffers per pair, whatever the pairs' lengths (the lengths live
    in device memory; the entry point checks this size before it launches)"""
    return max(int(n_pairs), 0) * PAGE_TEXT_SLICE_BYTES


def page_edit_distance(pool, pool_bytes, a_off, a_len, b_off, b_len, sigma, scratch, dist=None):
    """omp_page_edit_distance (csrc/page_text.hip; utils/page_text.py holds the specification): pool uint8 with pool_bytes valid codes
    (0 .. sigma - 1, or 255 = equals nothing), a_off / a_len / b_off / b_len int32 [P], scratch uint8 with at least page_scratch_bytes(P)
    bytes -> dist int32 [P]: the Levenshtein distance of every pair, -1 for a pair whose lengths or ranges are out of bounds."""
    P = int(a_len.numel())
    for name, t, dtype, numel in (('pool', pool, torch.uint8, pool_bytes), ('a_off', a_off, torch.int32, P), ('a_len', a_len, torch.int32, P),
                                  ('b_off', b_off, torch.int32, P), ('b_len', b_len, torch.int32, P), ('scratch', scratch, torch.uint8, 0)):
        if t is None:
            raise ValueError('%s is missing' % name)
        _c(t, name)
        if not t.is_cuda or t.dtype != dtype or t.numel() < numel:
            raise ValueError('%s must be a device %s tensor with at least %d elements, got %s x %d' % (name, dtype, numel, t.dtype, t.numel()))
    if dist is None:
        dist = torch.empty(max(P, 1), dtype=torch.int32, device=a_len.device)
    elif dist.dtype != torch.int32 or dist.numel() < P or not dist.is_contiguous():
        raise ValueError('dist must be a contiguous int32 tensor with at least %d elements' % P)
    rc = _lib.lib().omp_page_edit_distance(ptr(pool), int(pool_bytes), ptr(a_off), ptr(a_len), ptr(b_off), ptr(b_len), P, int(sigma), ptr(scratch),
                                           int(scratch.numel()), ptr(dist), stream())
    _lib.check(rc, 'omp_page_edit_distance')
    return dist[:P]


PAGE_ALIGN_CARRY_BYTES = 32768  # omp_page_align: the head of a pair's scratch (csrc/page_align.hip: PA_CARRY_BYTES == csrc/myers.h: PT_SLICE_BYTES)
PAGE_ALIGN_CELL_BYTES = 16      # omp_page_align: the record of one (64-row block, text column) (csrc/page_align.hip: PA_CELL_BYTES)


def page_align_scratch_bytes(la, lb):
    """the scratch omp_page_align needs for ONE pair of la x lb characters: the carries between stripes and two 64-bit words per
    (64-row block of a, column of b).  The device checks scratch_off[p] + this against scratch_bytes for every pair."""
    la, lb = max(int(la), 0), max(int(lb), 0)
    return PAGE_ALIGN_CARRY_BYTES + PAGE_ALIGN_CELL_BYTES * ((la + 63) // 64) * lb


def page_align(pool, pool_bytes, a_off, a_len, b_off, b_len, map_off, scratch_off, sigma, scratch, maps, maps_len=None, counts=None):
    """omp_page_align (csrc/page_align.hip; utils/page_align.py holds the specification): pool uint8 with pool_bytes valid codes
    (0 .. sigma - 1, or 255 = equals nothing), a_off / a_len / b_off / b_len int32 [P], map_off / scratch_off int64 [P] (pair p owns
    maps[map_off[p] : map_off[p] + la + lb] and page_align_scratch_bytes(la, lb) bytes of scratch from scratch_off[p], a multiple of 8),
    scratch uint8, maps int32 with maps_len entries (default: all of it) -> counts int32 [P, 4] = (match, sub, ins, del); maps holds
    a_map then b_map of every pair.  A pair whose lengths, ranges or slices are out of bounds gets counts of -1 and writes nothing."""
    P = int(a_len.numel())
    maps_len = int(maps.numel()) if maps_len is None else int(maps_len)
    for name, t, dtype, numel in (('pool', pool, torch.uint8, pool_bytes), ('a_off', a_off, torch.int32, P), ('a_len', a_len, torch.int32, P),
                                  ('b_off', b_off, torch.int32, P), ('b_len', b_len, torch.int32, P), ('map_off', map_off, torch.int64, P),
                                  ('scratch_off', scratch_off, torch.int64, P), ('scratch', scratch, torch.uint8, 0), ('maps', maps, torch.int32, maps_len)):
        if t is None:
            raise ValueError('%s is missing' % name)
        _c(t, name)
        if not t.is_cuda or t.dtype != dtype or t.numel() < numel:
            raise ValueError('%s must be a device %s tensor with at least %d elements, got %s x %d' % (name, dtype, numel, t.dtype, t.numel()))
    if counts is None:
        counts = torch.empty(4 * max(P, 1), dtype=torch.int32, device=a_len.device)
    elif not counts.is_cuda or counts.dtype != torch.int32 or counts.numel() < 4 * P or not counts.is_contiguous():
        raise ValueError('counts must be a contiguous device int32 tensor with at least %d elements' % (4 * P))
    rc = _lib.lib().omp_page_align(ptr(pool), int(pool_bytes), ptr(a_off), ptr(a_len), ptr(b_off), ptr(b_len), ptr(map_off), ptr(scratch_off), P, int(sigma),
                                   ptr(scratch), int(scratch.numel()), ptr(maps), maps_len, ptr(counts), stream())
    _lib.check(rc, 'omp_page_align')
    return counts.reshape(-1)[:4 * P].view(P, 4)


def _page_io(rows, things, jobs, J, H, device, best, n_hits, hits):
    """what the four page searches share: every (name, tensor, dtype, numel) row is a contiguous device tensor of its type with at least
    numel elements, jobs holds J (page, `things`) pairs, and best / n_hits / hits are made on `device`, or checked when the caller brings
    them -> [best, n_hits, hits], flat"""
    for name, t, dtype, numel in rows:
        if t is None:
            raise ValueError('%s is missing' % name)
        _c(t, name)
        if not t.is_cuda or t.dtype != dtype or t.numel() < numel:
            raise ValueError('%s must be a device %s tensor with at least %d elements, got %s x %d' % (name, dtype, numel, t.dtype, t.numel()))
    if jobs.numel() != 2 * J:
        raise ValueError('jobs must hold (page, %s) pairs, got %d integers' % (things, jobs.numel()))
    outs = []
    for name, t, numel in (('best', best, 2 * J), ('n_hits', n_hits, J), ('hits', hits, 3 * max(H, 0) * J)):
        if t is None:
            t = torch.empty(max(numel, 1), dtype=torch.int32, device=device)
        elif not t.is_cuda or t.dtype != torch.int32 or t.numel() < numel or not t.is_contiguous():
            raise ValueError('%s must be a contiguous device int32 tensor with at least %d elements' % (name, numel))
        outs.append(t)
    return outs


def _page_views(outs, J, H):
    """-> best [J, 2], n_hits [J], hits [J, H, 3]"""
    return outs[0][:2 * J].view(J, 2), outs[1][:J], outs[2][:3 * H * J].view(J, H, 3)


PAGE_SEARCH_CHUNK = 128        # omp_page_search: text columns per lane (csrc/page_frame.h: PG_CHUNK)
PAGE_SEARCH_HIT_BYTES = 512     # omp_page_search: scratch per job and kept hit: 64 lanes x (end, dist)


def page_search_scratch_bytes(n_jobs, max_hits):
    """the scratch omp_page_search needs for n_jobs jobs at max_hits: per job and lane a list of max_hits (end, dist) pairs, whatever
    the pages' lengths (the lengths live in device memory; the entry point checks this size before it launches)"""
    return max(int(n_jobs), 0) * max(int(max_hits), 0) * PAGE_SEARCH_HIT_BYTES


def page_search(pool, pool_bytes, page_off, page_len, query_off, query_len, k, jobs, sigma, max_hits, scratch, best=None, n_hits=None, hits=None):
    """omp_page_search (csrc/page_search.hip; utils/page_search.py holds the specification): pool uint8 with pool_bytes valid codes
    (0 .. sigma - 1, or 255 = equals nothing), page_off / page_len int32 [P], query_off / query_len / k int32 [Q], jobs int32 [J, 2] =
    (page, query), scratch uint8 with at least page_search_scratch_bytes(J, max_hits) bytes -> (best int32 [J, 2] = (dist, end),
    n_hits int32 [J], hits int32 [J, max_hits, 3] = (end, dist, start), -1 where there is no hit); n_hits = -1 for a job whose lengths,
    ranges or tolerance are out of bounds."""
    P, Q, J, H = int(page_len.numel()), int(query_len.numel()), int(jobs.numel()) // 2, int(max_hits)
    outs = _page_io((('pool', pool, torch.uint8, pool_bytes), ('page_off', page_off, torch.int32, P), ('page_len', page_len, torch.int32, P),
                     ('query_off', query_off, torch.int32, Q), ('query_len', query_len, torch.int32, Q), ('k', k, torch.int32, Q),
                     ('jobs', jobs, torch.int32, 2 * J), ('scratch', scratch, torch.uint8, 0)), 'query', jobs, J, H, page_len.device, best, n_hits, hits)
    rc = _lib.lib().omp_page_search(ptr(pool), int(pool_bytes), ptr(page_off), ptr(page_len), P, ptr(query_off), ptr(query_len), ptr(k), Q, ptr(jobs), J,
                                    int(sigma), H, ptr(scratch), int(scratch.numel()), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), stream())
    _lib.check(rc, 'omp_page_search')
    return _page_views(outs, J, H)


PAGE_PATTERN_CHUNK = 128       # omp_page_pattern_search: text columns per lane (csrc/page_frame.h: PG_CHUNK)
PAGE_PATTERN_HIT_BYTES = 512    # omp_page_pattern_search: scratch per job and kept hit: 64 lanes x (end, dist)


def page_pattern_scratch_bytes(n_jobs, max_hits):
    """the scratch omp_page_pattern_search needs for n_jobs jobs at max_hits: per job and lane a list of max_hits (end, dist) pairs,
    whatever the pages' lengths (the entry point checks this size before it launches)"""
    return max(int(n_jobs), 0) * max(int(max_hits), 0) * PAGE_PATTERN_HIT_BYTES


def page_pattern_search(pool, pool_bytes, page_off, page_len, masks, opt, pat_len, k, jobs, sigma, max_hits, scratch, best=None, n_hits=None, hits=None):
    """omp_page_pattern_search (csrc/page_pattern.hip; utils/page_pattern.py holds the specification): pool uint8 with pool_bytes valid
    codes, page_off / page_len int32 [P], masks int64 [Q, sigma + 1] (the 64-bit class words: bit i of masks[q, c] says that code c is in
    the class of position i; row sigma is read as 0), opt int64 [Q] (bit i: position i is optional), pat_len / k int32 [Q], jobs int32
    [J, 2] = (page, pattern), scratch uint8 with at least page_pattern_scratch_bytes(J, max_hits) bytes -> (best int32 [J, 2] = (dist,
    end), n_hits int32 [J], hits int32 [J, max_hits, 3] = (end, dist, start), -1 where there is no hit); n_hits = -1 for a job whose
    lengths, ranges, opt word or tolerance are out of bounds."""
    P, Q, J, H, S = int(page_len.numel()), int(pat_len.numel()), int(jobs.numel()) // 2, int(max_hits), int(sigma)
    outs = _page_io((('pool', pool, torch.uint8, pool_bytes), ('page_off', page_off, torch.int32, P), ('page_len', page_len, torch.int32, P),
                     ('masks', masks, torch.int64, Q * (max(S, 0) + 1)), ('opt', opt, torch.int64, Q), ('pat_len', pat_len, torch.int32, Q),
                     ('k', k, torch.int32, Q), ('jobs', jobs, torch.int32, 2 * J), ('scratch', scratch, torch.uint8, 0)), 'pattern', jobs, J, H,
                    page_len.device, best, n_hits, hits)
    rc = _lib.lib().omp_page_pattern_search(ptr(pool), int(pool_bytes), ptr(page_off), ptr(page_len), P, ptr(masks), ptr(opt), ptr(pat_len), ptr(k), Q,
                                            ptr(jobs), J, S, H, ptr(scratch), int(scratch.numel()), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), stream())
    _lib.check(rc, 'omp_page_pattern_search')
    return _page_views(outs, J, H)


PAGE_REGEX_CHUNK = 128         # omp_page_regex_search: text columns per lane (csrc/page_frame.h: PG_CHUNK)


def _regex_rows(pool, pool_bytes, page_off, page_len, masks, first, last, follow, pred, pat_len, P, Q, S):
    """the rows both expression searches check"""
    return (('pool', pool, torch.uint8, pool_bytes), ('page_off', page_off, torch.int32, P), ('page_len', page_len, torch.int32, P),
            ('masks', masks, torch.int64, Q * (max(S, 0) + 1)), ('first', first, torch.int64, Q), ('last', last, torch.int64, Q),
            ('follow', follow, torch.int64, 64 * Q), ('pred', pred, torch.int64, 64 * Q), ('pat_len', pat_len, torch.int32, Q))


def page_regex_search(pool, pool_bytes, page_off, page_len, masks, first, last, follow, pred, pat_len, jobs, sigma, max_hits, best=None, n_hits=None,
                      hits=None):
    """omp_page_regex_search (csrc/page_regex.hip; utils/page_regex.py holds the specification): pool uint8 with pool_bytes valid codes,
    page_off / page_len int32 [P], masks int64 [Q, sigma + 1] (the 64-bit class words: bit i of masks[q, c] says that code c is in the
    class of position i; row sigma is read as 0), first / last int64 [Q] (the positions a match can begin / end with), follow / pred int64
    [Q, 64] (the positions that can come after / before position i; rows at or above pat_len zero), pat_len int32 [Q], jobs int32 [J, 2] =
    (page, expression); the kernel needs no scratch -> (best int32 [J, 2] = (0, the least end) or (1, 0), n_hits int32 [J], hits int32
    [J, max_hits, 3] = (end, 0, start), -1 where there is no hit); n_hits = -1 for a job whose lengths, ranges or automaton words are
    out of bounds."""
    P, Q, J, H, S = int(page_len.numel()), int(pat_len.numel()), int(jobs.numel()) // 2, int(max_hits), int(sigma)
    rows = _regex_rows(pool, pool_bytes, page_off, page_len, masks, first, last, follow, pred, pat_len, P, Q, S)
    outs = _page_io(rows + (('jobs', jobs, torch.int32, 2 * J),), 'expression', jobs, J, H, page_len.device, best, n_hits, hits)
    rc = _lib.lib().omp_page_regex_search(ptr(pool), int(pool_bytes), ptr(page_off), ptr(page_len), P, ptr(masks), ptr(first), ptr(last), ptr(follow),
                                          ptr(pred), ptr(pat_len), Q, ptr(jobs), J, S, H, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), stream())
    _lib.check(rc, 'omp_page_regex_search')
    return _page_views(outs, J, H)


def page_regex_fuzzy_search(pool, pool_bytes, page_off, page_len, masks, first, last, follow, pred, pat_len, k, jobs, sigma, max_hits, best=None,
                            n_hits=None, hits=None):
    """omp_page_regex_fuzzy_search (csrc/page_regex.hip; utils/page_regex.py holds the specification): the inputs of page_regex_search
    and k int32 [Q], one tolerance 0 .. 4 per expression; the kernel needs no scratch -> (best int32 [J, 2] = (the least distance, the least
    end that attains it) or (k + 1, 0), n_hits int32 [J], hits int32 [J, max_hits, 3] = (end, dist, start), -1 where there is no hit);
    n_hits = -1 for a job whose lengths, ranges, automaton words or tolerance are out of bounds."""
    P, Q, J, H, S = int(page_len.numel()), int(pat_len.numel()), int(jobs.numel()) // 2, int(max_hits), int(sigma)
    rows = _regex_rows(pool, pool_bytes, page_off, page_len, masks, first, last, follow, pred, pat_len, P, Q, S)
    outs = _page_io(rows + (('k', k, torch.int32, Q), ('jobs', jobs, torch.int32, 2 * J)), 'expression', jobs, J, H, page_len.device, best, n_hits, hits)
    rc = _lib.lib().omp_page_regex_fuzzy_search(ptr(pool), int(pool_bytes), ptr(page_off), ptr(page_len), P, ptr(masks), ptr(first), ptr(last), ptr(follow),
                                                ptr(pred), ptr(pat_len), ptr(k), Q, ptr(jobs), J, S, H, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), stream())
    _lib.check(rc, 'omp_page_regex_fuzzy_search')
    return _page_views(outs, J, H)


def _reading_tables(polys, tables, host_tables, n_groups):
    N, G = int(polys.shape[0]), int(n_groups)
    for name, tt, numel in (('polys', polys, 32 * N), ('tables', tables, 3 * G + 1)):
        if not tt.is_cuda or tt.dtype != torch.int32 or not tt.is_contiguous() or tt.numel() != numel:
            raise ValueError('%s must be a contiguous device int32 tensor with %d elements' % (name, numel))
    if polys.dim() != 2 or polys.shape[1] != 32:
        raise ValueError('polys must be [N, 32]')
    host = np.ascontiguousarray(host_tables, dtype=np.int32).reshape(-1)
    if host.size != 3 * G + 1:
        raise ValueError('host_tables must hold %d int32 (group_start [G + 1], aspect [G, 2]), got %d' % (3 * G + 1, host.size))
    return N, G, host


def reading_links(polys, tables, host_tables, n_groups, grid, gap, back, offset):
    """omp_reading_links (csrc/reading.hip; utils/reading.py holds the specification): polys int32 [N, 32]; tables device int32
    [3 G + 1] = group_start [G + 1] | aspect [G, 2]; host_tables the same numbers on the host, which the entry point checks before
    it launches; gap, back, offset in permille.  -> (succ0 int32 [N], cost0 int64 [N]): every word's best follower before resolution."""
    N, G, host = _reading_tables(polys, tables, host_tables, n_groups)
    succ0 = torch.empty(N, dtype=torch.int32, device=polys.device)
    cost0 = torch.empty(N, dtype=torch.int64, device=polys.device)
    rc = _lib.lib().omp_reading_links(ptr(polys), N, ptr(tables), host.ctypes.data, G, int(grid), int(gap), int(back), int(offset), ptr(succ0),
                                      ptr(cost0), stream())
    _lib.check(rc, 'omp_reading_links')
    return succ0, cost0


def reading_lines(polys, tables, host_tables, n_groups, grid, succ0, cost0, out=None):
    """omp_reading_lines: reading_links' candidates -> lines.  -> ONE int32 tensor [5 N + G] = succ | pred | line | line_pos | rank |
    n_lines (split_reading_ints), so that a caller fetches everything in one copy."""
    N, G, host = _reading_tables(polys, tables, host_tables, n_groups)
    for name, tt, dtype in (('succ0', succ0, torch.int32), ('cost0', cost0, torch.int64)):
        if not tt.is_cuda or tt.dtype != dtype or not tt.is_contiguous() or tt.numel() != N:
            raise ValueError('%s must be a contiguous device %s tensor with %d elements' % (name, dtype, N))
    if out is None:
        out = torch.empty(5 * N + G, dtype=torch.int32, device=polys.device)
    elif out.dtype != torch.int32 or out.numel() != 5 * N + G or not out.is_contiguous():
        raise ValueError('out must be a contiguous int32 tensor with %d elements' % (5 * N + G))
    rc = _lib.lib().omp_reading_lines(ptr(polys), N, ptr(tables), host.ctypes.data, G, int(grid), ptr(succ0), ptr(cost0), ptr(out[:N]), ptr(out[N:2 * N]),
                                      ptr(out[2 * N:3 * N]), ptr(out[3 * N:4 * N]), ptr(out[4 * N:5 * N]), ptr(out[5 * N:]), stream())
    _lib.check(rc, 'omp_reading_lines')
    return out


def split_reading_ints(ints, n):
    """the int32 tensor of reading_lines (on either side of the copy) -> (succ, pred, line, line_pos, rank, n_lines)"""
    return tuple(ints[k * n:(k + 1) * n] for k in range(5)) + (ints[5 * n:],)


def reading_blocks(polys, tables, host_tables, n_groups, grid, lines, gap_x, gap_y, depth, out=None):
    """omp_reading_blocks (utils/reading.py: blocks_cpu is the specification): the XY-cut over the lines.  lines: reading_lines' int32
    tensor [5 N + G], on the device.  -> ONE int32 tensor [3 N + 2 G] = block | line | rank | n_blocks | levels (split_block_ints)."""
    N, G, host = _reading_tables(polys, tables, host_tables, n_groups)
    if not lines.is_cuda or lines.dtype != torch.int32 or not lines.is_contiguous() or lines.numel() != 5 * N + G:
        raise ValueError('lines must be the contiguous device int32 tensor of reading_lines with %d elements' % (5 * N + G))
    if out is None:
        out = torch.empty(3 * N + 2 * G, dtype=torch.int32, device=polys.device)
    elif out.dtype != torch.int32 or out.numel() != 3 * N + 2 * G or not out.is_contiguous():
        raise ValueError('out must be a contiguous int32 tensor with %d elements' % (3 * N + 2 * G))
    rc = _lib.lib().omp_reading_blocks(ptr(polys), N, ptr(tables), host.ctypes.data, G, int(grid), int(gap_x), int(gap_y), int(depth),
                                       ptr(lines[2 * N:3 * N]), ptr(lines[3 * N:4 * N]), ptr(lines[5 * N:]), ptr(out[:N]), ptr(out[N:2 * N]),
                                       ptr(out[2 * N:3 * N]), ptr(out[3 * N:3 * N + G]), ptr(out[3 * N + G:]), stream())
    _lib.check(rc, 'omp_reading_blocks')
    return out


def split_block_ints(ints, n, n_groups):
    """the int32 tensor of reading_blocks (on either side of the copy) -> (block, line, rank, n_blocks, levels)"""
    return tuple(ints[k * n:(k + 1) * n] for k in range(3)) + (ints[3 * n:3 * n + n_groups], ints[3 * n + n_groups:])


def tile_remap(polys, points, tables, n_tiles, n_pages, nb, page_bins, edge, drop_cut=True, cap=None):
    """omp_tile_remap (csrc/tiles.hip; utils/tiles.py: remap_cpu is the specification and pack_tables packs the table): polys int32
    [N, 32] and points int32 [N, 2] in tile bins, tables device int32 [6 T + 1 + 2 pages] = row_start | tile_rect | tile_page |
    page_size.  The tables go to the device as they are: a tile they describe wrongly is refused there (tile_count -1).
    -> dict(page_polys int32 [cap, 32], page_points int32 [cap, 2]: the kept words in page bins, on the device; ints: ONE int32 tensor
    [N + cap + 3 T + 1 + pages] = cut [N] | src_row [cap] | tile_count [T] | tile_dropped [T] | out_start [T + 1] | page_count [pages]
    (split_tile_ints), so that a caller fetches everything in one copy).  cap defaults to N; the cut entries of words of no accepted
    tile are -1, the src_row entries beyond the kept total -1."""
    N, T, G = int(polys.shape[0]), int(n_tiles), int(n_pages)
    if polys.dim() != 2 or polys.shape[1] != 32 or N < 1 or T < 1 or G < 1:
        raise ValueError('polys must be [N, 32] with at least one word, one tile and one page')
    for name, tt, numel in (('polys', polys, 32 * N), ('points', points, 2 * N), ('tables', tables, 6 * T + 1 + 2 * G)):
        if not tt.is_cuda or tt.dtype != torch.int32 or not tt.is_contiguous() or tt.numel() != numel:
            raise ValueError('%s must be a contiguous device int32 tensor with %d elements' % (name, numel))
    cap = N if cap is None else int(cap)
    if cap < 0:
        raise ValueError('cap must not be negative')
    dev = polys.device
    page_polys = torch.empty(max(cap, 1), 32, dtype=torch.int32, device=dev)
    page_points = torch.empty(max(cap, 1), 2, dtype=torch.int32, device=dev)
    scratch = torch.empty(N, 34, dtype=torch.int32, device=dev)
    ints = torch.full((N + max(cap, 1) + 3 * T + 1 + G,), -1, dtype=torch.int32, device=dev)
    c0 = N + max(cap, 1)
    rc = _lib.lib().omp_tile_remap(ptr(polys), ptr(points), N, ptr(tables), T, G, int(nb), int(page_bins), int(edge), 1 if drop_cut else 0,
                                   ptr(scratch), ptr(ints[:N]), ptr(page_polys), ptr(page_points), ptr(ints[N:c0]), cap, ptr(ints[c0:c0 + T]),
                                   ptr(ints[c0 + T:c0 + 2 * T]), ptr(ints[c0 + 2 * T:c0 + 3 * T + 1]), ptr(ints[c0 + 3 * T + 1:]), stream())
    _lib.check(rc, 'omp_tile_remap')
    if cap == 0:
        ints = torch.cat([ints[:N], ints[c0:]])
    return dict(page_polys=page_polys[:cap], page_points=page_points[:cap], ints=ints)


def split_tile_ints(ints, n, n_tiles, n_pages, cap=None):
    """the int32 tensor of tile_remap (on either side of the copy) -> (cut, src_row, tile_count, tile_dropped, out_start, page_count)"""
    c0 = n + (n if cap is None else cap)
    T = n_tiles
    return ints[:n], ints[n:c0], ints[c0:c0 + T], ints[c0 + T:c0 + 2 * T], ints[c0 + 2 * T:c0 + 3 * T + 1], ints[c0 + 3 * T + 1:c0 + 3 * T + 1 + n_pages]
