"""Mixed-size engine calls three ways: padded (one call, every image padded to the largest), ragged (one call, OmniParser.infer(ragged=True))
and one call per image -- img/s timed with hipEvents, plus the bytes the cross-attention family streams per call, computed from shapes.

  python tools/ragged_bench.py [--dtypes bf16,bf16x3] [--images 16] [--sizes 1024x768,768x1024] [--big] [--iters 3] [--warmup 1]
                               [--ways padded,ragged,per_image]

Seeded weights (bench.py's procedural checkpoint), seeded images, half of each of the two sizes, alternating.  Decoding is forced to
--instances point-sequence items per image (EOS suppressed), so all three ways decode the same number of steps.  --big adds a
1440x1920 / 1920x1440 run.  One JSON line per (dtype, sizes, way).  Under `rocprofv3 --kernel-trace --stats -- python ...` the
per-kernel statistics give the cross-attention kernels' time (dec_cross_attn_kernel, dec_cross_attn_q4_kernel, dec_cross_merge_kernel).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(dtype):
    from advancedliteratemachinery_amd.model import OmniParser
    from advancedliteratemachinery_amd.utils.parser import make_args
    from advancedliteratemachinery_amd.utils import synthetic as weights
    args = make_args(tfm_pre_norm=True, use_fpn=True, use_char_window_prompt=True)
    model = OmniParser(args, engine_dtype=dtype)
    model.load_state_dict(weights.make_state_dict(args, seed=0))
    return model.to('cuda'), args


def prompts(args):
    from advancedliteratemachinery_amd.engine.inference import build_prompts
    return build_prompts(args, 'cuda')


def cross_bytes(dec, args, keys, n_inst):
    """bytes of K and V^T the cross-attention kernels stream in one call: every decoder step reads each image's key blocks once per
    layer and head (<= 64 rows per image: one row group), K and V^T alike; keys = key slots read per image"""
    esz = 4 if dec.dtype == torch.float32 else 2   # fp32 slabs, or split planes (hi + lo); bf16
    n_prompt = len(prompts(args)[0].reshape(-1))
    steps = (n_prompt - 1 + 2 * n_inst) + (2 + 32) + (2 + args.rec_length)
    return dec.L * dec.nH * 64 * 2 * esz * steps * sum(keys)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--dtypes', default='bf16,bf16x3')
    p.add_argument('--images', type=int, default=16)
    p.add_argument('--sizes', default='1024x768,768x1024')
    p.add_argument('--big', action='store_true', help='also 1440x1920 / 1920x1440')
    p.add_argument('--instances', type=int, default=16)
    p.add_argument('--iters', type=int, default=3)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--ways', default='padded,ragged,per_image', help='which of the three ways to time (one way per rocprofv3 run)')
    a = p.parse_args()
    from advancedliteratemachinery_amd.model.omniparser import bucket_by_size, ragged_layout
    from advancedliteratemachinery_amd.utils.nested_tensor import nested_tensor_from_tensor_list
    mixes = [[tuple(int(v) for v in s.split('x')) for s in a.sizes.split(',')]]
    if a.big:
        mixes.append([(1440, 1920), (1920, 1440)])
    st = torch.cuda.Stream()
    for dtype in a.dtypes.split(','):
        model, args = build(dtype)
        seqs = prompts(args)
        _, dec = model.engine()
        KB = 16 if (dec.dtype == torch.float32 and not dec.kv_split) else 32
        for mix in mixes:
            g = torch.Generator().manual_seed(0)
            imgs = [torch.randn(3, *mix[i % len(mix)], generator=g).to('cuda') for i in range(a.images)]
            nt = nested_tensor_from_tensor_list(imgs)
            zero = [torch.zeros(1, *i.shape[1:], dtype=torch.bool, device='cuda') for i in imgs]
            ways = {
                'padded': lambda: model.infer(nt.tensors, nt.mask, seqs, forced_instances=a.instances),
                'ragged': lambda: model.infer(imgs, None, seqs, forced_instances=a.instances, ragged=True),
                'per_image': lambda: [model.infer(i[None], z, seqs, forced_instances=a.instances) for i, z in zip(imgs, zero)],
            }
            # memory keys per image (stride 16) and the key slots each way reads
            m_img = [((h + 15) // 16) * ((w + 15) // 16) for h, w in (i.shape[1:] for i in imgs)]
            H, W = nt.tensors.shape[2:]
            m_pad = ((H + 15) // 16) * ((W + 15) // 16)
            Mmax = ragged_layout(m_img)[0]
            read = {'padded': [(m_pad + KB - 1) // KB * KB] * len(imgs), 'ragged': [(m + KB - 1) // KB * KB for m in m_img],
                    'per_image': [(m + KB - 1) // KB * KB for m in m_img]}
            for way in a.ways.split(','):
                fn = ways[way]
                with torch.cuda.stream(st):
                    for _ in range(a.warmup):
                        fn()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(a.iters):
                        fn()
                    t1.record()
                st.synchronize()
                ms = t0.elapsed_time(t1) / a.iters
                print(json.dumps(dict(dtype=dtype, sizes=['%dx%d' % hw for hw in mix], images=a.images, instances=a.instances, way=way,
                                      ms_per_call=round(ms, 2), img_per_s=round(a.images * 1000.0 / ms, 2),
                                      size_groups=len(bucket_by_size([i.shape[1:] for i in imgs])),
                                      keys_per_image=sorted(set(m_img)), padded_keys=m_pad, ragged_row_stride=Mmax,
                                      cross_attn_bytes_per_call=cross_bytes(dec, args, read[way], a.instances))), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
