"""OmniParser: drop-in for the reference model class on the inference path.

Same constructor-by-args, same state-dict layout, same `forward(samples, sequence)` contract as
OCR/OmniParser/model/omniparser.py:7-32 (eval mode), with the computation executed by
libomp355 (hand-written gfx950 kernels).  Additions over the reference:
  * batches of B > 1 images (the reference asserts B == 1, engine/val.py:22): every image is
    decoded exactly as if it had been submitted alone; `forward` then returns a list of B results;
  * `forced_instances`: fixed-length decoding for throughput measurement with random weights;
  * `infer(..., ragged=True)`: images of different sizes in one call, each encoded and decoded at its own size (no
    padding anywhere) -- the reference's batch-1 answers with a batch's decode throughput;
  * `infer(..., windows=...)`: window prompts -- several spatial (and first-character) windows per image decoded as rows of ONE
    point phase over one encoder pass and one K/V projection.

Return value per image (reference transformer.py:240-246,286):
  text spotting : ([pt (1,2N), poly (1,32N), rec (1,N,rec_length)] int64, [probs (N,rec_length)])
  KIE           : list of (text, class_name, prob, [rects])
  no points     : None
"""
import os

import torch
import torch.nn as nn

from .. import ops
from ..utils.env import env_flag, env_int
from ..utils.nested_tensor import NestedTensor
from ..utils import windows as WN
from . import params
from .backbone import Encoder
from .transformer import Decoder, index2class

# 'bf16x3' = the parity engine: fp32 storage / fp32 non-GEMM kernels, large products as three bf16 products of split
# operands on the bf16 matrix cores (model/backbone.py, include/omp355.h omp_gemm_args.a_wrap)
_DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32, 'bf16x3': 'bf16x3', torch.bfloat16: torch.bfloat16,
           torch.float32: torch.float32}


def _image_sizes(sizes, B):
    """orig_size of seqs[3] (engine/val.py:33): a (2,) tensor, a (B,2) tensor or a list of B of them."""
    if isinstance(sizes, (list, tuple)) and len(sizes) == B and not isinstance(sizes[0], (int, float)):
        t = torch.stack([torch.as_tensor(s).reshape(2) for s in sizes])
    else:
        t = torch.as_tensor(sizes).reshape(-1, 2)
    if t.shape[0] == 1 and B > 1:
        t = t.expand(B, 2)
    return t.cpu()


def mask_extents(mask):
    """(h, w) of every image of a padded batch, read off its padding mask (True = padding): the image fills the top-left h x w
    corner, as nested_tensor_from_tensor_list puts it.  A mask of another shape is refused rather than guessed at."""
    m = mask.bool()
    B, H, W = m.shape
    h, w = (~m[:, :, 0]).sum(1), (~m[:, 0, :]).sum(1)
    ys, xs = torch.arange(H, device=m.device), torch.arange(W, device=m.device)
    rect = (ys[None, :, None] >= h[:, None, None]) | (xs[None, None, :] >= w[:, None, None])
    if not torch.equal(rect, m) or bool((h == 0).any()) or bool((w == 0).any()):
        raise ValueError('ragged: every image of a padded batch must fill the top-left corner of its mask (True = padding)')
    return list(zip(h.tolist(), w.tolist()))


def bucket_by_size(sizes):
    """[(h, w)] per image -> [((h, w), [image indices])]: one encoder pass per distinct size, in order of first appearance"""
    groups = {}
    for i, hw in enumerate(sizes):
        groups.setdefault(tuple(int(v) for v in hw), []).append(i)
    return list(groups.items())


def ragged_layout(keys, align=64):
    """memory keys M_b per image -> (Mmax, key_len, row0): image b's memory rows start at row0[b] = b * Mmax, with
    Mmax = round_up(max M_b, align) (a multiple of 64 keeps omp_kv_project_rows' bf16 path), and it attends over its first
    key_len[b] = M_b keys only (Decoder.project_memory)."""
    key_len = [int(n) for n in keys]
    Mmax = (max(key_len) + align - 1) // align * align
    return Mmax, key_len, [b * Mmax for b in range(len(key_len))]


class OmniParser(nn.Module):
    def __init__(self, args, swin_cfg=None, engine_dtype=None):
        super().__init__()
        self.args = args
        self.swin_cfg = dict(params.SWIN_B)
        self.swin_cfg.update(swin_cfg or {})
        self.use_fpn = bool(args.use_fpn)
        self.engine_dtype = _DTYPES[engine_dtype or getattr(args, 'engine_dtype', 'bf16')]
        spec = params.expected_state_dict(args, self.swin_cfg)
        shared = [['transformer.%s_decoder.norm.%s' % (k, leaf) for k in ('pt', 'poly', 'rec')]
                  for leaf in ('weight', 'bias')]
        params.attach_parameters(self, spec, shared)
        self._engine = None
        self._engine_key = None
        self.use_graph = True          # decoder steps replay as hipGraphs when run on a non-default stream
        self.overlap_decoders = True   # polygon || recognition decoders on two streams
        # images per encoder pass inside one engine call (see _encode_chunked); None = by engine (enc_chunk_default), OMP355_ENC_CHUNK is
        # the A/B knob of the sweeps
        self.enc_chunk = env_int('OMP355_ENC_CHUNK', 0, 0, 4096) or None
        self._streams = None
        self.phase_events = None       # set to [] to collect (name, torch.cuda.Event) marks per infer()
        self.eval()

    # -- engine lifecycle -------------------------------------------------------------------------
    def _key(self):
        ps = list(self.parameters())
        # OMP355_KV_SPLIT changes the layout of the K / V^T slabs the decoder is built around: part of the key
        return (ps[0].device, self.engine_dtype, sum(p._version for p in ps), id(ps[0]), env_flag('OMP355_KV_SPLIT', True))

    def engine(self):
        """(Encoder, Decoder) packed from the CURRENT parameters; rebuilt after load_state_dict/.to()."""
        key = self._key()
        if self._engine is None or key != self._engine_key:
            dev = key[0]
            if dev.type != 'cuda':
                raise RuntimeError('OmniParser runs on MI355X only: move the model to a cuda (HIP) device; '
                                   'there is no CPU fallback')
            sd = {k: v for k, v in self.state_dict().items()}
            x3 = self.engine_dtype == 'bf16x3'
            tdt = torch.float32 if x3 else self.engine_dtype
            with torch.cuda.device(dev):
                enc = Encoder(sd, self.args, self.swin_cfg, tdt, x3=x3)
                dec = Decoder(sd, self.args, tdt, dev, x3=x3)
            self._engine, self._engine_key = (enc, dec), key
        self._engine[1].use_graph = self.use_graph
        return self._engine

    def _mark(self, name):
        if self.phase_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.phase_events.append((name, ev))

    def _side_streams(self, dev):
        """Two extra HIP streams so the polygon and recognition decoders overlap (None -> sequential)."""
        if not self.overlap_decoders:
            return None
        if self._streams is None or self._streams[0].device != dev:
            # OMP355_SIDE_PRIO=1 (A/B of the paired schedule, Decoder.decode_poly_and_rec / omp_decoder_run_pair): the side streams at HIGH priority, so that
            # the row-owner chains they carry are placed before the cross-attention workgroups of the caller's stream when a launch drains.  Default 0:
            # high-priority streams take hardware queues of their own, and the four single-stream lanes of a pipelined run created afterwards then
            # share what is left -- bench.py's batch8 leg fell from 228 to 129 img/s with them (profiles/r06g_bench.json vs r06h)
            pr = -1 if env_flag('OMP355_SIDE_PRIO', False) else 0
            self._streams = (torch.cuda.Stream(device=dev, priority=pr), torch.cuda.Stream(device=dev, priority=pr))
        return self._streams

    def set_engine_dtype(self, dtype):
        self.engine_dtype = _DTYPES[dtype]
        self._engine = None

    # -- reference-compatible forward -------------------------------------------------------------
    @torch.no_grad()
    def forward(self, samples, sequence, forced_instances=None):
        if self.training:
            raise NotImplementedError('training is out of scope for the MI355X inference engine')
        if not isinstance(samples, NestedTensor) and hasattr(samples, 'tensors'):
            samples = NestedTensor(samples.tensors, samples.mask)
        img, mask = samples.tensors, samples.mask
        if mask is None:
            mask = torch.zeros(img.shape[0], img.shape[2], img.shape[3], dtype=torch.bool, device=img.device)
        results = self.infer(img, mask, sequence, forced_instances=forced_instances)
        return results[0] if img.shape[0] == 1 else results

    # -- batched inference ------------------------------------------------------------------------
    @torch.no_grad()
    def infer(self, img, mask, sequence, forced_instances=None, has_padding=None, lane=None, packed=None, ragged=False,
              windows=None, char_windows=None, clip_windows=False):
        """lane: a pipeline Lane (engine/pipeline.py) -- private decoder state + side streams, so several
        batches can be in flight on different HIP streams; None = the model's own state.
        packed = N (text spotting only): return (ids int32 [B, N, 34 + rec_length], probs [B, N, rec_length], n_inst [B]) device
        tensors -- the all-gather payload of utils/dist.py -- packed by ONE kernel from the decoders' buffers instead of the
        per-image result lists (no per-image host work or device copies).
        ragged=True: every image is encoded and decoded at its OWN size, as if it had been submitted alone -- `img` is a list of
        [3, h_b, w_b] device tensors (mask None), or a padded batch whose mask gives each image's extent (mask_extents).  Images
        of one size share an encoder pass; the decoders run once for all, each image's cross-attention reading its own M_b keys
        and no others (Decoder.project_memory key_len).  One size only: the padding-free path below, unchanged.  packed= is
        padded-only.
        windows (text spotting only; None = the call above, bit for bit): a list of windows [x0, y0, x1, y1] in coordinate bins shared
        by all images, or one such list per image (at most 64 each; utils/windows.py: grid_windows builds the reference's training
        grids).  Every window is decoded under its own prompt (window_prompts) as a row of ONE point phase; the windows of an image
        share its encoder pass, its K/V slabs and its cross-attention workgroups.  char_windows: a first-character window [c0, c1] for
        all windows, one per window, or one list per image (args.use_char_window_prompt only).  The points are gathered on the
        device (omp_window_points) and feed the polygon / recognition phases as in the plain call.  Per image the result is
        ([pt (1,2N), poly (1,32N), rec (1,N,rec_length)], [probs (N,rec_length)], window (N,) int64): the reference's shape with the
        instances of all windows concatenated in window order, and the index of the window each instance came from.
        clip_windows=True keeps a point only if the reference's membership rule holds against its own window (x0 < x <= x1 and
        y0 < y <= y1, dataset/collate_fn.py:80-81).  Off by default: the lower bounds are strict, so under the default window the
        rule also drops bin 0, which the plain call returns.  Works with ragged=True; packed= and args.infer_vie are refused."""
        windowed = windows is not None or char_windows is not None
        if windowed and packed is not None:
            raise ValueError('infer: windows= returns per-image results; packed= is the plain call\'s payload')
        if windowed and self.args.infer_vie:
            raise ValueError('infer: windows= is a text-spotting call; the KIE walk (args.infer_vie) reads one row per image')
        enc, dec = self.engine()
        side = None
        if lane is not None:
            dec, side = lane.decoder(dec), (lane.side if lane.side is not None else False)   # False: no side streams at all
        groups = None
        if ragged:
            imgs = self._ragged_images(img, mask)
            groups = bucket_by_size([tuple(i.shape[1:]) for i in imgs])
            if len(groups) == 1:   # nothing ragged about it: the ordinary call on the unpadded images
                (h, w), _ = groups[0]
                if not torch.is_tensor(img) or tuple(img.shape[2:]) != (h, w):
                    img = torch.stack(imgs)
                mask = torch.zeros(img.shape[0], h, w, dtype=torch.bool, device=img.device)
                has_padding, groups = False, None
            elif packed is not None:
                raise ValueError('infer: packed= results are produced for padded batches only; call with ragged=False')
        a = self.args
        dev = imgs[0].device if groups is not None else img.device
        B = len(imgs) if groups is not None else img.shape[0]
        with torch.cuda.device(dev):
            if groups is not None:
                self._mark('start')
                memory, mem_pos, Mmax, key_len = self._encode_ragged(enc, imgs, groups)
                self._mark('encode')
                kv = dec.project_memory(memory, mem_pos, B, Mmax, None, key_len=key_len)
            else:
                img = img.float().contiguous()
                if has_padding is None:
                    has_padding = bool(mask.any())
                self._mark('start')
                e = self._encode_chunked(enc, img, mask, no_padding=not has_padding)
                self._mark('encode')
                kv = dec.project_memory(e['memory'], e['mem_pos'], B, e['M'], e['key_mask'] if has_padding else None)
            prompt = [int(t) for t in sequence[0].reshape(-1).tolist()]
            poly_sos = int(sequence[1].reshape(-1)[0])
            rec_sos = int(sequence[2].reshape(-1)[0])
            if windowed:   # [rows, n_prompt] prompt rows + rows per image instead of the one flat prompt
                per_image = WN.resolve_windows(windows if windows is not None else [WN.default_window(a)], B)
                cw = WN.resolve_char_windows(char_windows, per_image)
                prompt = (torch.cat([WN.window_prompts(a, ws, c) for ws, c in zip(per_image, cw)], 0), [len(ws) for ws in per_image],
                          bool(clip_windows))
            self._mark('kv_project')
            dstream = getattr(lane, 'dec_stream', None) if lane is not None else None
            if dstream is not None:
                # decoder phases on the lane's high-priority stream; the lane stream rejoins below
                outer = torch.cuda.current_stream()
                dstream.wait_stream(outer)
                with torch.cuda.stream(dstream):
                    out = self._decode(dec, kv, prompt, poly_sos, rec_sos, sequence, forced_instances, B, dev, side, packed)
                outer.wait_stream(dstream)
                return out
            return self._decode(dec, kv, prompt, poly_sos, rec_sos, sequence, forced_instances, B, dev, side, packed)

    def enc_chunk_default(self):
        """Images per encoder pass.  What matters at 1024 x 1024 is the last, partial round of the stage-2 chains over the 256 compute
        units (18 of the 24 Swin blocks): a chunk of n images is n x 4096 / 80 workgroups of 80 rows (bf16) = n / 5 rounds, n x 4096 / 48 of
        48 rows (parity engine) = n / 3 rounds.  bf16: 32 -> 40 images (6.4 -> 8.0 rounds) took the encoder from 169.4 to 164.1 ms per 160
        images (profiles/r05n_enc_chunk_32_vs_40.txt), 80 (16.0 rounds, half the launches) to 160.9 (r05q); parity engine: 40 -> 54
        (13.33 -> 18.0 rounds: 160 images are then 54 rounds instead of 56) 375.5 -> 372.0 ms (profiles/r05q_enc_chunk.txt)."""
        return 54 if self.engine_dtype == 'bf16x3' else 80

    def _encode_chunked(self, enc, img, mask, no_padding=False):
        """The encoder gains nothing from more than a few images per launch (its kernels already fill the chip) while
        its activations grow with the batch; the decoders do gain (their steps are latency-bound).  So a large engine
        call is encoded `enc_chunk` images at a time; every chunk's input_proj writes its rows of the call's memory
        tensors directly (the first chunk's are copied once its shape is known)."""
        B, ch = img.shape[0], max(1, int(self.enc_chunk or self.enc_chunk_default()))
        kw = dict(no_padding=True) if no_padding else {}
        if B <= ch:
            return enc.encode(img, mask, **kw)
        first = enc.encode(img[:ch], mask[:ch], **kw)
        M = first['M']
        out = dict(first)
        full = {k: torch.empty((B * M,) + tuple(first[k].shape[1:]), dtype=first[k].dtype, device=first[k].device)
                for k in ('memory', 'mem_pos')}
        for k in full:
            full[k][:ch * M].copy_(first[k])
        pos, km = [first['pos']], [first['key_mask']]
        for i in range(ch, B, ch):
            n = min(ch, B - i)
            p = enc.encode(img[i:i + n], mask[i:i + n], out=(full['memory'][i * M:(i + n) * M], full['mem_pos'][i * M:(i + n) * M]), **kw)
            pos.append(p['pos'])
            km.append(p['key_mask'])
        out.update(full)
        out['pos'] = torch.cat(pos, 0)   # small (diagnostics / parity tests only: the decoders read mem_pos)
        out['key_mask'] = torch.cat(km, 0)
        return out

    @staticmethod
    def _ragged_images(img, mask):
        """the images of a ragged call, unpadded: a list / tuple of [3, h, w] tensors as given, or the extents of a padded batch"""
        if torch.is_tensor(img):
            if img.dim() != 4:
                raise ValueError('ragged: a padded batch is [B, 3, H, W] (got %s)' % (tuple(img.shape),))
            if mask is None:
                return list(img)
            return [im[:, :h, :w] for im, (h, w) in zip(img, mask_extents(mask))]
        imgs = list(img)
        if not imgs or any(not torch.is_tensor(i) or i.dim() != 3 for i in imgs):
            raise ValueError('ragged: give a list of [3, h, w] image tensors or a padded batch and its mask')
        if len(set(i.device for i in imgs)) != 1:
            raise ValueError('ragged: all images of a call live on one device')
        return imgs

    def _encode_ragged(self, enc, imgs, groups):
        """One encoder pass per size group (chunked as _encode_chunked does); every image's memory and mem_pos rows are placed at
        row0[b] = b * Mmax of the call's memory tensors, the rows beyond its M_b stay zero (finite: they are projected into the slabs).
        -> (memory, mem_pos, Mmax, key_len)"""
        B, dev = len(imgs), imgs[0].device
        parts, keys = [], [0] * B
        for (h, w), idx in groups:
            x = torch.stack([imgs[i] for i in idx]).float().contiguous()
            e = self._encode_chunked(enc, x, torch.zeros(len(idx), h, w, dtype=torch.bool, device=dev), no_padding=True)
            parts.append((idx, e['M'], e['memory'], e['mem_pos']))
            for i in idx:
                keys[i] = e['M']
        Mmax, key_len, row0 = ragged_layout(keys)
        mem0 = parts[0][2]
        memory = torch.zeros((B * Mmax, mem0.shape[1]), dtype=mem0.dtype, device=dev)
        mem_pos = torch.zeros_like(memory)
        for idx, M, mem, mp in parts:
            rows = (torch.tensor([row0[i] for i in idx])[:, None] + torch.arange(M)[None, :]).reshape(-1).to(dev)
            memory.index_copy_(0, rows, mem)
            mem_pos.index_copy_(0, rows, mp)
        return memory, mem_pos, Mmax, key_len

    def _decode(self, dec, kv, prompt, poly_sos, rec_sos, sequence, forced_instances, B, dev, side, packed=None):
        """point decoder -> polygon || recognition decoders (or the KIE walk) on the current stream"""
        a = self.args
        if packed is not None and a.infer_vie:   # before any work: the KIE branch below returns early
            raise ValueError('packed results are the text-spotting payload; KIE returns entity lists')
        if isinstance(prompt, tuple):
            return self._decode_windows(dec, kv, prompt, poly_sos, rec_sos, forced_instances, B, dev, side)
        pts = dec.decode_points(kv, prompt, forced_instances=forced_instances)
        self._mark('pt_decode')
        if a.infer_vie:
            sizes = sequence[3]
            return self._kie(dec, kv, pts, poly_sos, rec_sos, sizes, B, side)
        counts = [int(ids.numel()) // 2 for ids, _ in pts]
        R = sum(counts)
        if R == 0:
            if packed is not None:
                return (torch.zeros(B, packed, 34 + a.rec_length, dtype=torch.int32, device=dev),
                        torch.zeros(B, packed, a.rec_length, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
            return [None] * B
        points = torch.cat([ids.reshape(-1, 2) for ids, _ in pts], 0).to(dev, torch.int32)
        (poly, _), (rec, rprob) = dec.decode_poly_and_rec(kv, points, counts, poly_sos, rec_sos, a.rec_length,
                                                          streams=(side or None) if side is not None else self._side_streams(dev))
        if packed is not None:   # one launch from the decoders' own buffers (views into the phase tensors)
            self._mark('poly_rec_decode')
            return ops.pack_spotting(points, poly, rec, rprob, counts, int(packed), a.rec_length)
        poly, rec, rprob = poly.long(), rec.long(), rprob.clone()
        self._mark('poly_rec_decode')
        out, r0 = [], 0
        for b in range(B):
            n = counts[b]
            if n == 0:
                out.append(None)
                continue
            sl = slice(r0, r0 + n)
            out.append(([points[sl].long().reshape(1, -1), poly[sl].reshape(1, -1), rec[sl].unsqueeze(0)],
                        [rprob[sl]]))
            r0 += n
        return out

    def _decode_windows(self, dec, kv, prompt, poly_sos, rec_sos, forced_instances, B, dev, side):
        """the windowed call: point phase of sum W_b rows -> omp_window_points (the points never visit the host; only the counts come
        back, in one small copy, to size the next phases) -> polygon || recognition decoders over all windows' instances"""
        a = self.args
        prompts, rows_per_image, clip = prompt
        st = dec.decode_points(kv, prompts, forced_instances=forced_instances, rows_per_image=rows_per_image)
        ph, rows = st['ph'], st['rows']
        points, _, cnt = ops.window_points(ph.seq, ph.finished, ph.lengths, st['row_image'], B, st['n_prompt'], st['sampled'], clip=clip)
        row_count, _, row_start, image_count = ops.split_window_counts(cnt.cpu(), rows)
        self._mark('pt_decode')
        R = int(row_start[rows])
        if R == 0:
            return [None] * B
        counts = image_count.tolist()
        points = points[:R]
        (poly, _), (rec, rprob) = dec.decode_poly_and_rec(kv, points, counts, poly_sos, rec_sos, a.rec_length,
                                                          streams=(side or None) if side is not None else self._side_streams(dev))
        poly, rec, rprob = poly.long(), rec.long(), rprob.clone()
        self._mark('poly_rec_decode')
        out, r0, w0 = [], 0, 0
        for b in range(B):
            n, W = counts[b], rows_per_image[b]
            window = torch.repeat_interleave(torch.arange(W), row_count[w0:w0 + W].long())
            w0 += W
            if n == 0:
                out.append(None)
                continue
            sl = slice(r0, r0 + n)
            out.append(([points[sl].long().reshape(1, -1), poly[sl].reshape(1, -1), rec[sl].unsqueeze(0)], [rprob[sl]], window))
            r0 += n
        return out

    # -- KIE assembly (reference transformer.py:143-217) --------------------------------------------------
    def _kie(self, dec, kv, pts, poly_sos, rec_sos, sizes, B, side=None):
        a = self.args
        nb = a.num_bins
        events, words, counts = [], [], []
        for b in range(B):
            ids = pts[b][0].tolist()
            ev, n, i, cnt = [], len(ids), 0, 0
            while i < n:
                if ids[i] < nb:
                    if i + 1 <= n - 1 and ids[i + 1] < nb:
                        ev.append(('word', len(words)))
                        words.append((ids[i], ids[i + 1]))
                        cnt += 1
                        i += 2
                    else:
                        i += 1
                else:
                    ev.append(('class', i))
                    i += 1
            events.append(ev)
            counts.append(cnt)
        poly = rec = None
        if words:
            points = torch.tensor(words, dtype=torch.int32, device=kv['K'].device)
            (poly, _), (rec, _) = dec.decode_poly_and_rec(kv, points, counts, poly_sos, rec_sos, a.rec_length,
                                                          infer_vie=True,
                                                          streams=(side or None) if side is not None else self._side_streams(kv['K'].device))
            poly, rec = poly.cpu(), rec.cpu()
        i2c = index2class(a)
        sizes = _image_sizes(sizes, B)
        out = []
        for b in range(B):
            ids, probs = pts[b][0].tolist(), pts[b][1].tolist()
            if len(ids) == 0:
                out.append(None)
                continue
            ih, iw = sizes[b][0].item(), sizes[b][1].item()
            res, cur_words, cur_rects = [], [], []
            for kind, v in events[b]:
                if kind == 'word':
                    pp = poly[v].reshape(-1, 2)
                    cur_rects.append([iw * pp[:, 0].min().item() / nb, ih * pp[:, 1].min().item() / nb,
                                      iw * pp[:, 0].max().item() / nb, ih * pp[:, 1].max().item() / nb])
                    chars = []
                    for t in rec[v].tolist():
                        if t == a.recog_pad_index or t == a.rec_eos_index:
                            break
                        if t == a.recog_pad_index - 1:
                            continue
                        chars.append(a.chars[t - nb])
                    cur_words.append(''.join(chars))
                else:
                    res.append((' '.join(cur_words), i2c[ids[v]], probs[v], cur_rects))
                    cur_words, cur_rects = [], []
            out.append(res)
        return out
