"""Polygon-rectified word crops for the recogniser.

An OmniParser detection is a 16-point polygon: 8 points along the top edge of the word in reading order, then 8 along the
bottom edge walking back (the closed ring of the reference's datasets, utils/misc.py: gen_bezier_ctrl_points /
bezier2polygon).  Two steps turn it into MGP-STR's input:

  (a) rectify: sample the image along the polygon into a uint8 strip of the word's own resolution, sh x sw x 3;
  (b) resize:  the strip goes through exactly what a box crop goes through (utils/preprocess.py: CropResizer) -- Pillow's
      8-bit bicubic `resize((out_w, out_h))`, then ToTensor.

Step (a) works at the word's resolution and leaves anti-aliasing to (b), so a horizontal rectangle gives the very bytes of
the image slice and the polygon path EQUALS the box path wherever the box path was right.

The map is integer (Q = 16 fractional bits, `//` = floor division) so that host and device agree on every byte.  With
T[k] = P[k], B[k] = P[15 - k], k = 0..7:

    strip size (float64, from the unquantised points):
        sw = clamp(rint(0.5 * (len(polyline T) + len(polyline B))), 1, SMAX)
        sh = clamp(rint(mean_k |T[k] - B[k]|), 1, SMAX)
    Pq = rint(P * ONE) as int64
    column c:  n = 7 * (2c + 1); den = 2 * sw; k = min(n // den, 6); r = n - k * den
        top(c) = T[k] + (2 * (T[k+1] - T[k]) * r + den) // (2 * den)          (bot(c) alike with B)
    row j:  m = 2j + 1; dv = 2 * sh
        pt(j, c) = top(c) + (2 * (bot(c) - top(c)) * m + dv) // (2 * dv)
    sample:  sx = clamp(pt.x - ONE / 2, 0, (W - 1) << Q); ix = sx >> Q; fx = sx & (ONE - 1); ix1 = min(ix + 1, W - 1)   (y alike)
        a = p[iy][ix] * (ONE - fx) + p[iy][ix1] * fx;   b = the same on row iy1
        strip[j][c] = (a * (ONE - fy) + b * fy + (1 << 31)) >> 32

Pixel i covers [i, i + 1) with its centre at i + 0.5, as in the records.  Any 16 points are legal: sizes clamp to [1, SMAX],
sample coordinates clamp to the image, and point coordinates are clamped to +-COORD_MAX pixels (non-finite ones count as 0)
before anything else so that no product above leaves 64 bits.

`rectify_polygon_cpu` is that map in numpy (the specification; the CPU tests exercise it), `PolygonCropper` runs it on the
device: omp_polygon_rectify + omp_resize_crops (csrc/word_crop.hip), two launches and one upload per chunk whatever the
number of crops.
"""
import numpy as np
import torch

from .. import _lib, ops
from .preprocess import resize_coeffs

Q = 16
ONE = 1 << Q
SMAX = 4096
COORD_MAX = float(1 << 24)

# omp_rectify_desc / omp_resize_desc (include/omp355.h), field for field
RECTIFY_DESC = np.dtype([('src', '<u8'), ('pitch', '<i8'), ('w', '<i4'), ('h', '<i4'), ('sh', '<i4'), ('sw', '<i4'), ('strip_off', '<i8'),
                         ('tile0', '<i8'), ('pq', '<i8', (32,))])
RESIZE_DESC = np.dtype([('src', '<u8'), ('pitch', '<i8'), ('in_h', '<i4'), ('in_w', '<i4'), ('xb', '<i4'), ('kx', '<i4'), ('ksx', '<i4'),
                        ('yb', '<i4'), ('ky', '<i4'), ('ksy', '<i4')])
assert RECTIFY_DESC.itemsize == 304 and RESIZE_DESC.itemsize == 48


def _points(polys):
    """[..., 16, 2] float64, finite and inside +-COORD_MAX"""
    p = np.asarray(polys, dtype=np.float64)
    if p.shape[-2:] != (16, 2):
        raise ValueError('a polygon is 16 (x, y) points, got shape %s' % (p.shape,))
    return np.clip(np.nan_to_num(p, nan=0.0, posinf=COORD_MAX, neginf=-COORD_MAX), -COORD_MAX, COORD_MAX)


def _strip_sizes(p):
    """p: [N, 16, 2] from _points -> (sh, sw) int64 [N]"""
    t, b = p[:, :8], p[:, 15:7:-1]
    lt = np.sqrt(((t[:, 1:] - t[:, :-1]) ** 2).sum(-1)).sum(-1)
    lb = np.sqrt(((b[:, 1:] - b[:, :-1]) ** 2).sum(-1)).sum(-1)
    hh = np.sqrt(((t - b) ** 2).sum(-1)).mean(-1)
    sw = np.clip(np.rint(0.5 * (lt + lb)), 1, SMAX).astype(np.int64)
    sh = np.clip(np.rint(hh), 1, SMAX).astype(np.int64)
    return sh, sw


def polygon_strip_size(poly):
    """16 (x, y) points -> (sh, sw): the strip is as high as the mean distance between the edges and as wide as the mean
    length of the two edges, whole pixels, each in [1, SMAX]."""
    sh, sw = _strip_sizes(_points(poly)[None])
    return int(sh[0]), int(sw[0])


def _quantise(p):
    return np.rint(p * ONE).astype(np.int64)


def rectify_polygon_cpu(image_u8, poly, size=None):
    """uint8 [H, W, 3] image, 16 (x, y) points -> uint8 [sh, sw, 3] strip: the map of the module docstring, in numpy int64."""
    img = np.asarray(image_u8)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError('rectify_polygon_cpu takes a uint8 [H, W, C] image')
    H, W = img.shape[:2]
    p = _points(poly)
    sh, sw = size or polygon_strip_size(p)
    pq = _quantise(p)
    T, B = pq[:8], pq[15:7:-1]
    c = np.arange(sw, dtype=np.int64)
    n = 7 * (2 * c + 1)
    den = 2 * sw
    k = np.minimum(n // den, 6)
    r = n - k * den

    def edge(E):
        return E[k] + (2 * (E[k + 1] - E[k]) * r[:, None] + den) // (2 * den)

    top, bot = edge(T), edge(B)                                           # [sw, 2]
    m = 2 * np.arange(sh, dtype=np.int64) + 1
    dv = 2 * sh
    pt = top[None] + (2 * (bot - top)[None] * m[:, None, None] + dv) // (2 * dv)   # [sh, sw, 2]
    sx = np.clip(pt[..., 0] - ONE // 2, 0, (W - 1) << Q)
    sy = np.clip(pt[..., 1] - ONE // 2, 0, (H - 1) << Q)
    ix, fx = sx >> Q, (sx & (ONE - 1))[..., None]
    iy, fy = sy >> Q, (sy & (ONE - 1))[..., None]
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    im = img.astype(np.int64)
    a = im[iy, ix] * (ONE - fx) + im[iy, ix1] * fx
    b = im[iy1, ix] * (ONE - fx) + im[iy1, ix1] * fx
    return ((a * (ONE - fy) + b * fy + (1 << (2 * Q - 1))) >> (2 * Q)).astype(np.uint8)


class PolygonCropper(object):
    """Polygon-rectified word crops on the device: uint8 [H, W, 3] device images + (image index, 16 x 2 points) -> fp32
    [N, 3, out_h, out_w] in [0, 1], equal to rectify_polygon_cpu + Pillow `resize((out_w, out_h), BICUBIC)` + ToTensor on
    every float.  Per chunk: one upload (descriptors of both kernels + Pillow's coefficient tables, packed) and two launches.
    A chunk ends at `max_crops` crops or when its strips would exceed `scratch_bytes` (one strip can be 48 MB; a single
    strip larger than the budget still runs, alone)."""

    def __init__(self, device, out_h=32, out_w=128, scratch_bytes=256 << 20, max_crops=4096, filt='bicubic'):
        self.device = torch.device(device)
        self.out_h, self.out_w, self.filt = out_h, out_w, filt
        self.scratch_bytes, self.max_crops = int(scratch_bytes), int(max_crops)
        p = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)     # ToTensor: p / 255 in float32
        self.lut = p[None, :].expand(3, 256).contiguous().to(self.device)
        self._tables = {}
        self._scratch = None
        self.last_chunks = 0

    def _axis(self, n_in, n_out):
        """-> (ksize, int32 [n_out * 2 + n_out * ksize] = bounds then coefficients) or (0, None) when the size stays"""
        key = (n_in, n_out)
        t = self._tables.get(key)
        if t is None:
            if len(self._tables) > 4096:
                self._tables.clear()
            if n_in == n_out:
                t = (0, None)
            else:
                ks, b, k = resize_coeffs(n_in, n_out, self.filt)
                t = (ks, np.concatenate([b.ravel(), k.ravel()]).astype(np.int32))
            self._tables[key] = t
        return t

    def _chunks(self, nbytes):
        start, used = 0, 0
        for i, b in enumerate(nbytes):
            if i > start and (used + b > self.scratch_bytes or i - start >= self.max_crops):
                yield start, i
                start, used = i, 0
            used += b
        if len(nbytes) > start:
            yield start, len(nbytes)

    @torch.no_grad()
    def __call__(self, images, polys):
        """images: list of contiguous uint8 [H, W, 3] device tensors; polys: list of (image index, 16 x 2 points in that
        image's pixels).  -> fp32 [N, 3, out_h, out_w]."""
        N = len(polys)
        out = torch.empty(N, 3, self.out_h, self.out_w, dtype=torch.float32, device=self.device)
        self.last_chunks = 0
        if N == 0:
            return out
        for im in images:
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_cuda or not im.is_contiguous():
                raise ValueError('PolygonCropper takes contiguous uint8 [H, W, 3] device tensors')
            if im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError('empty image %s' % (tuple(im.shape),))
        owner = np.asarray([int(p[0]) for p in polys], dtype=np.int64)
        if owner.min() < 0 or owner.max() >= len(images):
            raise ValueError('polygon refers to image %d of %d' % (int(owner.max() if owner.min() >= 0 else owner.min()), len(images)))
        pts = _points([p[1] for p in polys])
        sh, sw = _strip_sizes(pts)
        pq = _quantise(pts).reshape(N, 32)
        nbytes = sh * sw * 3
        tiles = ((sw + 63) // 64) * ((sh + 3) // 4)
        im_ptr = np.asarray([im.data_ptr() for im in images], dtype=np.uint64)[owner]
        im_pitch = np.asarray([im.stride(0) for im in images], dtype=np.int64)[owner]
        im_w = np.asarray([im.shape[1] for im in images], dtype=np.int64)[owner]
        im_h = np.asarray([im.shape[0] for im in images], dtype=np.int64)[owner]
        h = _lib.lib()
        plane = 3 * self.out_h * self.out_w
        for i0, i1 in self._chunks(nbytes.tolist()):
            n = i1 - i0
            need = int(nbytes[i0:i1].sum())
            if self._scratch is None or self._scratch.numel() < need:
                self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
            scratch = self._scratch
            off = np.cumsum(nbytes[i0:i1]) - nbytes[i0:i1]
            rd = np.zeros(n, dtype=RECTIFY_DESC)
            rd['src'], rd['pitch'], rd['w'], rd['h'] = im_ptr[i0:i1], im_pitch[i0:i1], im_w[i0:i1], im_h[i0:i1]
            rd['sh'], rd['sw'], rd['strip_off'], rd['pq'] = sh[i0:i1], sw[i0:i1], off, pq[i0:i1]
            rd['tile0'] = np.cumsum(tiles[i0:i1]) - tiles[i0:i1]
            zd = np.zeros(n, dtype=RESIZE_DESC)
            zd['src'] = np.uint64(scratch.data_ptr()) + off.astype(np.uint64)
            zd['pitch'], zd['in_h'], zd['in_w'] = sw[i0:i1] * 3, sh[i0:i1], sw[i0:i1]
            # Pillow's tables of the chunk, each distinct (size in, size out) once
            parts, where, length = [], {}, 0
            cols = {k: np.zeros(n, dtype=np.int32) for k in ('xb', 'kx', 'ksx', 'yb', 'ky', 'ksy')}
            for axis, sizes, n_out in (('x', sw[i0:i1].tolist(), self.out_w), ('y', sh[i0:i1].tolist(), self.out_h)):
                for i, n_in in enumerate(sizes):
                    slot = where.get((n_in, n_out))
                    if slot is None:
                        ks, flat = self._axis(n_in, n_out)
                        slot = (length, ks)
                        if ks:
                            parts.append(flat)
                            length += flat.size
                        where[(n_in, n_out)] = slot
                    if slot[1]:
                        cols[axis + 'b'][i], cols['k' + axis][i], cols['ks' + axis][i] = slot[0], slot[0] + 2 * n_out, slot[1]
            for k, v in cols.items():
                zd[k] = v
            table = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
            if table.size >= 1 << 31:
                raise ValueError('coefficient tables of one chunk exceed 2^31 entries')
            blob = np.concatenate([rd.view(np.uint8), zd.view(np.uint8), table.view(np.uint8)])
            dev = torch.from_numpy(blob).to(self.device)                    # the chunk's one upload
            base = dev.data_ptr()
            zd_ptr, tb_ptr = base + rd.nbytes, base + rd.nbytes + zd.nbytes
            rc = h.omp_polygon_rectify(base, n, int(tiles[i0:i1].sum()), ops.ptr(scratch), scratch.numel(), ops.stream())
            _lib.check(rc, 'omp_polygon_rectify')
            rc = h.omp_resize_crops(zd_ptr, n, tb_ptr if table.size else None, table.size, ops.ptr(self.lut),
                                    out.data_ptr() + i0 * plane * 4, self.out_h, self.out_w, ops.stream())
            _lib.check(rc, 'omp_resize_crops')
            self.last_chunks += 1
        return out
