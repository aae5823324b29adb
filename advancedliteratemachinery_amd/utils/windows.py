"""Window prompts: the point decoder's own prompt as a caller's argument.

The point decoder is conditioned on a prompt [x0, y0, x1, y1, (c0, c1,) pt_sos]: a spatial window in coordinate bins and, with
`use_char_window_prompt`, a first-character window.  The reference trains on such windows (OCR/OmniParser/dataset/collate_fn.py:46-115:
eight grid partitions and random rectangles; a word belongs to a window when x0 < x <= x1 and y0 < y <= y1) and its forward accepts any
of them; only its evaluation loop fixes the prompt to the whole image (engine/val.py:25-33).  This module holds the host side:

  grid_windows       the windows of an nx x ny partition, computed as collate_fn.py:60-69 computes them
  window_prompts     windows (and character windows) -> the int prompt rows the point decoder reads, validated
  gather_points_cpu  the numpy SPECIFICATION of omp_window_points (csrc/window_points.hip): the point rows of a finished point phase
                     -> one compacted list of (x, y) points, per-row counts, optionally clipped to each row's window
"""
import numpy as np
import torch

MAX_WINDOWS = 64   # rows of one image per cross-attention workgroup (model/transformer.py: Decoder.make_tiles)

# the eight partitions the reference draws its grid windows from (collate_fn.py:55-56)
TRAINING_GRIDS = ((3, 3), (3, 1), (1, 3), (3, 2), (2, 3), (2, 2), (2, 1), (1, 2))


def grid_windows(nx, ny, num_bins):
    """The nx * ny windows [x0, y0, x1, y1] of a grid partition, x the outer loop (collate_fn.py:60-69).  Neighbouring windows share
    their border bin: the membership rule (x0 < x <= x1) gives it to the window that ends there."""
    nx, ny, num_bins = int(nx), int(ny), int(num_bins)
    if nx < 1 or ny < 1 or num_bins < 2:
        raise ValueError('grid_windows: nx, ny >= 1 and num_bins >= 2 (got %d x %d over %d bins)' % (nx, ny, num_bins))
    inter_x = min(int(num_bins / nx), num_bins - 1)
    inter_y = min(int(num_bins / ny), num_bins - 1)
    out = []
    for i in range(nx):
        for j in range(ny):
            x0, y0 = i * inter_x, j * inter_y
            out.append([x0, y0, min(x0 + inter_x, num_bins - 1), min(y0 + inter_y, num_bins - 1)])
    return out


def default_window(args):
    return [0, 0, args.num_bins - 1, args.num_bins - 1]


def window_prompts(args, windows=None, char_windows=None):
    """-> int64 tensor [W, n_prompt]: [x0, y0, x1, y1, pt_sos] per window, or with args.use_char_window_prompt
    [x0, y0, x1, y1, num_bins + c0, num_bins + c1, pt_sos].  windows: a list of [x0, y0, x1, y1] (None: the one default window
    [0, 0, num_bins - 1, num_bins - 1]); char_windows: one [c0, c1] per window, or a single [c0, c1] for all of them (None: the default
    [0, len(args.chars)] of engine/val.py:26)."""
    nb, nc = int(args.num_bins), len(args.chars)
    if windows is None:
        windows = [default_window(args)]
    windows = [list(w) for w in windows]
    if not windows:
        raise ValueError('window_prompts: at least one window')
    if len(windows) > MAX_WINDOWS:
        raise ValueError('window_prompts: at most %d windows per image (got %d)' % (MAX_WINDOWS, len(windows)))
    if char_windows is not None and not args.use_char_window_prompt:
        raise ValueError('window_prompts: char_windows needs args.use_char_window_prompt (the prompt has no character tokens otherwise)')
    for w in windows:
        if len(w) != 4 or any(int(v) != v for v in w):
            raise ValueError('window_prompts: a window is four integer bins [x0, y0, x1, y1], got %r' % (w,))
        x0, y0, x1, y1 = (int(v) for v in w)
        if min(x0, y0, x1, y1) < 0 or max(x0, y0, x1, y1) > nb - 1:
            raise ValueError('window_prompts: window %r leaves the bins [0, %d]' % (w, nb - 1))
        if x0 > x1 or y0 > y1:
            raise ValueError('window_prompts: window %r has x0 > x1 or y0 > y1' % (w,))
    rows = [[int(v) for v in w] for w in windows]
    if args.use_char_window_prompt:
        if char_windows is None:
            cw = [[0, nc]] * len(rows)
        else:
            cw = [list(c) for c in char_windows] if len(char_windows) and isinstance(char_windows[0], (list, tuple)) else [list(char_windows)]
            if len(cw) == 1:
                cw = cw * len(rows)
            if len(cw) != len(rows):
                raise ValueError('window_prompts: %d char_windows for %d windows' % (len(cw), len(rows)))
        for c in cw:
            if len(c) != 2 or any(int(v) != v for v in c):
                raise ValueError('window_prompts: a character window is two integers [c0, c1], got %r' % (c,))
            c0, c1 = int(c[0]), int(c[1])
            if c0 > c1 or c0 < 0 or c1 > nc:
                raise ValueError('window_prompts: character window %r is not an ordered pair inside [0, %d]' % (c, nc))
        rows = [r + [nb + int(c[0]), nb + int(c[1])] for r, c in zip(rows, cw)]
    return torch.tensor([r + [int(args.pt_sos_index)] for r in rows], dtype=torch.int64)


def resolve_windows(windows, n_images, grid=None, num_bins=None):
    """`windows=` / `grid=` as the engine entry points take them -> one window list per image, or None when neither is given.
    windows: a list of windows shared by all images, or a list of n_images window lists."""
    if grid is not None:
        if windows is not None:
            raise ValueError('give windows= or grid=, not both')
        windows = grid_windows(grid[0], grid[1], num_bins)
    if windows is None:
        return None
    windows = list(windows)
    if not windows:
        raise ValueError('windows: at least one window')
    first = windows[0]
    per_image = len(first) > 0 and isinstance(first[0], (list, tuple))
    if not per_image:
        return [[list(w) for w in windows] for _ in range(n_images)]
    if len(windows) != n_images:
        raise ValueError('windows: %d window lists for %d images' % (len(windows), n_images))
    return [[list(w) for w in ws] for ws in windows]


def resolve_char_windows(char_windows, per_image):
    """char_windows= beside resolve_windows' result: None, one [c0, c1] for every window, a list with one pair per window shared by
    all images, or one such list per image -> one list (or None) per image"""
    if char_windows is None:
        return [None] * len(per_image)
    cw = list(char_windows)
    if cw and not isinstance(cw[0], (list, tuple)):
        return [[list(cw)] * len(ws) for ws in per_image]
    if cw and cw[0] and isinstance(cw[0][0], (list, tuple)):
        if len(cw) != len(per_image):
            raise ValueError('char_windows: %d lists for %d images' % (len(cw), len(per_image)))
        return [[list(c) for c in one] for one in cw]
    return [[list(c) for c in cw] for _ in per_image]


def gather_points_cpu(seq, finished, lengths, n_prompt, sampled, clip=False):
    """numpy specification of omp_window_points.  seq int [rows, seq_ld]: the point phase's token buffer, row r = its prompt
    (seq[r, 0:4] is the row's window) followed by the sampled tokens; finished / lengths [rows]: the sampling kernels' EOS flag and, for
    a finished row, the position of its EOS; sampled: sampling steps executed.
    Row r's tokens are seq[r, n_prompt:end], end = lengths[r] if finished[r] else n_prompt + sampled (clamped into [n_prompt, seq_ld]),
    an odd tail dropped (reference transformer.py:138-139), read as (x, y) pairs.  clip=True keeps a pair only under the reference's
    membership rule, verbatim from collate_fn.py:80-81:  x > x0 and x <= x1 and y > y0 and y <= y1.  The lower bounds are STRICT, so
    under the default window [0, 0, nb - 1, nb - 1] the rule drops bin 0 as well -- which is why clip is off by default.
    -> points int32 [R, 2] (row order, inside a row the decoder's order: a stable compaction), inst_row int32 [R] (the row of every
       point), row_count int32 [rows] (points kept per row), dropped int32 [rows] (pairs the clip removed)"""
    seq = np.asarray(seq)
    finished, lengths = np.asarray(finished).reshape(-1), np.asarray(lengths).reshape(-1)
    rows, ld = seq.shape
    n_prompt, sampled = int(n_prompt), int(sampled)
    if clip and n_prompt < 4:
        raise ValueError('gather_points_cpu: clip reads the window from seq[r, 0:4]: n_prompt >= 4')
    pts, owner = [], []
    row_count, dropped = np.zeros(rows, np.int32), np.zeros(rows, np.int32)
    for r in range(rows):
        end = int(lengths[r]) if finished[r] else n_prompt + sampled
        end = min(max(end, n_prompt), ld)
        pairs = seq[r, n_prompt:n_prompt + (end - n_prompt) // 2 * 2].reshape(-1, 2)
        if clip:
            x0, y0, x1, y1 = (int(v) for v in seq[r, 0:4])
            keep = (pairs[:, 0] > x0) & (pairs[:, 0] <= x1) & (pairs[:, 1] > y0) & (pairs[:, 1] <= y1)
            dropped[r] = int((~keep).sum())
            pairs = pairs[keep]
        row_count[r] = pairs.shape[0]
        pts.append(pairs)
        owner.append(np.full(pairs.shape[0], r, np.int32))
    points = np.concatenate(pts, 0).astype(np.int32).reshape(-1, 2) if pts else np.zeros((0, 2), np.int32)
    inst_row = np.concatenate(owner, 0).astype(np.int32) if owner else np.zeros(0, np.int32)
    return points, inst_row, row_count, dropped
