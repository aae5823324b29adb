"""Ground-truth readers for engine/evaluate.py.  Both give, per image, a list of words
{'poly': [[x, y], ...] in image pixels (3 .. 16 vertices), 'text': str, 'dc': bool}; json and numpy only."""
import json
import os

from .scoring import bezier_polygon


def decode_rec(rec, chars):
    """the reference's transcription encoding (dataset/text_spotting.py): character indices, len(chars) = unknown, len(chars) + 1 =
    padding -> (text without the unknown characters, whether it held one)"""
    out, unknown = [], False
    for t in rec:
        t = int(t)
        if t > len(chars):
            break                       # padding: the word ends here
        if t == len(chars):
            unknown = True
            continue
        if t < 0:
            raise ValueError('negative character index %d in rec' % t)
        out.append(chars[t])
    return ''.join(out), unknown


def load_coco_bezier(anno_file, args, dc_unknown=True):
    """the reference's annotation layout: COCO JSON whose annotations carry `bezier_pts` (16 floats: two cubic Beziers, upper then
    lower), `rec` (args.rec_length character indices into args.chars) and `iscrowd`.
    -> (images, ground_truth): images = [{'id', 'file_name', 'height', 'width'}] in file order, ground_truth = per image the list of
    words.  iscrowd gives don't-care; with dc_unknown a word that holds the unknown index is don't-care too (its text cannot be
    spelled with args.chars)."""
    with open(anno_file) as f:
        doc = json.load(f)
    images = [dict(id=im['id'], file_name=im['file_name'], height=int(im['height']), width=int(im['width'])) for im in doc.get('images', [])]
    slot = {im['id']: k for k, im in enumerate(images)}
    gt = [[] for _ in images]
    for a in doc.get('annotations', []):
        if a['image_id'] not in slot:
            raise ValueError('annotation %r names image %r, which the file does not list' % (a.get('id'), a['image_id']))
        rec = list(a.get('rec', []))
        if len(rec) != int(args.rec_length):
            raise ValueError('annotation %r: rec holds %d indices, args.rec_length is %d' % (a.get('id'), len(rec), int(args.rec_length)))
        text, unknown = decode_rec(rec, args.chars)
        gt[slot[a['image_id']]].append(dict(poly=bezier_polygon(a['bezier_pts']).tolist(), text=text,
                                            dc=bool(a.get('iscrowd', 0)) or (bool(dc_unknown) and unknown)))
    return images, gt


def load_icdar_txt(path, points=None):
    """one image's ICDAR-style file: lines `x1,y1,...,xk,yk,transcription` with k = 3 .. 16 vertices; the transcription is everything
    after the last coordinate, commas included; `###` marks don't-care -> the list of words.  points=k fixes the number of vertices
    (ICDAR 2015: 4).  Without it the coordinates are the longest run of leading numbers that is even and leaves a field for the
    transcription, which reads `...,x4,y4,2019` and `...,x4,y4,1,000` correctly; a transcription of SEVERAL numeric fields needs
    points=."""
    words = []
    with open(path, encoding='utf-8-sig') as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip('\r\n')
            if not line.strip():
                continue
            parts = line.split(',')
            c = 0
            while c < len(parts) and c < 32 and _is_number(parts[c]):
                c += 1
            if points is not None:
                if c < 2 * int(points):
                    raise ValueError('%s:%d: expected %d vertices' % (path, ln, int(points)))
                c = 2 * int(points)
            else:
                c -= 1 if c == len(parts) else 0
                c -= c % 2
            if c < 6 or c > 32 or c >= len(parts):
                raise ValueError('%s:%d: expected x1,y1,...,xk,yk,transcription with 3 .. 16 vertices' % (path, ln))
            text = ','.join(parts[c:])
            words.append(dict(poly=[[float(parts[k]), float(parts[k + 1])] for k in range(0, c, 2)], text=text, dc=text == '###'))
    return words


def _is_number(field):
    try:
        float(field)
        return True
    except ValueError:
        return False


def load_icdar_dir(folder, file_names, points=None):
    """per image the words of <folder>/gt_<stem>.txt or <folder>/<stem>.txt"""
    out = []
    for name in file_names:
        stem = os.path.splitext(os.path.basename(name))[0]
        for cand in ('gt_%s.txt' % stem, '%s.txt' % stem):
            if os.path.exists(os.path.join(folder, cand)):
                out.append(load_icdar_txt(os.path.join(folder, cand), points))
                break
        else:
            raise FileNotFoundError('no ground truth for %s in %s' % (name, folder))
    return out
