"""The seeded cases of the instance-overlay tests: case(name) -> (img uint8 [H,W,3], masks bool [n,H,W], boxes int32
[n,4] xywh, keywords of ops.draw_instances / overlay_restatement.draw)."""
import zlib

import numpy as np


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def frame(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def blobs(rng, n, H, W, keep=None):
    """n random rectangles-with-holes masks and boxes near them (some of them off the frame); keep = (y, x): a pixel every mask covers"""
    masks = np.zeros((n, H, W), bool)
    boxes = np.zeros((n, 4), np.int32)
    for i in range(n):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        y1, x1 = int(rng.integers(y0, H)) + 1, int(rng.integers(x0, W)) + 1
        if keep is not None:
            y0, x0, y1, x1 = min(y0, keep[0]), min(x0, keep[1]), max(y1, keep[0] + 1), max(x1, keep[1] + 1)
        masks[i, y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) < 0.8
        if keep is not None:
            masks[i, keep[0], keep[1]] = True
        boxes[i] = (x0 - int(rng.integers(0, 3)), y0 - int(rng.integers(0, 3)), x1 - x0 + int(rng.integers(0, 4)), y1 - y0 + int(rng.integers(0, 4)))
    return masks, boxes


def _basic(name, H, W, n, keep=None, **kw):
    rng = _rng(name)
    masks, boxes = blobs(rng, n, H, W, keep)
    return frame(rng, H, W), masks, boxes, kw


def _edges(name):
    """an all-empty and an all-set mask; boxes partly and wholly off the frame, of zero and negative width, smaller than the line"""
    rng = _rng(name)
    H, W = 33, 61
    masks, boxes = blobs(rng, 8, H, W)
    masks[0], masks[1] = False, True
    boxes[:] = [(-5, -4, 20, 12), (50, 25, 30, 30), (-40, -40, 10, 10), (200, 5, 10, 10), (30, 10, 0, 12), (12, 20, 9, 0), (40, 5, -3, 6),
                (20, 15, 2, 1)]
    return frame(rng, H, W), masks, boxes, {}


def _custom_colors(name):
    img, masks, boxes, _ = _basic(name, 33, 61, 6)
    return img, masks, boxes, {'colors': _rng(name + 'c').integers(0, 256, (6, 3), dtype=np.uint8)}


CASES = {
    '5x7': lambda nm: _basic(nm, 5, 7, 3),
    '33x61': lambda nm: _basic(nm, 33, 61, 9),
    '64x256-tiles': lambda nm: _basic(nm, 64, 256, 7),
    '70x130-depth100': lambda nm: _basic(nm, 70, 130, 100, keep=(35, 65), mask_alpha=0.4),
    '40x48-n300': lambda nm: _basic(nm, 40, 48, 300),
    'n0': lambda nm: _basic(nm, 17, 23, 0),
    'n1': lambda nm: _basic(nm, 17, 23, 1),
    'edges': _edges,
    'thick-line': lambda nm: {**dict(zip('imb', _edges(nm)[:3])), 'k': {'line_width': 9}},
    'reordered': lambda nm: _basic(nm, 33, 61, 9, indices=[8, 3, 0, 7, 1, 2, 6, 5, 4]),
    'subset': lambda nm: _basic(nm, 33, 61, 9, indices=[7, 2]),
    'repeat': lambda nm: _basic(nm, 33, 61, 9, indices=[1, 4, 1, 1, 30 % 9]),
    'no-indices': lambda nm: _basic(nm, 33, 61, 9, indices=[]),
    'colors': _custom_colors,
    'no-bbox': lambda nm: _basic(nm, 33, 61, 9, draw_bbox=False),
    'no-mask': lambda nm: _basic(nm, 33, 61, 9, draw_ins_mask=False),
    'contours': lambda nm: _basic(nm, 33, 61, 9, draw_ins_contour=True),
    'contours-only': lambda nm: _basic(nm, 70, 130, 40, draw_bbox=False, draw_ins_mask=False, draw_ins_contour=True),
    'line-1': lambda nm: _basic(nm, 33, 61, 9, line_width=1),
    '9x260-two-tiles-wide': lambda nm: _basic(nm, 9, 260, 40, draw_ins_contour=True),
}


def case(name):
    got = CASES[name](name)
    if isinstance(got, dict):
        return got['i'], got['m'], got['b'], got['k']
    return got
