"""numpy restatement of the instance-overlay contract: the box band, the float32 chain, the contours and the
line-width rule.  Written from the contract, not from the kernels; tests/test_overlay.py holds it against the reference's own picture
(tests/golden/pin_draw_instances.npz) and tests/test_gpu_overlay.py holds the device against it, byte for byte."""
import numpy as np

from cartoonsegmentation_amd.anime_instances import get_color as color        # the palette (data; pinned by the fixture's picture)


def line_width(H, W):
    return max(round((H + W + 3) / 2 * 0.003), 2)


def band(H, W, box, t):
    """bool [H,W]: the outline of the xywh box, t pixels thick"""
    x1, y1, x2, y2 = int(box[0]), int(box[1]), int(box[0]) + int(box[2]), int(box[1]) + int(box[3])
    a = t // 2
    b = t - a
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    outer = (xs >= x1 - a) & (xs <= x2 + a) & (ys >= y1 - a) & (ys <= y2 + a)
    inner = (xs >= x1 + b) & (xs <= x2 - b) & (ys >= y1 + b) & (ys <= y2 - b)
    return outer & ~inner


def contour(mask):
    """bool [H,W]: the mask's pixels with a 4-neighbour outside the mask or outside the frame"""
    m = np.pad(mask.astype(bool), 1)
    inside = m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
    return mask.astype(bool) & ~inside


def draw(img, masks, bboxes, colors=None, indices=None, draw_bbox=True, draw_ins_mask=True, draw_ins_contour=False, mask_alpha=0.75,
         line_width_=None):
    H, W = img.shape[:2]
    idx = list(range(len(masks))) if indices is None else list(indices)
    cols = [color(i) for i in idx] if colors is None else [tuple(int(v) for v in c) for c in colors]
    out = img.copy()
    if draw_bbox:
        t = line_width(H, W) if line_width_ is None else line_width_
        for i, c in zip(idx, cols):
            out[band(H, W, bboxes[i], t)] = c
    if draw_ins_mask:
        alpha = np.float32(mask_alpha)
        rest = np.float32(1) - alpha
        d = out.astype(np.float32)
        for i, c in zip(idx, cols):
            m = masks[i].astype(bool)
            d[m] = d[m] * rest + alpha * np.array(c, np.float32)        # float32 products, rounded one by one, then the sum
        out = d.astype(np.uint8)
    if draw_ins_contour:
        for i, c in zip(idx, cols):
            out[contour(masks[i])] = c
    return out
