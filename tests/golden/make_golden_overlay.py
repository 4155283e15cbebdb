#!/usr/bin/env python3
"""Generate tests/golden/pin_draw_instances.npz by EXECUTING the reference's own AnimeInstances.draw_instances(img, draw_bbox=False)
(animeinsseg/anime_instances.py:131-194; loaded through ref_loader.load_anime_instances()) on a 33 x 61 frame with 14 random masks
that overlap 12 deep or more: at alpha 0.75 the float32 chain first rounds (in its sum) at depth 9.  The product d * 0.25 is exact,
so this picture cannot tell a fused multiply-add; the depth-100 case at alpha 0.4 of tests/overlay_cases.py does.  The boxes
are not drawn: cv2.rectangle(LINE_AA) is not available and is [EXT].

Build container only (needs the reference tree).  Stored: the inputs and the reference's picture, data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

AnimeInstances = ref_loader.load_anime_instances()
H, W, N = 33, 61, 14


def inputs(seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    masks = rng.random((N, H, W)) < 0.3
    masks[:13, 8:25, 10:50] |= rng.random((13, 17, 40)) < 0.97
    masks[:, 16, 30] = True
    boxes = np.stack([rng.integers(0, 30, N), rng.integers(0, 15, N), rng.integers(1, 30, N), rng.integers(1, 15, N)], 1).astype(np.int32)
    return img, masks, boxes


img, masks, boxes = inputs(414)
assert int(masks.sum(0).max()) >= 12
inst = AnimeInstances(masks=masks.copy(), bboxes=boxes.copy(), scores=np.ones(N, np.float32))
drawn = inst.draw_instances(img.copy(), draw_bbox=False)
order = [9, 2, 13, 2, 0]
drawn_order = inst.draw_instances(img.copy(), draw_bbox=False, draw_indices=order)
assert drawn.dtype == np.uint8 and drawn.shape == img.shape
out = os.path.join(HERE, "pin_draw_instances.npz")
np.savez_compressed(out, img=img, masks=np.packbits(masks, axis=None), shape=np.array(masks.shape), boxes=boxes, drawn=drawn,
                    order=np.array(order), drawn_order=drawn_order)
print(out, os.path.getsize(out), "bytes; depth", int(masks.sum(0).max()))
