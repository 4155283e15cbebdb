"""Configurations and inputs shared by tests/test_sam.py, tests/test_gpu_sam.py and tests/golden/make_golden_sam.py (helper, not collected)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sam_tiny.npz')

# config A: 7 x 7 grid, window 3 (pads to 9), one global block, head dimension 32; decoder width 32 (8 heads: d = 4, cross-attention d = 2)
CFG_A = dict(embed=64, depth=3, heads=2, global_blocks=(1,), window=3, image=112, patch=16, out_chans=32, mlp_dim=128, dec_mlp=64, iou_hidden=32)
BOXES_A = [[10.0, 20.0, 70.0, 90.0], [30.5, 5.0, 100.0, 60.0]]
SEED_A = 1
# config B: one head (d = 64), window 4 on a 9 x 9 grid (pads to 12), three boxes, one degenerate (x0 == x1)
CFG_B = dict(CFG_A, heads=1, window=4, image=144)
BOXES_B = [[10.0, 20.0, 70.0, 90.0], [30.0, 5.0, 120.0, 60.0], [50.0, 40.0, 50.0, 100.0]]
SEED_B = 2

MEAN, STD = np.array([123.675, 116.28, 103.53]), np.array([58.395, 57.12, 57.375])


def image_u8(h, w, seed):
    """smooth uint8 BGR test image (blobs and a ramp: structure for the boxes to grab)"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        img[..., c] = 96 + 60 * np.sin(xx / (5.0 + 3 * c) + g.uniform(0, 6)) * np.cos(yy / (7.0 - c) + g.uniform(0, 6)) + 0.4 * (xx + yy)
    for _ in range(4):
        cy, cx, r = g.uniform(0.2, 0.8) * h, g.uniform(0.2, 0.8) * w, g.uniform(0.08, 0.2) * min(h, w)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += g.uniform(-80, 80, 3)
    return np.clip(img, 0, 255).astype(np.uint8)


def prepared(img_u8):
    """square uint8 BGR image of the model's size -> the model's input [1, 3, S, S] in float64 (RGB, normalised; no resize, no padding)"""
    return (((img_u8[..., ::-1].astype(np.float64) - MEAN) / STD).transpose(2, 0, 1))[None].copy()
