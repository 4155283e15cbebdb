"""Generator of tests/golden/sam_tiny.npz: transformers' SamModel in float64 at config A of tests/sam_cases.py, on the seeded unit-scale
weights of tests/sam_restatement.random_state_dict.  Numeric arrays only: the weights' seed, the input image, the boxes, SamModel's
low-res logits and IoU predictions.  Run from the repository root:  python tests/golden/make_golden_sam.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import sam_cases as C  # noqa: E402
import sam_restatement as R  # noqa: E402
from cartoonsegmentation_amd.nets.sam import SamConfig, sam_param_shapes  # noqa: E402

if __name__ == '__main__':
    cfg = SamConfig(**C.CFG_A)
    sd = R.random_state_dict(sam_param_shapes(cfg), C.SEED_A)
    img = C.image_u8(cfg.image, cfg.image, 7)
    low, iou = R.hf_forward(R.hf_model(cfg, sd), torch.as_tensor(C.prepared(img)), C.BOXES_A)
    np.savez_compressed(C.GOLDEN, seed=np.int64(C.SEED_A), image_u8=img, boxes=np.asarray(C.BOXES_A, np.float64),
                        low_res_logits=low.numpy(), iou=iou.numpy())
    print(C.GOLDEN, os.path.getsize(C.GOLDEN), float(np.abs(low.numpy()).max()))
