"""The end-to-end mask cases of tests/test_gpu_sam.py and the CPU premise test in tests/test_sam.py (helper, not collected): images whose
longest side is the height (90 x 70) and the width (64 x 112), so both get resized and padded; three boxes, one clipped by the border."""
import functools

import sam_cases as C
import sam_restatement as R
from cartoonsegmentation_amd.nets.sam import SamConfig, sam_param_shapes

CASES = [
    dict(name='90x70', h=90, w=70, img_seed=11, seed=5, boxes=[[5, 8, 40, 60], [20, 30, 69, 89], [-6, 50, 30, 95]]),
    dict(name='64x112', h=64, w=112, img_seed=12, seed=6, boxes=[[10, 5, 60, 50], [50, 20, 111, 63], [80, -4, 120, 30]]),
]


def config():
    return SamConfig(**C.CFG_A)


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = next(c for c in CASES if c['name'] == name)
    cfg = config()
    sd = R.random_state_dict(sam_param_shapes(cfg), case['seed'])
    return R.Model(sd, cfg).apply_sam(C.image_u8(case['h'], case['w'], case['img_seed']), case['boxes'])


def reference(case):
    """-> (float64 full-size logits [n, H, W], IoU [n]) of the restatement, computed once per case"""
    return _reference(case['name'])
