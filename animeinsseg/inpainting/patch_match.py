"""Drop-in for the reference's animeinsseg/inpainting/patch_match.py (the libpatchmatch ctypes binding): the same names and
signatures, computed by the HIP PatchMatch of libcsm355 (cartoonsegmentation_amd.ops.patchmatch_inpaint; contract DESIGN.md
§4.5).  The result is deterministic for a given seed; it is not libpatchmatch's (no shared RNG state across calls, our pyramid,
distance and vote).  Importing this module loads no library."""
from typing import Optional, Union

import numpy as np
from PIL import Image

__all__ = ['set_random_seed', 'set_verbose', 'inpaint', 'inpaint_regularity']

_seed = 0
_verbose = False


def set_random_seed(seed: int):
    """the seed of the counter hash of every later inpaint call (libpatchmatch seeds libc rand(), whose state then advances)"""
    global _seed
    _seed = int(seed) & 0xFFFFFFFF


def set_verbose(verbose: bool):
    """accepted for the reference's interface; the device path prints nothing"""
    global _verbose
    _verbose = bool(verbose)


ImageLike = Union[np.ndarray, Image.Image]


def inpaint(image: ImageLike, mask: Optional[ImageLike] = None, *, global_mask: Optional[ImageLike] = None,
            patch_size: int = 15) -> np.ndarray:
    """PatchMatch inpainting (Barnes et al., SIGGRAPH 2009) of the 3-channel uint8 `image` where `mask` (1-channel uint8,
    non-zero = hole) is set; with mask=None the purely white pixels (255, 255, 255) are the holes.  `global_mask` (1-channel
    uint8): non-zero pixels never serve inside a source patch (our reading of the reference's "target mask of the output
    image").  Returns a new uint8 [H,W,3] array; known pixels are unchanged."""
    image, mask, global_mask = _checked_arguments(image, mask, global_mask)
    import torch
    from cartoonsegmentation_amd import ops
    dev = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None
    if dev is None:
        from cartoonsegmentation_amd._lib import CsmError
        raise CsmError("patch_match.inpaint needs a GPU: libcsm355 has no CPU path")
    gm = None if global_mask is None else torch.from_numpy(global_mask).to(dev)
    out = ops.patchmatch_inpaint(torch.from_numpy(image).to(dev), torch.from_numpy(mask).to(dev), gm, patch_size=patch_size,
                                 seed=_seed)
    return out.cpu().numpy()


def inpaint_regularity(image: ImageLike, mask: Optional[ImageLike], ijmap: np.ndarray, *, global_mask: Optional[ImageLike] = None,
                       patch_size: int = 15, guide_weight: float = 0.25) -> np.ndarray:
    raise NotImplementedError("patch_match.inpaint_regularity (libpatchmatch's ijmap-guided variant) is not built: no caller of "
                              "the reference uses it; inpaint() is")


def _checked_arguments(image, mask, global_mask):
    """inpaint's argument rules: PIL images or arrays; the image uint8 [H,W,3]; each mask uint8 [H,W] or [H,W,1], returned as
    [H,W,1]; mask=None marks the pixels equal to (255, 255, 255).  Anything else fails an assert, as the original binding does."""
    img = _as_array(image)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, "image must be uint8 [H,W,3]"
    hole = (img == 255).all(axis=-1).astype(np.uint8)[:, :, None] if mask is None else _mask_hw1(mask)
    return img, hole, None if global_mask is None else _mask_hw1(global_mask)


def _as_array(x):
    """a writable C-contiguous ndarray (a PIL image is copied)"""
    return np.array(x) if isinstance(x, Image.Image) else np.ascontiguousarray(x)


def _mask_hw1(m):
    a = _as_array(m)
    assert a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 1)), "a mask must be uint8 [H,W] or [H,W,1]"
    return a.reshape(a.shape[0], a.shape[1], 1)
