"""Drop-in surface of the reference's animeinsseg/models/animeseg_refine/__init__.py (anime-seg background removal):
    from animeinsseg.models.animeseg_refine import load_refinenet, get_mask, AnimeSegmentation
load_refinenet('animeseg') returns the ISNet-IS (ISNetDIS(in_ch=3)) as a device model; get_mask runs the letterbox, the net and the
resize back on the MI355X (csm_animeseg_prepare -> layer program -> csm_animeseg_mask).  fp32 throughout: get_mask's use_amp is
accepted and ignored."""
import numpy as np
import torch

from cartoonsegmentation_amd import _lib
from cartoonsegmentation_amd._lib import check, f32, i32, ptr, stream_ptr
from cartoonsegmentation_amd.nets import build_isnet
from cartoonsegmentation_amd.runtime import CompiledProgram
from cartoonsegmentation_amd.segmentation import ANIMESEG_CKPT, animeseg_size, load_animeseg_weights

__all__ = ['AnimeSegmentation', 'load_refinenet', 'get_mask', 'get_cutout']


class AnimeSegmentation:
    """inference part of the reference's AnimeSegmentation('isnet_is') (animeseg_refine/__init__.py:58-99): __call__(x) maps
    float [n,3,s,s] to sigmoid(d1) [n,1,s,s] (its forward; square inputs, as get_mask makes).  One compiled program per input shape, weights shared."""

    def __init__(self, ws, device):
        self.ws, self.device = ws, torch.device(device)
        self._programs, self._weights = {}, {}

    def eval(self):
        return self

    def to(self, device):
        if torch.device(device) != self.device:
            self.device, self._programs, self._weights = torch.device(device), {}, {}
        return self

    def logits(self, x):
        """d1 logits [n,1,s,s] of a float [n,3,s,s] device tensor"""
        n, c, h, w = (int(v) for v in x.shape)
        if c != 3:
            raise _lib.CsmError("ISNet-IS takes 3 input channels, got %d" % c)
        if (n, h, w) not in self._programs:
            self._programs[(n, h, w)] = CompiledProgram(build_isnet(self.ws, n, h, w, in_ch=3), self.device, shared=self._weights)
        y = torch.empty((n, 1, h, w), dtype=torch.float32, device=self.device)
        self._programs[(n, h, w)].run(x.to(self.device, torch.float32).contiguous(), y)
        return y

    def __call__(self, x):
        L = _lib.load()
        y = self.logits(x)
        n, _, s, w = (int(v) for v in y.shape)
        if s != w:
            raise _lib.CsmError("AnimeSegmentation takes square s x s inputs (get_mask's canvas), got %dx%d" % (s, w))
        p = torch.empty_like(y)
        for i in range(n):       # csm_animeseg_mask over the whole plane at its own size: the sigmoid of the get_mask tail
            check(L.csm_animeseg_mask(ptr(y[i]), i32(s), i32(s), i32(s), i32(s), i32(s), f32(0.5), ptr(p[i]), ptr(None), stream_ptr()),
                  "animeseg_mask")
        return p

    forward = __call__


def load_refinenet(refine_method='animeseg', device: str = None) -> AnimeSegmentation:
    """animeseg_refine/__init__.py:154-166.  'animeseg' loads models/anime-seg/isnetis.ckpt (any layout AnimeSegmentation.try_load
    accepts), or closed-form weights when the file is absent and CSM_SYNTHETIC_WEIGHTS=1."""
    import os
    if refine_method == 'refinenet_isnet':
        raise NotImplementedError("load_refinenet('refinenet_isnet') is not part of this surface: use AnimeInsSeg(refine_kwargs="
                                  "{'refine_method': 'refinenet_isnet'})")
    if refine_method != 'animeseg':
        raise NotImplementedError(refine_method)
    if not torch.cuda.is_available():
        raise _lib.CsmError("AnimeSegmentation needs an MI355X: libcsm355 has no CPU path")
    _lib.load()
    ws = load_animeseg_weights(ANIMESEG_CKPT, os.environ.get('CSM_SYNTHETIC_WEIGHTS', '0') == '1')
    return AnimeSegmentation(ws, device or 'cuda').eval()


def _probability(model, input_img, s, what):
    """get_mask's chain on the device: (the uint8 image [h0,w0,3], the foreground probability float32 [h0,w0]) as device tensors"""
    L = _lib.load()
    img = input_img if isinstance(input_img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(input_img))
    img = img.to(model.device).contiguous()
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise _lib.CsmError("%s expects a uint8 HxWx3 image" % what)
    h0, w0 = int(img.shape[0]), int(img.shape[1])
    h, w = animeseg_size(h0, w0, s)
    x = torch.empty((1, 3, s, s), dtype=torch.float32, device=model.device)
    check(L.csm_animeseg_prepare(ptr(img), i32(h0), i32(w0), i32(h), i32(w), i32(s), i32(0), ptr(x), stream_ptr()), "animeseg_prepare")
    logits = model.logits(x)
    prob = torch.empty((h0, w0), dtype=torch.float32, device=model.device)
    check(L.csm_animeseg_mask(ptr(logits), i32(s), i32(h), i32(w), i32(h0), i32(w0), f32(0.5), ptr(prob), ptr(None), stream_ptr()),
          "animeseg_mask")
    return img, prob


def get_mask(model, input_img, use_amp=True, s=640):
    """animeseg_refine/__init__.py:169-188: RGB u8 image [h0,w0,3] (numpy or tensor) -> foreground probability float32 numpy
    [h0,w0,1].  use_amp is ignored (fp32)."""
    return _probability(model, input_img, s, "get_mask")[1].cpu().numpy()[:, :, np.newaxis]


def get_cutout(model, input_img, use_amp=True, s=640):
    """anime-seg's "matted" output (the reference's commented-out `rst.png`, animeinsseg/__init__.py:115-116:
    concatenate((img, mask * 255), axis=2)): get_mask's chain with the probability kept on the device, then the image with the
    probability as its alpha.  Returns uint8 numpy [h0,w0,4]: the input's three channels in their order, then
    A = (uint8)(clamp(p, 0, 1) * 255), truncated as the reference's astype does; colour is zero wherever A is 0
    (ops.cutout_bgra with a float alpha plane).  use_amp is ignored (fp32)."""
    from cartoonsegmentation_amd import ops
    img, prob = _probability(model, input_img, s, "get_cutout")
    whole = torch.ones((1,) + tuple(prob.shape), dtype=torch.uint8, device=prob.device)
    return ops.cutout_bgra(img, whole, alpha=prob)[0].cpu().numpy()
