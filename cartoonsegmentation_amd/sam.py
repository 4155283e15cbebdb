"""Segment Anything with box prompts on libcsm355 -- what the reference's `detector: sam` path reaches through `from sam import apply_sam`
(anime_3dkenburns/kenburns_effect.py:848-860; the module itself is not vendored there).  Restated from the published definition:
segment_anything's `SamPredictor.set_image` + `predict(box=..., multimask_output=False)`, one image embedding for all boxes of an image.

Everything runs on the device: csm_sam_preprocess (BGR uint8 -> RGB, longest side to the model size, normalise, zero-pad), the encoder
program (nets/sam.py: build_sam_encoder), csm_sam_box_tokens, the decoder program with the box as its batch dimension, and
csm_sam_postprocess (low-res logits -> model size -> crop -> image size -> > 0).  Nothing goes to the host between them.

Deliberate difference to segment_anything [documented, DESIGN.md 4.18]: ResizeLongestSide.apply_image resizes the uint8 image through PIL
(antialiased, rounded back to uint8); here the resize is the float bilinear of align_corners=False with no rounding in between.
"""
import collections
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, f64, i32, ptr, stream_ptr
from .nets.sam import SamConfig, build_sam_decoder, build_sam_encoder, infer_config, prompt_constants
from .runtime import CompiledProgram
from .weights import StateDictWeights, SynthWeights

DEFAULT_CKPT = 'models/sam/sam_vit_h_4b8939.pth'


def resolve_ckpt(path=None):
    """config key `sam_ckpt`, overridden by env CSM_SAM_CKPT"""
    return os.environ.get('CSM_SAM_CKPT') or path or DEFAULT_CKPT


def load_sam_weights(path=None, synthetic=None):
    """-> (weight source, SamConfig): the checkpoint's state dict (vit_b / vit_l / vit_h inferred from its shapes), or closed-form
    SynthWeights('sam.') when the file is absent and CSM_SYNTHETIC_WEIGHTS=1 (preset from CSM_SAM_PRESET, default vit_h)"""
    path = resolve_ckpt(path)
    if os.path.exists(path):
        sd = torch.load(path, map_location='cpu', weights_only=False)
        return StateDictWeights(sd), infer_config(sd)
    synthetic = os.environ.get('CSM_SYNTHETIC_WEIGHTS', '0') == '1' if synthetic is None else synthetic
    if not synthetic and not str(path).startswith('synthetic'):
        raise FileNotFoundError("%s (set CSM_SAM_CKPT, or CSM_SYNTHETIC_WEIGHTS=1 for closed-form weights)" % path)
    return SynthWeights('sam.'), SamConfig(os.environ.get('CSM_SAM_PRESET', 'vit_h'))


class Sam:
    """SamPredictor-like: set_image(img) encodes once, predict_boxes(boxes) decodes any number of boxes against that embedding.

    One decoder program exists per batch size (the box is the batch dimension); the `max_programs` most recently used stay resident
    (default 4, env CSM_SAM_PROGRAM_CACHE), sharing one packed weight image.  A call with more boxes than fit the scratch budget
    (`scratch_bytes`, default 2 GiB, env CSM_SAM_SCRATCH_MB) runs in chunks; a box's result does not depend on the chunk it runs in."""

    def __init__(self, ws_or_path=None, device=None, cfg=None, max_programs=None, scratch_bytes=None):
        if not torch.cuda.is_available():
            raise _lib.CsmError("Sam needs an MI355X: libcsm355 has no CPU path")
        _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device in (None, 'cuda') else torch.device(device)
        if ws_or_path is None or isinstance(ws_or_path, (str, os.PathLike)):
            self.ws, found = load_sam_weights(ws_or_path)
            self.cfg = cfg or found
        else:
            self.ws = ws_or_path
            self.cfg = cfg or (infer_config(ws_or_path.sd) if isinstance(ws_or_path, StateDictWeights) else SamConfig('vit_h'))
        self.max_programs = max(1, int(max_programs if max_programs is not None else os.environ.get('CSM_SAM_PROGRAM_CACHE', '4')))
        self.scratch_bytes = int(scratch_bytes if scratch_bytes is not None else int(os.environ.get('CSM_SAM_SCRATCH_MB', '2048')) << 20)
        self._encoder, self._decoders, self._shared = None, collections.OrderedDict(), {}
        self._consts = torch.from_numpy(prompt_constants(self.ws, self.cfg)).to(self.device)
        self._per_box = None
        self._emb, self._size = None, None
        self.evictions = 0

    # ---- programs -------------------------------------------------------------------------------------------------------------------------
    def encoder(self):
        if self._encoder is None:
            self._encoder = CompiledProgram(build_sam_encoder(self.ws, self.cfg, 1), self.device)
        return self._encoder

    def decoder(self, n):
        if n in self._decoders:
            self._decoders.move_to_end(n)
            return self._decoders[n]
        while len(self._decoders) >= self.max_programs:
            self._decoders.popitem(last=False)
            self.evictions += 1
        if self.evictions:
            torch.cuda.current_stream(self.device).synchronize()     # (the evicted program may still be executing on this stream)
        self._decoders[n] = CompiledProgram(build_sam_decoder(self.ws, self.cfg, n), self.device, shared=self._shared)
        return self._decoders[n]

    def chunk_size(self, n):
        """boxes per decoder run under the scratch budget (at least one)"""
        if self._per_box is None:
            self._per_box = 4 * max(1, build_sam_decoder(self.ws, self.cfg, 1).workspace_floats)
        return max(1, min(n, self.scratch_bytes // self._per_box))

    # ---- SamPredictor surface --------------------------------------------------------------------------------------------------------
    def preprocess_shape(self, H, W):
        s = self.cfg.image / max(H, W)
        return int(H * s + 0.5), int(W * s + 0.5)                   # ResizeLongestSide.get_preprocess_shape

    def set_image(self, img):
        """img: uint8 BGR [H, W, 3], numpy or device tensor"""
        t = img.to(self.device) if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img)).to(self.device)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise _lib.CsmError("Sam.set_image: uint8 HxWx3 (BGR) expected")
        t = t.contiguous()
        H, W = int(t.shape[0]), int(t.shape[1])
        nh, nw = self.preprocess_shape(H, W)
        S = self.cfg.image
        x = torch.empty((1, 3, S, S), dtype=torch.float32, device=self.device)
        check(_lib.load().csm_sam_preprocess(ptr(t), i32(H), i32(W), i32(S), i32(nh), i32(nw), ptr(x), stream_ptr()), "sam_preprocess")
        self.set_prepared(x, (H, W))
        return self

    def set_prepared(self, x, size=None):
        """x: the model's input [1, 3, S, S] (normalised, padded) as a float32 device tensor; size = (H, W) of the original image"""
        S, g = self.cfg.image, self.cfg.grid
        if not x.is_cuda or x.dtype != torch.float32 or tuple(x.shape) != (1, 3, S, S):
            raise _lib.CsmError("Sam.set_prepared: float32 device tensor [1,3,%d,%d] expected" % (S, S))
        emb = torch.empty((1, self.cfg.out_chans, g, g), dtype=torch.float32, device=self.device)
        self.encoder().run(x.contiguous(), emb)
        self._emb, self._size = emb, tuple(size) if size is not None else (S, S)
        return emb

    def _boxes(self, boxes):
        if isinstance(boxes, torch.Tensor):
            b = boxes.to(device=self.device, dtype=torch.float32)
        else:
            b = torch.as_tensor(np.asarray(boxes, np.float32).reshape(-1, 4), device=self.device)
        return b.reshape(-1, 4).contiguous()

    def low_res(self, boxes, frame='image'):
        """-> (low-res logits of mask 0 [n, 4g, 4g], IoU predictions [n]) on the device.  frame='image': boxes in the original image's
        pixels (SamPredictor.predict); 'model': already in the model's input frame"""
        if self._emb is None:
            raise _lib.CsmError("Sam: set_image first")
        b = self._boxes(boxes)
        n, cfg = int(b.shape[0]), self.cfg
        L = 4 * cfg.grid
        low = torch.empty((n, 1, L, L), dtype=torch.float32, device=self.device)
        iou = torch.empty((n, cfg.mask_tokens, 1, 1), dtype=torch.float32, device=self.device)
        if n == 0:
            return low[:, 0], iou[:, 0, 0, 0]
        sx = sy = 1.0
        if frame == 'image':
            (H, W), (nh, nw) = self._size, self.preprocess_shape(*self._size)
            sx, sy = nw / W, nh / H                                                # ResizeLongestSide.apply_coords
        step = self.chunk_size(n)
        for s in range(0, n, step):
            m = min(step, n - s)
            tok = torch.empty((m, cfg.out_chans, cfg.n_tokens, 1), dtype=torch.float32, device=self.device)
            check(_lib.load().csm_sam_box_tokens(ptr(b[s:]), i32(m), f64(sx), f64(sy), i32(cfg.image), ptr(self._consts), i32(cfg.out_chans),
                                                 i32(1 + cfg.mask_tokens), ptr(tok), stream_ptr()), "sam_box_tokens")
            self.decoder(m).run(self._emb, tok, low[s:s + m], iou[s:s + m])
        return low[:, 0], iou[:, 0, 0, 0]

    def predict_boxes(self, boxes_xyxy):
        """boxes [n, 4] xyxy in image pixels (list, numpy or device tensor) -> (masks bool [n, H, W], IoU predictions float32 [n]), both on
        the device.  No boxes: empty results, nothing is launched."""
        if self._emb is None:
            raise _lib.CsmError("Sam: set_image first")
        H, W = self._size
        b = self._boxes(boxes_xyxy)
        n = int(b.shape[0])
        if n == 0:
            return torch.zeros((0, H, W), dtype=torch.bool, device=self.device), torch.zeros(0, dtype=torch.float32, device=self.device)
        low, iou = self.low_res(b)
        nh, nw = self.preprocess_shape(H, W)
        masks = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
        check(_lib.load().csm_sam_postprocess(ptr(low), i32(n), i32(low.shape[-1]), i32(self.cfg.image), i32(nh), i32(nw), i32(H), i32(W), ptr(masks),
                                              stream_ptr()), "sam_postprocess")
        return masks.view(torch.bool), iou.contiguous()


_default = None


def default_sam(path=None, device=None):
    """the process-wide predictor apply_sam uses (built on first use from `path` / CSM_SAM_CKPT / the default checkpoint)"""
    global _default
    if _default is None:
        _default = Sam(path, device)
    return _default


def apply_sam(img, boxes, to_numpy=True, sam=None):
    """the reference's `sam.apply_sam(img, bbox)`: img uint8 BGR [H, W, 3], boxes [[x0, y0, x1, y1], ...] -> masks bool [n, H, W]
    (numpy by default, as the reference consumes them; to_numpy=False keeps them on the device)"""
    sam = sam or default_sam()
    masks, _ = sam.set_image(img).predict_boxes(boxes)
    return masks.cpu().numpy() if to_numpy else masks
