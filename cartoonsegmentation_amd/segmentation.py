"""AnimeInsSeg -- host-side mirror of animeinsseg/__init__.py::AnimeInsSeg (reference :185-708) on libcsm355.

Same constructor / infer() signature and result type (AnimeInstances), so run_segmentation.ipynb drops in.
Flow per image (reference :464-504, :447-462, :638-665), everything on the MI355X, masks never leave HBM:
  uint8 image --csm_det_preprocess--> RTMDet-Ins layer program --csm_det_decode--> csm_nms --csm_det_gather-->
  csm_maskhead_logits --> csm_mask_resize_threshold --> [ISNet refine: csm_refine_prepare_batch --> ISNet layer
  program --> csm_refine_threshold] --> AnimeInstances(masks bool [n,H,W], bboxes xywh int32, scores).
Equally sized frames share one detector run and ISNet batches, and their glue runs once for all frames: csm_nms_batch,
csm_det_masks_batch, csm_refine_prepare_many and one csm_refine_threshold per ISNet batch (CSM_SEG_GLUE_BATCH=0: item by item).
refine_method='animeseg' (reference :78-115, :623-630) instead runs the anime-seg ISNet-IS over the frame:
  csm_animeseg_prepare --> ISNetDIS(in_ch=3) layer program --> csm_animeseg_mask (fg) --> csm_animeseg_select (in place).
The reference makes 5 host<->device crossings per image; here the only syncs are the data-dependent counts.

Checkpoints: a real `rtmdetl_e60.ckpt` (mmdet state_dict + cfg text) and `refine_last.ckpt` import through
StateDictWeights; `ckpt="synthetic"` uses closed-form weights (no checkpoint exists in this container).
mmdet's pieces are restated from mmdet 3.3.0 (not vendored in the reference => parity unpinned).
"""
import ctypes
import json
import math
import os
from typing import List, Union

import numpy as np
import torch

from . import _lib
from ._lib import check, f32, i32, ptr, stream_ptr
from .anime_instances import AnimeInstances
from .nets import RTMDetConfig, build_isnet, build_rtmdet
from .runtime import CompiledProgram
from .weights import StateDictWeights, SynthWeights

VALID_REFINEMETHODS = {'refinenet_isnet', 'animeseg', 'none'}
ANIMESEG_CKPT = 'models/anime-seg/isnetis.ckpt'                 # animeinsseg/models/animeseg_refine/__init__.py:158


def rescale_size(h, w, scale):
    """mmcv.image.rescale_size for scale=(S,S): factor = min(long/max, short/min); int(x*f+0.5)"""
    long_e, short_e = max(scale), min(scale)
    f = min(long_e / max(h, w), short_e / min(h, w))
    return int(h * float(f) + 0.5), int(w * float(f) + 0.5)


def scaledown_size(h, w, max_size):
    """utils/io_utils.py:254-274 scaledown_maxsize size rule (never upsamples)"""
    r = max_size / max(h, w)
    if r < 1:
        if h > w:
            h, w = max_size, max(1, int(round(w * r)))
        else:
            w, h = max_size, max(1, int(round(h * r)))
    return h, w


def animeseg_size(h0, w0, s):
    """get_mask letterbox rule (animeinsseg/models/animeseg_refine/__init__.py:170-174): long side s, short side
    int(s * short / long) -- Python float division, then truncation."""
    if h0 > w0:
        h, w = s, int(s * w0 / h0)
    else:
        h, w = int(s * h0 / w0), s
    if h < 1 or w < 1:
        raise _lib.CsmError("animeseg refine: a %dx%d frame letterboxes to %dx%d at size %d (aspect ratio too extreme)" % (h0, w0, h, w, s))
    return h, w


def animeseg_state_dict(blob):
    """the three layouts AnimeSegmentation.try_load accepts (animeseg_refine/__init__.py:75-85) -> ISNetDIS parameter names:
    a Lightning checkpoint ('epoch' present, weights under 'state_dict'), a flat AnimeSegmentation state dict ('net.*' and
    'gt_encoder.*' keys), or a bare ISNetDIS state dict.  'net.' is stripped; the training-only gt_encoder is dropped."""
    sd = blob['state_dict'] if 'epoch' in blob else blob
    if any(k.startswith('net.') for k in sd):
        sd = {k[4:]: v for k, v in sd.items() if k.startswith('net.')}
    return sd


def load_animeseg_weights(ckpt=None, synthetic=False):
    """StateDictWeights of the anime-seg ISNet-IS checkpoint, or the closed-form SynthWeights('animeseg.') when the file is
    absent and synthetic weights are allowed"""
    ckpt = ckpt or ANIMESEG_CKPT
    if os.path.exists(ckpt):
        return StateDictWeights(animeseg_state_dict(torch.load(ckpt, map_location='cpu', weights_only=False)))
    if not synthetic:
        raise FileNotFoundError(ckpt)
    return SynthWeights('animeseg.')


def _parse_mm_cfg(text):
    """evaluate the mmengine config text stored in the checkpoint (animeinsseg/__init__.py:196-197) without
    mmengine: it is plain Python made of literals and dict(...) calls."""
    env = {'__builtins__': {}, 'dict': dict, 'list': list, 'tuple': tuple, 'True': True, 'False': False, 'None': None}
    loc = {}
    exec(text.replace('file_client_args', 'backend_args'), env, loc)   # noqa: S102 (checkpoint is as trusted as torch.load)
    return loc


def config_from_ckpt_cfg(cfg_text):
    loc = _parse_mm_cfg(cfg_text)
    m = loc['model']
    c = RTMDetConfig()
    bb, head = m.get('backbone', {}), m.get('bbox_head', {})
    c.deepen_factor, c.widen_factor = bb.get('deepen_factor', 1.0), bb.get('widen_factor', 1.0)
    c.expand_ratio = bb.get('expand_ratio', c.expand_ratio)
    c.num_classes = head.get('num_classes', 1)
    c.feat_channels = head.get('feat_channels', 256)
    c.stacked_convs = head.get('stacked_convs', 2)
    c.share_conv = head.get('share_conv', True)
    c.num_prototypes = head.get('num_prototypes', c.num_prototypes)
    c.dyconv_channels = head.get('dyconv_channels', c.dyconv_channels)
    c.num_dyconvs = head.get('num_dyconvs', c.num_dyconvs)
    ag = head.get('anchor_generator', {})
    c.strides = tuple(ag.get('strides', c.strides))
    # BatchNorm eps: a norm_cfg without `eps` means torch's default 1e-5; no norm_cfg at all means the mmdet class default
    # (CSPNeXt / CSPNeXtPAFPN: dict(type='BN', momentum=0.03, eps=0.001); RTMDetHead: dict(type='BN') -> 1e-5)
    c.bn_eps_backbone = bb['norm_cfg'].get('eps', 1e-5) if 'norm_cfg' in bb else 1e-3
    nk = m.get('neck', {})
    c.bn_eps_neck = nk['norm_cfg'].get('eps', 1e-5) if 'norm_cfg' in nk else 1e-3
    c.bn_eps_head = head['norm_cfg'].get('eps', 1e-5) if 'norm_cfg' in head else 1e-5
    dp = m.get('data_preprocessor', {})
    c.mean, c.std = tuple(dp.get('mean', c.mean)), tuple(dp.get('std', c.std))
    t = m.get('test_cfg', {})
    c.nms_pre, c.score_thr = t.get('nms_pre', c.nms_pre), t.get('score_thr', c.score_thr)
    c.nms_iou = t.get('nms', {}).get('iou_threshold', c.nms_iou)
    c.max_per_img, c.mask_thr_binary = t.get('max_per_img', c.max_per_img), t.get('mask_thr_binary', c.mask_thr_binary)
    c.min_bbox_size = t.get('min_bbox_size', c.min_bbox_size)
    return c


def coco_image_paths(json_path, val_dir=None):
    """the part of pycocotools.COCO that _infer_save_annotations uses (reference :523-537): getImgIds() = the ids of `images` in
    first-insertion order (a later entry with the same id replaces the earlier one), loadImgs(id)[0]['file_name'].  Returns the
    image paths under val_dir (default: dirname(dirname(json_path))/val) and {path: image id}."""
    with open(json_path, 'r') as f:
        dataset = json.load(f)
    metas = {}
    for im in dataset.get('images', []):
        metas[im['id']] = im
    if val_dir is None:
        val_dir = os.path.join(os.path.dirname(os.path.dirname(json_path)), 'val')
    paths, ids = [], {}
    for iid, meta in metas.items():
        p = os.path.join(val_dir, meta['file_name'])
        ids[p] = iid
        paths.append(p)
    return paths, ids


class AnimeInsSeg:
    def __init__(self, ckpt: str, default_det_size: int = 640, device: str = None,
                 refine_kwargs: dict = {'refine_method': 'refinenet_isnet'},
                 tagger_path: str = 'models/wd-v1-4-swinv2-tagger-v2/model.onnx', mask_thr=0.3):
        if device is None:
            device = 'cuda'
        if not torch.cuda.is_available():
            raise _lib.CsmError("AnimeInsSeg needs an MI355X: libcsm355 has no CPU path")
        _lib.load()
        self.device = torch.device(device if device != 'cuda' else 'cuda:%d' % torch.cuda.current_device())
        self.ckpt, self.default_det_size, self.mask_thr = ckpt, default_det_size, mask_thr
        self.tagger, self.tagger_path = None, tagger_path
        if ckpt is None or str(ckpt).startswith('synthetic'):
            self.cfg, self._det_ws = RTMDetConfig(), SynthWeights('rtmdet.')
        else:
            blob = torch.load(ckpt, map_location='cpu', weights_only=False)
            self.cfg = config_from_ckpt_cfg(blob['meta']['cfg'])
            self._det_ws = StateDictWeights(blob['state_dict'])
        self._det_programs, self._det_weights = {}, {}          # (weights: packed images on the device by packing signature)
        self._refine_programs, self._refine_weights, self._refine_ws = {}, {}, None
        self._animeseg_programs, self._animeseg_weights, self._animeseg_ws = {}, {}, None
        self.refine_method = None
        self.refine_batch = int(os.environ.get('CSM_REFINE_BATCH', '16'))   # instances per ISNet run when frames are batched
        self.det_batch = max(1, int(os.environ.get('CSM_DET_BATCH', '16')))  # frames per detector run (longer lists are chunked)
        # the per-instance / per-frame glue of equally sized frames as a handful of native launches (csm_nms_batch, csm_det_masks_batch,
        # csm_refine_prepare_many, one csm_refine_threshold per ISNet chunk); 0 = the per-item calls (same bits: the A/B switch)
        self.seg_glue_batch = os.environ.get('CSM_SEG_GLUE_BATCH', '1') != '0'
        self.device_decode = os.environ.get('CSM_DEVICE_DECODE', '0') == '1'  # path inputs: baseline JPEG and 8-bit PNG files are decoded on the device
        self.set_refine_method(**(refine_kwargs or {'refine_method': 'none'}))

    # ---- configuration (reference :395-399, :623-636, :704-708) --------------------------------
    def set_detect_size(self, det_size: Union[int, tuple]):
        self.default_det_size = det_size if isinstance(det_size, int) else max(det_size)

    def set_refine_method(self, refine_method: str = 'none', refine_size: int = 720, refinenet_ckpt: str = None, **kw):
        if refine_method not in VALID_REFINEMETHODS:
            raise NotImplementedError('Invalid refine method: %s' % refine_method)
        self.refine_method, self.refine_size = refine_method, refine_size
        if refine_method == 'animeseg' and self._animeseg_ws is None:
            synthetic = str(self.ckpt).startswith('synthetic') or os.environ.get('CSM_SYNTHETIC_WEIGHTS', '0') == '1'
            self._animeseg_ws = load_animeseg_weights(refinenet_ckpt, synthetic)
        if refine_method == 'refinenet_isnet' and self._refine_ws is None:
            refinenet_ckpt = refinenet_ckpt or 'models/AnimeInstanceSegmentation/refine_last.ckpt'   # utils/constants.py:80
            synthetic = str(self.ckpt).startswith('synthetic') or os.environ.get('CSM_SYNTHETIC_WEIGHTS', '0') == '1'
            if not os.path.exists(refinenet_ckpt) and not synthetic:
                raise FileNotFoundError(refinenet_ckpt)
            if os.path.exists(refinenet_ckpt):
                sd = torch.load(refinenet_ckpt, map_location='cpu', weights_only=False)
                sd = sd.get('state_dict', sd)
                self._refine_ws = StateDictWeights({k.replace('net.', '', 1) if k.startswith('net.') else k: v for k, v in sd.items()})
            else:
                self._refine_ws = SynthWeights('isnet.')

    def set_mask_threshold(self, mask_thr: float):
        self.cfg.mask_thr_binary = mask_thr

    def set_max_instance(self, num_ins):
        self.cfg.max_per_img = num_ins

    # ---- compiled programs ----------------------------------------------------------------------
    def _detector(self, S, n=1):
        if (S, n) not in self._det_programs:
            rp, _ = build_rtmdet(self._det_ws, n, S, S, self.cfg)
            cp = CompiledProgram(rp.prog, self.device, shared=self._det_weights)     # (shared between shapes only where the packing is the same)
            self._det_programs[(S, n)] = (rp, cp)
        return self._det_programs[(S, n)]

    def _refiner(self, n, T):
        if (n, T) not in self._refine_programs:
            prog = build_isnet(self._refine_ws, n, T, T)
            cp = CompiledProgram(prog, self.device, shared=self._refine_weights)
            self._refine_programs[(n, T)] = cp
        return self._refine_programs[(n, T)]

    def _animeseg_net(self, n, s):
        """ISNet-IS (ISNetDIS(in_ch=3)) program for a batch of n letterboxed s x s frames"""
        if (n, s) not in self._animeseg_programs:
            prog = build_isnet(self._animeseg_ws, n, s, s, in_ch=3)
            self._animeseg_programs[(n, s)] = CompiledProgram(prog, self.device, shared=self._animeseg_weights)
        return self._animeseg_programs[(n, s)]

    # ---- public entry (reference :401-445) --------------------------------------------------------
    def infer(self, imgs, pred_score_thr: float = 0.3, refine_kwargs: dict = None, output_type: str = "tensor",
              det_size: int = None, save_dir: str = '', save_visualization: bool = False, save_annotation: str = '',
              infer_tags: bool = False, obj_id_start: int = -1, img_id_start: int = -1, verbose: bool = False,
              infer_grey: bool = False, save_mask_only: bool = False, val_dir=None, max_instances: int = 100, **kw):
        if det_size is not None:
            self.set_detect_size(det_size)
        if refine_kwargs is not None:
            self.set_refine_method(**refine_kwargs)
        self.set_max_instance(max_instances)
        if save_visualization or infer_tags:
            raise NotImplementedError("infer() does not draw or tag (SURVEY 2.1); pictures are written by save_visualization(out_file, img, "
                                      "instances) and _infer_save_annotations(..., save_visualization_only=True)")
        if isinstance(imgs, str) and imgs.endswith('.txt'):         # reference :437-439: a list of image paths
            from utils.io_utils import read_imglst_from_txt
            imgs = read_imglst_from_txt(imgs)
        if save_annotation:                                         # reference :441-443 (save_mask_only is not forwarded there)
            return self._infer_save_annotations(imgs, pred_score_thr, save_dir, save_annotation, obj_id_start, img_id_start, val_dir)
        assert output_type in {'tensor', 'numpy'}
        return_list = isinstance(imgs, list)
        if isinstance(imgs, str):                                 # prepare_data_pipeline, reference :667-693: a directory or one file
            if os.path.isdir(imgs):
                from utils.io_utils import find_all_imgs
                imgs, return_list = find_all_imgs(imgs, abs_path=True), True
            elif imgs.endswith('.json'):
                raise NotImplementedError("COCO files are read by the annotation export only (infer(..., save_annotation=path))")
        imgs = imgs if return_list else [imgs]
        insts = self._infer_frames(imgs, pred_score_thr)
        if output_type == 'numpy':
            for inst in insts:
                inst.to_numpy()
        return insts if return_list else insts[0]

    def _infer_frames(self, imgs, pred_score_thr):
        """detector + refine of a list of images (paths or BGR arrays) -> AnimeInstances with device masks"""
        if any(isinstance(im, str) for im in imgs):               # single_image_preprocess, reference :62-64: mmcv.imread(path)
            imgs = self._load(imgs)
        same = len(imgs) > 1 and all(tuple(im.shape) == tuple(imgs[0].shape) for im in imgs)
        if same:            # equally sized frames: one batched detector run + refine batches shared across frames
            dets = self.detect_raw_batch(imgs)
            insts = self._instances_from_run(dets, pred_score_thr) if self.seg_glue_batch else None
            if insts is None:
                insts = [self._instances_from(d, pred_score_thr) for d in dets]
            if self.refine_method == 'refinenet_isnet':
                self._refine_many(list(zip(insts, imgs)), self.refine_size)
            elif self.refine_method == 'animeseg':
                self._animeseg_refine(list(zip(insts, imgs)), self.refine_size)
        else:
            insts = []
            for img in imgs:
                inst = self._det_forward(img, pred_score_thr)
                if self.refine_method == 'refinenet_isnet':
                    self._postprocess_refine(inst, img, refine_size=self.refine_size)
                elif self.refine_method == 'animeseg':
                    self._animeseg_refine([(inst, img)], self.refine_size)
                insts.append(inst)
        return insts

    def _load(self, imgs):
        """the path entries of `imgs` as images: imread (host, PIL), or with device_decode imread_device_many, one call per det_batch
        chunk (baseline JPEG and 8-bit PNG files are then decoded on the device, DESIGN.md §4.8 and §4.9, and with
        CSM_DEVICE_DECODE_WEBP=1 lossless WebP files as well, §4.15, and with CSM_DEVICE_DECODE_WEBP_LOSSY=1 beside it lossy ones,
        §4.16; every other file still goes through imread)"""
        from utils.io_utils import imread, imread_device_many
        if not self.device_decode:
            return [imread(im) if isinstance(im, str) else im for im in imgs]
        out = list(imgs)
        where = [i for i, im in enumerate(imgs) if isinstance(im, str)]
        for c0 in range(0, len(where), self.det_batch):
            part = where[c0:c0 + self.det_batch]
            for i, t in zip(part, imread_device_many([imgs[i] for i in part], self.device)):
                out[i] = t
        return out

    # ---- COCO annotation export (reference :506-621, :667-693) -------------------------------------------
    def _infer_save_annotations(self, imgs, pred_score_thr, save_dir, save_annotation, obj_id_start, img_id_start, val_dir,
                                save_mask_only: bool = False, save_cutout_only: bool = False, save_visualization_only: bool = False):
        """infer every image and write the COCO instance-segmentation file `save_annotation`; returns None.  Frames run in chunks of
        det_batch (the batched detector / refine when a chunk's frames are equally sized); each chunk's masks are RLE-encoded on the
        device (ops.mask_rle_encode) and released before the next chunk, and no mask is copied to the host.

        save_mask_only (reference :597-598, :616): instead of the file, one 0 / 255 grey `mask_{ii:03d}_{img_name}.png` per instance
        in save_dir, PNG-encoded on the device (ops.png_encode); no JSON is written.  infer() does not forward it, as in the
        reference.

        save_cutout_only (the reference's commented-out `rst.png`, :115-116): instead of the file, one
        `cutout_{ii:03d}_{img_name}.webp` per instance in save_dir: the instance cut out of its frame with transparency, composed
        and coded as lossless WebP on the device from each chunk's device masks (AnimeInstances.save_cutouts); no
        JSON is written, and infer() does not forward it.

        save_visualization_only (the reference's save_visualization branch, :582-584): instead of the file, one picture per image,
        `save_dir/<img_name>` (the reference's out_file), the instances drawn over the frame and the file coded on the device
        (ops.draw_instances_many, one call per chunk; utils.io_utils.imwrite); no JSON is written, and infer() does
        not forward it.  A target that is the same file as its source image is a ValueError before anything is written."""
        from utils.constants import CATEGORIES
        from utils.io_utils import dict2json, find_all_imgs
        from . import ops
        imgp2ids = None
        if isinstance(imgs, str) and imgs.endswith('.json'):
            imgs, imgp2ids = coco_image_paths(imgs, val_dir)
        target_dir = './workspace/output'
        if isinstance(imgs, str):
            if os.path.isdir(imgs):
                target_dir, imgs = imgs, find_all_imgs(imgs, abs_path=True)
            elif os.path.isfile(imgs):
                target_dir, imgs = os.path.dirname(imgs), [imgs]
            else:
                raise FileNotFoundError(imgs)
        elif not isinstance(imgs, list):
            imgs = [imgs]
        if save_dir == '':
            save_dir = os.path.join(target_dir, os.path.basename(str(self.ckpt)).replace('.ckpt', '').replace('.pth', '').replace('.pt', ''))
        if save_visualization_only:
            for src in imgs:
                if isinstance(src, str) and os.path.realpath(os.path.join(save_dir, os.path.basename(src))) == os.path.realpath(src):
                    raise ValueError("save_visualization_only: %s would be overwritten by its own picture; choose another save_dir" % src)
        os.makedirs(save_dir, exist_ok=True)
        image_meta, det_annotations = [], []
        obj_id, image_id = obj_id_start + 1, img_id_start + 1
        for c0 in range(0, len(imgs), self.det_batch):
            chunk = imgs[c0:c0 + self.det_batch]
            frames = self._load(chunk)
            insts = self._infer_frames(frames, pred_score_thr)
            if save_visualization_only:
                from utils.io_utils import imwrite
                for k, (src, drawn) in enumerate(zip(chunk, ops.draw_instances_many(frames, insts))):
                    imwrite(drawn, os.path.join(save_dir, os.path.basename(src) if isinstance(src, str) else f'{c0 + k}'.zfill(12) + '.jpg'))
                continue
            for k, (src, frame, inst) in enumerate(zip(chunk, frames, insts)):
                img_name = os.path.basename(src) if isinstance(src, str) else f'{c0 + k}'.zfill(12) + '.jpg'
                if imgp2ids is not None:
                    image_id = imgp2ids[src]
                im_h, im_w = (int(v) for v in frame.shape[:2])
                image_meta.append({"id": image_id, "height": im_h, "width": im_w, "file_name": img_name})
                if save_cutout_only:
                    if not inst.is_empty:
                        inst.save_cutouts(frame, save_dir, img_name)
                elif save_mask_only:
                    if not inst.is_empty:
                        for j, data in enumerate(ops.png_encode(inst.masks.bool())):
                            with open(os.path.join(save_dir, 'mask_' + str(j).zfill(3) + '_' + img_name + '.png'), 'wb') as f:
                                f.write(data)
                elif not inst.is_empty:
                    counts, areas = ops.mask_rle_encode(inst.masks)
                    size = [int(inst.masks.shape[1]), int(inst.masks.shape[2])]         # the mask's shape, as the reference encodes it
                    scores = inst.scores.tolist()
                    bboxes = inst.bboxes.cpu().numpy().astype(np.float32).tolist()
                    for j in range(len(inst)):
                        det_annotations.append({'id': obj_id, 'category_id': 0, 'iscrowd': 0, 'score': float(scores[j]),
                                                'segmentation': {'size': size, 'counts': counts[j]}, 'image_id': image_id,
                                                'area': int(areas[j]), 'tag_string': inst.tags[j],
                                                'tag_string_character': inst.character_tags[j], 'bbox': bboxes[j]})
                        obj_id += 1
                image_id += 1
            del insts, frames
        if not (save_mask_only or save_cutout_only or save_visualization_only):
            dict2json({"info": {}, "licenses": [], "images": image_meta, "annotations": det_annotations, "categories": CATEGORIES},
                      save_annotation)
        return None

    def save_visualization(self, out_file: str, img, instances):
        """reference :696-698: the instances drawn over `img` (AnimeInstances.draw_instances(on_device=True)) written to out_file;
        drawn and coded on the device (AnimeInstances.save_visualization)"""
        return instances.save_visualization(img, out_file)

    # ---- detector forward + post-process (reference :447-462 + mmdet predict_by_feat) ---------------
    def _upload(self, img):
        if isinstance(img, torch.Tensor):
            t = img.to(self.device)
        else:
            t = torch.from_numpy(np.ascontiguousarray(img)).to(self.device)
        assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3, "expected uint8 HxWx3 (BGR)"
        return t.contiguous()

    def detect_raw(self, img):
        """returns dict with kept boxes/scores/kernels/priors (score-sorted, after NMS) + scale info"""
        return self.detect_raw_batch([img])[0]

    def detect_raw_batch(self, imgs):
        """MI355X addition: frames of equal size run through ONE detector program (batch n) -- the small feature maps
        of the head/neck then fill the chip.  Every op is per-sample; the only batch-size dependence is the host's split-K
        choice (csm_op.ksplit follows the total pixel count), i.e. fp32 summation grouping at the ulp level."""
        L, cfg = _lib.load(), self.cfg
        imgs_d = [self._upload(im) for im in imgs]
        H, W = int(imgs_d[0].shape[0]), int(imgs_d[0].shape[1])
        assert all(tuple(t.shape) == (H, W, 3) for t in imgs_d), "detect_raw_batch needs equally sized images"
        if len(imgs_d) > self.det_batch:
            # bounded workspace and a bounded set of compiled programs: full chunks of det_batch frames plus one remainder
            # program.  The prototype maps of earlier chunks are copied out (the next chunk overwrites the workspace).
            outs = []
            for c0 in range(0, len(imgs_d), self.det_batch):
                part = self.detect_raw_batch(imgs_d[c0:c0 + self.det_batch])
                if c0 + self.det_batch < len(imgs_d):
                    for d in part:
                        if d['n']:
                            d['mask_feat'] = d['cp'].view(d['rp'].mask_feat)[d['bi']][..., :cfg.num_prototypes].clone()
                outs += part
            return outs
        nb = len(imgs_d)
        S = self.default_det_size
        rh, rw = rescale_size(H, W, (S, S))
        w_scale, h_scale = rw / W, rh / H
        rp, cp = self._detector(S, nb)
        x = torch.empty((nb, 3, S, S), dtype=torch.float32, device=self.device)
        mean = (ctypes.c_float * 3)(*cfg.mean); std = (ctypes.c_float * 3)(*cfg.std)
        for bi, img_d in enumerate(imgs_d):
            check(L.csm_det_preprocess(ptr(img_d), i32(H), i32(W), i32(rh), i32(rw), i32(S), i32(S), mean, std,
                                       f32(cfg.pad_value), ptr(x[bi]), stream_ptr()), "det_preprocess")
        cp.run(x)
        return self._decode_batch(rp, cp, nb, H, W, S, rh, rw, w_scale, h_scale)

    def _decode_batch(self, rp, cp, nb, H, W, S, rh, rw, w_scale, h_scale):
        """mmdet RTMDetInsHead.predict_by_feat / _bbox_mask_post_process up to and including NMS, for all images of the batch, on the
        device with FIXED shapes and one host sync (csm_det_decode -> csm_nms -> csm_det_gather, csrc/detdecode.hip): instead of
        filtering (`scores > score_thr`, data-dependent sizes) invalid candidates carry score -1, which the stable descending sorts
        push behind every valid one; they cannot suppress a valid box in the greedy NMS (a box only suppresses lower-ranked ones) and
        are dropped at the end.  Same kept set and order as the filter-then-topk of the reference."""
        L, cfg, dev = _lib.load(), self.cfg, self.device
        nc, nl, G, M = cfg.num_classes, len(cfg.strides), cfg.num_gen_params, cfg.max_per_img
        if cfg.score_thr < 0:
            raise _lib.CsmError("score_thr must be >= 0 (scores are sigmoids; the device top-k orders their bit patterns)")

        def base(v):                                       # device address of the first element of an NHWC view in the workspace
            return cp.workspace.data_ptr() + 4 * (v.buf.offset + v.coff)
        vp = ctypes.c_void_p * nl
        cls_p, reg_p, ker_p = (vp(*[base(t[l]) for l in range(nl)]) for t in (rp.cls, rp.reg, rp.kern))
        level_hw = (ctypes.c_int * (2 * nl))(*[v for l in range(nl) for v in (rp.cls[l].h, rp.cls[l].w)])
        strides = (ctypes.c_int * nl)(*[int(s) for s in cfg.strides])
        lds3 = (ctypes.c_int * (3 * nl))(*[v for l in range(nl) for v in (rp.cls[l].buf.c, rp.reg[l].buf.c, rp.kern[l].buf.c)])
        slots = L.csm_det_decode_slots(level_hw, i32(nl), i32(nc), i32(cfg.nms_pre))
        if slots < 0:
            raise _lib.CsmError("detector decode: nms_pre <= 1024 and at most 4096 candidates per image are supported")
        K = min(slots, 4096)
        scores = torch.empty((nb, K), dtype=torch.float32, device=dev)
        boxes = torch.empty((nb, K, 4), dtype=torch.float32, device=dev)
        src = torch.empty((nb, K), dtype=torch.int32, device=dev)
        labels = torch.empty((nb, K), dtype=torch.int32, device=dev)
        offs = torch.empty((nb, K), dtype=torch.float32, device=dev) if nc > 1 else None
        scratch = torch.empty(L.csm_det_decode_scratch_bytes(i32(nb), i32(slots)), dtype=torch.uint8, device=dev)
        sfx, sfy = float(np.float32(1 / w_scale)), float(np.float32(1 / h_scale))                                      # rescale=True
        check(L.csm_det_decode(cls_p, reg_p, level_hw, strides, lds3, i32(nl), i32(nb), i32(nc), f32(cfg.score_thr), i32(cfg.nms_pre),
                               f32(rw), f32(rh), f32(sfx), f32(sfy), f32(cfg.min_bbox_size), i32(K), ptr(scores), ptr(boxes), ptr(src),
                               ptr(labels), ptr(offs), ptr(scratch), stream_ptr()), "det_decode")
        keep = torch.zeros((nb, M), dtype=torch.int32, device=dev)
        batched = self.seg_glue_batch
        if batched:
            # kept scores and kept counts share one block, so the host gets both in ONE read: [nb * M] float32, then [nb] int32
            read = torch.empty(nb * M + nb, dtype=torch.float32, device=dev)
            k_scores, nk = read[:nb * M].view(nb, M), read[nb * M:].view(torch.int32)
            nscr = torch.empty(L.csm_nms_batch_scratch_bytes(i32(nb), i32(K)), dtype=torch.uint8, device=dev)
            check(L.csm_nms_batch(ptr(boxes), ptr(offs), i32(nb), i32(K), f32(cfg.nms_iou), i32(M), ptr(keep), ptr(nk), ptr(nscr),
                                  stream_ptr()), "nms_batch")
        else:
            nk = torch.zeros(nb, dtype=torch.int32, device=dev)
            nscr = torch.empty(L.csm_nms_scratch_bytes(i32(K)), dtype=torch.uint8, device=dev)
            for bi in range(nb):
                check(L.csm_nms(ptr(boxes[bi]), ptr(None if offs is None else offs[bi]), i32(K), f32(cfg.nms_iou), i32(M),
                                ptr(keep[bi]), ptr(nk[bi:bi + 1]), ptr(nscr), stream_ptr()), "nms")
            k_scores = torch.empty((nb, M), dtype=torch.float32, device=dev)
        k_boxes = torch.empty((nb, M, 4), dtype=torch.float32, device=dev)
        k_labels = torch.empty((nb, M), dtype=torch.int32, device=dev)
        k_priors = torch.empty((nb, M, 4), dtype=torch.float32, device=dev)
        k_kernels = torch.empty((nb, M, G), dtype=torch.float32, device=dev)
        check(L.csm_det_gather(ker_p, level_hw, strides, lds3, i32(nl), i32(nb), i32(K), i32(M), i32(G), ptr(keep), ptr(scores), ptr(boxes),
                               ptr(src), ptr(labels), ptr(k_scores), ptr(k_boxes), ptr(k_labels), ptr(k_priors), ptr(k_kernels),
                               stream_ptr()), "det_gather")
        if batched:
            host = read.cpu().numpy()                                              # the one host sync (and host read) of the decode
            nk_h, ks_h = host[nb * M:].view(np.int32).tolist(), host[:nb * M].reshape(nb, M).tolist()
        else:
            nk_h, ks_h = nk.tolist(), k_scores.tolist()                            # the one host sync of the decode
        run = dict(nb=nb, M=M, boxes=k_boxes, scores=k_scores, priors=k_priors, kernels=k_kernels)    # the run's [nb, M, ...] blocks
        outs = []
        for bi in range(nb):
            n = sum(1 for j in range(nk_h[bi]) if ks_h[bi][j] > cfg.score_thr)    # valid ones come first in keep[]
            out = dict(H=H, W=W, S=S, rh=rh, rw=rw, w_scale=w_scale, h_scale=h_scale, rp=rp, cp=cp, bi=bi, n=n, run=run)
            if n:
                out.update(boxes=k_boxes[bi, :n], scores=k_scores[bi, :n], priors=k_priors[bi, :n], kernels=k_kernels[bi, :n],
                           labels=k_labels[bi, :n], scores_host=ks_h[bi][:n])
            outs.append(out)
        return outs

    def _masks_from(self, d, sel=None):
        """dynamic-conv mask head + resize + sigmoid + threshold -> uint8 [n,H,W] on device"""
        L, cfg = _lib.load(), self.cfg
        pri, ker = (d['priors'], d['kernels']) if sel is None else (d['priors'][sel].contiguous(), d['kernels'][sel].contiguous())
        n = int(pri.shape[0])
        mf, ld, h, w = self._mask_feat_of(d)
        logits = torch.empty((n, h, w), dtype=torch.float32, device=self.device)
        check(L.csm_maskhead_logits(ptr(mf), i32(ld), i32(h), i32(w), i32(cfg.num_prototypes), i32(cfg.dyconv_channels),
                                    ptr(ker), ptr(pri), i32(n), i32(cfg.strides[0]), ptr(logits), stream_ptr()), "maskhead")
        up = cfg.strides[0]
        # mmdet quirk kept: scale_factor = [1/w_scale, 1/h_scale] is applied as (height, width)
        rh2 = math.ceil(h * up * (1 / d['w_scale'])); rw2 = math.ceil(w * up * (1 / d['h_scale']))
        # `[..., :ori_h, :ori_w]` is a slice: for ~20 % of image shapes ceil(S / scale) is 1-2 px short of the original size and
        # mmdet returns masks that much smaller (the ISNet refine brings them back to (H, W); AnimeInstances.resize handles the rest)
        oh, ow = min(rh2, d['H']), min(rw2, d['W'])
        masks = torch.empty((n, oh, ow), dtype=torch.uint8, device=self.device)
        check(L.csm_mask_resize_threshold(ptr(logits), i32(n), i32(h), i32(w), i32(up), i32(rh2), i32(rw2), i32(oh),
                                          i32(ow), f32(cfg.mask_thr_binary), ptr(masks), stream_ptr()), "mask_resize")
        return masks

    @staticmethod
    def _mask_feat_of(d, mask_feat=None):
        """(tensor, channel pitch, h, w) of the prototype map a detection dict refers to: an owned NHWC copy when one was taken
        (infer_embeddings / chunked batches), else the live view inside the detector workspace (valid until the next run)"""
        mf = mask_feat if mask_feat is not None else d.get('mask_feat')
        if mf is not None:
            mf = mf.contiguous()
            return mf, int(mf.shape[2]), int(mf.shape[0]), int(mf.shape[1])
        v = d['rp'].mask_feat
        b = v.buf
        return d['cp'].workspace[b.offset + d.get('bi', 0) * v.h * v.w * b.c:], b.c, v.h, v.w

    def _det_forward(self, img, pred_score_thr: float = 0.3) -> AnimeInstances:
        return self._instances_from(self.detect_raw(img), pred_score_thr)

    def _instances_from(self, d, pred_score_thr: float = 0.3) -> AnimeInstances:
        if d['n'] == 0:
            return AnimeInstances()
        hs = d.get('scores_host')
        if hs is not None:                                                         # reference :452, decided from the synced copy
            idx = [j for j, v in enumerate(hs) if np.float32(v) > np.float32(pred_score_thr)]
            if not idx:
                return AnimeInstances()
            sel = torch.tensor(idx, dtype=torch.long, device=self.device)
        else:
            sel = (d['scores'] > pred_score_thr).nonzero()[:, 0]
            if sel.numel() < 1:
                return AnimeInstances()
        masks = self._masks_from(d, sel).bool()
        bboxes = d['boxes'][sel].to(torch.int32)                                   # :458-459 xyxy -> xywh (truncation)
        bboxes[:, 2:] -= bboxes[:, :2]
        return AnimeInstances(masks, bboxes, d['scores'][sel])

    def _instances_from_run(self, dets, pred_score_thr: float = 0.3):
        """_instances_from for all frames of ONE detector run in one native call (csm_det_masks_batch): every frame's masks are rows
        of one uint8 [sum n_k, oh, ow] block (handed out as bool views: the kernel writes 0 / 1 only), its boxes rows of one int32
        block, its scores a view of the run's kept scores.  The kept detections are in descending score order, so `> pred_score_thr`
        selects a prefix, whose length comes from the host copy of the scores.  Returns None (the caller then goes frame by frame)
        when the frames are not those of one run with the prototype maps still in the workspace, or a selection is not a prefix."""
        L, cfg = _lib.load(), self.cfg
        run = dets[0].get('run')
        if run is None or len(dets) != run['nb'] or any(d.get('run') is not run or d['bi'] != k or 'mask_feat' in d for k, d in enumerate(dets)):
            return None
        n_k = []
        for d in dets:
            idx = [j for j, v in enumerate(d['scores_host']) if np.float32(v) > np.float32(pred_score_thr)] if d['n'] else []
            if idx != list(range(len(idx))):
                return None
            n_k.append(len(idx))
        total = sum(n_k)
        if total == 0:
            return [AnimeInstances() for _ in dets]
        d0 = dets[0]
        v = d0['rp'].mask_feat
        b = v.buf
        feat = d0['cp'].workspace[b.offset:]                       # sample k's map: v.h * v.w * b.c floats per sample further on
        h, w, up = v.h, v.w, cfg.strides[0]
        rh2 = math.ceil(h * up * (1 / d0['w_scale'])); rw2 = math.ceil(w * up * (1 / d0['h_scale']))      # as in _masks_from
        oh, ow = min(rh2, d0['H']), min(rw2, d0['W'])
        logits = torch.empty((total, h, w), dtype=torch.float32, device=self.device)
        masks = torch.empty((total, oh, ow), dtype=torch.uint8, device=self.device)
        bboxes = torch.empty((total, 4), dtype=torch.int32, device=self.device)
        check(L.csm_det_masks_batch(ptr(feat), ctypes.c_int64(v.h * v.w * b.c), i32(b.c), i32(h), i32(w), i32(cfg.num_prototypes),
                                    i32(cfg.dyconv_channels), ptr(run['kernels']), ptr(run['priors']), ptr(run['boxes']), i32(run['nb']),
                                    i32(run['M']), (ctypes.c_int * len(n_k))(*n_k), i32(up), i32(up), i32(rh2), i32(rw2), i32(oh), i32(ow),
                                    f32(cfg.mask_thr_binary), ptr(logits), ptr(masks), ptr(bboxes), stream_ptr()), "det_masks_batch")
        insts, s = [], 0
        for k, n in enumerate(n_k):
            insts.append(AnimeInstances(masks[s:s + n].view(torch.bool), bboxes[s:s + n], run['scores'][k, :n]) if n else AnimeInstances())
            s += n
        return insts

    # ---- Web-UI helpers (reference :241-393): detector embeddings + box-prompted masks ---------------------
    def infer_embeddings(self, imgs, det_size=None):
        """reference :241-337: returns (img, instance_data, mask_feat) with the NMS'ed detections *before* mask
        generation; instance_data is a dict with bboxes [n,4] xyxy, scores, priors, kernels (+ internal handles)."""
        if det_size is not None:
            self.set_detect_size(det_size)
        img = imgs[0] if isinstance(imgs, list) else imgs
        d = self.detect_raw(img)
        if d['n'] == 0:
            d.update(boxes=torch.zeros((0, 4), device=self.device), scores=torch.zeros(0, device=self.device),
                     priors=torch.zeros((0, 4), device=self.device), kernels=torch.zeros((0, self.cfg.num_gen_params), device=self.device))
        d['bboxes'] = d['boxes']
        # an OWNED copy (the reference returns an owned tensor, animeinsseg/__init__.py:339-360): the detector workspace is
        # overwritten by the next infer()/detect_raw() of any image
        mask_feat = d['cp'].view(d['rp'].mask_feat)[d.get('bi', 0)][..., :self.cfg.num_prototypes].clone()
        d['mask_feat'] = mask_feat
        return img, d, mask_feat

    def segment_with_bboxes(self, img, bboxes, instance_data, mask_feat=None):
        """reference :339-393: for every query box (xyxy) pick the detection with the highest IoU, build its mask
        (x8 bilinear -> resize to [long_side, long_side] -> crop -> sigmoid > 0.5) and refine."""
        L, cfg, d = _lib.load(), self.cfg, instance_data
        if d['n'] == 0 or len(bboxes) == 0:
            return AnimeInstances()
        q = torch.as_tensor(np.asarray(bboxes), dtype=d['boxes'].dtype, device=self.device).view(-1, 4)
        t = d['boxes']
        lt, rb = torch.max(q[:, None, :2], t[None, :, :2]), torch.min(q[:, None, 2:], t[None, :, 2:])
        inter = (rb - lt).clamp(min=0).prod(2)
        area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])          # noqa: E731  torchvision box_iou
        iou = inter / (area(q)[:, None] + area(t)[None, :] - inter)
        idx = iou.argmax(1)
        H, W = d['H'], d['W']
        long_side = max(H, W)
        feat, ld, fh, fw = self._mask_feat_of(d, mask_feat)          # the caller's tensor, as in the reference
        n = int(idx.numel())
        logits = torch.empty((n, fh, fw), dtype=torch.float32, device=self.device)
        # named, so both gathers are alive when the kernel is enqueued: two temporaries in one argument list can be handed the SAME
        # block by the caching allocator (the first is released before the second is allocated)
        ker_sel, pri_sel = d['kernels'][idx].contiguous(), d['priors'][idx].contiguous()
        check(L.csm_maskhead_logits(ptr(feat), i32(ld), i32(fh), i32(fw), i32(cfg.num_prototypes), i32(cfg.dyconv_channels),
                                    ptr(ker_sel), ptr(pri_sel), i32(n), i32(cfg.strides[0]), ptr(logits), stream_ptr()), "maskhead")
        masks = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
        check(L.csm_mask_resize_threshold(ptr(logits), i32(n), i32(fh), i32(fw), i32(cfg.strides[0]), i32(long_side),
                                          i32(long_side), i32(H), i32(W), f32(0.5), ptr(masks), stream_ptr()), "mask_resize")
        bb = t[idx].to(torch.int32)
        bb[:, 2:] -= bb[:, :2]
        inst = AnimeInstances(masks.bool(), bb, d['scores'][idx])
        if self.refine_method == 'refinenet_isnet':
            self._postprocess_refine(inst, img, refine_size=self.refine_size)
        return inst

    def _refine_many(self, pairs, refine_size=720, max_batch=None):
        """ISNet refine of several (instances, image) pairs of equal image size with shared batches (per-sample results are
        those of _postprocess_refine; the reference's per-image limit of 4 only bounds its memory use)."""
        L = _lib.load()
        batched = self.seg_glue_batch
        jobs = []
        for inst, img in pairs:
            if inst.is_empty:
                continue
            img_d = self._upload(img)
            segs = inst.masks.to(self.device)
            if batched and segs.dtype == torch.bool and segs.is_contiguous():
                segs = segs.view(torch.uint8)                       # bool storage is 0 / 1 bytes: no copy
            else:
                segs = segs.to(torch.uint8).contiguous()
            jobs.append((inst, img_d, segs))
        if not jobs:
            return
        H, W = int(jobs[0][1].shape[0]), int(jobs[0][1].shape[1])
        T = refine_size
        rh, rw = scaledown_size(H, W, T)
        Hm, Wm = int(jobs[0][2].shape[1]), int(jobs[0][2].shape[2])       # equal image sizes => equal detector mask sizes
        rhm, rwm = scaledown_size(Hm, Wm, T)
        flat = [(j, k) for j, (_, _, segs) in enumerate(jobs) for k in range(segs.shape[0])]
        max_batch = max_batch or self.refine_batch
        if batched:
            # ONE output block for the step: `flat` is frame-major, so a chunk's outputs are consecutive rows and a frame's masks a
            # row range; per ISNet chunk one prepare launch (pointer tables) and one threshold launch
            block = torch.empty((len(flat), H, W), dtype=torch.uint8, device=self.device)
            for c0 in range(0, len(flat), max_batch):
                chunk = flat[c0:c0 + max_batch]
                b = len(chunk)
                cp = self._refiner(b, T)
                batch = torch.empty((b, 4, T, T), dtype=torch.float32, device=self.device)
                VP = ctypes.c_void_p * b
                check(L.csm_refine_prepare_many(VP(*[jobs[j][1].data_ptr() for j, _ in chunk]),
                                                VP(*[jobs[j][2].data_ptr() + k * Hm * Wm for j, k in chunk]), i32(b), i32(H), i32(W),
                                                i32(rh), i32(rw), i32(Hm), i32(Wm), i32(rhm), i32(rwm), i32(T), ptr(batch), stream_ptr()),
                      "refine_prepare_many")
                logits = torch.empty((b, 1, T, T), dtype=torch.float32, device=self.device)
                cp.run(batch, logits)
                check(L.csm_refine_threshold(ptr(logits), i32(b), i32(T), i32(T), i32(rh), i32(rw), i32(H), i32(W),
                                             f32(self.mask_thr), ptr(block[c0:c0 + b]), stream_ptr()), "refine_threshold")
            s = 0
            for inst, _, segs in jobs:
                inst.masks = block[s:s + segs.shape[0]].view(torch.bool)
                s += segs.shape[0]
            return
        outs = [torch.empty((segs.shape[0], H, W), dtype=torch.uint8, device=self.device) for _, _, segs in jobs]
        for c0 in range(0, len(flat), max_batch):
            chunk = flat[c0:c0 + max_batch]
            b = len(chunk)
            cp = self._refiner(b, T)
            batch = torch.empty((b, 4, T, T), dtype=torch.float32, device=self.device)
            for i, (j, k) in enumerate(chunk):
                check(L.csm_refine_prepare_batch(ptr(jobs[j][1]), ptr(jobs[j][2][k:k + 1]), i32(1), i32(H), i32(W), i32(rh), i32(rw),
                                                 i32(Hm), i32(Wm), i32(rhm), i32(rwm), i32(T), ptr(batch[i:i + 1]), stream_ptr()),
                      "refine_prepare")
            logits = torch.empty((b, 1, T, T), dtype=torch.float32, device=self.device)
            cp.run(batch, logits)
            for i, (j, k) in enumerate(chunk):
                check(L.csm_refine_threshold(ptr(logits[i:i + 1]), i32(1), i32(T), i32(T), i32(rh), i32(rw), i32(H), i32(W),
                                             f32(self.mask_thr), ptr(outs[j][k:k + 1]), stream_ptr()), "refine_threshold")
        for (inst, _, _), o in zip(jobs, outs):
            inst.masks = o.bool()

    # ---- ISNet refine (reference :638-665, :37-55) ---------------------------------------------------
    def _postprocess_refine(self, instances: AnimeInstances, img, refine_size: int = 720, max_refine_batch: int = 4, **kw):
        if instances.is_empty:
            return
        L = _lib.load()
        img_d = self._upload(img)
        H, W = int(img_d.shape[0]), int(img_d.shape[1])
        was_numpy = instances.is_numpy
        segs = (torch.from_numpy(instances.masks) if was_numpy else instances.masks).to(self.device).to(torch.uint8).contiguous()
        n, T = int(segs.shape[0]), refine_size
        rh, rw = scaledown_size(H, W, T)
        Hm, Wm = int(segs.shape[1]), int(segs.shape[2])
        rhm, rwm = scaledown_size(Hm, Wm, T)                       # resize_pad(seg): the seg's own shape (reference :47)
        out = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
        for k0 in range(0, n, max_refine_batch):
            b = min(max_refine_batch, n - k0)
            cp = self._refiner(b, T)
            batch = torch.empty((b, 4, T, T), dtype=torch.float32, device=self.device)
            check(L.csm_refine_prepare_batch(ptr(img_d), ptr(segs[k0:k0 + b]), i32(b), i32(H), i32(W), i32(rh), i32(rw), i32(Hm),
                                             i32(Wm), i32(rhm), i32(rwm), i32(T), ptr(batch), stream_ptr()), "refine_prepare")
            logits = torch.empty((b, 1, T, T), dtype=torch.float32, device=self.device)
            cp.run(batch, logits)
            check(L.csm_refine_threshold(ptr(logits), i32(b), i32(T), i32(T), i32(rh), i32(rw), i32(H), i32(W),
                                         f32(self.mask_thr), ptr(out[k0:k0 + b]), stream_ptr()), "refine_threshold")
        masks = out.bool()
        instances.masks = masks.cpu().numpy() if was_numpy else masks

    # ---- anime-seg refine (reference :78-115, :623-630; get_mask: animeseg_refine/__init__.py:169-188) ---------------------------
    def _animeseg_fg(self, imgs_d, s, bgr_to_rgb=True, thr=0.5, prob=False):
        """foreground of equally sized frames (u8 HWC on the device): one ISNet-IS batch of the letterboxed frames, then
        sigmoid -> crop -> resize back -> (> thr) per frame.  Returns u8 [n,H0,W0] (or the fp32 probabilities with prob=True)."""
        L = _lib.load()
        H0, W0 = int(imgs_d[0].shape[0]), int(imgs_d[0].shape[1])
        h, w = animeseg_size(H0, W0, s)
        n = len(imgs_d)
        out = torch.empty((n, H0, W0), dtype=torch.float32 if prob else torch.uint8, device=self.device)
        for c0 in range(0, n, self.refine_batch):
            chunk = imgs_d[c0:c0 + self.refine_batch]
            b = len(chunk)
            x = torch.empty((b, 3, s, s), dtype=torch.float32, device=self.device)
            for i, img_d in enumerate(chunk):
                check(L.csm_animeseg_prepare(ptr(img_d), i32(H0), i32(W0), i32(h), i32(w), i32(s), i32(1 if bgr_to_rgb else 0),
                                             ptr(x[i]), stream_ptr()), "animeseg_prepare")
            logits = torch.empty((b, 1, s, s), dtype=torch.float32, device=self.device)
            self._animeseg_net(b, s).run(x, logits)
            for i in range(b):
                o = out[c0 + i]
                check(L.csm_animeseg_mask(ptr(logits[i]), i32(s), i32(h), i32(w), i32(H0), i32(W0), f32(thr), ptr(o if prob else None),
                                          ptr(None if prob else o), stream_ptr()), "animeseg_mask")
        return out

    def _animeseg_refine(self, pairs, refine_size=720):
        """animeseg_refine for (instances, BGR image) pairs of equal image size, in place.  Frames without instances do not run the
        net (reference :81-83).  Masks stay in their container: a bool tensor on its device, or bool numpy."""
        L = _lib.load()
        jobs = [(inst, self._upload(img)) for inst, img in pairs if not inst.is_empty]
        if not jobs:
            return
        fg = self._animeseg_fg([img_d for _, img_d in jobs], refine_size)
        W0 = int(fg.shape[2])
        for (inst, _), f in zip(jobs, fg):
            was_numpy = inst.is_numpy
            src = torch.from_numpy(inst.masks) if was_numpy else inst.masks
            masks = src.to(self.device).to(torch.uint8).contiguous()
            k, Hm, Wm = (int(v) for v in masks.shape)
            if Hm > f.shape[0] or Wm > W0:
                raise _lib.CsmError("animeseg refine: %dx%d masks exceed the %dx%d frame" % (Hm, Wm, f.shape[0], W0))
            counts = torch.empty(2 * k, dtype=torch.int32, device=self.device)
            check(L.csm_animeseg_select(ptr(masks), i32(k), i32(Hm), i32(Wm), ptr(f), i32(W0), ptr(counts), stream_ptr()),
                  "animeseg_select")
            refined = masks.bool()
            inst.masks = refined.cpu().numpy() if was_numpy else refined.to(src.device)
