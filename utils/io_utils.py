"""reference utils/io_utils.py -- the image helpers on the hot path's edge: find_all_imgs (:92-103), scaledown_maxsize
(:254-274), resize_pad (:277-292), plus imread / imwrite (mmcv.imread / mmcv.imwrite stand-ins: the reference's callers decode and
encode with mmcv / cv2, which this image does not have; imwrite compresses on the MI355X, csrc/png.hip and csrc/mjpeg.hip).  The resamplers run on the MI355X (cv2's uint8 INTER_LINEAR arithmetic restated in imageops.hip).
The annotation helpers: NumpyEncoder / json2dict / dict2json (:24-47), mask2rle (:327-333; the RLE is built on the MI355X,
csrc/maskrle.hip) and read_imglst_from_txt (animeinsseg/__init__.py:179-183)."""
import json
import os
import os.path as osp
from pathlib import Path

import numpy as np

IMG_EXT = {'.bmp', '.jpg', '.png', '.jpeg'}


def find_all_imgs(img_dir, abs_path=False):
    out = []
    for filename in os.listdir(img_dir):
        if Path(filename).suffix.lower() not in IMG_EXT:
            continue
        out.append(osp.join(img_dir, filename) if abs_path else filename)
    return out


def imread(path):
    """uint8 BGR HxWx3 like mmcv.imread / cv2.imread(IMREAD_COLOR) (EXIF orientation applied, alpha dropped)"""
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        im = ImageOps.exif_transpose(im).convert('RGB')
        return np.ascontiguousarray(np.asarray(im)[:, :, ::-1])


def imread_device_many(paths, device=None, stats=None, progressive=None, webp=None, webp_lossy=None, gif=None):
    """imread for a list of paths with the pixels on the device: a list of uint8 BGR [H,W,3] tensors.  A .jpg / .jpeg file that the
    device decoder takes (cartoonsegmentation_amd.jpegcode.probe: baseline, Huffman, grey or Y Cb Cr at 4:4:4 / 4:2:2 / 4:2:0) and
    whose EXIF orientation is 1 or absent is decoded on the MI355X by ops.jpeg_decode, all such files in one call: only the file's
    bytes are uploaded.  A .png file that cartoonsegmentation_amd.pngread.probe accepts (8 bits per sample; grey, RGB, palette,
    grey + alpha or RGBA; not interlaced, not animated, no orientation) is decoded by ops.png_decode, again all such files in one
    call.  Every other file (BMP, progressive or rotated JPEG, 16-bit or interlaced PNG, ...) goes through imread and an upload.
    The device decodes follow the contracts of DESIGN.md §4.8 (JPEG) and §4.9 (PNG: equal to imread on every byte).  `stats` (a
    dict) receives 'jpeg', 'png' and 'host': the indices of the paths that took each route.

    progressive=True (None reads the environment variable CSM_DEVICE_DECODE_PROGRESSIVE, '1' = on; the default is off) also sends
    the progressive .jpg / .jpeg files that jpegcode.probe(data, progressive=True) accepts and whose orientation is 1 or absent to
    the device, in the same ops.jpeg_decode call as the baseline ones; rotated progressive files and scan scripts
    that the probe refuses stay with imread.  `stats` then also receives 'jpeg_progressive', the indices of those files, which are
    listed in 'jpeg' as well.

    webp=True (None reads the environment variable CSM_DEVICE_DECODE_WEBP, '1' = on; the default is off) also sends every .webp file
    that cartoonsegmentation_amd.webpread.probe accepts (lossless, not animated, orientation 1 or absent) to the device
    (ops.webp_decode, DESIGN.md §4.15: equal to imread on every byte), all such files in one call.  Lossy and animated files, and
    files with more prefix-code groups than the decoder's cap, stay with imread.  `stats` then also receives 'webp', the indices of
    the files decoded on the device.  With the option off nothing changes: a .webp path goes through imread.

    webp_lossy=True (None reads the environment variable CSM_DEVICE_DECODE_WEBP_LOSSY, '1' = on; the default is off) has an effect
    only together with the webp option: the lossy .webp files that webpread.probe(data, lossy=True) accepts (a VP8 key frame with or
    without an ALPH chunk, not animated, orientation 1 or absent) then go to the device as well (equal to imread on
    every byte), in the same ops.webp_decode call as the lossless ones.  `stats['webp']` lists them with the lossless files, and
    `stats` also receives 'webp_lossy', the indices of the lossy ones.  With the option off, routing and `stats` are unchanged.

    gif=True (None reads the environment variable CSM_DEVICE_DECODE_GIF, '1' = on; the default is off) also sends every .gif file
    that cartoonsegmentation_amd.gifread.probe accepts to the device (ops.gif_decode, DESIGN.md §4.17: equal on every byte to what
    PIL shows, which for the first frame is what imread returns), all such files in one call, and returns frame 0 of each.  `stats`
    then also receives 'gif', the indices of those files.  With the option off, routing and `stats` are unchanged."""
    import torch
    from cartoonsegmentation_amd import gifread, jpegcode, ops, pngread, webpread
    if gif is None:
        gif = os.environ.get('CSM_DEVICE_DECODE_GIF', '0') == '1'
    if webp is None:
        webp = os.environ.get('CSM_DEVICE_DECODE_WEBP', '0') == '1'
    if webp_lossy is None:
        webp_lossy = os.environ.get('CSM_DEVICE_DECODE_WEBP_LOSSY', '0') == '1'
    webp_lossy = bool(webp and webp_lossy)
    if progressive is None:
        progressive = os.environ.get('CSM_DEVICE_DECODE_PROGRESSIVE', '0') == '1'
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    out = [None] * len(paths)
    idx, datas, infos = [], [], []
    pidx, pdatas, pinfos = [], [], []
    widx, wdatas, winfos = [], [], []
    gidx, gdatas, ginfos = [], [], []
    host = []
    for i, path in enumerate(paths):
        suffix = Path(str(path)).suffix.lower()
        if suffix in ('.jpg', '.jpeg'):
            with open(path, 'rb') as f:
                data = f.read()
            try:
                info = jpegcode.probe(data, progressive=True) if progressive else jpegcode.probe(data)
            except jpegcode.Unsupported:
                info = None
            if info is not None and info['orientation'] in (None, 1):
                idx.append(i); datas.append(data); infos.append(info)
                continue
        elif suffix == '.png':
            with open(path, 'rb') as f:
                data = f.read()
            try:
                info = pngread.probe(data)
            except pngread.Unsupported:
                info = None
            if info is not None:
                pidx.append(i); pdatas.append(data); pinfos.append(info)
                continue
        elif suffix == '.webp' and webp:
            with open(path, 'rb') as f:
                data = f.read()
            try:
                info = webpread.probe(data, lossy=True) if webp_lossy else webpread.probe(data)
            except webpread.Unsupported:
                info = None
            if info is not None:
                widx.append(i); wdatas.append(data); winfos.append(info)
                continue
        elif suffix == '.gif' and gif:
            with open(path, 'rb') as f:
                data = f.read()
            try:
                info = gifread.probe(data)
            except gifread.Unsupported:
                info = None
            if info is not None:
                gidx.append(i); gdatas.append(data); ginfos.append(info)
                continue
        host.append(i)
        out[i] = torch.from_numpy(imread(path)).to(dev)
    if datas:
        for i, t in zip(idx, ops.jpeg_decode(datas, dev, _infos=infos, progressive=bool(progressive))):
            out[i] = t
    if pdatas:
        for i, t in zip(pidx, ops.png_decode(pdatas, dev, _infos=pinfos)):
            out[i] = t
    if gdatas:
        for i, t in zip(gidx, ops.gif_decode(gdatas, dev, _infos=ginfos)):
            out[i] = t[0]
    while wdatas:
        try:
            for i, t in zip(widx, ops.webp_decode(wdatas, dev, _infos=winfos, lossy=webp_lossy)):
                out[i] = t
            break
        except webpread.Unsupported as e:                          # files over the group cap: they go through imread, the rest again
            if not e.files:
                raise
            for j in sorted(e.files, reverse=True):
                i = widx.pop(j); wdatas.pop(j); winfos.pop(j)
                host.append(i)
                out[i] = torch.from_numpy(imread(paths[i])).to(dev)
            host.sort()
    if stats is not None:
        stats.update(jpeg=idx, png=pidx, host=host)
        if webp:
            stats['webp'] = widx
        if gif:
            stats['gif'] = gidx
        if webp_lossy:
            stats['webp_lossy'] = [i for i, info in zip(widx, winfos) if info['kind'] == 'lossy']
        if progressive:
            stats['jpeg_progressive'] = [i for i, info in zip(idx, infos) if info['progressive']]
    return out


def imread_device(path, device=None, progressive=None, webp=None, webp_lossy=None, gif=None):
    """imread with the pixels on the device: see imread_device_many"""
    return imread_device_many([path], device, progressive=progressive, webp=webp, webp_lossy=webp_lossy, gif=gif)[0]


def imwrite(img, file_path, auto_mkdir=True):
    """mmcv.imwrite / cv2.imwrite stand-in: `img` is a BGR [H,W,3] or grey [H,W] uint8 image, a numpy array (uploaded) or a device
    tensor; it is compressed on the MI355X and only the file's bytes reach the host.  .png: lossless (ops.png_encode); .jpg /
    .jpeg: ops.jpeg_encode at cv2's defaults (quality 95, 4:2:0; colour only); .webp: lossless WebP (ops.webp_encode_lossless),
    which alone also takes a B, G, R, A image [H,W,4] and writes its alpha.  Any other suffix raises ValueError.  Returns True."""
    suffix = Path(str(file_path)).suffix.lower()
    if suffix not in ('.png', '.jpg', '.jpeg', '.webp'):
        raise ValueError("imwrite: %r is not written here (.png, .jpg, .jpeg and .webp are)" % suffix)
    import torch
    from cartoonsegmentation_amd import ops
    t = img if isinstance(img, torch.Tensor) else torch.tensor(np.asarray(img)).cuda()
    if t.dim() == 3 and t.shape[2] == 1:
        t = t[:, :, 0]
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3 and not (suffix == '.webp' and t.shape[2] == 4)):
        raise ValueError("imwrite: an [H,W] or [H,W,3] image (for .webp also [H,W,4]) is expected (got shape %s)" % (tuple(t.shape),))
    if suffix == '.webp':
        data = ops.webp_encode_lossless([t])[0]
    elif suffix == '.png':
        data = ops.png_encode(t.unsqueeze(0), bgr=True)[0]
    else:
        if t.dim() == 2:
            raise ValueError("imwrite: the JPEG encoder takes colour images [H,W,3] only")
        data = ops.jpeg_encode(t, quality=95, subsampling='420')[0]
    if auto_mkdir:
        os.makedirs(osp.dirname(osp.abspath(str(file_path))), exist_ok=True)
    with open(file_path, 'wb') as f:
        f.write(data)
    return True


def scaledown_size(im_h, im_w, max_size, divisior=None):
    """the size rule of scaledown_maxsize (utils/io_utils.py:256-270)"""
    r = max_size / max(im_h, im_w)
    if r < 1:
        if im_h > im_w:
            im_h, im_w = max_size, max(1, int(round(im_w * r)))
        else:
            im_w, im_h = max_size, max(1, int(round(im_h * r)))
    if divisior is not None:
        im_w = int(np.ceil(im_w / divisior) * divisior)
        im_h = int(np.ceil(im_h / divisior) * divisior)
    return im_h, im_w


def scaledown_maxsize(img, max_size: int, divisior: int = None):
    """utils/io_utils.py:254-274: cv2.resize(INTER_LINEAR) so that max(h, w) <= max_size (never enlarges, except for the
    `divisior` round-up).  numpy in -> numpy out, device tensor in -> device tensor out."""
    import torch
    from cartoonsegmentation_amd import ops
    h0, w0 = img.shape[:2]
    h, w = scaledown_size(h0, w0, max_size, divisior)
    if (h, w) == (h0, w0):
        return img
    if isinstance(img, torch.Tensor):
        if img.dtype == torch.uint8:
            return ops.resize_u8_linear(img, h, w)
        return ops.resize_f32_linear(img.float(), h, w).to(img.dtype if img.is_floating_point() else torch.float32)
    if img.dtype == np.uint8:
        return ops.resize_u8_linear(torch.from_numpy(np.ascontiguousarray(img)).cuda(), h, w).cpu().numpy()
    if img.dtype == np.bool_:
        raise TypeError("scaledown_maxsize: cv2.resize does not take bool arrays either -- pass uint8 or float32 masks")
    # float masks / images (prepare_refine_batch calls resize_pad(seg, ...), animeinsseg/__init__.py:47): cv2's float INTER_LINEAR
    out = ops.resize_f32_linear(torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).cuda(), h, w).cpu().numpy()
    return out.astype(img.dtype) if img.dtype in (np.float64, np.float16) else out


def resize_pad(img, tgt_size: int, pad_value=(0, 0, 0)):
    """utils/io_utils.py:277-292: scaledown_maxsize, then pad bottom / right to tgt_size x tgt_size; returns (img, (pt, pb, pl, pr))"""
    img = scaledown_maxsize(img, tgt_size)
    h, w = img.shape[:2]
    pb, pr = tgt_size - h, tgt_size - w
    if pb + pr > 0:
        import torch
        v = pad_value[0] if isinstance(pad_value, (tuple, list)) else pad_value
        if isinstance(img, torch.Tensor):
            out = img.new_full((tgt_size, tgt_size) + tuple(img.shape[2:]), v)
            out[:h, :w] = img
            img = out
        else:
            pads = [(0, pb), (0, pr)] + [(0, 0)] * (img.ndim - 2)
            if isinstance(pad_value, (tuple, list)) and img.ndim == 3 and len(set(pad_value)) > 1:
                out = np.empty((tgt_size, tgt_size, img.shape[2]), img.dtype)
                out[:] = np.asarray(pad_value, img.dtype)
                out[:h, :w] = img
                img = out
            else:
                img = np.pad(img, pads, mode='constant', constant_values=v)
    return img, (0, pb, 0, pr)


class NumpyEncoder(json.JSONEncoder):
    """utils/io_utils.py:24-35: numpy arrays -> lists, numpy scalars -> bool / float / int"""
    def default(self, obj):
        if isinstance(obj, np.ndarray):
            return obj.tolist()
        if isinstance(obj, np.bool_):
            return bool(obj)
        if isinstance(obj, np.floating):
            return float(obj)
        if isinstance(obj, np.integer):
            return int(obj)
        return json.JSONEncoder.default(self, obj)


def json2dict(json_path: str):
    with open(json_path, 'r', encoding='utf8') as f:
        return json.loads(f.read())


def dict2json(adict: dict, json_path: str):
    with open(json_path, "w", encoding="utf-8") as f:
        f.write(json.dumps(adict, ensure_ascii=False, cls=NumpyEncoder))


def read_imglst_from_txt(filep):
    """animeinsseg/__init__.py:179-183: one image path per line"""
    with open(filep, 'r', encoding='utf8') as f:
        return f.read().splitlines()


def mask2rle(mask, decode_for_json: bool = True):
    """utils/io_utils.py:327-333: {'size': [h, w], 'counts': COCO compressed RLE of mask > 0} (str, or bytes with
    decode_for_json=False).  mask: an [h, w] numpy array (uploaded) or device tensor; the string is built on the MI355X."""
    import torch
    from cartoonsegmentation_amd import ops
    if isinstance(mask, torch.Tensor):
        m = mask if mask.dtype in (torch.bool, torch.uint8) else mask > 0
    else:
        a = np.asarray(mask)
        m = torch.from_numpy(np.ascontiguousarray(a if a.dtype in (np.bool_, np.uint8) else a > 0)).cuda()
    if m.dim() != 2:
        raise ValueError("mask2rle: an [h, w] mask is expected (got shape %s)" % (tuple(m.shape),))
    counts, _ = ops.mask_rle_encode(m)
    return {'size': [int(m.shape[0]), int(m.shape[1])], 'counts': counts[0] if decode_for_json else counts[0].encode()}
