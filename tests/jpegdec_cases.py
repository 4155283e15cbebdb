"""The files of tests/test_jpegdec.py (CPU) and tests/test_gpu_jpegdec.py (GPU): made at test time by PIL's encoder and by the
project's own (mjpeg_restatement.encode) from drawn-looking, flat and uniform-noise frames.  Nothing here reads a fixture."""
import functools
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mjpeg_restatement as ENC  # noqa: E402
from test_mjpeg import cartoon  # noqa: E402

SIZES = [(1, 1), (5, 7), (8, 8), (16, 16), (33, 17), (17, 33), (24, 40), (192, 256)]       # (H, W)
MODES = ['grey', '444', '422', '420']
RESTARTS = ['none', 'mcu1', 'mcu3', 'row']
PIL_SUBSAMPLING = {'444': 0, '422': 1, '420': 2}


def frame(content, H, W, seed=0):
    """uint8 BGR [H,W,3]"""
    if content == 'cartoon':
        return cartoon(H, W, seed)
    if content == 'flat':
        return np.full((H, W, 3), (40, 120, 200), np.uint8)
    if content == 'noise':
        return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    raise ValueError(content)


def pil_jpeg(img_bgr, mode, quality=90, restart='none', optimize=False, **extra):
    """a baseline JPEG of the BGR frame by PIL's encoder"""
    kw = dict(quality=quality, optimize=optimize, **extra)
    if mode == 'grey':
        im = Image.fromarray(np.ascontiguousarray(img_bgr[:, :, 1]))
    else:
        im = Image.fromarray(np.ascontiguousarray(img_bgr[:, :, ::-1]))
        kw['subsampling'] = PIL_SUBSAMPLING[mode]
    if restart == 'mcu1':
        kw['restart_marker_blocks'] = 1
    elif restart == 'mcu3':
        kw['restart_marker_blocks'] = 3
    elif restart == 'row':
        kw['restart_marker_rows'] = 1
    buf = io.BytesIO()
    im.save(buf, 'JPEG', **kw)
    return buf.getvalue()


def _cases():
    out = []
    for si, (H, W) in enumerate(SIZES):
        for mi, mode in enumerate(MODES):
            # every (mode, restart) pair occurs at two sizes, once with typical and once with optimised tables
            out.append(dict(enc='pil', content='cartoon', H=H, W=W, mode=mode, restart=RESTARTS[(si + mi) % 4], optimize=si >= 4,
                            quality=90, seed=si))
    # a flat frame at quality 1: blocks of a few bits, dozens of them in one subsequence
    for mode in ('grey', '420'):
        out.append(dict(enc='pil', content='flat', H=64, W=96, mode=mode, restart='none', optimize=False, quality=1, seed=0))
    # noise at quality 100: 16-bit codes, blocks without EOB, blocks longer than a subsequence
    for mode, restart in (('444', 'none'), ('420', 'mcu3'), ('grey', 'row')):
        out.append(dict(enc='pil', content='noise', H=40, W=48, mode=mode, restart=restart, optimize=False, quality=100, seed=3))
    # noise at a low quality: long zero runs inside a block (ZRL)
    out.append(dict(enc='pil', content='noise', H=40, W=48, mode='422', restart='none', optimize=False, quality=30, seed=3))
    # the project's own encoder (a restart interval of one MCU row)
    for mode, (H, W) in (('420', (24, 40)), ('444', (33, 17)), ('420', (192, 256))):
        out.append(dict(enc='own', content='cartoon', H=H, W=W, mode=mode, restart='row', optimize=False, quality=90, seed=1))
    return out


CASES = _cases()


def case_id(c):
    return "%s-%s-%dx%d-%s-%s-%s-q%d" % (c['enc'], c['content'], c['W'], c['H'], c['mode'], c['restart'],
                                          'opt' if c['optimize'] else 'typ', c['quality'])


@functools.lru_cache(maxsize=None)
def _file(key):
    c = dict(key)
    img = frame(c['content'], c['H'], c['W'], c['seed'])
    if c['enc'] == 'own':
        return ENC.encode(img, c['quality'], c['mode'])
    return pil_jpeg(img, c['mode'], c['quality'], c['restart'], c['optimize'])


def case_file(c):
    return _file(tuple(sorted(c.items())))


def pil_decode(data):
    """PIL's (libjpeg's default) decode as BGR [H,W,3]; a grey file gives three equal channels"""
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


# ---- files with a property of the byte stream, found by searching seeds ---------------------------------------------------
def entropy_bytes(data):
    from cartoonsegmentation_amd import jpegcode
    s, e = jpegcode.probe(data)['entropy']
    return np.frombuffer(data[s:e], np.uint8)


def has_property(kind, data, S):
    """'stuffed_straddle': an FF 00 pair whose 00 is the first byte of a subsequence; 'marker_straddle': a restart marker whose
    second byte is; 'marker_start': a restart marker whose FF is"""
    e = entropy_bytes(data).astype(np.int64)
    ff = np.nonzero(e[:-1] == 0xFF)[0]
    nxt = e[ff + 1]
    if kind == 'stuffed_straddle':
        return bool((((ff + 1) % S == 0) & (nxt == 0)).any())
    rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    if kind == 'marker_straddle':
        return bool((((ff + 1) % S == 0) & rst).any())
    if kind == 'marker_start':
        return bool(((ff % S == 0) & (ff > 0) & rst).any())
    raise ValueError(kind)


SPECIAL_KINDS = ('stuffed_straddle', 'marker_straddle', 'marker_start')


@functools.lru_cache(maxsize=None)
def special_file(kind, S):
    """a noise file (4:2:0, quality 95, a restart marker behind every MCU) that has the property at subsequence size S"""
    for seed in range(2000):
        data = pil_jpeg(frame('noise', 48, 64, 100 + seed), '420', 95, 'mcu1')
        if has_property(kind, data, S):
            return data
    raise AssertionError("no seed gives a file with %s at S = %d" % (kind, S))


# ---- the reference of a case, computed once and shared ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(data):
    import jpegdec_restatement as R
    from cartoonsegmentation_amd import jpegcode
    info = jpegcode.probe(data)
    coef = R.decode_coefficients(data, info)
    px = R.pixels(info, coef)
    coef.setflags(write=False)
    px.setflags(write=False)
    return info, coef, px


def reference(data):
    """(probe's description, coefficients, uint8 BGR pixels) of the restatement's serial decode; read-only arrays"""
    return _reference(bytes(data))
