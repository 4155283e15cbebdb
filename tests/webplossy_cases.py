"""The files of the lossy WebP decoder's tests, generated at test time and cached per process.

    NAMES                  the files the decoder takes: written by Pillow (libwebp's encoder) at several methods and qualities, by
                           the project's own VP8 writer (its restatement), by the transcoder below for the header choices libwebp's
                           encoder does not make, and Pillow RGBA files with hand-made ALPH chunks swapped in
    case_file(name)        the bytes of one
    reference(name)        imread's pixels of one: uint8 B, G, R [H,W,3]
    reference_bgra(name)   PIL's RGBA of one as B, G, R, A
    REFUSED                {name: (build, a word of the reason)} of files webpread.probe(lossy=True) refuses
    transcode(..)          a Pillow file's symbols re-coded under other header choices

Every side stays at or below 320 except in 'long_diagonal', whose reconstruction diagonal is longer than RECON_MBS_PER_STEP."""
import io
import os
import struct
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webp_restatement as E  # noqa: E402
import webpdec_cases as C  # noqa: E402
import webpdec_restatement as LL  # noqa: E402
import webplossy_restatement as R  # noqa: E402

RECON_MBS_PER_STEP = 32          # csrc/webplossy.hip kReconMbs: k_vd_recon and k_vd_filter take this many macroblocks of a diagonal per step


# ---- pictures -----------------------------------------------------------------------------------------------------------------
def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


def flat(H, W, seed):
    """three small flat discs on a flat ground: the project's own writer skips most macroblocks of it (libwebp's codes them as empty)"""
    rng = np.random.default_rng(12 if seed is None else seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.full((H, W, 3), 200, np.uint8)
    for _ in range(3):
        cy, cx, rad = rng.integers(0, H), rng.integers(0, W), rng.integers(4, max(5, min(H, W) // 6))
        img[(y - cy) ** 2 + (x - cx) ** 2 < rad * rad] = rng.integers(0, 256, 3)
    return img


def pil_webp(img, method, quality, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'WEBP', method=method, quality=quality, **kw)
    return b.getvalue()


PICTURES = {
    'cartoon': lambda: C.cartoon(96, 128, 3), 'photo': lambda: C.photo(100, 120, 9), 'noise': lambda: noise(48, 64, 11),
    'indexed': lambda: C.indexed(64, 83, 5, 6), 'flat': lambda: flat(80, 96, 12),
}
PIL_CASES = [(p, m, q) for p in ('cartoon', 'photo', 'noise', 'indexed') for m in (0, 4, 6) for q in (20, 75, 100)] + [('flat', 4, 75)]
SIZES = [(1, 1), (16, 16), (17, 33), (1, 37), (37, 1), (16, 300), (300, 16)]                    # H, W


# ---- the transcoder -------------------------------------------------------------------------------------------------------------
BMODE_BITS = {R.B_DC: ((0, 0),), R.B_TM: ((0, 1), (1, 0)), R.B_VE: ((0, 1), (1, 1), (2, 0)),
              R.B_HE: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 0)), R.B_RD: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 0)),
              R.B_VR: ((0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 1)), R.B_LD: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 0)),
              R.B_VL: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 0)), R.B_HD: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 0)),
              R.B_HU: ((0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 1))}
YMODE_BITS = {R.DC_PRED: ((156, 0), (163, 0)), R.V_PRED: ((156, 0), (163, 1)), R.H_PRED: ((156, 1), (128, 0)), R.TM_PRED: ((156, 1), (128, 1))}
UVMODE_BITS = {R.DC_PRED: ((142, 0),), R.V_PRED: ((142, 1), (114, 0)), R.H_PRED: ((142, 1), (114, 1), (183, 0)),
               R.TM_PRED: ((142, 1), (114, 1), (183, 1))}


def _put_optional(e, v, n):
    e.put_bits(int(v != 0), 1)
    if v:
        e.put_bits(abs(v), n)
        e.put_bits(int(v < 0), 1)


def transcode(vp8, **choice):
    """The symbols of the key frame `vp8` (modes, quantised levels) coded again with the boolean coder of the writer's restatement
    under the header fields in `choice` (the names of webplossy_restatement.read_header; 'segments': a [mbh][mbw] map that replaces
    the file's).  The coefficient probabilities are the defaults.  The pixels change; what libwebp shows for the new file is the
    reference."""
    f = R.parse(vp8)
    h = dict(f['header'])
    segments = choice.pop('segments', None)
    h.update(choice)
    mbw, mbh = f['mbw'], f['mbh']
    nparts = 1 << h['log2parts']
    e = E.BoolEncoder()
    e.put_bits(h['colour_space'], 1)
    e.put_bits(h['clamp'], 1)
    e.put_bits(h['segmentation'], 1)
    if h['segmentation']:
        e.put_bits(h['update_map'], 1)
        e.put_bits(h['update_data'], 1)
        if h['update_data']:
            e.put_bits(h['absolute'], 1)
            for v in h['seg_quant']:
                _put_optional(e, v, 7)
            for v in h['seg_level']:
                _put_optional(e, v, 6)
        if h['update_map']:
            for p in h['seg_probs']:
                e.put_bits(int(p != 255), 1)
                if p != 255:
                    e.put_bits(p, 8)
    e.put_bits(h['simple'], 1)
    e.put_bits(h['level'], 6)
    e.put_bits(h['sharpness'], 3)
    e.put_bits(h['lf_delta'], 1)
    if h['lf_delta']:
        e.put_bits(1, 1)
        for v in list(h['ref_lf_delta']) + list(h['mode_lf_delta']):
            _put_optional(e, v, 6)
    e.put_bits(h['log2parts'], 2)
    e.put_bits(h['qi'], 7)
    for v in h['qdelta']:
        _put_optional(e, v, 4)
    e.put_bits(0, 1)                                                # refresh_entropy_probs
    for p in E.COEFF_UPDATE_PROBS:
        e.put(p, 0)
    e.put_bits(h['use_skip'], 1)
    if h['use_skip']:
        e.put_bits(h['prob_skip'] or 128, 8)
    prob_skip = h['prob_skip'] or 128
    pairs = [[] for _ in range(nparts)]
    top_modes = [R.B_DC] * (4 * mbw)
    top_nz = [[0] * 9 for _ in range(mbw)]
    for mby in range(mbh):
        out = pairs[mby % nparts]
        left_modes, left_nz = [R.B_DC] * 4, [0] * 9
        for mbx in range(mbw):
            m = f['mbs'][mby][mbx]
            if h['segmentation'] and h['update_map']:
                seg = m['segment'] if segments is None else segments[mby][mbx]
                sp = h['seg_probs']
                e.put(sp[0], seg >> 1)
                e.put(sp[2] if seg >> 1 else sp[1], seg & 1)
            skip = bool(h['use_skip']) and not any(any(lv) for lv in m['levels'])
            if h['use_skip']:
                e.put(prob_skip, int(skip))
            e.put(145, 1 - m['is_b'])
            if m['is_b']:
                for by in range(4):
                    for bx in range(4):
                        mode = m['bmodes'][4 * by + bx]
                        p = R.KF_BMODE_PROBS[top_modes[4 * mbx + bx]][left_modes[by]]
                        for node, bit in BMODE_BITS[mode]:
                            e.put(p[node], bit)
                        top_modes[4 * mbx + bx] = left_modes[by] = mode
            else:
                for p, bit in YMODE_BITS[m['ymode']]:
                    e.put(p, bit)
                top_modes[4 * mbx:4 * mbx + 4] = [m['ymode']] * 4
                left_modes = [m['ymode']] * 4
            for p, bit in UVMODE_BITS[m['uvmode']]:
                e.put(p, bit)
            tn = top_nz[mbx]
            if skip:
                for k in range(8):
                    tn[k] = left_nz[k] = 0
                if not m['is_b']:
                    tn[8] = left_nz[8] = 0
                continue
            first, kind = 0, 3
            if not m['is_b']:
                tn[8] = left_nz[8] = E.block_pairs(m['levels'][24], 0, 1, tn[8] + left_nz[8], out)
                first, kind = 1, 0
            for by in range(4):
                for bx in range(4):
                    tn[bx] = left_nz[by] = E.block_pairs(m['levels'][4 * by + bx], first, kind, tn[bx] + left_nz[by], out)
            for c in range(2):
                for by in range(2):
                    for bx in range(2):
                        a, b = 4 + 2 * c + bx, 4 + 2 * c + by
                        tn[a] = left_nz[b] = E.block_pairs(m['levels'][16 + 4 * c + 2 * by + bx], 0, 2, tn[a] + left_nz[b], out)
    return E.vp8_frame(e.finish(), [E.code_pairs(p) for p in pairs], f['width'], f['height'])


def _segment_map(mbh, mbw):
    return [[(x + 2 * y) % 4 for x in range(mbw)] for y in range(mbh)]


SEGMENTED = dict(segmentation=1, update_map=1, update_data=1, absolute=1, seg_probs=[120, 90, 200], segments=_segment_map(6, 8))
# name: (source picture, method, quality, header choices).  The cartoon at method 4 holds whole-block and sub-block macroblocks
TRANSCODED = {
    't_parts2': ('cartoon', 4, 75, dict(log2parts=1)),
    't_parts4': ('cartoon', 4, 75, dict(log2parts=2)),
    't_parts8': ('cartoon', 4, 75, dict(log2parts=3)),
    't_seg_absolute': ('cartoon', 4, 75, dict(SEGMENTED, seg_quant=[10, 40, 70, 100], seg_level=[5, 20, 40, 63])),
    't_seg_delta': ('cartoon', 4, 75, dict(SEGMENTED, absolute=0, seg_quant=[-20, 0, 15, 40], seg_level=[-10, 0, 8, 30])),
    't_seg_map_only': ('cartoon', 4, 75, dict(SEGMENTED, update_data=0)),
    't_lf_delta': ('cartoon', 4, 75, dict(lf_delta=1, ref_lf_delta=[-7, 0, 0, 0], mode_lf_delta=[12, 0, 0, 0], level=20)),
    't_sharp3': ('cartoon', 4, 20, dict(sharpness=3)),
    't_sharp7': ('cartoon', 4, 20, dict(sharpness=7)),
    't_simple_bpred': ('cartoon', 4, 75, dict(simple=1, level=24)),
    't_level0': ('cartoon', 4, 75, dict(level=0)),
    't_level63': ('cartoon', 4, 75, dict(level=63, segmentation=0)),    # without the source's segments: its levels are absolute
    't_noskip': ('own_flat_48x64', None, None, dict(use_skip=0)),
    't_colour_bits': ('cartoon', 4, 75, dict(colour_space=1, clamp=1)),
    't_qdeltas': ('cartoon', 4, 75, dict(SEGMENTED, seg_quant=[3, 60, 100, 125], seg_level=[0, 0, 0, 0], qdelta=[-15, 15, -12, 14, -9])),
}


# ---- hand-made ALPH chunks ----------------------------------------------------------------------------------------------------
def alph_chunk(alpha, compression, filt):
    """the ALPH chunk's bytes of the plane `alpha` [H,W] uint8: the filter applied, then raw bytes or a headerless VP8L stream"""
    a = alpha.astype(np.int64)
    H, W = a.shape
    pred = np.zeros_like(a)
    if filt:
        left = np.concatenate([np.zeros((H, 1), np.int64), a[:, :-1]], axis=1)
        top = np.concatenate([np.zeros((1, W), np.int64), a[:-1]], axis=0)
        tl = np.concatenate([np.zeros((1, W), np.int64), left[:-1]], axis=0)
        pred = left.copy() if filt == 1 else top.copy() if filt == 2 else np.clip(left + top - tl, 0, 255)
        pred[0, 1:] = a[0, :-1]
        pred[1:, 0] = a[:-1, 0]
        pred[0, 0] = 0
    d = ((a - pred) & 255).astype(np.uint32)
    if compression == 0:
        body = d.astype(np.uint8).tobytes()
    else:
        stream = LL.vp8l_chunk(C.write_vp8l(0xff000000 | d << 8, transforms=((0, 3),) if filt & 1 else (), cache_bits=2 * (filt >> 1),
                                            has_alpha=False))
        body = stream[5:]
    return bytes([compression | filt << 2]) + body


def lossy_extended(vp8, W, H, alph=None, before=b'', after=b'', flags=None, canvas=None):
    f = (0x10 if alph is not None else 0) if flags is None else flags
    cw, ch = canvas or (W, H)
    body = C.chunk(b'VP8X', bytes([f, 0, 0, 0]) + struct.pack('<I', cw - 1)[:3] + struct.pack('<I', ch - 1)[:3]) + before
    if alph is not None:
        body += C.chunk(b'ALPH', alph)
    return C.riff(body + C.chunk(b'VP8 ', vp8) + after)


ALPH_CASES = ['alph_c%d_f%d' % (c, f) for c in (0, 1) for f in range(4)]


def _alph_case(name):
    c, f = int(name[6]), int(name[9])
    img = C.cartoon(40, 52, 14, 4)
    vp8, _ = R.container(pil_webp(img, 4, 75, alpha_quality=100))
    return lossy_extended(vp8, 52, 40, alph_chunk(img[..., 3], c, f))


def _own(H, W, quality, seed):
    picture = flat(H, W, seed) if seed is None else C.cartoon(H, W, seed)
    return E.still_file(E.encode_frame(np.ascontiguousarray(picture[..., ::-1]), quality)['vp8'])


def _meta():
    """VP8X + ICCP + ALPH + VP8 + EXIF (orientation 1) + XMP: what libwebp's muxer writes around a lossy image with alpha"""
    vp8, alph = R.container(pil_webp(C.cartoon(20, 24, 30, 4), 4, 75))
    return lossy_extended(vp8, 24, 20, alph, before=C.chunk(b'ICCP', b'not a real profile'),
                          after=C.chunk(b'EXIF', C.exif(1)) + C.chunk(b'XMP ', b'<x:xmpmeta/>'), flags=0x10 | 0x20 | 0x08 | 0x04)


OWN = {'own_37x53': (37, 53, 60, 1), 'own_272x544': (544, 272, 75, 2), 'own_flat_48x64': (48, 64, 75, None)}     # H, W, quality, seed (None: flat)
NAMES = (['%s_m%d_q%d' % c for c in PIL_CASES] + ['rgba_aq100', 'rgba_aq50'] + ['size_%dx%d' % s for s in SIZES] + ['long_diagonal']
         + sorted(OWN) + sorted(TRANSCODED) + ALPH_CASES + ['vp8x_meta'])
_files, _refs = {}, {}


def case_file(name):
    if name not in _files:
        if name in TRANSCODED:
            pic, m, q, choice = TRANSCODED[name]
            vp8, _ = R.container(case_file(pic) if pic in OWN else pil_webp(PICTURES[pic](), m, q))
            _files[name] = E.still_file(transcode(vp8, **choice))
        elif name in ALPH_CASES:
            _files[name] = _alph_case(name)
        elif name in OWN:
            _files[name] = _own(*OWN[name])
        elif name == 'vp8x_meta':
            _files[name] = _meta()
        elif name.startswith('rgba_aq'):
            _files[name] = pil_webp(C.cartoon(70, 90, 13, 4), 4, 75, alpha_quality=int(name[7:]))
        elif name.startswith('size_'):
            H, W = (int(v) for v in name[5:].split('x'))
            _files[name] = pil_webp(C.cartoon(H, W, 40 + H), 4, 75)
        elif name == 'long_diagonal':                               # 33 x 65 macroblocks: 33 of them stand on the diagonal of step 64
            _files[name] = pil_webp(flat(16 * (RECON_MBS_PER_STEP + 1), 16 * (2 * RECON_MBS_PER_STEP + 1), 15), 4, 50)
        else:
            pic, m, q = name.rsplit('_', 2)
            _files[name] = pil_webp(PICTURES[pic](), int(m[1:]), int(q[1:]))
    return _files[name]


def reference_bgra(name):
    if name not in _refs:
        with Image.open(io.BytesIO(case_file(name))) as im:
            _refs[name] = np.ascontiguousarray(np.asarray(im.convert('RGBA'))[..., [2, 1, 0, 3]])
    return _refs[name]


def reference(name):
    """imread's pixels (the test of the routing reads the same through utils.io_utils.imread from a path)"""
    from PIL import ImageOps
    with Image.open(io.BytesIO(case_file(name))) as im:
        return np.ascontiguousarray(np.asarray(ImageOps.exif_transpose(im).convert('RGB'))[:, :, ::-1])


# ---- refused files --------------------------------------------------------------------------------------------------------------
def _small():
    """(VP8 chunk, ALPH chunk) of a 24 x 20 file with alpha"""
    return R.container(pil_webp(C.cartoon(20, 24, 31, 4), 0, 75))


def _patched(at, value, mask=0xff):
    def build():
        vp8 = bytearray(_small()[0])
        vp8[at] = (vp8[at] & ~mask & 0xff) | value
        return E.still_file(bytes(vp8))
    return build


def _first_partition_overrun():
    vp8 = bytearray(_small()[0])
    tag = int.from_bytes(vp8[:3], 'little')
    vp8[:3] = ((tag & 0x1f) | len(vp8) << 5).to_bytes(3, 'little')
    return E.still_file(bytes(vp8))


def _huge():
    vp8 = bytearray(_small()[0])
    vp8[6:10] = struct.pack('<HH', 16383, 16383)
    return E.still_file(bytes(vp8))


def _alph_head(head):
    def build():
        vp8, alph = _small()
        return lossy_extended(vp8, 24, 20, bytes([head]) + alph[1:])
    return build


REFUSED = {
    'animated': (lambda: E.encode_animation([np.ascontiguousarray(C.cartoon(16, 16, 34 + k)[..., ::-1]) for k in range(2)]), 'animated'),
    'inter_frame': (_patched(0, 1, 1), 'key frame'),
    'hidden_frame': (_patched(0, 0, 0x10), 'key frame'),
    'version4': (_patched(0, 4 << 1, 7 << 1), 'key frame'),
    'start_code': (_patched(4, 0x02), 'start code'),
    'first_partition': (_first_partition_overrun, 'first partition'),
    'scale_x': (_patched(7, 0x40, 0xc0), 'scale'),
    'scale_y': (_patched(9, 0x80, 0xc0), 'scale'),
    'canvas': (lambda: lossy_extended(_small()[0], 24, 20, canvas=(25, 20)), 'canvas'),
    'flag_without_alph': (lambda: lossy_extended(_small()[0], 24, 20, flags=0x10), 'alpha flag'),
    'alph_without_flag': (lambda: lossy_extended(_small()[0], 24, 20, _small()[1], flags=0), 'alpha flag'),
    'alph_compression2': (_alph_head(2), 'ALPH header'),
    'alph_reserved': (_alph_head(0x41), 'ALPH header'),
    'pixels': (_huge, 'more pixels'),
    'exif6': (lambda: lossy_extended(_small()[0], 24, 20, after=C.chunk(b'EXIF', C.exif(6)), flags=0x08), 'orientation 6'),
    'xmp_orientation': (lambda: lossy_extended(_small()[0], 24, 20, after=C.chunk(b'XMP ', b'<x tiff:Orientation="6"/>'), flags=0x04), 'XMP'),
}
