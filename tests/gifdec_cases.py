"""The GIF files of the decoder's tests, assembled by a small writer of its own: an LZW encoder with a chosen
minimum code size, an optional deferred clear and a clear every k codes, sub-blocks of a chosen size, interlace, rectangles,
local tables, graphic control extensions.  Pillow's writer always uses code size 8 and, on noisy input, full-frame rectangles, so
it cannot reach most of these.  case_file(name) is the file, STREAMS[name] (after case_file) the code statistics of its frames,
reference(name, alpha) what Pillow shows: [n,H,W,3] B, G, R or [n,H,W,4] B, G, R, A."""
import io
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CANVAS_H, CANVAS_W = 23, 17
STREAMS = {}                        # name -> per frame {'codes', 'clears', 'max_next', 'self_ref', 'bytes'}
_FILES = {}


# ---- the LZW encoder -----------------------------------------------------------------------------------------------------------
def lzw_encode(indices, mcs, defer=False, clear_every=0, first_clear=True, stats=None):
    """the LZW bytes of the indices (raster order) at minimum code size mcs.  The code widths follow the decoder's rule: an entry
    after every code but the first after a clear, one bit wider when the next free entry reaches 1 << width, 12 at the most.  A
    full dictionary is answered by a clear code (or, with defer, never: the width stays 12 and nothing is added); clear_every = k
    also sends a clear after every k codes."""
    px = [int(v) for v in np.asarray(indices).reshape(-1)]
    clear, end = 1 << mcs, (1 << mcs) + 1
    acc, nbits, out = 0, 0, bytearray()
    st = {'codes': 0, 'clears': 0, 'max_next': 0, 'self_ref': 0}
    width, dnext, fresh = mcs + 1, clear + 2, True      # the decoder's state

    def put(code):
        nonlocal acc, nbits, width, dnext, fresh
        acc |= code << nbits
        nbits += width
        while nbits >= 8:
            out.append(acc & 255)
            acc >>= 8
            nbits -= 8
        st['codes'] += 1
        if code == clear:
            width, dnext, fresh = mcs + 1, clear + 2, True
            st['clears'] += 1
        elif code != end:
            if fresh:
                fresh = False
            elif dnext < 4096:
                if code == dnext:
                    st['self_ref'] += 1
                dnext += 1
                if dnext == (1 << width) and width < 12:
                    width += 1
            st['max_next'] = max(st['max_next'], dnext)

    if first_clear:
        put(clear)
    table, enext, since = {}, clear + 2, 0
    i = 0
    while i < len(px):
        cur = px[i]
        i += 1
        while i < len(px) and (cur, px[i]) in table:
            cur = table[(cur, px[i])]
            i += 1
        put(cur)
        since += 1
        if i < len(px):
            if enext < 4096:
                table[(cur, px[i])] = enext
                enext += 1
            if (enext == 4096 and not defer) or (clear_every and since >= clear_every):
                put(clear)
                table, enext, since = {}, clear + 2, 0
    put(end)
    if nbits:
        out.append(acc & 255)
    if stats is not None:
        stats.update(st, bytes=len(out))
    return bytes(out)


def sub_blocks(stream, size=255):
    out = bytearray()
    for s in range(0, len(stream), size):
        part = stream[s:s + size]
        out.append(len(part))
        out += part
    out.append(0)
    return bytes(out)


def lace_order(H):
    return [r for start, step in ((0, 8), (4, 8), (2, 4), (1, 2)) for r in range(start, H, step)]


def frame(indices, left=0, top=0, mcs=None, lace=False, transparent=None, disposal=0, delay=None, palette=None, gce=None,
          junk=b'', block=255, **enc):
    return dict(indices=np.asarray(indices, np.uint8), left=left, top=top, mcs=mcs, lace=lace, transparent=transparent,
                disposal=disposal, delay=delay, palette=palette, gce=gce, junk=junk, block=block, enc=enc)


def table_bits(entries):
    bits = 1
    while (1 << bits) < entries:
        bits += 1
    return bits


def gif_bytes(H, W, frames, palette=None, background=0, loop=None, version=b'GIF89a', comment=None, trailer=True, stats=None):
    """a GIF file of the frames (dicts from frame()) on an H x W logical screen; palette: uint8 [2^k, 3] R, G, B or None"""
    out = bytearray(version)
    if palette is not None:
        bits = table_bits(len(palette))
        assert len(palette) == 1 << bits
        out += struct.pack('<HH', W, H) + bytes([0x80 | 0x70 | (bits - 1), background, 0]) + np.asarray(palette, np.uint8).tobytes()
    else:
        out += struct.pack('<HH', W, H) + bytes([0x70, background, 0])
    if loop is not None:
        out += bytes([0x21, 0xFF, 11]) + b'NETSCAPE2.0' + bytes([3, 1]) + struct.pack('<H', loop) + bytes([0])
    if comment is not None:
        out += bytes([0x21, 0xFE]) + sub_blocks(comment, 100)
    for f in frames:
        ind = f['indices']
        h, w = ind.shape
        need_gce = f['gce'] if f['gce'] is not None else (f['transparent'] is not None or f['disposal'] or f['delay'] is not None)
        if need_gce:
            flags = (f['disposal'] << 2) | (1 if f['transparent'] is not None else 0)
            out += bytes([0x21, 0xF9, 4, flags]) + struct.pack('<H', f['delay'] or 0) + bytes([f['transparent'] or 0, 0])
        flags = 0x40 if f['lace'] else 0
        local = f['palette']
        if local is not None:
            bits = table_bits(len(local))
            assert len(local) == 1 << bits
            flags |= 0x80 | (bits - 1)
        out += bytes([0x2C]) + struct.pack('<HHHH', f['left'], f['top'], w, h) + bytes([flags])
        if local is not None:
            out += np.asarray(local, np.uint8).tobytes()
        mcs = f['mcs'] if f['mcs'] is not None else max(2, table_bits(int(ind.max()) + 1))
        rows = ind[lace_order(h)] if f['lace'] else ind
        st = {}
        stream = lzw_encode(rows, mcs, stats=st, **f['enc']) + f['junk']
        st['bytes'] = len(stream)
        if stats is not None:
            stats.append(st)
        out += bytes([mcs]) + sub_blocks(stream, f['block'])
    if trailer:
        out.append(0x3B)
    return bytes(out)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def colours(n, seed):
    """n distinct-looking colours, never the grey ramp that Pillow shows through mode L"""
    p = np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)
    p[0] = (200, 30, 90)
    return p


PAL16 = colours(16, 1)


def _single(H, W, mcs, seed, **kw):
    rng = np.random.default_rng(seed)
    return lambda st: gif_bytes(H, W, [frame(rng.integers(0, 1 << mcs, (H, W)), mcs=mcs, **kw)], colours(1 << mcs, mcs), stats=st)


def _noise_8(**enc):
    ind = np.random.default_rng(8).integers(0, 256, (64, 80))
    return lambda st: gif_bytes(64, 80, [frame(ind, mcs=8, **enc)], colours(256, 8), stats=st)


def _anim(frames, palette=PAL16, background=0, loop=0, H=CANVAS_H, W=CANVAS_W, **kw):
    return lambda st: gif_bytes(H, W, frames, palette, background=background, loop=loop, stats=st, **kw)


def _idx(h, w, seed, hi=16, lo=0):
    return np.random.default_rng(seed).integers(lo, hi, (h, w))


def _disposals(transparent):
    t = transparent
    return [frame(_idx(CANVAS_H, CANVAS_W, 20), mcs=4, transparent=t, disposal=1, delay=5),
            frame(_idx(9, 8, 21), left=3, top=4, mcs=4, transparent=t, disposal=2, delay=5),
            frame(_idx(11, 6, 22), left=9, top=10, mcs=4, transparent=t, disposal=3, delay=5),
            frame(_idx(5, 13, 23), left=2, top=1, mcs=4, transparent=t, disposal=0, delay=5),
            frame(_idx(7, 7, 24), left=5, top=12, mcs=4, transparent=t, disposal=3, delay=5),
            frame(_idx(8, 9, 25), left=0, top=0, mcs=4, transparent=t, disposal=2, delay=5),
            frame(_idx(6, 6, 26), left=10, top=15, mcs=4, transparent=t, disposal=1, delay=5)]


def _pillow_clip(seed, n, H, W, **save):
    def build(st):
        from PIL import Image
        rng = np.random.default_rng(seed)
        base = rng.integers(0, 256, (H, W, 3)).astype(np.uint8) // 64 * 64
        ims = []
        for k in range(n):
            a = base.copy()
            a[2 + k:9 + k, 3:11] = (255, 10 * k, 0)
            ims.append(Image.fromarray(a))
        buf = io.BytesIO()
        ims[0].save(buf, 'GIF', save_all=True, append_images=ims[1:], duration=40, loop=0, **save)
        return buf.getvalue()
    return build


def _gifcode_clip(st):
    import gif_restatement as G
    ind = np.random.default_rng(31).integers(0, 256, (3, 21, 34)).astype(np.uint8)
    ind[1, 5:15] = 7
    return G.encode_indices(ind, colours(256, 31), fps=20, loop=2, order=[0, 1, 2, 1])


BUILDERS = {}
for _m in range(2, 9):
    BUILDERS['mcs%d' % _m] = _single(9, 13, _m, 100 + _m)
BUILDERS.update({
    'size_1x1': _single(1, 1, 2, 1), 'size_1x7': _single(1, 7, 3, 2), 'size_5x1': _single(5, 1, 2, 3),
    'dict_clear': _noise_8(), 'dict_defer': _noise_8(defer=True), 'dict_every100': _noise_8(clear_every=100),
    'flat': lambda st: gif_bytes(40, 40, [frame(np.full((40, 40), 5), mcs=3)], colours(8, 40), stats=st),
    'no_first_clear': _single(9, 13, 4, 77, first_clear=False),
    'blocks': _single(29, 31, 5, 5),
    'junk': _single(9, 13, 4, 6, junk=b'\x5a\xa5\xff\x00\x13'),
    'small_blocks': _single(9, 13, 6, 7, block=7),
    'comment87': lambda st: gif_bytes(6, 5, [frame(_idx(6, 5, 9, 4), mcs=2, gce=False)], colours(4, 9), version=b'GIF87a',
                                      comment=b'x' * 250, trailer=False, stats=st),
})
for _h in (1, 2, 3, 4, 5, 9):
    BUILDERS['lace_h%d' % _h] = _single(_h, 7, 3, 50 + _h, lace=True)
BUILDERS.update({
    'anim_rects': _anim([frame(_idx(CANVAS_H, CANVAS_W, 10), mcs=4, delay=4),
                         frame(_idx(6, 5, 11), left=CANVAS_W - 5, top=2, mcs=4, delay=4, disposal=1),
                         frame(_idx(4, 9, 12), left=3, top=CANVAS_H - 4, mcs=4, delay=4, disposal=1, lace=True),
                         frame(_idx(1, 1, 13), left=8, top=8, mcs=4, delay=4, disposal=1),
                         frame(_idx(3, 3, 14), left=CANVAS_W - 3, top=CANVAS_H - 3, mcs=4, delay=4, disposal=1)]),
    'anim_disposal_t': _anim(_disposals(3)),
    'anim_disposal_nt': _anim(_disposals(None)),
    'anim_mixed_t': _anim([frame(_idx(CANVAS_H, CANVAS_W, 60), mcs=4, disposal=2, delay=3),
                           frame(_idx(9, 9, 61), left=1, top=1, mcs=4, transparent=2, disposal=2, delay=3),
                           frame(_idx(9, 9, 62), left=5, top=9, mcs=4, disposal=3, delay=3),
                           frame(_idx(9, 9, 63), left=8, top=14, mcs=4, transparent=9, disposal=1, delay=3)], background=6),
    'anim_t0_only': _anim([frame(_idx(CANVAS_H, CANVAS_W, 64), mcs=4, transparent=4, disposal=1, delay=3),
                           frame(_idx(9, 9, 65), left=1, top=1, mcs=4, disposal=2, delay=3),
                           frame(_idx(9, 9, 66), left=5, top=9, mcs=4, disposal=3, delay=3),
                           frame(_idx(9, 9, 67), left=8, top=3, mcs=4, transparent=1, disposal=1, delay=3)], background=2),
    'anim_local': _anim([frame(_idx(CANVAS_H, CANVAS_W, 30), mcs=4, delay=2, disposal=2, transparent=1),
                         frame(_idx(10, 10, 31), left=2, top=3, mcs=4, delay=2, palette=colours(16, 32), disposal=2),
                         frame(_idx(12, 9, 33), left=6, top=8, mcs=4, delay=2, palette=colours(4, 34), disposal=2, transparent=14),
                         frame(_idx(12, 9, 35), left=1, top=1, mcs=4, delay=2, palette=colours(8, 36), disposal=1),
                         frame(_idx(5, 5, 37), left=0, top=0, mcs=4, delay=2)], background=13),
    'anim_local0_short': _anim([frame(_idx(CANVAS_H, CANVAS_W, 38), mcs=4, delay=2, palette=colours(4, 39), disposal=2),
                                frame(_idx(10, 10, 40), left=2, top=3, mcs=4, delay=2)], palette=colours(8, 41), background=6),
    'anim_no_global': _anim([frame(_idx(CANVAS_H, CANVAS_W, 42), mcs=4, delay=2, palette=colours(16, 43), disposal=2),
                             frame(_idx(10, 10, 44), left=2, top=3, mcs=4, delay=2, palette=colours(16, 45))], palette=None, background=5),
    'anim_small0': _anim([frame(_idx(8, 7, 46), left=4, top=6, mcs=4, delay=2, disposal=1),
                          frame(_idx(10, 10, 47), left=0, top=0, mcs=4, delay=2, disposal=1)]),
    'anim_small0_t': _anim([frame(_idx(8, 7, 48), left=4, top=6, mcs=4, delay=2, disposal=1, transparent=5),
                            frame(_idx(10, 10, 49), left=0, top=0, mcs=4, delay=2, disposal=1, transparent=5)]),
    'anim_prev0': _anim([frame(_idx(12, 12, 70), left=2, top=2, mcs=4, delay=2, disposal=3),
                         frame(_idx(10, 10, 71), left=0, top=0, mcs=4, delay=2, disposal=1)]),
    'anim_prev0_t': _anim([frame(_idx(12, 12, 72), left=2, top=2, mcs=4, delay=2, disposal=3, transparent=7),
                           frame(_idx(10, 10, 73), left=5, top=9, mcs=4, delay=2, disposal=1, transparent=7),
                           frame(_idx(4, 4, 74), left=0, top=0, mcs=4, delay=2, disposal=1)]),
    'anim_sticky': _anim([frame(_idx(CANVAS_H, CANVAS_W, 75), mcs=4, delay=2, disposal=2),
                          frame(_idx(6, 6, 76), left=3, top=3, mcs=4, delay=2, disposal=0),
                          frame(_idx(6, 6, 77), left=9, top=12, mcs=4, delay=2, disposal=0),
                          frame(_idx(3, 3, 78), left=0, top=0, mcs=4, gce=False)]),
    'anim_bg': _anim([frame(_idx(CANVAS_H, CANVAS_W, 79), mcs=4, delay=2, disposal=2),
                      frame(_idx(6, 6, 80), left=3, top=3, mcs=4, delay=2, disposal=2),
                      frame(_idx(6, 6, 81), left=9, top=12, mcs=4, delay=2, disposal=1)], background=11),
    'anim_delay0': _anim([frame(_idx(CANVAS_H, CANVAS_W, 82), mcs=4, delay=0, disposal=1),
                          frame(_idx(6, 6, 83), left=3, top=3, mcs=4, delay=0, disposal=1),
                          frame(_idx(6, 6, 84), left=4, top=4, mcs=4, delay=65535, disposal=1)], loop=7),
    'pillow_a': _pillow_clip(1, 3, 20, 24),
    'pillow_b': _pillow_clip(2, 4, 33, 19, optimize=True, disposal=2),
    'gifcode': _gifcode_clip,
})
NAMES = list(BUILDERS)
SINGLE = [n for n in NAMES if not n.startswith(('anim_', 'pillow_', 'gifcode'))]


def case_file(name):
    if name not in _FILES:
        st = []
        _FILES[name] = BUILDERS[name](st)
        STREAMS[name] = st
    return _FILES[name]


def pillow_frames(data, alpha=False):
    """what Pillow shows after seek(i): uint8 [n,H,W,3] B, G, R, or [n,H,W,4] B, G, R, A; and the durations in ms"""
    from PIL import Image
    out, dur = [], []
    with Image.open(io.BytesIO(data)) as im:
        i = 0
        while True:
            try:
                im.seek(i)
            except EOFError:
                break
            a = np.asarray(im.convert('RGBA' if alpha else 'RGB'))
            out.append(np.concatenate([a[:, :, 2::-1], a[:, :, 3:]], axis=2))
            dur.append(int(im.info.get('duration', 0)))
            i += 1
    return np.stack(out), dur


_REF = {}


def reference(name, alpha=False):
    if (name, alpha) not in _REF:
        _REF[name, alpha] = pillow_frames(case_file(name), alpha)
    return _REF[name, alpha][0]


def durations(name):
    reference(name)
    return _REF[name, False][1]


# ---- files that probe refuses: name -> (builder, a word of the reason) -----------------------------------------------------------
def _one(H=4, W=4, **kw):
    return frame(_idx(H, W, 90, 4), mcs=2, **kw)


def _with_mcs(m):
    data = bytearray(gif_bytes(4, 4, [_one(gce=False)], colours(4, 1)))
    at = 13 + 12 + 10
    assert data[at] == 2
    data[at] = m
    return bytes(data)


REFUSED = {
    'not_gif': (lambda: b'GIF88a' + bytes(20), 'not a GIF'),
    'no_image': (lambda: gif_bytes(4, 4, [], colours(4, 1), loop=0), 'no image'),
    'beyond_right': (lambda: gif_bytes(4, 4, [_one(left=1)], colours(4, 1)), 'beyond the logical screen'),
    'beyond_bottom': (lambda: gif_bytes(4, 4, [_one(), _one(top=2)], colours(4, 1)), 'beyond the logical screen'),
    'no_table': (lambda: gif_bytes(4, 4, [_one()], None), 'colour table'),
    'mcs1': (lambda: _with_mcs(1), 'minimum code size'),
    'mcs9': (lambda: _with_mcs(9), 'minimum code size'),
    'truncated_header': (lambda: gif_bytes(4, 4, [_one()], colours(4, 1))[:10], 'truncated'),
    'truncated_table': (lambda: gif_bytes(4, 4, [_one()], colours(4, 1))[:20], 'truncated'),
    'truncated_data': (lambda: gif_bytes(4, 4, [_one()], colours(4, 1))[:-4], 'truncated'),
    'grey_ramp': (lambda: gif_bytes(4, 4, [_one()], np.repeat(np.arange(4, dtype=np.uint8)[:, None], 3, 1)), 'grey ramp'),
}


def corrupt_streams():
    """(an early end code, an invalid code) as (pixels, minimum code size, LZW bytes) for the rectangle of 'mcs4': streams the walker
    answers with its error words 4 and 1 (csm_lzw.h), on the host under the sanitizers first, then on the device"""
    from cartoonsegmentation_amd import gifread
    data = case_file('mcs4')
    fr = gifread.probe(data)['frames'][0]
    s = gifread.lzw_stream(data, fr).tobytes()
    early = lzw_encode(np.random.default_rng(104).integers(0, 16, 50), 4)                     # 50 of the 117 pixels, then the end code
    # clear, literal 1, then code 31 at width 5: far above the next free entry (18)
    invalid = struct.pack('<H', 16 | 1 << 5 | 31 << 10) + s[2:]
    return (9 * 13, 4, early), (9 * 13, 4, invalid)
