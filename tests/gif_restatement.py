"""The GIF contract of DESIGN.md §4.10 restated in numpy / pure Python, written from the contract and not from csrc/gif.hip: the cell
table, the dither and the nearest-colour mapping, the segmented LZW coder with its width rules, the sub-block framing and the
container, and an independent LZW decoder that follows Pillow's rules.  The palette itself comes from gifcode.build_palette (host
product code, tested on its own in tests/test_gif.py)."""
import struct

import numpy as np

S = 3839                                                        # pixels per segment
CLEAR, EOI = 256, 257
BAYER = np.array([[0, 32, 8, 40, 2, 34, 10, 42], [48, 16, 56, 24, 50, 18, 58, 26], [12, 44, 4, 36, 14, 46, 6, 38],
                  [60, 28, 52, 20, 62, 30, 54, 22], [3, 35, 11, 43, 1, 33, 9, 41], [51, 19, 59, 27, 49, 17, 57, 25],
                  [15, 47, 7, 39, 13, 45, 5, 37], [63, 31, 55, 23, 61, 29, 53, 21]], np.int64)


def rgb_of(frames, bgr=True):
    """[n,H,W,3] int64 in R, G, B order from uint8 frames [n,H,W,3] or [H,W,3]"""
    f = np.asarray(frames)
    f = f[None] if f.ndim == 3 else f
    return (f[..., ::-1] if bgr else f).astype(np.int64)


def cell_table(frames, bgr=True):
    """uint32 [32768,4]: per cell (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3) the pixel count and the sums of r & 7, g & 7, b & 7"""
    p = rgb_of(frames, bgr).reshape(-1, 3)
    key = (p[:, 0] >> 3) << 10 | (p[:, 1] >> 3) << 5 | (p[:, 2] >> 3)
    t = np.zeros((32768, 4), np.int64)
    t[:, 0] = np.bincount(key, minlength=32768)
    for c in range(3):
        t[:, 1 + c] = np.bincount(key, weights=(p[:, c] & 7), minlength=32768).astype(np.int64)
    return t.astype(np.uint32)


def nearest(pix, palette):
    """index of the palette entry with the smallest squared distance to each R, G, B row of pix; the lowest index on ties"""
    pal = np.asarray(palette).astype(np.int64)
    out = np.empty(pix.shape[0], np.uint8)
    for s in range(0, pix.shape[0], 4096):
        d = ((pix[s:s + 4096, None, :] - pal[None]) ** 2).sum(axis=2)
        out[s:s + 4096] = np.argmin(d, axis=1)                   # numpy's argmin takes the first of equal minima
    return out


def quantize(frames, palette, dither='ordered', bgr=True):
    """uint8 [n,H,W] indices.  A pixel that equals a palette entry takes that entry (the lowest such index) whatever the dither;
    every other pixel is searched as it is ('none') or with (BAYER[y & 7][x & 7] >> 3) - 4 added to each channel and clamped to
    [0, 255] ('ordered')."""
    p = rgb_of(frames, bgr)
    n, H, W, _ = p.shape
    plain = nearest(p.reshape(-1, 3), palette).reshape(n, H, W)
    if dither == 'none':
        return plain
    assert dither == 'ordered'
    off = (BAYER[np.arange(H)[:, None] & 7, np.arange(W)[None, :] & 7] >> 3) - 4
    q = np.clip(p + off[None, :, :, None], 0, 255)
    moved = nearest(q.reshape(-1, 3), palette).reshape(n, H, W)
    exact = (np.asarray(palette).astype(np.int64)[plain] == p).all(axis=3)
    return np.where(exact, plain, moved).astype(np.uint8)


# ---- LZW ---------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.acc, self.fill, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= v << self.fill
        self.fill += n
        while self.fill >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.fill -= 8

    def done(self):
        if self.fill:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def lzw(indices, trace=None):
    """the LZW bytes of one frame's indices (any shape, raster order).  trace (a dict) collects what the coverage check of
    tests/test_gif.py asks about: the widths Clear and EOI were written at, the last entry a decoder adds in a segment, and
    whether a code equal to the next free code was emitted."""
    px = np.asarray(indices, np.uint8).reshape(-1).tolist()
    assert px
    bits, width = Bits(), 9
    tr = trace if trace is not None else {}
    for key in ('clear_widths', 'eoi_widths', 'last_entries'):
        tr.setdefault(key, set())
    tr.setdefault('code_equals_next', False)
    for s0 in range(0, len(px), S):
        seg = px[s0:s0 + S]
        bits.put(CLEAR, width)
        tr['clear_widths'].add(width)
        width, free, table = 9, 258, {}
        emitted = 0
        prefix = seg[0]
        for c in seg[1:]:
            got = table.get((prefix, c))
            if got is not None:
                prefix = got
                continue
            bits.put(prefix, width)                              # not the segment's last code: it adds an entry
            emitted += 1
            if prefix == free - 1 and prefix >= 258:
                # the decoder's next free code is one behind the coder's: the entry added at the previous code is the newest
                tr['code_equals_next'] = True
            table[(prefix, c)] = free
            free += 1
            if free > (1 << width) and width < 12:
                width += 1
            prefix = c
        bits.put(prefix, width)                                  # the last code: the decoder adds one more entry, the coder none
        emitted += 1
        if prefix == free - 1 and prefix >= 258:
            tr['code_equals_next'] = True
        if emitted >= 2:
            tr['last_entries'].add(256 + emitted)
        if free + 1 > (1 << width) and width < 12:
            width += 1
    bits.put(EOI, width)
    tr['eoi_widths'].add(width)
    return bits.done()


def unlzw(stream, pixels):
    """decode LZW bytes by Pillow's rules: an entry after every code but the first after a Clear, one bit wider when the entry just
    added was (1 << width) - 1, never wider than 12; returns uint8 [pixels]"""
    acc = int.from_bytes(stream, 'little')
    pos, width, out = 0, 9, []
    strings, last = None, None
    while True:
        assert pos + width <= 8 * len(stream), "the stream ends inside a code"
        code = (acc >> pos) & ((1 << width) - 1)
        pos += width
        if code == CLEAR:
            strings, last, width = [(i,) for i in range(256)] + [None, None], None, 9
            continue
        if code == EOI:
            break
        assert strings is not None, "data before the first Clear"
        if last is None:
            assert code < 256
            cur = strings[code]
        else:
            assert code <= len(strings), "a code beyond the next free one"
            cur = strings[code] if code < len(strings) else strings[last] + (strings[last][0],)
            if len(strings) < 4096:
                strings.append(strings[last] + (cur[0],))
                if len(strings) - 1 == (1 << width) - 1 and width < 12:
                    width += 1
        out.extend(cur)
        last = code
    assert (8 * len(stream) - pos) < 8 and (acc >> pos) == 0, "bits behind the EOI"
    assert len(out) == pixels, (len(out), pixels)
    return np.array(out, np.uint8)


def bound(H, W):
    return (12 * (H * W + -(-H * W // S) + 1) + 7) // 8


# ---- container ---------------------------------------------------------------------------------------------------------------
def frame_blocks(stream):
    out = bytearray()
    for s in range(0, len(stream), 255):
        part = stream[s:s + 255]
        out.append(len(part))
        out += part
    out.append(0)
    return bytes(out)


def gif(streams, W, H, palette, fps=25, loop=0, order=None):
    order = list(range(len(streams))) if order is None else list(order)
    delay = int(np.floor(100.0 / fps + 0.5))
    out = bytearray(b'GIF89a')
    out += struct.pack('<HH', W, H) + bytes([0x80 | 0x70 | 0x07, 0, 0])
    out += np.asarray(palette, np.uint8).tobytes()
    if len(order) > 1:
        out += bytes([0x21, 0xFF, 11]) + b'NETSCAPE2.0' + bytes([3, 1]) + struct.pack('<H', loop) + bytes([0])
    for i in order:
        out += bytes([0x21, 0xF9, 4, 0]) + struct.pack('<H', delay) + bytes([0, 0])
        out += bytes([0x2C]) + struct.pack('<HHHH', 0, 0, W, H) + bytes([0]) + bytes([8])
        out += frame_blocks(streams[i])
    out.append(0x3B)
    return bytes(out)


def encode_indices(indices, palette, fps=25, loop=0, order=None):
    """the complete file of uint8 indices [n,H,W] under the palette"""
    ind = np.asarray(indices)
    return gif([lzw(f) for f in ind], ind.shape[2], ind.shape[1], palette, fps, loop, order)
