"""Host side of the GIF writer (contract DESIGN.md §4.10; device side csrc/gif.hip): the median-cut palette from the device's
cell table, the sub-block framing of the LZW bytes and the GIF89a container.  Pure Python / numpy; no device code."""
import math
import struct

import numpy as np

SEGMENT = 3839                 # pixels per LZW segment: 257 + SEGMENT = 4096, so a segment's dictionary can never overflow
CELLS = 32768                  # 15-bit cells (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3)
MAX_PIXELS = 2 ** 32 // 8      # the cell table is uint32: a sum of low fields stays below 7 * pixels
# the 8x8 Bayer matrix, [y & 7][x & 7]; the dither offset of a pixel is (BAYER >> 3) - 4, in [-4, 3]
BAYER = np.array([[0, 32, 8, 40, 2, 34, 10, 42],
                  [48, 16, 56, 24, 50, 18, 58, 26],
                  [12, 44, 4, 36, 14, 46, 6, 38],
                  [60, 28, 52, 20, 62, 30, 54, 22],
                  [3, 35, 11, 43, 1, 33, 9, 41],
                  [51, 19, 59, 27, 49, 17, 57, 25],
                  [15, 47, 7, 39, 13, 45, 5, 37],
                  [63, 31, 55, 23, 61, 29, 53, 21]], np.uint8)


def stream_bound(H, W):
    """bytes that bound the LZW stream of one H x W frame: every pixel a 12-bit code, a Clear per segment, the EOI"""
    px = int(H) * int(W)
    return (12 * (px + (px + SEGMENT - 1) // SEGMENT + 1) + 7) // 8


def grey_palette():
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def check_palette(palette):
    p = np.asarray(palette)
    if p.dtype != np.uint8 or p.shape != (256, 3):
        raise ValueError("gif: the palette must be uint8 [256,3] in R, G, B order (got %s %s)" % (p.dtype, p.shape))
    return np.ascontiguousarray(p)


def build_palette(table):
    """The 256-entry R, G, B palette of a clip from its cell table (uint32 [32768,4]: pixel count and the sums of r & 7, g & 7,
    b & 7 of every cell): a deterministic median cut over the occupied cells, weighted by count.  A box is a set of cells; its
    side along a channel is the largest minus the smallest 5-bit coordinate.  While there are fewer than 256 boxes, the box with
    the largest count x longest side (ties: the box that holds the lowest cell key) is split along its longest side (ties: r
    before g before b): its cells sorted by (coordinate, cell key), the first k go left, k the smallest number whose count
    reaches half the box's (at least 1, at most all but one).  The boxes sorted by their lowest cell key give the entries: the
    weighted mean colour, rounded half up; unused entries are (0, 0, 0).  With at most 256 occupied cells every box ends as one
    cell, and a cell that holds one colour gives exactly that colour."""
    t = np.asarray(table)
    if t.shape != (CELLS, 4):
        raise ValueError("build_palette: a [32768,4] cell table expected (got %s)" % (t.shape,))
    t = t.astype(np.int64)
    keys = np.nonzero(t[:, 0])[0]
    palette = np.zeros((256, 3), np.uint8)
    if keys.size == 0:
        return palette
    count = t[keys, 0]
    coord = np.stack([keys >> 10, (keys >> 5) & 31, keys & 31], axis=1)
    total = coord * 8 * count[:, None] + t[keys, 1:4]           # sum of the full 8-bit channel values of every cell

    def describe(idx):
        c = coord[idx]
        side = c.max(axis=0) - c.min(axis=0)
        ch = int(np.argmax(side))                                # the first of equal sides: r, then g, then b
        return {'idx': idx, 'ch': ch, 'score': int(count[idx].sum()) * int(side[ch]), 'low': int(keys[idx].min())}

    boxes = [describe(np.arange(keys.size))]
    while len(boxes) < 256:
        best = max(boxes, key=lambda b: (b['score'], -b['low']))
        if best['score'] == 0:                                   # every box is one cell
            break
        idx, ch = best['idx'], best['ch']
        idx = idx[np.lexsort((keys[idx], coord[idx, ch]))]
        cum = np.cumsum(count[idx])
        k = int(np.searchsorted(2 * cum, cum[-1], side='left')) + 1
        k = min(max(k, 1), idx.size - 1)
        boxes = [b for b in boxes if b is not best] + [describe(idx[:k]), describe(idx[k:])]
    boxes.sort(key=lambda b: b['low'])
    for j, b in enumerate(boxes):
        den = int(count[b['idx']].sum())
        num = total[b['idx']].sum(axis=0)
        palette[j] = [(2 * int(v) + den) // (2 * den) for v in num]
    return palette


def delay_cs(fps):
    """the frame delay in centiseconds: 100 / fps rounded half up; ValueError outside [1, 65535]"""
    fps = float(fps)
    d = int(math.floor(100.0 / fps + 0.5)) if fps > 0 and math.isfinite(fps) else 0
    if not 1 <= d <= 65535:
        raise ValueError("gif: fps %r gives a frame delay of %d centiseconds; it must be in [1, 65535]" % (fps, d))
    return d


def sub_blocks(stream):
    """the LZW bytes framed into data sub-blocks of at most 255 bytes, with the terminator"""
    data = np.frombuffer(stream, np.uint8)
    n = data.size
    full, rest = divmod(n, 255)
    out = np.empty(n + full + (1 if rest else 0) + 1, np.uint8)
    body = out[:256 * full].reshape(full, 256)
    body[:, 0] = 255
    body[:, 1:] = data[:255 * full].reshape(full, 255)
    if rest:
        out[256 * full] = rest
        out[256 * full + 1:-1] = data[255 * full:]
    out[-1] = 0
    return out.tobytes()


def gif_file(streams, width, height, palette, fps=25, loop=0, order=None):
    """The complete GIF89a file of the LZW streams `streams` (a list of bytes from ops.gif_streams, all width x height): header,
    logical screen descriptor with a 256-entry global colour table, the palette, the NETSCAPE2.0 loop extension (omitted for a
    single output frame), and per output frame a graphic control extension (disposal 0, no transparency, the delay), an image
    descriptor of the full canvas, the minimum code size 8 and the framed stream; then the trailer.  `order` lists, for each
    output frame, the index of the stream it takes (default: every stream once, in order)."""
    order = list(range(len(streams))) if order is None else [int(i) for i in order]
    if not order:
        raise ValueError("gif: at least one frame is needed")
    if any(i < 0 or i >= len(streams) for i in order):
        raise ValueError("gif: order refers to a frame outside the %d encoded ones" % len(streams))
    width, height, loop = int(width), int(height), int(loop)
    if not (1 <= width <= 65535 and 1 <= height <= 65535 and 0 <= loop <= 65535):
        raise ValueError("gif: width and height must be in [1, 65535] and loop in [0, 65535]")
    delay = delay_cs(fps)
    palette = check_palette(palette)
    parts = [b'GIF89a', struct.pack('<HHBBB', width, height, 0xF7, 0, 0), palette.tobytes()]
    if len(order) > 1:
        parts.append(b'\x21\xFF\x0BNETSCAPE2.0\x03\x01' + struct.pack('<H', loop) + b'\x00')
    framed = {}
    for i in order:
        if i not in framed:
            framed[i] = sub_blocks(streams[i])
        parts.append(b'\x21\xF9\x04\x00' + struct.pack('<H', delay) + b'\x00\x00')
        parts.append(b'\x2C' + struct.pack('<HHHHB', 0, 0, width, height, 0) + b'\x08')
        parts.append(framed[i])
    parts.append(b'\x3B')
    return b''.join(parts)
