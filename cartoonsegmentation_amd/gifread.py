"""Host side of the GIF decoder (contract DESIGN.md §4.17; pure Python / numpy, no device): the container parser in front of
csrc/gifdec.hip.  (gifcode.py is the encoder's host side.)

    probe(data)            a plain description of a GIF file the device decoder takes (logical screen, global colour table, loop
                           count, and per image its rectangle, local table, interlace flag, transparent index, disposal, delay,
                           minimum code size and the byte ranges of its data sub-blocks), or Unsupported(reason).  It walks block
                           headers and checks every length against the buffer; it never interprets the LZW data.
    lzw_stream(..)         the joined data sub-blocks of one image: compressed bytes only
    image_descriptor(..)   the int32 row of csm_gif_decode for one image
    file_descriptor(..)    the int32 row of csm_gif_decode for one file

The rule behind every refusal: on a file probe accepts, frame i of the device result equals what Pillow shows after seek(i) on
every byte.  Where Pillow does something this decoder does not restate (a canvas that grows with an image beyond the logical
screen, mode L for a file without colour table or with a grey-ramp one, code sizes above 8), the file is refused.
"""
import struct

import numpy as np

DESC_WORDS = 16
FILE_WORDS = 16
FLAG_INTERLACE = 1
FILE_FLAG_ALPHA = 1                     # frame 0 declared a transparent index: the canvas carries alpha
MAX_PIXELS = 2 ** 31 - 1                # positions in an image's pixels are 32 bits on the device


class Unsupported(ValueError):
    """the file is not one the device decoder takes; str(e) is the reason"""


def _grey_ramp(table):
    """Pillow's test for a table it does not need: entry i is (i, i, i) throughout"""
    t = np.frombuffer(table, np.uint8).reshape(-1, 3)
    return bool((t == np.arange(t.shape[0], dtype=np.uint8)[:, None]).all())


def _sub_blocks(data, p, what):
    """the (start, end) ranges of the data sub-blocks that begin at p, and the position behind their terminator"""
    n = len(data)
    ranges = []
    while True:
        if p >= n:
            raise Unsupported("truncated: the sub-blocks of %s run past the end of the file" % what)
        size = data[p]
        p += 1
        if size == 0:
            return ranges, p
        if p + size > n:
            raise Unsupported("truncated: a sub-block of %s runs past the end of the file" % what)
        ranges.append((p, p + size))
        p += size


def probe(data):
    """see the module docstring.  Returns {'width', 'height' (the logical screen), 'version', 'background' (the background colour
    index; 0 without a global table), 'global_palette' (bytes R, G, B or None), 'loop' (the NETSCAPE loop count or None),
    'frames'}; a frame is {'left', 'top', 'width', 'height', 'interlace', 'transparent' (index or None), 'disposal' (0 keep, 2 to
    background, 3 to previous: what is done with the frame's rectangle before the next frame, a disposal of 0 in the file having
    kept the previous frame's method), 'duration' (ms), 'palette' (local table, bytes, or None), 'min_code_size', 'blocks' (the
    (start, end) ranges of the data sub-blocks), 'stream_bytes'}."""
    data = bytes(data) if not isinstance(data, (bytes, bytearray)) else data
    n = len(data)
    if n < 6 or bytes(data[:6]) not in (b'GIF87a', b'GIF89a'):
        raise Unsupported("not a GIF file")
    if n < 13:
        raise Unsupported("truncated: no logical screen descriptor")
    width, height, flags, background, _ = struct.unpack('<HHBBB', data[6:13])
    p = 13
    info = {'width': width, 'height': height, 'version': bytes(data[:6]), 'background': 0, 'global_palette': None, 'loop': None}
    if flags & 0x80:
        size = 3 << ((flags & 7) + 1)
        if p + size > n:
            raise Unsupported("truncated: the global colour table runs past the end of the file")
        info['global_palette'] = bytes(data[p:p + size])
        info['background'] = background
        p += size
        if _grey_ramp(info['global_palette']):
            raise Unsupported("a grey ramp as global colour table (Pillow shows such a file through mode L)")
    frames = []
    method = 0                                      # a disposal of 0 keeps the method of the frame before
    transparent, duration = None, 0
    while p < n:
        intro = data[p]
        p += 1
        if intro == 0x3B:
            break
        if intro == 0x21:
            if p >= n:
                raise Unsupported("truncated: an extension without label")
            label = data[p]
            ranges, p = _sub_blocks(data, p + 1, "an extension")
            first = bytes(data[ranges[0][0]:ranges[0][1]]) if ranges else b''
            if label == 0xF9 and ranges:
                if len(first) < 4:
                    raise Unsupported("a graphic control extension of %d bytes" % len(first))
                if first[0] & 1:
                    transparent = first[3]
                duration = struct.unpack('<H', first[1:3])[0] * 10
                if (first[0] >> 2) & 7:
                    method = (first[0] >> 2) & 7
            elif label == 0xFF and not frames and first.startswith(b'NETSCAPE2.0') and len(ranges) > 1:
                second = bytes(data[ranges[1][0]:ranges[1][1]])
                if len(second) >= 3 and second[0] == 1:
                    info['loop'] = struct.unpack('<H', second[1:3])[0]
        elif intro == 0x2C:
            if p + 9 > n:
                raise Unsupported("truncated: an image descriptor runs past the end of the file")
            left, top, w, h, iflags = struct.unpack('<HHHHB', data[p:p + 9])
            p += 9
            if left + w > width or top + h > height:
                raise Unsupported("an image reaching beyond the logical screen (Pillow grows its canvas)")
            if w == 0 or h == 0:
                raise Unsupported("an image without pixels")
            palette = None
            if iflags & 0x80:
                size = 3 << ((iflags & 7) + 1)
                if p + size > n:
                    raise Unsupported("truncated: a local colour table runs past the end of the file")
                palette = bytes(data[p:p + size])
                p += size
                if _grey_ramp(palette):
                    raise Unsupported("a grey ramp as local colour table (Pillow shows such a frame through mode L)")
            elif info['global_palette'] is None:
                raise Unsupported("a frame with neither a local nor a global colour table")
            if p >= n:
                raise Unsupported("truncated: no image data")
            mcs = data[p]
            if not 2 <= mcs <= 8:
                raise Unsupported("a minimum code size of %d (2 .. 8 are decoded)" % mcs)
            ranges, p = _sub_blocks(data, p + 1, "an image")
            frames.append({'left': left, 'top': top, 'width': w, 'height': h, 'interlace': bool(iflags & 0x40),
                           'transparent': transparent, 'disposal': 0 if method < 2 else 2 if method == 2 else 3,
                           'duration': duration, 'palette': palette, 'min_code_size': mcs, 'blocks': ranges,
                           'stream_bytes': sum(e - s for s, e in ranges)})
            transparent, duration = None, 0
        # any other byte between blocks is skipped, as Pillow skips it
    if not frames:
        raise Unsupported("a file with no image")
    if width * height > MAX_PIXELS:
        raise Unsupported("a logical screen of more than 2^31 - 1 pixels")
    info['frames'] = frames
    return info


def lzw_stream(data, frame):
    """the joined data sub-blocks of one image (uint8 array)"""
    out = np.empty(frame['stream_bytes'], np.uint8)
    o = 0
    for s, e in frame['blocks']:
        out[o:o + e - s] = np.frombuffer(data, np.uint8, e - s, s)
        o += e - s
    return out


def palette_of(info, frame):
    """the colour table a frame is shown through: its local one, else the global one"""
    return frame['palette'] if frame['palette'] is not None else info['global_palette']


def _split(off):
    return off & 0x7FFFFFFF, off >> 31


def image_descriptor(frame, file_index, stream_off, palette_off, palette_entries, idx_off):
    """the int32 [DESC_WORDS] row of csm_gif_decode for one image (include/csm355.h)"""
    d = np.zeros(DESC_WORDS, np.int64)
    d[0], d[1], d[2], d[3] = frame['height'], frame['width'], frame['top'], frame['left']
    d[4], d[5], d[6] = stream_off, frame['stream_bytes'], frame['min_code_size']
    d[7] = FLAG_INTERLACE if frame['interlace'] else 0
    d[8] = -1 if frame['transparent'] is None else frame['transparent']
    d[9] = frame['disposal']
    d[10], d[11] = palette_off, palette_entries
    d[12], d[13] = _split(idx_off)
    d[14] = file_index
    if stream_off + frame['stream_bytes'] + 16 >= 2 ** 31 or palette_off + 768 >= 2 ** 31:
        raise Unsupported("more than 2 GiB of compressed data in one call")
    return d.astype(np.int32)


def file_descriptor(info, first_image, out_off, channels):
    """the int32 [FILE_WORDS] row of csm_gif_decode for one file"""
    d = np.zeros(FILE_WORDS, np.int64)
    d[0], d[1], d[2], d[3] = info['height'], info['width'], first_image, len(info['frames'])
    d[4], d[5] = _split(out_off)
    d[6] = info['background']
    d[7] = FILE_FLAG_ALPHA if info['frames'][0]['transparent'] is not None else 0
    return d.astype(np.int32)
