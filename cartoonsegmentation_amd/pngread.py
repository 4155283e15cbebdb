"""Host side of the PNG decoder (contract DESIGN.md §4.9; pure Python / numpy, no device): the chunk parser in front of
csrc/pngdec.hip.  (pngcode.py is the encoder's host side.)

    probe(data)        a plain description of a PNG file the device decoder takes (size, colour type, palette, the byte ranges of the
                       IDAT payloads, the stream's last four bytes), or Unsupported(reason).  It walks chunk headers, checks every chunk
                       length against the buffer, the chunk order, every chunk's CRC and the two bytes of the zlib header; it never
                       interprets the deflate data.
    zlib_stream(..)    the concatenated IDAT payloads of a probed file
    descriptor(..)     the int32 row of csm_png_decode for one file

The rule behind every refusal: on a file probe accepts, the device result equals utils.io_utils.imread (PIL's decode, EXIF
orientation applied, converted to RGB) on every byte.  Where PIL does more with a chunk than ignore it, the file is refused and goes
through imread as before.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
DESC_WORDS = 12
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
MAX_RAW_BYTES = 2 ** 31 - 1             # H * (1 + W * channels): positions in the raw bytes are 32 bits on the device
MAX_PIXELS = 89478485                   # PIL warns above this size and refuses twice as much: such files stay with imread
# text chunks through which PIL finds an orientation (Image.getexif)
ORIENTATION_KEYWORDS = (b'Raw profile type exif', b'XML:com.adobe.xmp')
KNOWN_CRITICAL = (b'IHDR', b'PLTE', b'IDAT', b'IEND')


class Unsupported(ValueError):
    """the file is not one the device decoder takes; str(e) is the reason"""


def _exif_orientation(t):
    """orientation of the TIFF block of an eXIf chunk: 0 when it has none, 1..8, or -1 for a block this parser does not follow"""
    if len(t) < 8 or t[:2] not in (b'II', b'MM'):
        return -1
    e = '<' if t[:2] == b'II' else '>'
    if struct.unpack(e + 'H', t[2:4])[0] != 42:
        return -1
    off = struct.unpack(e + 'I', t[4:8])[0]
    if off + 2 > len(t):
        return -1
    n = struct.unpack(e + 'H', t[off:off + 2])[0]
    if off + 2 + 12 * n > len(t):
        return -1
    for k in range(n):
        p = off + 2 + 12 * k
        tag, typ, cnt = struct.unpack(e + 'HHI', t[p:p + 8])
        if tag == 0x0112:
            if typ != 3 or cnt != 1:
                return -1
            return struct.unpack(e + 'H', t[p + 8:p + 10])[0]
    return 0


def probe(data):
    """see the module docstring.  Returns {'width', 'height', 'colour_type', 'channels', 'palette' (uint8 [256, 3], R G B,
    zero-padded), 'idat' (list of (start, end) payload ranges, empty ones included), 'stream_bytes', 'adler' (the last four bytes of the stream: the Adler-32
    trailer unless bytes follow it, which zlib, PIL and the device decoder ignore; the device reads the trailer behind the deflate data's
    end), 'orientation' (None or 1)}."""
    data = memoryview(data).cast('B') if not isinstance(data, (bytes, bytearray)) else data
    n = len(data)
    if n < 8 or bytes(data[:8]) != SIGNATURE:
        raise Unsupported("not a PNG file")
    p = 8
    info = None
    palette = None
    idat, idat_closed, seen_iend, orientation = [], False, False, None
    first = True
    while p < n:
        if p + 12 > n:
            raise Unsupported("a chunk header runs past the end of the file")
        length, = struct.unpack('>I', data[p:p + 4])
        kind = bytes(data[p + 4:p + 8])
        if length > n - p - 12:
            raise Unsupported("chunk %r runs past the end of the file" % kind)
        body = p + 8
        crc, = struct.unpack('>I', data[body + length:body + length + 4])
        if zlib.crc32(data[p + 4:body + length]) != crc:
            raise Unsupported("chunk %r has a bad CRC" % kind)
        if first != (kind == b'IHDR'):
            raise Unsupported("IHDR is not the first chunk, or not the only one")
        first = False
        if kind == b'IHDR':
            if length != 13:
                raise Unsupported("IHDR of %d bytes" % length)
            w, h, depth, ct, comp, filt, lace = struct.unpack('>IIBBBBB', data[body:body + 13])
            if w == 0 or h == 0 or w >= 2 ** 31 or h >= 2 ** 31:
                raise Unsupported("zero or invalid width or height")
            if ct not in CHANNELS:
                raise Unsupported("colour type %d" % ct)
            if depth != 8:
                raise Unsupported("bit depth %d (8 is decoded)" % depth)
            if comp != 0 or filt != 0:
                raise Unsupported("unknown compression or filter method")
            if lace != 0:
                raise Unsupported("interlaced (Adam7)")
            if h * (1 + w * CHANNELS[ct]) > MAX_RAW_BYTES:
                raise Unsupported("the raw image data exceed 32-bit positions")
            if w * h > MAX_PIXELS:
                raise Unsupported("more pixels than imread takes without a warning")
            info = {'width': w, 'height': h, 'colour_type': ct, 'channels': CHANNELS[ct]}
        elif kind == b'PLTE':
            if palette is not None or idat or length == 0 or length % 3 or length > 768:
                raise Unsupported("a misplaced or malformed PLTE chunk")
            palette = np.zeros((256, 3), np.uint8)
            palette[:length // 3] = np.frombuffer(data, np.uint8, length, body).reshape(-1, 3)
        elif kind == b'IDAT':
            if idat_closed:
                raise Unsupported("IDAT chunks that are not consecutive")
            idat.append((body, body + length))
        elif kind == b'IEND':
            seen_iend = True
            break
        elif kind in (b'acTL', b'fcTL', b'fdAT'):
            raise Unsupported("an animated PNG (%s)" % kind.decode())
        elif kind == b'eXIf':
            o = _exif_orientation(bytes(data[body:body + length]))
            if o not in (0, 1):
                raise Unsupported("EXIF orientation %s" % ("unreadable" if o < 0 else o))
            orientation = 1 if o == 1 else orientation
        elif kind in (b'tEXt', b'zTXt', b'iTXt'):
            text = bytes(data[body:body + min(length, 80)])
            key = text.split(b'\x00', 1)[0]
            if key in ORIENTATION_KEYWORDS:
                raise Unsupported("a text chunk %r that may carry an orientation" % key.decode('latin-1'))
            if kind == b'zTXt' or (kind == b'iTXt' and length >= len(key) + 2 and data[body + len(key) + 1] != 0):
                raise Unsupported("a compressed text chunk (PIL inflates it while opening, with limits of its own)")
        elif not (kind[0] & 0x20) and kind not in KNOWN_CRITICAL:
            raise Unsupported("unknown critical chunk %r" % kind)
        if idat and kind != b'IDAT':
            idat_closed = True
        p = body + length + 4
    if info is None:
        raise Unsupported("no IHDR chunk")
    if not idat:
        raise Unsupported("no IDAT chunk")
    if not seen_iend:
        raise Unsupported("no IEND chunk")
    if info['colour_type'] == 3 and palette is None:
        raise Unsupported("a palette image without PLTE")
    total = sum(e - s for s, e in idat)
    if total < 6:
        raise Unsupported("a zlib stream of %d bytes" % total)
    # the first two and the last four bytes of the stream, wherever the chunk boundaries fall
    head, tail = bytearray(), bytearray()
    for s, e in idat:
        if len(head) < 2:
            head += data[s:min(e, s + 2 - len(head))]
    for s, e in reversed(idat):
        if len(tail) < 4:
            tail[:0] = data[max(s, e - (4 - len(tail))):e]
    cmf, flg = head[0], head[1]
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or (flg & 0x20) or (cmf * 256 + flg) % 31:
        raise Unsupported("a zlib header the decoder does not take (CM 8, window <= 32 KiB, no FDICT, FCHECK)")
    info['palette'] = palette if palette is not None else np.zeros((256, 3), np.uint8)
    info['idat'] = idat
    info['stream_bytes'] = total
    info['adler'] = int.from_bytes(bytes(tail), 'big')
    info['orientation'] = orientation
    return info


def zlib_stream(data, info):
    """the concatenated IDAT payloads (uint8 array): the file's zlib stream"""
    out = np.empty(info['stream_bytes'], np.uint8)
    o = 0
    for s, e in info['idat']:
        out[o:o + e - s] = np.frombuffer(data, np.uint8, e - s, s)
        o += e - s
    return out


def descriptor(info, stream_off, palette_off, out_off):
    """the int32 [DESC_WORDS] row of csm_png_decode (include/csm355.h)"""
    d = np.zeros(DESC_WORDS, np.int64)
    d[0], d[1], d[2] = info['height'], info['width'], info['colour_type']
    d[3], d[4], d[5] = stream_off, info['stream_bytes'], palette_off
    d[7], d[8] = out_off & 0x7FFFFFFF, out_off >> 31
    if stream_off + info['stream_bytes'] + 16 >= 2 ** 31 or palette_off + 768 >= 2 ** 31:
        raise Unsupported("more than 2 GiB of compressed data in one call")
    return d.astype(np.int32)
