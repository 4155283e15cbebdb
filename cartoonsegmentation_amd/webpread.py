"""Host side of the lossless WebP decoder (contract DESIGN.md §4.15; pure Python / numpy, no device): the RIFF container parser in
front of csrc/webpdec.hip.  (webpcode.py is the encoders' host side.)

    probe(data)        a plain description of a WebP file the device decoder takes (size, the header's alpha flag, the byte range of
                       the VP8L chunk's payload), or Unsupported(reason).  It walks the RIFF chunk headers, checks every length
                       against the buffer and reads the five bytes of the VP8L header; it never interprets the entropy-coded data.
    payload(..)        the VP8L chunk's payload of a probed file
    descriptor(..)     the int32 row of csm_webp_decode for one file

Accepted: a bare 'VP8L' file, and 'VP8X' followed by 'VP8L', where 'ICCP' and 'XMP ' chunks are ignored (libwebp and PIL hand back
the stored values, whatever the profile says) and an 'EXIF' chunk is taken when its orientation is absent or 1.  Refused, each with
its reason: lossy files ('VP8 ', with or without 'ALPH'), animations ('ANIM' / 'ANMF'), a version field other than 0, a RIFF or chunk
length that runs past the data, other orientations, and an 'XMP ' chunk that names an orientation (PIL's exif_transpose reads it).

The rule behind every refusal: on a file probe accepts, the device result equals what PIL (libwebp) decodes on every byte.
"""
import struct

import numpy as np

DESC_WORDS = 12
GROUP_CAP = 2600                        # prefix-code groups per file (csrc/csm_vp8l.h kGroupCap); a file above it goes through imread
MAX_PIXELS = 89478485                   # PIL warns above this size and refuses twice as much: such files stay with imread
ERR_CAP = 32                            # the bit of a file's error word that says "valid, but more groups than the cap"


class Unsupported(ValueError):
    """the file is not one the device decoder takes; str(e) is the reason.  `files`: for a refusal after the decode (more groups
    than GROUP_CAP), the indices of those files in the call"""
    files = ()


def probe(data):
    """see the module docstring.  Returns {'width', 'height', 'alpha' (the VP8L header's flag: False means A = 255 whatever the
    stream holds), 'payload' ((start, end) of the VP8L chunk's bytes), 'extended' (a VP8X file), 'orientation' (None or 1)}."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("probe: bytes expected (got %s)" % type(data).__name__)
    data = bytes(data)
    n = len(data)
    if n < 12 or data[:4] != b'RIFF' or data[8:12] != b'WEBP':
        raise Unsupported("not a WebP file")
    riff, = struct.unpack('<I', data[4:8])
    if riff + 8 > n:
        raise Unsupported("the RIFF length runs past the end of the file")
    if riff < 4 or riff & 1:
        raise Unsupported("an invalid RIFF length")
    end = riff + 8                                          # bytes behind the RIFF chunk are ignored, as libwebp ignores them
    p = 12
    first, extended, canvas, found, orientation = True, False, None, None, None
    while p < end and found is None:
        if p + 8 > end:
            raise Unsupported("a chunk header runs past the end of the file")
        kind = data[p:p + 4]
        length, = struct.unpack('<I', data[p + 4:p + 8])
        body = p + 8
        if length > end - body:
            raise Unsupported("chunk %r runs past the end of the file" % kind)
        if kind == b'VP8 ':
            raise Unsupported("a lossy file (VP8 ); only lossless (VP8L) is decoded")
        if kind == b'ALPH':
            raise Unsupported("a lossy file with an alpha plane (ALPH); only lossless (VP8L) is decoded")
        if kind in (b'ANIM', b'ANMF'):
            raise Unsupported("an animated file (%s)" % kind.decode())
        if kind == b'VP8X':
            if not first or length < 10:
                raise Unsupported("a misplaced or malformed VP8X chunk")
            flags = data[body]
            if flags & 0x02:
                raise Unsupported("an animated file (VP8X animation flag)")
            canvas = (1 + int.from_bytes(data[body + 4:body + 7], 'little'), 1 + int.from_bytes(data[body + 7:body + 10], 'little'))
            extended = True
        elif kind == b'VP8L':
            found = (body, body + length)
        elif not extended:
            raise Unsupported("chunk %r in front of the image of a simple file" % kind)
        elif kind == b'EXIF':
            from . import jpegcode
            t = data[body:body + length]
            o = jpegcode._orientation(t if t[:6] == b'Exif\x00\x00' else b'Exif\x00\x00' + t)
            if o not in (None, 1):
                raise Unsupported("EXIF orientation %s" % o)
            orientation = o
        elif kind == b'XMP ':
            if b'Orientation' in data[body:body + length]:
                raise Unsupported("an XMP chunk that names an orientation")
        first = False
        p = body + length + (length & 1)
    if found is None:
        raise Unsupported("no VP8L chunk")
    # chunks behind the image: EXIF and XMP stand there in files libwebp's muxer wrote
    p = found[1] + ((found[1] - found[0]) & 1)
    while extended and p + 8 <= end:
        kind = data[p:p + 4]
        length, = struct.unpack('<I', data[p + 4:p + 8])
        body = p + 8
        if length > end - body:
            raise Unsupported("chunk %r runs past the end of the file" % kind)
        if kind in (b'ANIM', b'ANMF', b'VP8 ', b'VP8L', b'ALPH'):
            raise Unsupported("a second image or an animation chunk (%s) behind the image" % kind.decode('latin-1'))
        if kind == b'EXIF':
            from . import jpegcode
            t = data[body:body + length]
            o = jpegcode._orientation(t if t[:6] == b'Exif\x00\x00' else b'Exif\x00\x00' + t)
            if o not in (None, 1):
                raise Unsupported("EXIF orientation %s" % o)
            orientation = o
        elif kind == b'XMP ' and b'Orientation' in data[body:body + length]:
            raise Unsupported("an XMP chunk that names an orientation")
        p = body + length + (length & 1)
    s, e = found
    if e - s < 5:
        raise Unsupported("a VP8L chunk of %d bytes" % (e - s))
    if data[s] != 0x2f:
        raise Unsupported("a VP8L chunk without its signature byte")
    bits = int.from_bytes(data[s + 1:s + 5], 'little')
    width, height = (bits & 0x3fff) + 1, ((bits >> 14) & 0x3fff) + 1
    alpha, version = bool((bits >> 28) & 1), bits >> 29
    if version != 0:
        raise Unsupported("VP8L version %d (0 is decoded)" % version)
    if canvas is not None and canvas != (width, height):
        raise Unsupported("a VP8X canvas of %dx%d around an image of %dx%d" % (canvas + (width, height)))
    if width * height > MAX_PIXELS:
        raise Unsupported("more pixels than imread takes without a warning")
    return {'width': width, 'height': height, 'alpha': alpha, 'payload': found, 'extended': extended, 'orientation': orientation}


def payload(data, info):
    """the VP8L chunk's payload (uint8 array)"""
    s, e = info['payload']
    return np.frombuffer(data, np.uint8, e - s, s)


def descriptor(info, blob_off, out_off, channels=3):
    """the int32 [DESC_WORDS] row of csm_webp_decode (include/csm355.h)"""
    s, e = info['payload']
    if channels not in (3, 4):
        raise ValueError("descriptor: 3 or 4 output channels")
    if blob_off + (e - s) + 16 >= 2 ** 31:
        raise Unsupported("more than 2 GiB of compressed data in one call")
    d = np.zeros(DESC_WORDS, np.int64)
    d[0], d[1], d[2], d[3] = info['height'], info['width'], int(info['alpha']), channels
    d[4], d[5] = blob_off, e - s
    d[7], d[8] = out_off & 0x7FFFFFFF, out_off >> 31
    return d.astype(np.int32)
