"""Host side of the WebP decoders (contracts DESIGN.md §4.15, lossless, and §4.16, lossy; pure Python / numpy, no device): the RIFF
container parser in front of csrc/webpdec.hip and csrc/webplossy.hip.  (webpcode.py is the encoders' host side.)

    probe(data)        a plain description of a WebP file the device decoder takes (size, the header's alpha flag, the byte range of
                       the VP8L chunk's payload), or Unsupported(reason).  It walks the RIFF chunk headers, checks every length
                       against the buffer and reads the five bytes of the VP8L header; it never interprets the entropy-coded data.
                       probe(data, lossy=True) also takes lossy files (below) and says which kind it met
    payload(..)        the VP8L (or VP8) chunk's payload of a probed file
    descriptor(..)     the int32 row of csm_webp_decode for one file
    lossy_descriptor(..)   the int32 row of csm_webp_lossy_decode for one file
    animation_frames(data)   the VP8 chunks and durations of an animated file as video.write_webp writes it

Accepted: a bare 'VP8L' file, and 'VP8X' followed by 'VP8L', where 'ICCP' and 'XMP ' chunks are ignored (libwebp and PIL hand back
the stored values, whatever the profile says) and an 'EXIF' chunk is taken when its orientation is absent or 1.  Refused, each with
its reason: lossy files ('VP8 ', with or without 'ALPH'), animations ('ANIM' / 'ANMF'), a version field other than 0, a RIFF or chunk
length that runs past the data, other orientations, and an 'XMP ' chunk that names an orientation (PIL's exif_transpose reads it).

With lossy=True also accepted: a bare 'VP8 ' file, and 'VP8X' (+ 'ICCP') (+ 'ALPH') + 'VP8 ' (+ 'EXIF' / 'XMP ' as above).  Read from
the ten plain bytes in front of the boolean-coded data and refused with a reason: a frame tag that is not a shown key frame of version
0..3, a wrong start code, a first-partition size that runs past the chunk, non-zero scale bits, a VP8X canvas that differs from the
frame size, a VP8X alpha flag that disagrees with the presence of 'ALPH', an 'ALPH' header byte with compression above 1 or reserved
bits set.

The rule behind every refusal: on a file probe accepts, the device result equals what PIL (libwebp) decodes on every byte.
"""
import struct

import numpy as np

DESC_WORDS = 12
GROUP_CAP = 2600                        # prefix-code groups per file (csrc/csm_vp8l.h kGroupCap); a file above it goes through imread
MAX_PIXELS = 89478485                   # PIL warns above this size and refuses twice as much: such files stay with imread
ERR_CAP = 32                            # the bit of a file's error word that says "valid, but more groups than the cap"
LOSSY_ERR_CAP = ERR_CAP << 8            # the same bit in csm_webp_lossy_decode's word: the alpha plane's stream is over the cap


class Unsupported(ValueError):
    """the file is not one the device decoder takes; str(e) is the reason.  `files`: for a refusal after the decode (more groups
    than GROUP_CAP), the indices of those files in the call"""
    files = ()


def probe(data, lossy=False):
    """see the module docstring.  Returns {'width', 'height', 'alpha' (the VP8L header's flag: False means A = 255 whatever the
    stream holds), 'payload' ((start, end) of the VP8L chunk's bytes), 'extended' (a VP8X file), 'orientation' (None or 1)}.
    With lossy=True the result also has 'kind': 'lossless' or 'lossy'; a lossy result's 'payload' is the VP8 chunk's byte range,
    'alph' the ALPH chunk's (or None), and 'alpha' says whether the file has an alpha plane."""
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
    kind_found, alph, alpha_flag = 'lossless', None, False
    while p < end and found is None:
        if p + 8 > end:
            raise Unsupported("a chunk header runs past the end of the file")
        kind = data[p:p + 4]
        length, = struct.unpack('<I', data[p + 4:p + 8])
        body = p + 8
        if length > end - body:
            raise Unsupported("chunk %r runs past the end of the file" % kind)
        if kind == b'VP8 ' and not lossy:
            raise Unsupported("a lossy file (VP8 ); only lossless (VP8L) is decoded")
        if kind == b'ALPH' and not lossy:
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
            extended, alpha_flag = True, bool(flags & 0x10)
        elif kind == b'VP8L':
            if alph is not None:
                raise Unsupported("an ALPH chunk in front of a lossless image")
            found = (body, body + length)
        elif kind == b'VP8 ':
            found, kind_found = (body, body + length), 'lossy'
        elif kind == b'ALPH' and extended:
            if alph is not None:
                raise Unsupported("a second ALPH chunk")
            alph = (body, body + length)
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
        raise Unsupported("no VP8L chunk" if not lossy else "no VP8L or VP8 chunk")
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
    if kind_found == 'lossy':
        return _probe_lossy(data, found, alph, alpha_flag, canvas, extended, orientation)
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
    info = {'width': width, 'height': height, 'alpha': alpha, 'payload': found, 'extended': extended, 'orientation': orientation}
    if lossy:
        info['kind'] = 'lossless'
    return info


def _probe_lossy(data, found, alph, alpha_flag, canvas, extended, orientation):
    """the ten plain bytes of a VP8 chunk and the first of an ALPH chunk; never the boolean-coded data"""
    s, e = found
    if e - s < 10:
        raise Unsupported("a VP8 chunk of %d bytes" % (e - s))
    tag = int.from_bytes(data[s:s + 3], 'little')
    if tag & 1 or not (tag >> 4) & 1 or (tag >> 1) & 7 > 3:
        raise Unsupported("a frame tag that is not a shown key frame of version 0..3")
    if data[s + 3:s + 6] != b'\x9d\x01\x2a':
        raise Unsupported("a VP8 chunk without its start code")
    if (tag >> 5) > e - s - 10:
        raise Unsupported("a first partition that runs past the VP8 chunk")
    w, h = struct.unpack('<HH', data[s + 6:s + 10])
    if (w | h) >> 14:
        raise Unsupported("a frame with scale bits set")
    width, height = w & 0x3fff, h & 0x3fff
    if width == 0 or height == 0:
        raise Unsupported("an empty frame")
    if canvas is not None and canvas != (width, height):
        raise Unsupported("a VP8X canvas of %dx%d around an image of %dx%d" % (canvas + (width, height)))
    if extended and alpha_flag != (alph is not None):
        raise Unsupported("a VP8X alpha flag that disagrees with the presence of an ALPH chunk")
    if alph is not None:
        if alph[1] - alph[0] < 1:
            raise Unsupported("an empty ALPH chunk")
        head = data[alph[0]]
        if head & 3 > 1 or head >> 6:
            raise Unsupported("an ALPH header byte of 0x%02x (compression 0 or 1, reserved bits 0 are decoded)" % head)
    if width * height > MAX_PIXELS:
        raise Unsupported("more pixels than imread takes without a warning")
    return {'width': width, 'height': height, 'alpha': alph is not None, 'payload': found, 'alph': alph, 'extended': extended,
            'orientation': orientation, 'kind': 'lossy'}


def payload(data, info):
    """the VP8L (a lossy file: the VP8) chunk's payload (uint8 array)"""
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


def lossy_descriptor(info, blob_off, out_off, channels=3, alph_head=0, alph_off=0):
    """the int32 [DESC_WORDS] row of csm_webp_lossy_decode (include/csm355.h); alph_head: the ALPH chunk's first byte, alph_off:
    where the bytes behind it stand in the blob"""
    s, e = info['payload']
    if channels not in (3, 4):
        raise ValueError("lossy_descriptor: 3 or 4 output channels")
    alph = info['alph']
    if max(blob_off + (e - s), alph_off + (alph[1] - alph[0] if alph else 0)) + 16 >= 2 ** 31:
        raise Unsupported("more than 2 GiB of compressed data in one call")
    d = np.zeros(DESC_WORDS, np.int64)
    d[0], d[1], d[2], d[3] = info['height'], info['width'], int(alph is not None), channels
    d[4], d[5] = blob_off, e - s
    d[7], d[8] = out_off & 0x7FFFFFFF, out_off >> 31
    if alph:
        d[6], d[9], d[10] = alph_head, alph_off, alph[1] - alph[0] - 1
    return d.astype(np.int32)


def animation_frames(data):
    """The frames of an animated file as video.write_webp writes it: 'VP8X' with the animation flag, 'ANIM', then 'ANMF' chunks
    that each stand at offset 0, cover the canvas and hold one bare 'VP8 ' chunk.  Returns (width, height, [(start, end) of every
    VP8 chunk's bytes], [duration in ms]); anything else (sub-rectangles, alpha, lossless frames) raises Unsupported."""
    data = bytes(data)
    n = len(data)
    if n < 12 or data[:4] != b'RIFF' or data[8:12] != b'WEBP':
        raise Unsupported("not a WebP file")
    end = struct.unpack('<I', data[4:8])[0] + 8
    if end > n:
        raise Unsupported("the RIFF length runs past the end of the file")
    p, canvas, frames, durations = 12, None, [], []
    while p + 8 <= end:
        kind = data[p:p + 4]
        length, = struct.unpack('<I', data[p + 4:p + 8])
        body = p + 8
        if length > end - body:
            raise Unsupported("chunk %r runs past the end of the file" % kind)
        if kind == b'VP8X':
            if p != 12 or length < 10 or not data[body] & 0x02:
                raise Unsupported("not an animated file")
            if data[body] & 0x10:
                raise Unsupported("an animation with alpha")
            canvas = (1 + int.from_bytes(data[body + 4:body + 7], 'little'), 1 + int.from_bytes(data[body + 7:body + 10], 'little'))
        elif canvas is None:
            raise Unsupported("not an animated file")
        elif kind == b'ANMF':
            if length < 16 + 8:
                raise Unsupported("a malformed ANMF chunk")
            x, y = int.from_bytes(data[body:body + 3], 'little'), int.from_bytes(data[body + 3:body + 6], 'little')
            size = (1 + int.from_bytes(data[body + 6:body + 9], 'little'), 1 + int.from_bytes(data[body + 9:body + 12], 'little'))
            if (x, y) != (0, 0) or size != canvas:
                raise Unsupported("an animation frame that does not cover the canvas")
            inner, ilen = data[body + 16:body + 20], struct.unpack('<I', data[body + 20:body + 24])[0]
            if inner != b'VP8 ' or length != 24 + ilen + (ilen & 1):
                raise Unsupported("an animation frame that is not one bare VP8 chunk (%s)" % inner.decode('latin-1'))
            found = (body + 24, body + 24 + ilen)
            info = _probe_lossy(data, found, None, False, canvas, False, None)
            frames.append(info['payload'])
            durations.append(int.from_bytes(data[body + 12:body + 15], 'little'))
        elif kind in (b'VP8 ', b'VP8L', b'ALPH'):
            raise Unsupported("a still image in an animated file")
        p = body + length + (length & 1)
    if not frames:
        raise Unsupported("an animation without frames")
    return canvas[0], canvas[1], frames, durations
