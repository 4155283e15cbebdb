"""Motion-JPEG AVI container, animated-PNG container, animated-GIF and animated-WebP file (pure host code): the video files of the
Ken Burns path, from frames that ops.jpeg_encode / ops.png_streams / ops.gif_streams / ops.webp_streams compressed on the device.
read_video reads all four back (read_avi, read_apng, read_gif, read_webp), the frames decoded on the device; the container
parsers behind read_avi and read_apng (avi_frames, apng_frames) are host-only.

A classic RIFF AVI (AVI 1.0, no OpenDML extension, so below 2 GiB):

    RIFF 'AVI '
      LIST 'hdrl'
        'avih'  MainAVIHeader (56 B)
        LIST 'strl'
          'strh'  AVIStreamHeader (56 B): 'vids' / 'MJPG'
          'strf'  BITMAPINFOHEADER (40 B): biCompression 'MJPG', 24 bit
      LIST 'movi'
        '00dc' <JPEG file> ...          one chunk per output frame, padded to an even size
      'idx1'  16 B per chunk: '00dc', AVIIF_KEYFRAME, offset from the 'movi' fourcc, size

An APNG (APNG specification 1.0) is a PNG whose first frame is the default image:

    signature, IHDR, acTL (frames, plays = 0: for ever)
    fcTL (sequence 0), IDAT <zlib stream of frame 0>
    fcTL, fdAT <sequence number + zlib stream> ...      per further output frame; sequence numbers count fcTL and fdAT together
    IEND

An animated GIF (GIF89a) is laid out by gifcode.gif_file, an animated WebP by webpcode.animation_file
(DESIGN.md §4.12).
"""
import struct

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
MAX_FILE_BYTES = 2 ** 31              # RIFF sizes of an AVI 1.0 file stay below 2 GiB


def _chunk(fourcc, payload):
    return fourcc + struct.pack('<I', len(payload)) + payload + (b'\x00' if len(payload) & 1 else b'')


def _list(kind, payload):
    return b'LIST' + struct.pack('<I', 4 + len(payload)) + kind + payload


def playback_order(n):
    """the reference's ping-pong (kenburns_effect.py:1088: seq + seq[::-1][1:-1]) as indices into n frames"""
    seq = list(range(n))
    return seq + seq[::-1][1:-1]


def write_mjpeg_avi(path, jpegs, width, height, fps=25, order=None):
    """Write the JPEG files `jpegs` (a list of bytes, all width x height) as a Motion-JPEG AVI at `fps` frames per second.
    `order` lists, for each output chunk, the index of the encoded frame it takes (default: every frame once, in order), so a
    frame is encoded once and may be written several times.  Raises ValueError for a file of 2 GiB or more (OpenDML is not
    written).  Returns the number of bytes written."""
    order = list(range(len(jpegs))) if order is None else [int(i) for i in order]
    if any(i < 0 or i >= len(jpegs) for i in order):
        raise ValueError("write_mjpeg_avi: order refers to a frame outside the %d encoded ones" % len(jpegs))
    width, height, fps = int(width), int(height), int(fps)
    if not (1 <= width <= 65535 and 1 <= height <= 65535 and fps >= 1):
        raise ValueError("write_mjpeg_avi: width and height must be in [1, 65535] and fps >= 1")
    n = len(order)
    sizes = [len(jpegs[i]) for i in order]
    padded = [s + (s & 1) for s in sizes]
    movi_bytes = 4 + sum(8 + p for p in padded)                    # 'movi' + the chunks
    biggest = max(sizes, default=0)
    usec = (1000000 + fps // 2) // fps
    avih = struct.pack('<14I', usec, min(biggest * fps, 0xFFFFFFFF), 0, AVIF_HASINDEX, n, 0, 1, biggest, width, height, 0, 0, 0, 0)
    strh = b'vids' + b'MJPG' + struct.pack('<IHHIIIIIIIIHHHH', 0, 0, 0, 0, 1, fps, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack('<IiiHH4sIiiII', 40, width, height, 1, 24, b'MJPG', width * height * 3, 0, 0, 0, 0)
    hdrl = _list(b'hdrl', _chunk(b'avih', avih) + _list(b'strl', _chunk(b'strh', strh) + _chunk(b'strf', strf)))
    idx1_bytes = 8 + 16 * n
    riff_bytes = 4 + len(hdrl) + 8 + movi_bytes + idx1_bytes       # after the 8 bytes of 'RIFF' <size>
    if riff_bytes + 8 >= MAX_FILE_BYTES:
        raise ValueError("write_mjpeg_avi: the file would take %d bytes; AVI 1.0 stays below 2 GiB (OpenDML is not written)" % (riff_bytes + 8))
    index = []
    off = 4                                                        # from the 'movi' fourcc
    for s, p in zip(sizes, padded):
        index.append(b'00dc' + struct.pack('<III', AVIIF_KEYFRAME, off, s))
        off += 8 + p
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', riff_bytes) + b'AVI ' + hdrl)
        f.write(b'LIST' + struct.pack('<I', movi_bytes) + b'movi')
        for i in order:
            f.write(_chunk(b'00dc', jpegs[i]))
        f.write(_chunk(b'idx1', b''.join(index)))
    return riff_bytes + 8


def write_apng(path, streams, width, height, colour_type, fps=25, order=None):
    """Write the zlib streams `streams` (a list of bytes from ops.png_streams, all width x height of `colour_type` 0 grey or 2 RGB)
    as a lossless animated PNG that shows every frame for 1 / fps seconds and loops for ever.  `order` as in write_mjpeg_avi: a
    frame is encoded once and may be written several times.  Every frame covers the whole canvas (dispose NONE, blend SOURCE).
    Returns the number of bytes written."""
    from .pngcode import PNG_SIGNATURE, chunk, ihdr
    order = list(range(len(streams))) if order is None else [int(i) for i in order]
    if not order:
        raise ValueError("write_apng: at least one frame is needed")
    if any(i < 0 or i >= len(streams) for i in order):
        raise ValueError("write_apng: order refers to a frame outside the %d encoded ones" % len(streams))
    width, height, fps = int(width), int(height), int(fps)
    if not (1 <= width <= 65535 and 1 <= height <= 65535 and 1 <= fps <= 65535 and colour_type in (0, 2)):
        raise ValueError("write_apng: width, height and fps must be in [1, 65535] and colour_type 0 or 2")
    parts = [PNG_SIGNATURE, ihdr(width, height, colour_type), chunk(b'acTL', struct.pack('>II', len(order), 0))]
    seq = 0
    for k, i in enumerate(order):
        parts.append(chunk(b'fcTL', struct.pack('>IIIIIHHBB', seq, width, height, 0, 0, 1, fps, 0, 0)))
        seq += 1
        if k == 0:
            parts.append(chunk(b'IDAT', streams[i]))
        else:
            parts.append(chunk(b'fdAT', struct.pack('>I', seq) + streams[i]))
            seq += 1
    parts.append(chunk(b'IEND', b''))
    data = b''.join(parts)
    with open(path, 'wb') as f:
        f.write(data)
    return len(data)


def write_gif(path, streams, width, height, palette, fps=25, loop=0, order=None):
    """Write the LZW streams `streams` (a list of bytes from ops.gif_streams, all width x height, indices into the uint8 [256,3]
    R, G, B `palette`) as an animated GIF that shows every frame for round(100 / fps) centiseconds and repeats `loop` times (0: for
    ever).  `order` as in write_mjpeg_avi: a frame is coded once and may be written several times.  Returns the number of bytes
    written."""
    from .gifcode import gif_file
    data = gif_file(streams, width, height, palette, fps=fps, loop=loop, order=order)
    with open(path, 'wb') as f:
        f.write(data)
    return len(data)


def write_webp(path, streams, width, height, fps=25, loop=0, order=None):
    """Write the VP8 key frames `streams` (a list of bytes from ops.webp_streams, all width x height) as an animated WebP that
    shows every frame for round(1000 / fps) ms and repeats `loop` times (0: for ever).  `order` as in write_mjpeg_avi: a frame is
    coded once and may be written several times.  Returns the number of bytes written."""
    from .webpcode import animation_file
    data = animation_file(streams, width, height, fps=fps, loop=loop, order=order)
    with open(path, 'wb') as f:
        f.write(data)
    return len(data)


def read_webp(path_or_bytes, device=None):
    """Read an animated WebP as write_webp writes it (every frame at offset 0, covering the canvas, one bare VP8 key frame without
    alpha): (uint8 device tensor [n,H,W,3] in B, G, R order, frames in file order; the n durations in ms).  All frames are decoded
    in one ops.webp_decode call (the lossy decoder, DESIGN.md §4.16: equal to what PIL shows after seek(i) on every byte); only the
    VP8 chunks' bytes are uploaded.  Any other animation (sub-rectangles, alpha, lossless frames) raises webpread.Unsupported."""
    import torch
    from . import ops, webpread
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, 'rb') as f:
            data = f.read()
    width, height, frames, durations = webpread.animation_frames(data)
    infos = [{'width': width, 'height': height, 'alpha': False, 'payload': fr, 'alph': None, 'extended': False, 'orientation': None,
              'kind': 'lossy'} for fr in frames]
    tensors = ops.webp_decode([data] * len(frames), device, _infos=infos, lossy=True)
    return torch.stack(tensors), durations


class Unsupported(ValueError):
    """the clip is not one read_avi / read_apng take; str(e) is the reason"""


def _file_bytes(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes)
    with open(path_or_bytes, 'rb') as f:
        return f.read()


def _riff_chunks(data, start, end, what):
    """(fourcc, payload start, payload size) of the chunks in data[start:end], every size checked against the range"""
    p = start
    while p + 8 <= end:
        fourcc = bytes(data[p:p + 4])
        size, = struct.unpack('<I', data[p + 4:p + 8])
        if size > end - p - 8:
            raise Unsupported("truncated: chunk %r of %s runs past its end" % (fourcc, what))
        yield fourcc, p + 8, size
        p += 8 + size + (size & 1)


def avi_frames(data):
    """Host only: (width, height, the JPEG files of the '00dc' chunks in 'movi' order, ms per frame as a float) of an AVI 1.0 file
    with one Motion-JPEG video stream, as write_mjpeg_avi writes it.  An OpenDML file, a second stream, another codec, a chunk that
    is no complete JPEG file (SOI ... EOI) or a truncated container raises Unsupported; nothing inside the JPEG data is
    interpreted (jpegcode.probe does that)."""
    data = bytes(data)
    if len(data) < 12 or data[:4] != b'RIFF' or data[8:12] != b'AVI ':
        raise Unsupported("not a RIFF AVI file")
    riff_end = 8 + struct.unpack('<I', data[4:8])[0]
    if riff_end > len(data):
        raise Unsupported("truncated: the RIFF size runs past the end of the file")
    if data[riff_end:riff_end + 4] == b'RIFF':
        raise Unsupported("an OpenDML file (a second RIFF list)")
    strh = strf = None
    streams, frames, seen_movi = 0, [], False
    for fourcc, at, size in _riff_chunks(data, 12, riff_end, "the file"):
        if fourcc != b'LIST' or size < 4:
            continue
        kind = data[at:at + 4]
        if kind == b'hdrl':
            for f2, at2, size2 in _riff_chunks(data, at + 4, at + size, "'hdrl'"):
                if f2 == b'LIST' and data[at2:at2 + 4] == b'strl':
                    streams += 1
                    for f3, at3, size3 in _riff_chunks(data, at2 + 4, at2 + size2, "'strl'"):
                        if f3 == b'strh' and strh is None:
                            strh = data[at3:at3 + size3]
                        elif f3 == b'strf' and strf is None:
                            strf = data[at3:at3 + size3]
                elif f2 == b'LIST' and data[at2:at2 + 4] == b'odml':
                    raise Unsupported("an OpenDML file ('odml' header)")
        elif kind == b'movi':
            if seen_movi:
                raise Unsupported("more than one 'movi' list")
            seen_movi = True
            for f2, at2, size2 in _riff_chunks(data, at + 4, at + size, "'movi'"):
                if f2 == b'00dc':
                    frames.append(data[at2:at2 + size2])
                elif f2 == b'LIST':
                    raise Unsupported("'rec ' lists inside 'movi'")
    if streams != 1 or strh is None or strf is None or len(strh) < 32 or len(strf) < 20:
        raise Unsupported("one video stream with 'strh' and 'strf' is expected (found %d stream lists)" % streams)
    if strh[:4] != b'vids':
        raise Unsupported("stream 0 is %r, not video" % strh[:4])
    handler, compression = strh[4:8].upper(), strf[16:20].upper()
    if compression != b'MJPG' or handler not in (b'MJPG', b'\x00\x00\x00\x00'):
        raise Unsupported("codec %r / %r (Motion-JPEG is read)" % (strh[4:8], strf[16:20]))
    scale, rate = struct.unpack('<II', strh[20:28])
    if scale == 0 or rate == 0:
        raise Unsupported("a frame rate of %d / %d" % (rate, scale))
    width, height = struct.unpack('<ii', strf[4:12])
    if not seen_movi or not frames:
        raise Unsupported("no '00dc' chunk")
    for k, fr in enumerate(frames):
        if len(fr) < 4 or fr[:2] != b'\xff\xd8' or fr[-2:] != b'\xff\xd9':
            raise Unsupported("chunk %d is not a complete JPEG file" % k)
    return width, abs(height), frames, 1000.0 * scale / rate


def read_avi(path_or_bytes, device=None):
    """Read a Motion-JPEG AVI as write_mjpeg_avi writes it, or any AVI 1.0 file whose '00dc' chunks are complete baseline JPEG files
    of one size: (uint8 device tensor [n,H,W,3] in B, G, R order, chunks in 'movi' order; the n durations in ms, from the stream
    header's scale / rate).  All chunks are decoded in one ops.jpeg_decode call; only their bytes are uploaded.
    Anything else raises video.Unsupported or jpegcode.Unsupported (a JPEG without Huffman tables, a progressive one)."""
    import torch
    from . import jpegcode, ops
    width, height, frames, ms = avi_frames(_file_bytes(path_or_bytes))
    infos = [jpegcode.probe(f) for f in frames]
    if any((i['width'], i['height']) != (width, height) for i in infos):
        raise Unsupported("JPEG chunks whose size is not the stream's %d x %d" % (width, height))
    return torch.stack(ops.jpeg_decode(frames, device, _infos=infos)), [ms] * len(frames)


def apng_frames(data):
    """Host only: (width, height, one stand-alone PNG file per frame, the durations in ms as floats) of an APNG as write_apng writes
    it: 8 bits, colour type 0 or 2, not interlaced, every frame covering the canvas at offset 0 with dispose NONE and blend SOURCE,
    the default image being frame 0.  Each file is rebuilt from the frame's IDAT / fdAT payloads under the APNG's IHDR; the zlib
    data are not touched.  Anything else raises Unsupported."""
    import zlib
    from .pngcode import PNG_SIGNATURE, chunk
    data = bytes(data)
    if data[:8] != PNG_SIGNATURE:
        raise Unsupported("not a PNG file")
    p, n = 8, len(data)
    ihdr_body, frames_declared, seq = None, None, 0
    frames, durations, current, ended = [], [], None, False
    while p < n:
        if p + 12 > n:
            raise Unsupported("truncated: a chunk header runs past the end of the file")
        length, = struct.unpack('>I', data[p:p + 4])
        kind = data[p + 4:p + 8]
        if length > n - p - 12:
            raise Unsupported("truncated: chunk %r runs past the end of the file" % kind)
        body = data[p + 8:p + 8 + length]
        if zlib.crc32(data[p + 4:p + 8 + length]) != struct.unpack('>I', data[p + 8 + length:p + 12 + length])[0]:
            raise Unsupported("chunk %r has a bad CRC" % kind)
        p += 12 + length
        if (ihdr_body is None) != (kind == b'IHDR'):
            raise Unsupported("IHDR is not the first chunk, or not the only one")
        if kind == b'IHDR':
            if length != 13:
                raise Unsupported("IHDR of %d bytes" % length)
            width, height, depth, ct, comp, filt, lace = struct.unpack('>IIBBBBB', body)
            if depth != 8 or ct not in (0, 2) or comp or filt or lace:
                raise Unsupported("bit depth %d, colour type %d, interlace %d (8 bits, grey or RGB, not interlaced are read)" % (depth, ct, lace))
            ihdr_body = body
        elif kind == b'acTL':
            if length != 8 or frames_declared is not None or frames:
                raise Unsupported("a misplaced or malformed acTL chunk")
            frames_declared = struct.unpack('>I', body[:4])[0]
        elif kind == b'fcTL':
            if length != 26 or frames_declared is None:
                raise Unsupported("a misplaced or malformed fcTL chunk")
            s, w, h, x, y, num, den, dispose, blend = struct.unpack('>IIIIIHHBB', body)
            if s != seq:
                raise Unsupported("sequence number %d where %d is due" % (s, seq))
            seq += 1
            if (w, h, x, y) != (width, height, 0, 0):
                raise Unsupported("a frame that does not cover the canvas")
            if dispose != 0 or blend != 0:
                raise Unsupported("dispose %d / blend %d (NONE / SOURCE are read)" % (dispose, blend))
            if current is not None and not current:
                raise Unsupported("a frame without data")
            current = []
            frames.append(current)
            durations.append(1000.0 * num / (den or 100))
        elif kind == b'IDAT':
            if frames_declared is None:
                raise Unsupported("not an animated PNG (no acTL chunk before the image data)")
            if current is None or len(frames) != 1:
                raise Unsupported("a default image that is not frame 0")
            current.append(body)
        elif kind == b'fdAT':
            if current is None or len(frames) < 2 or length < 4:
                raise Unsupported("a misplaced fdAT chunk")
            if struct.unpack('>I', body[:4])[0] != seq:
                raise Unsupported("sequence number %d where %d is due" % (struct.unpack('>I', body[:4])[0], seq))
            seq += 1
            current.append(body[4:])
        elif kind == b'IEND':
            ended = True
            break
        elif kind in (b'PLTE', b'tRNS'):
            raise Unsupported("a %s chunk (palette and transparency are not read)" % kind.decode())
        elif not (kind[0] & 0x20):
            raise Unsupported("unknown critical chunk %r" % kind)
    if ihdr_body is None or not ended:
        raise Unsupported("truncated: no IHDR or no IEND chunk")
    if frames_declared is None:
        raise Unsupported("not an animated PNG (no acTL chunk)")
    if not frames or len(frames) != frames_declared or not frames[-1]:
        raise Unsupported("%d frames with data where acTL declares %d" % (len(frames), frames_declared))
    files = [PNG_SIGNATURE + chunk(b'IHDR', ihdr_body) + chunk(b'IDAT', b''.join(parts)) + chunk(b'IEND', b'') for parts in frames]
    return width, height, files, durations


def read_apng(path_or_bytes, device=None):
    """Read an animated PNG as write_apng writes it (see apng_frames): (uint8 device tensor [n,H,W,3] in B, G, R order, grey frames
    with three equal channels; the n durations in ms, from the fcTL chunks).  The host rebuilds one stand-alone PNG per frame and
    all of them are decoded in one ops.png_decode call; only the compressed bytes are uploaded.  Anything else
    raises video.Unsupported."""
    import torch
    from . import ops
    _, _, files, durations = apng_frames(_file_bytes(path_or_bytes))
    return torch.stack(ops.png_decode(files, device)), durations


def read_gif(path_or_bytes, device=None, alpha=False):
    """Read a GIF file, animated or not: (uint8 device tensor [n,H,W,3] in B, G, R order or, with alpha=True, [n,H,W,4] in B, G, R,
    A order, frame i equal on every byte to what PIL shows after seek(i); the n durations in ms).  Everything behind the container
    walk runs on the device in one ops.gif_decode call; only the compressed bytes and the colour tables are
    uploaded.  The loop count is gifread.probe(data)['loop'].  A file the decoder does not take raises gifread.Unsupported."""
    from . import gifread, ops
    data = _file_bytes(path_or_bytes)
    info = gifread.probe(data)
    return ops.gif_decode(data, device, alpha=alpha, _infos=[info]), [fr['duration'] for fr in info['frames']]


def read_video(path, device=None):
    """The reader for what kenburns.npyframes2video writes, by suffix: .gif (read_gif), .avi (read_avi), .apng (read_apng), .webp
    (read_webp): (uint8 device tensor [n,H,W,3] in B, G, R order; the n durations in ms).  Any other suffix raises ValueError."""
    import os
    suffix = os.path.splitext(str(path))[1].lower()
    readers = {'.gif': read_gif, '.avi': read_avi, '.apng': read_apng, '.webp': read_webp}
    if suffix not in readers:
        raise ValueError("read_video: %r is not read here (.gif, .avi, .apng and .webp are)" % suffix)
    return readers[suffix](path, device)
