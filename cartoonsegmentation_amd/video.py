"""Motion-JPEG AVI container, animated-PNG container, animated-GIF and animated-WebP file (pure host code): the video files of the
Ken Burns path, from frames that ops.jpeg_encode / ops.png_streams / ops.gif_streams / ops.webp_streams compressed on the device.
read_webp reads the animated WebP files back, its frames decoded on the device.

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
