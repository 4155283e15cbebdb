"""Motion-JPEG AVI container (pure host code): the video file of the Ken Burns path, from frames that ops.jpeg_encode
compressed on the device.

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
