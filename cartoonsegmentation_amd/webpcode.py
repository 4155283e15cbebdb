"""Host side of the WebP writer (contract DESIGN.md §4.12; device side csrc/webp.hip): the VP8 frame header around the partitions
the device coded, and the RIFF containers of a still and of an animation.  Pure Python; no device code."""
import math
import numbers
import struct

MAX_SIDE = 16383               # the frame header and the VP8X canvas hold 14-bit sizes
MAX_FIRST_BYTES = 1 << 19      # the frame tag holds the first partition's size in 19 bits
MAX_PART_BYTES = 1 << 24       # a token partition's size is written in 3 bytes
MAX_FILE_BYTES = 2 ** 32 - 10  # RIFF sizes are 32 bits


def check_size(width, height, what="webp"):
    width, height = int(width), int(height)
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise ValueError("%s: width and height must be in [1, %d] (got %dx%d)" % (what, MAX_SIDE, width, height))
    return width, height


def check_quality(quality, what="webp"):
    if isinstance(quality, bool) or not isinstance(quality, numbers.Integral) or not 1 <= quality <= 100:
        raise ValueError("%s: quality must be an integer in [1, 100] (got %r)" % (what, quality))
    return int(quality)


def quality_to_qi(quality):
    """the frame's one quantiser index: quality 100..1 onto 0..127, ((100 - quality) * 127 + 49) // 99"""
    return ((100 - int(quality)) * 127 + 49) // 99


def partitions(height):
    """token partitions of a frame: min(8, the largest power of two not above its macroblock rows), so that none is empty"""
    rows = (int(height) + 15) // 16
    return 1 << min(3, rows.bit_length() - 1)


def duration_ms(fps):
    """the frame duration in milliseconds: 1000 / fps rounded half up; ValueError outside [1, 2^24 - 1]"""
    try:
        fps = float(fps)
    except (TypeError, ValueError):
        raise ValueError("webp: fps must be a number (got %r)" % (fps,))
    d = int(math.floor(1000.0 / fps + 0.5)) if fps > 0 and math.isfinite(fps) else 0
    if not 1 <= d < 1 << 24:
        raise ValueError("webp: fps %r gives a frame duration of %d ms; it must be in [1, 16777215]" % (fps, d))
    return d


def vp8_frame(first, parts, width, height):
    """One VP8 key frame from its coded partitions: the 3-byte frame tag (key frame, version 1, shown, the first partition's
    size), the start code 9D 01 2A, width and height (scale 0), the first partition, the size of every token partition but the
    last in 3 bytes, the token partitions."""
    width, height = check_size(width, height)
    if len(parts) != partitions(height):
        raise ValueError("webp: %d token partitions for a frame of height %d (expected %d)" % (len(parts), height, partitions(height)))
    if len(first) >= MAX_FIRST_BYTES or any(len(p) >= MAX_PART_BYTES for p in parts):
        raise ValueError("webp: a partition is too long for the frame header (first %d bytes, largest token partition %d)"
                         % (len(first), max(len(p) for p in parts)))
    tag = 0 | 1 << 1 | 1 << 4 | len(first) << 5
    head = struct.pack('<I', tag)[:3] + b'\x9d\x01\x2a' + struct.pack('<HH', width, height)
    return head + bytes(first) + b''.join(struct.pack('<I', len(p))[:3] for p in parts[:-1]) + b''.join(bytes(p) for p in parts)


def _chunk(fourcc, payload):
    return fourcc + struct.pack('<I', len(payload)) + payload + (b'\x00' if len(payload) & 1 else b'')


def _u24(v):
    return struct.pack('<I', v)[:3]


def _riff(body):
    if len(body) > MAX_FILE_BYTES:
        raise ValueError("webp: the file would take %d bytes; RIFF sizes are 32 bits" % (len(body) + 8))
    return b'RIFF' + struct.pack('<I', len(body)) + body


def still_file(stream):
    """the simple-format file of one VP8 frame: RIFF <size> WEBP, one 'VP8 ' chunk (padded to an even size)"""
    return _riff(b'WEBP' + _chunk(b'VP8 ', bytes(stream)))


def animation_file(streams, width, height, fps=25, loop=0, order=None):
    """The extended-format file of the VP8 frames `streams` (a list of bytes from ops.webp_streams, all width x height): VP8X
    (animation flag, the canvas), ANIM (background 0, `loop` repetitions, 0 = for ever), then per output frame one ANMF: offset
    0, the full canvas, round(1000 / fps) ms, "do not blend", no disposal, and the frame's 'VP8 ' chunk.  `order` lists, for each
    output frame, the index of the stream it takes (default: every stream once, in order)."""
    order = list(range(len(streams))) if order is None else [int(i) for i in order]
    if not order:
        raise ValueError("webp: at least one frame is needed")
    if any(i < 0 or i >= len(streams) for i in order):
        raise ValueError("webp: order refers to a frame outside the %d encoded ones" % len(streams))
    width, height = check_size(width, height)
    loop = int(loop)
    if not 0 <= loop <= 65535:
        raise ValueError("webp: loop must be in [0, 65535] (got %d)" % loop)
    head = _u24(0) + _u24(0) + _u24(width - 1) + _u24(height - 1) + _u24(duration_ms(fps)) + b'\x02'
    parts = [b'WEBP', _chunk(b'VP8X', b'\x02\x00\x00\x00' + _u24(width - 1) + _u24(height - 1)),
             _chunk(b'ANIM', struct.pack('<IH', 0, loop))]
    framed = {}
    for i in order:
        if i not in framed:
            framed[i] = _chunk(b'ANMF', head + _chunk(b'VP8 ', bytes(streams[i])))
        parts.append(framed[i])
    return _riff(b''.join(parts))
