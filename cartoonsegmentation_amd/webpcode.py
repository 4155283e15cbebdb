"""Host side of the WebP writer (contract DESIGN.md §4.12; device side csrc/webp.hip): the VP8 frame header around the partitions
the device coded, and the RIFF containers of a still and of an animation; and of the lossless writer (contract DESIGN.md §4.13;
device side csrc/webpll.hip): the prefix codes and every header bit of a VP8L payload from the histograms the device measured, the
table the write call reads, and the container.  Pure Python; no device code."""
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


def check_method(method, what="webp"):
    """the lossy writer's coding method: the integer 0 (16x16 prediction, default probabilities) or 1 (B_PRED and
    probability updates; §4.12b)"""
    if isinstance(method, bool) or not isinstance(method, numbers.Integral) or method not in (0, 1):
        raise ValueError("%s: method must be the integer 0 or 1 (got %r)" % (what, method))
    return int(method)


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


# ---- lossless WebP (VP8L; contract DESIGN.md §4.13; device side csrc/webpll.hip) ----------------------------------------------
# The device measures five histograms per plane (the predictor-mode image, then the residual image); the host builds the prefix
# codes and every header bit from them, sizes the stream exactly, and hands the codes back for the write call.
LL_MAX_SIDE = 16384            # VP8L holds width - 1 and height - 1 in 14 bits
LL_BLOCK_BITS = 4              # one predictor mode per 16 x 16 pixels
LL_MAX_REF = 4096              # the longest backward reference
LL_ALPHABETS = (280, 256, 256, 256, 40)        # green + 24 length prefixes, red, blue, alpha, 40 distance prefixes
LL_BASE = (0, 280, 536, 792, 1048)             # where each alphabet starts in a plane's 1088 counts or codes
LL_SYMS = 1088
LL_MAX_BITS = 15
LL_CL_MAX_BITS = 7
LL_CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
LL_TABLE_WORDS = 1352          # the host table row of one plane (include/csm355.h, csm_webpll_write)
LL_HEADER_WORDS_MAX = 256
LL_T_OFF, LL_T_BYTES, LL_T_START, LL_T_HDR_WORD, LL_T_HDR_COUNT, LL_T_HDR = 1088, 1090, 1091, 1093, 1094, 1095


def ll_check_size(width, height, what="webp_encode_lossless"):
    width, height = int(width), int(height)
    if not (1 <= width <= LL_MAX_SIDE and 1 <= height <= LL_MAX_SIDE):
        raise ValueError("%s: width and height must be in [1, %d] (got %dx%d)" % (what, LL_MAX_SIDE, width, height))
    return width, height


def ll_prefix_extra_bits(p):
    """extra bits behind the length or distance prefix symbol p"""
    return 0 if p < 4 else (p >> 1) - 1


def ll_write_code(b, hist):
    """One prefix code from its counts into the bit string b; returns (lengths, bit-reversed codes).  With no or one used symbol
    it is a simple code of one symbol (symbol 0 if none is used) and every occurrence costs zero bits; otherwise a normal code by
    pngcode.limited_lengths (limit 15; the code-length code limit 7), with every length of the alphabet written."""
    from . import pngcode
    hist = [int(v) for v in hist]
    used = [s for s, c in enumerate(hist) if c > 0]
    if len(used) < 2:
        s = used[0] if used else 0
        if s > 255:
            raise ValueError("webp: a simple code cannot hold symbol %d" % s)
        b.put(1, 1); b.put(0, 1)
        if s < 2:
            b.put(0, 1); b.put(s, 1)
        else:
            b.put(1, 1); b.put(s, 8)
        return [0] * len(hist), [0] * len(hist)
    lengths = pngcode.limited_lengths(hist, LL_MAX_BITS)
    symbols = pngcode.run_code(lengths)
    cl_hist = [0] * 19
    for s, _, _ in symbols:
        cl_hist[s] += 1
    cl_len = pngcode.limited_lengths(cl_hist, LL_CL_MAX_BITS)
    cl_code = pngcode.canonical_codes(cl_len)
    count = max(4, max(k for k in range(19) if cl_len[LL_CL_ORDER[k]]) + 1)
    b.put(0, 1); b.put(count - 4, 4)
    for k in range(count):
        b.put(cl_len[LL_CL_ORDER[k]], 3)
    b.put(0, 1)
    for s, eb, ev in symbols:
        b.put(cl_code[s], cl_len[s])
        b.put(ev, eb)
    return lengths, pngcode.canonical_codes(lengths)


def ll_plane_code(b, hist):
    """The five codes of one plane from its 1088 counts, written into b.  Returns (entries, pixel_bits): entries[s] = bit-reversed
    code | length << 16 for the 1088 symbols, pixel_bits = the exact bits of the plane's pixels under these codes."""
    hist = [int(v) for v in hist]
    if len(hist) != LL_SYMS or min(hist) < 0:
        raise ValueError("webp: 1088 counts are expected")
    entries, bits = [], 0
    for a, (base, n) in enumerate(zip(LL_BASE, LL_ALPHABETS)):
        h = hist[base:base + n]
        lengths, codes = ll_write_code(b, h)
        entries += [c | l << 16 for c, l in zip(codes, lengths)]
        bits += sum(c * l for c, l in zip(h, lengths))
        if a == 0:
            bits += sum(h[256 + p] * ll_prefix_extra_bits(p) for p in range(24))
        elif a == 4:
            bits += sum(h[p] * ll_prefix_extra_bits(p) for p in range(40))
    return entries, bits


def ll_image_code(hist_modes, hist_pixels, width, height, has_alpha):
    """Everything the host decides for one image.  Returns a dict: 'bytes' of the VP8L payload, and per plane (0 the mode image,
    1 the residuals) 'entries', 'start' (the bit at which the plane's pixels begin), 'header' (LSB-first integer) and
    'header_at' / 'header_bits' (where the bits in front of the plane's pixels lie)."""
    from .pngcode import _Bits
    width, height = ll_check_size(width, height)
    a = _Bits()
    a.put(0x2f, 8); a.put(width - 1, 14); a.put(height - 1, 14); a.put(1 if has_alpha else 0, 1); a.put(0, 3)
    a.put(1, 1); a.put(2, 2)                               # subtract-green
    a.put(1, 1); a.put(0, 2); a.put(LL_BLOCK_BITS - 2, 3)  # predictor; its sub-image follows
    a.put(0, 1)                                            # no colour cache
    e0, bits0 = ll_plane_code(a, hist_modes)
    c = _Bits()
    c.put(0, 1)                                            # no further transform
    c.put(0, 1); c.put(0, 1)                               # no colour cache, no meta prefix codes
    e1, bits1 = ll_plane_code(c, hist_pixels)
    at1 = a.n + bits0
    total = at1 + c.n + bits1
    return {'bytes': (total + 7) // 8, 'bits': total,
            'planes': [{'entries': e0, 'start': a.n, 'header': a.value, 'header_at': 0, 'header_bits': a.n, 'pixel_bits': bits0},
                       {'entries': e1, 'start': at1 + c.n, 'header': c.value, 'header_at': at1, 'header_bits': c.n, 'pixel_bits': bits1}]}


def ll_table_row(plane, offset, nbytes):
    """the uint32 [1352] row of csm_webpll_write (include/csm355.h) for one plane of ll_image_code; offset: where the image's
    payload begins in the blob (a multiple of 4)"""
    import numpy as np
    row = np.zeros(LL_TABLE_WORDS, dtype=np.uint32)
    row[:LL_SYMS] = plane['entries']
    row[LL_T_OFF], row[LL_T_OFF + 1] = offset & 0xFFFFFFFF, offset >> 32
    row[LL_T_BYTES] = nbytes
    row[LL_T_START], row[LL_T_START + 1] = plane['start'] & 0xFFFFFFFF, plane['start'] >> 32
    at = plane['header_at']
    h = plane['header'] << (at & 31)                       # shifted onto the stream's 32-bit words
    count = ((at & 31) + plane['header_bits'] + 31) // 32
    if count > LL_HEADER_WORDS_MAX:
        raise ValueError("webp: a header of %d bits does not fit the table" % plane['header_bits'])
    row[LL_T_HDR_WORD], row[LL_T_HDR_COUNT] = at >> 5, count
    for k in range(count):
        row[LL_T_HDR + k] = (h >> (32 * k)) & 0xFFFFFFFF
    return row


def ll_worst_case_bytes(width, height):
    """The contract's cap on a file: every pixel of both planes as four literals of 15 bits, ten code headers
    of the longest form (63 bits and 7 per symbol), the 53 other header bits, and the 20 container bytes."""
    wb, hb = -(-width >> LL_BLOCK_BITS), -(-height >> LL_BLOCK_BITS)
    bits = 53 + 2 * sum(63 + 7 * n for n in LL_ALPHABETS) + 60 * (width * height + wb * hb)
    return 20 + ((bits + 7) // 8 + 1) // 2 * 2


def lossless_file(payload):
    """the simple-format file of one VP8L payload: RIFF <size> WEBP, one 'VP8L' chunk (padded to an even size)"""
    return _riff(b'WEBP' + _chunk(b'VP8L', bytes(payload)))
