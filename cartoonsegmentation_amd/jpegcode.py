"""Host side of the JPEG decoder (contract DESIGN.md §4.8; pure Python / numpy, no device): the marker parser and the tables that
csrc/jpegdec.hip reads.

    probe(data)        a plain description of a baseline JPEG file (size, components, tables, restart interval, the byte range of
                       the entropy-coded segment, EXIF orientation), or Unsupported(reason) for a stream the decoder does not take.
                       Reads marker segments only, never entropy data, and checks every segment length against the buffer.
                       With progressive=True a progressive file (SOF2) is described too: 'scans' lists its scans.
    scan_levels(info)  the scans of a progressive file by dependency level
    scan_tables(info)  the decode tables of each scan of a progressive file
    scan_intervals(..) where the restart intervals of a scan begin
    scan_descriptor(..) the int32 row of csm_jpeg_decode_progressive for one scan
    huffman_table(..)  the decode table of one Huffman code as the kernels read it (TABLE_BYTES bytes)
    file_tables(info)  the table region of one file: HUFF_SLOTS decode tables and the quantisation tables in natural order
    descriptor(..)     the int32 row of csm_jpeg_decode for one file
"""
import struct

import numpy as np

# zigzag[i] = natural (row-major) index of the i-th coefficient of the scan
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

HUFF_SLOTS = 6                          # distinct Huffman tables of one file: a DC and an AC table per component at the most
LUT_BITS = 8
TABLE_BYTES = 2 * (1 << LUT_BITS) + 4 * 18 + 4 * 18 + 256       # uint16 lut[256], int32 maxcode[18], int32 valoff[18], uint8 vals[256]
QUANT_BYTES = 3 * 64 * 2                # uint16 [3][64], natural order, one per component
FILE_TABLE_BYTES = HUFF_SLOTS * TABLE_BYTES + QUANT_BYTES
DESC_WORDS = 20
MAX_ENTROPY_BYTES = 1 << 28             # bit positions stay below 2^31


class Unsupported(ValueError):
    """the stream is not one the device decoder takes; str(e) is the reason"""


def _orientation(payload):
    """EXIF orientation (1..8) of an APP1 payload, or None: IFD0 tag 0x0112 of the TIFF block behind 'Exif\\0\\0'"""
    if payload[:6] != b'Exif\x00\x00':
        return None
    t = payload[6:]
    if len(t) < 8 or t[:2] not in (b'II', b'MM'):
        return None
    e = '<' if t[:2] == b'II' else '>'
    if struct.unpack(e + 'H', t[2:4])[0] != 42:
        return None
    off = struct.unpack(e + 'I', t[4:8])[0]
    if off + 2 > len(t):
        return None
    n = struct.unpack(e + 'H', t[off:off + 2])[0]
    for k in range(n):
        p = off + 2 + 12 * k
        if p + 12 > len(t):
            return None
        tag, typ, cnt = struct.unpack(e + 'HHI', t[p:p + 8])
        if tag == 0x0112:
            if typ != 3 or cnt != 1:
                return None
            v = struct.unpack(e + 'H', t[p + 8:p + 10])[0]
            return v if 1 <= v <= 8 else None
    return None


def _check_huffman(bits, vals):
    """a BITS / HUFFVAL pair defines a prefix code whose codes fit their lengths (T.81 Annex C)"""
    code = 0
    for ln in range(1, 17):
        if code + bits[ln - 1] > (1 << ln):
            return False
        code = (code + bits[ln - 1]) << 1
    return len(vals) == sum(bits) and len(vals) <= 256


def _entropy_end(data, start):
    """offset of the first marker behind `start` that is neither a stuffed FF 00, a restart marker nor a fill byte, and that
    marker's code; (None, None) when there is none"""
    p = start
    n = len(data)
    while True:
        p = data.find(b'\xff', p)
        if p < 0 or p + 1 >= n:
            return None, None
        m = data[p + 1]
        if m == 0x00 or 0xD0 <= m <= 0xD7:
            p += 2
        elif m == 0xFF:
            p += 1
        else:
            return p, m


def _take_dht(seg, huffman):
    q = 0
    while q < len(seg):
        if q + 17 > len(seg):
            raise Unsupported("malformed DHT segment")
        tc, th = seg[q] >> 4, seg[q] & 15
        bits = list(seg[q + 1:q + 17])
        cnt = sum(bits)
        if tc > 1 or th > 3 or q + 17 + cnt > len(seg):
            raise Unsupported("malformed DHT segment")
        vals = list(seg[q + 17:q + 17 + cnt])
        if not _check_huffman(bits, vals):
            raise Unsupported("malformed DHT segment: not a prefix code")
        huffman[(tc, th)] = (bits, vals)
        q += 17 + cnt


def _take_dqt(seg, qtables):
    q = 0
    while q < len(seg):
        pq, tq = seg[q] >> 4, seg[q] & 15
        if pq != 0:
            raise Unsupported("16-bit quantisation tables")
        if tq > 3 or q + 65 > len(seg):
            raise Unsupported("malformed DQT segment")
        qtables[tq] = list(seg[q + 1:q + 65])
        q += 65


def _take_dri(seg):
    if len(seg) != 2:
        raise Unsupported("malformed DRI segment")
    return (seg[0] << 8) | seg[1]


MAX_SCANS = 64
MAX_AL = 13


def _progressive_scans(data, p, frame, qtables, huffman, ri):
    """The scans of a progressive file from the first SOS (its length field at `p`) to EOI: the list of probe's 'scans', and the
    restart interval in force at the end.  Checks the scan script (T.81 G.1.1.1.1 and the rules of DESIGN.md §4.11)."""
    n = len(data)
    comps = frame['components']
    nc = len(comps)
    ids = [c['id'] for c in comps]
    cur = [[None] * 64 for _ in range(nc)]              # the point transform each coefficient stands at; None: no scan yet
    scans = []
    total = 0
    while True:
        ln = (data[p] << 8) | data[p + 1]
        seg = data[p + 2:p + ln]
        if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
            raise Unsupported("malformed SOS segment")
        ns = seg[0]
        if not 1 <= ns <= nc:
            raise Unsupported("malformed SOS segment: %d components in a scan of a %d-component frame" % (ns, nc))
        sc = []
        for i in range(ns):
            cid, t = seg[1 + 2 * i], seg[2 + 2 * i]
            if cid not in ids:
                raise Unsupported("malformed SOS segment: unknown component %d" % cid)
            ci = ids.index(cid)
            if sc and ci <= sc[-1][0]:
                raise Unsupported("the scan's components are not in frame order")
            if (t >> 4) > 3 or (t & 15) > 3:
                raise Unsupported("malformed SOS segment: Huffman table id above 3")
            sc.append((ci, t >> 4, t & 15))
        ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
        if ss > 63 or se > 63 or se < ss:
            raise Unsupported("malformed SOS segment: spectral selection %d..%d" % (ss, se))
        if ss == 0:
            if se != 0:
                raise Unsupported("a scan that mixes DC and AC coefficients (spectral selection 0..%d)" % se)
            if ns != nc and ns != 1:
                raise Unsupported("a DC scan of %d of %d components" % (ns, nc))
        else:
            if ns != 1:
                raise Unsupported("an interleaved AC scan (%d components)" % ns)
            if cur[sc[0][0]][0] is None:
                raise Unsupported("an AC scan of component %d before its DC scan" % sc[0][0])
        if al > MAX_AL:
            raise Unsupported("successive approximation: point transform %d above %d" % (al, MAX_AL))
        if ah != 0 and ah != al + 1:
            raise Unsupported("successive approximation: a refinement from bit %d to bit %d (one bit per scan is taken)" % (ah, al))
        for ci, _, _ in sc:
            for k in range(ss, se + 1):
                have = cur[ci][k]
                if ah == 0:
                    if have is not None:
                        raise Unsupported("coefficient %d of component %d has two first scans" % (k, ci))
                elif have != ah:
                    raise Unsupported("a refinement of coefficient %d of component %d from bit %d, which stands at %s"
                                      % (k, ci, ah, "no scan" if have is None else "bit %d" % have))
                cur[ci][k] = al
        need = [] if ah else ([(0, td) for _, td, _ in sc] if ss == 0 else [(1, sc[0][2])])
        for key in need:
            if key not in huffman:
                raise Unsupported("missing %s Huffman table %d" % ("AC" if key[0] else "DC", key[1]))
        start = p + ln
        end, m = _entropy_end(data, start)
        if end is None:
            raise Unsupported("truncated file: no EOI marker")
        total += end - start
        if total > MAX_ENTROPY_BYTES:
            raise Unsupported("more than %d bytes of entropy data" % MAX_ENTROPY_BYTES)
        scans.append({'components': sc, 'ss': ss, 'se': se, 'ah': ah, 'al': al, 'entropy': (start, end), 'restart_interval': ri,
                      'huffman': dict(huffman)})
        if len(scans) > MAX_SCANS:
            raise Unsupported("more than %d scans" % MAX_SCANS)
        if m == 0xD9:
            break
        # the segments between two scans
        p = end
        while True:
            while p < n and data[p] == 0xFF:
                p += 1
            if p >= n:
                raise Unsupported("truncated file: no EOI marker")
            m = data[p]
            p += 1
            if m == 0xD9:
                break
            if m == 0xDC:
                raise Unsupported("DNL")
            if m not in (0xC4, 0xDA, 0xDB, 0xDD, 0xFE) and not 0xE0 <= m <= 0xEF:
                raise Unsupported("marker FF%02X between two scans" % m)
            if p + 2 > n:
                raise Unsupported("truncated file: cut inside a segment")
            ln = (data[p] << 8) | data[p + 1]
            if ln < 2 or p + ln > n:
                raise Unsupported("truncated file: cut inside a segment (marker FF%02X at offset %d)" % (m, p - 2))
            if m == 0xDA:
                break
            seg = data[p + 2:p + ln]
            if m == 0xC4:
                _take_dht(seg, huffman)
            elif m == 0xDB:
                _take_dqt(seg, qtables)
            elif m == 0xDD:
                ri = _take_dri(seg)
            p += ln
            if p >= n or data[p] != 0xFF:
                raise Unsupported("malformed file: no marker at offset %d" % p)
        if m == 0xD9:
            break
    for ci in range(nc):
        left = [k for k in range(64) if cur[ci][k] != 0]
        if left:
            raise Unsupported("the file ends before full precision: coefficient %d of component %d %s"
                              % (left[0], ci, "has no scan" if cur[ci][left[0]] is None else "stands at bit %d" % cur[ci][left[0]]))
    return scans, ri


def probe(data, progressive=False):
    """Description of the baseline JPEG file `data` (bytes): a dict with 'height', 'width', 'sof' (0 or 1), 'components' (a list of
    {'id', 'h', 'v', 'tq', 'td', 'ta'} in scan order), 'qtables' ({id: 64 entries in zigzag order}), 'huffman' ({(class, id): (BITS
    [16], HUFFVAL)}, class 0 = DC, 1 = AC), 'restart_interval' (0 = none), 'entropy' ((start, end): the bytes between SOS and
    EOI), 'orientation' (EXIF, 1..8 or None), 'jfif' and 'adobe_transform' (None without an Adobe segment).  Raises Unsupported
    with a reason for everything else, a truncated or malformed file included.

    'progressive' is False for these.  With progressive=True a progressive file (SOF2, Huffman) is described as well: 'sof' is 2,
    'progressive' True, 'components' carry no 'td' / 'ta', 'entropy' spans all scans, and 'scans' lists in file order
        {'components': [(component index, td, ta)], 'ss', 'se', 'ah', 'al', 'entropy': (start, end), 'restart_interval',
         'huffman': {(class, id): (BITS, HUFFVAL)}}
    with the Huffman tables and the restart interval in force at that SOS.  The scan script must satisfy T.81 G.1.1.1.1 and: a DC
    scan holds all components or one; an AC scan follows its component's first DC scan; every refinement lowers the point
    transform by one bit; no coefficient has two first scans; at EOI every coefficient of every component stands at bit 0; at
    most MAX_SCANS scans.  Each other script raises Unsupported with its own reason."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("probe: bytes expected (got %s)" % type(data).__name__)
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b'\xff\xd8':
        raise Unsupported("not a JPEG file: no SOI marker")
    qtables, huffman = {}, {}
    frame = None
    ri = 0
    jfif = False
    adobe = None
    orientation = None
    p = 2
    while True:
        if p >= n:
            raise Unsupported("truncated file: the marker segments end before SOS")
        if data[p] != 0xFF:
            raise Unsupported("malformed file: no marker at offset %d" % p)
        while p < n and data[p] == 0xFF:          # fill bytes
            p += 1
        if p >= n:
            raise Unsupported("truncated file: the marker segments end before SOS")
        m = data[p]
        p += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            raise Unsupported("malformed file: marker FF%02X before SOS" % m)
        if m == 0xD8:
            raise Unsupported("malformed file: a second SOI")
        if m == 0xD9:
            raise Unsupported("no scan: EOI before SOS")
        if m == 0x00:
            raise Unsupported("malformed file: FF 00 outside entropy data")
        if p + 2 > n:
            raise Unsupported("truncated file: cut inside a segment")
        ln = (data[p] << 8) | data[p + 1]
        if ln < 2 or p + ln > n:
            raise Unsupported("truncated file: cut inside a segment (marker FF%02X at offset %d)" % (m, p - 2))
        seg = data[p + 2:p + ln]
        if m == 0xC2 and not progressive:
            raise Unsupported("progressive (SOF2)")
        if m in (0xC0, 0xC1, 0xC2):
            if frame is not None:
                raise Unsupported("several frames")
            if len(seg) < 6:
                raise Unsupported("malformed SOF segment")
            prec, H, W, nf = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8:
                raise Unsupported("%d-bit samples" % prec)
            if len(seg) != 6 + 3 * nf:
                raise Unsupported("malformed SOF segment")
            if H == 0:
                raise Unsupported("DNL: the frame header has no height")
            if W == 0:
                raise Unsupported("malformed SOF segment: width 0")
            comps = [{'id': seg[6 + 3 * i], 'h': seg[7 + 3 * i] >> 4, 'v': seg[7 + 3 * i] & 15, 'tq': seg[8 + 3 * i]} for i in range(nf)]
            frame = {'sof': m - 0xC0, 'height': H, 'width': W, 'components': comps}
        elif m in (0xC3, 0xC5, 0xC6, 0xC7):
            raise Unsupported("lossless or hierarchical coding (SOF%d)" % (m - 0xC0))
        elif m in (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise Unsupported("arithmetic coding")
        elif m == 0xC8:
            raise Unsupported("reserved JPEG extension marker")
        elif m == 0xC4:
            _take_dht(seg, huffman)
        elif m == 0xDB:
            _take_dqt(seg, qtables)
        elif m == 0xDD:
            ri = _take_dri(seg)
        elif m == 0xDC:
            raise Unsupported("DNL")
        elif m == 0xE0:
            if seg[:5] == b'JFIF\x00':
                jfif = True
        elif m == 0xE1:
            o = _orientation(seg)
            if o is not None and orientation is None:
                orientation = o
        elif m == 0xEE:
            if seg[:5] == b'Adobe' and len(seg) >= 12:
                adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise Unsupported("malformed file: SOS before SOF")
            if frame['sof'] == 2:
                break                              # the scans of a progressive file are read below, from this SOS
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise Unsupported("malformed SOS segment")
            ns = seg[0]
            comps = frame['components']
            if ns != len(comps):
                raise Unsupported("several scans: the first scan holds %d of %d components" % (ns, len(comps)))
            for i, c in enumerate(comps):
                if seg[1 + 2 * i] != c['id']:
                    raise Unsupported("the scan's components are not in frame order")
                c['td'], c['ta'] = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
            if (seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]) != (0, 63, 0):
                raise Unsupported("not a sequential scan (spectral selection or successive approximation)")
            p += ln
            break
        # every other APPn, COM and reserved segment is skipped by its length
        p += ln
    start = p
    comps = frame['components']
    nc = len(comps)
    if nc == 4:
        raise Unsupported("four components (CMYK / YCCK)")
    if nc not in (1, 3):
        raise Unsupported("%d components" % nc)
    if nc == 3:
        if not jfif and adobe is not None and adobe != 1:
            raise Unsupported("RGB-coded stream (Adobe transform %d)" % adobe)
        if not jfif and adobe is None and [c['id'] for c in comps] == [82, 71, 66]:
            raise Unsupported("RGB-coded stream (component ids R, G, B)")
        if (comps[1]['h'], comps[1]['v'], comps[2]['h'], comps[2]['v']) != (1, 1, 1, 1) or \
                (comps[0]['h'], comps[0]['v']) not in ((1, 1), (2, 1), (2, 2)):
            raise Unsupported("sampling factors %s (4:4:4, 4:2:2 and 4:2:0 are taken)"
                              % ', '.join('%dx%d' % (c['h'], c['v']) for c in comps))
    else:
        if not (1 <= comps[0]['h'] <= 4 and 1 <= comps[0]['v'] <= 4):
            raise Unsupported("malformed SOF segment: sampling factor 0")
        comps[0]['h'] = comps[0]['v'] = 1        # a one-component scan is not interleaved: its sampling factors do not matter
    if frame['sof'] == 2:
        scans, ri = _progressive_scans(data, p, frame, qtables, huffman, ri)
        for c in comps:
            if c['tq'] not in qtables:
                raise Unsupported("missing quantisation table %d" % c['tq'])
        out = dict(frame)
        out.update(qtables=qtables, huffman=huffman, restart_interval=ri, entropy=(scans[0]['entropy'][0], scans[-1]['entropy'][1]),
                   orientation=orientation, jfif=jfif, adobe_transform=adobe, progressive=True, scans=scans)
        return out
    for c in comps:
        if c['tq'] not in qtables:
            raise Unsupported("missing quantisation table %d" % c['tq'])
        if (0, c['td']) not in huffman:
            raise Unsupported("missing DC Huffman table %d" % c['td'])
        if (1, c['ta']) not in huffman:
            raise Unsupported("missing AC Huffman table %d" % c['ta'])
    end, m = _entropy_end(data, start)
    if end is None:
        raise Unsupported("truncated file: no EOI marker")
    if m == 0xDC:
        raise Unsupported("DNL")
    if m != 0xD9:
        raise Unsupported("several scans (marker FF%02X behind the first scan)" % m)
    if end - start > MAX_ENTROPY_BYTES:
        raise Unsupported("more than %d bytes of entropy data" % MAX_ENTROPY_BYTES)
    out = dict(frame)
    out.update(qtables=qtables, huffman=huffman, restart_interval=ri, entropy=(start, end), orientation=orientation, jfif=jfif,
               adobe_transform=adobe, progressive=False)
    return out


# ---- the tables of the kernels -----------------------------------------------------------------------------------------------
def huffman_table(bits, vals):
    """(lut uint16 [256], maxcode int32 [18], valoff int32 [18], vals uint8 [256]) of one code (T.81 Annex C / F.2.2.3): lut[the
    next 8 bits] = length << 8 | symbol for codes of up to 8 bits, else 0; a code of `l` bits with value c <= maxcode[l] (-1: no
    code of that length) is the symbol vals[valoff[l] + c]"""
    lut = np.zeros(1 << LUT_BITS, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    v = np.zeros(256, np.uint8)
    v[:len(vals)] = vals
    code, k = 0, 0
    for ln in range(1, 17):
        cnt = bits[ln - 1]
        if cnt:
            valoff[ln] = k - code
            if ln <= LUT_BITS:
                for i in range(cnt):
                    lo = (code + i) << (LUT_BITS - ln)
                    lut[lo:lo + (1 << (LUT_BITS - ln))] = (ln << 8) | vals[k + i]
            code += cnt
            k += cnt
            maxcode[ln] = code - 1
        code <<= 1
    return lut, maxcode, valoff, v


def table_slots(info):
    """the distinct Huffman tables of the file's components, in order of first use, and per component the slot of its DC and AC
    table: ([(class, id)], dc_slot [nc], ac_slot [nc])"""
    keys, dcs, acs = [], [], []
    for c in info['components']:
        for cls, tid, dst in ((0, c['td'], dcs), (1, c['ta'], acs)):
            if (cls, tid) not in keys:
                keys.append((cls, tid))
            dst.append(keys.index((cls, tid)))
    return keys, dcs, acs


def file_tables(info):
    """the FILE_TABLE_BYTES table region of one file: the decode tables of table_slots(info), then one uint16 [64] quantisation
    table per component in natural order"""
    out = np.zeros(FILE_TABLE_BYTES, np.uint8)
    keys, _, _ = table_slots(info)
    for s, key in enumerate(keys):
        lut, maxcode, valoff, v = huffman_table(*info['huffman'][key])
        out[s * TABLE_BYTES:(s + 1) * TABLE_BYTES] = np.concatenate([lut.view(np.uint8), maxcode.view(np.uint8), valoff.view(np.uint8), v])
    q = np.zeros((3, 64), np.uint16)
    for i, c in enumerate(info['components']):
        q[i, list(ZIGZAG)] = info['qtables'][c['tq']]
    out[HUFF_SLOTS * TABLE_BYTES:] = q.view(np.uint8).ravel()
    return out


def descriptor(info, ent_off, tab_off, out_off):
    """the int32 [DESC_WORDS] row of csm_jpeg_decode (include/csm355.h) for one file whose entropy bytes lie at `ent_off` and whose
    table region at `tab_off` of the blob, and whose pixels go to byte `out_off` of the output"""
    comps = info['components']
    _, dcs, acs = table_slots(info)
    d = np.zeros(DESC_WORDS, np.int32)
    d[0:6] = (info['height'], info['width'], len(comps), comps[0]['h'], comps[0]['v'], info['restart_interval'])
    d[6:9] = (ent_off, info['entropy'][1] - info['entropy'][0], tab_off)
    d[9:9 + len(comps)] = dcs
    d[12:12 + len(comps)] = acs
    d[15], d[16] = out_off & 0x7FFFFFFF, out_off >> 31
    return d


# ---- progressive files (csrc/jpegprog.hip) ------------------------------------------------------------------
SCAN_DESC_WORDS = 16


def scan_levels(info):
    """The scans of a progressive file by dependency level: scan j depends on scan i < j when they share a component and their
    coefficient ranges intersect; a scan's level is one more than the highest level it depends on.  A list of lists of scan indices;
    the scans of one level write disjoint coefficients."""
    scans = info['scans']
    level = []
    for j, b in enumerate(scans):
        lv = 0
        cb = {c for c, _, _ in b['components']}
        for i in range(j):
            a = scans[i]
            if cb & {c for c, _, _ in a['components']} and a['ss'] <= b['se'] and b['ss'] <= a['se']:
                lv = max(lv, level[i] + 1)
        level.append(lv)
    return [[j for j in range(len(scans)) if level[j] == lv] for lv in range(max(level) + 1)]


def scan_tables(info):
    """Per scan of a progressive file its decode tables as the kernels read them (huffman_table, TABLE_BYTES bytes each): one DC
    table per component of a DC first scan (in the scan's component order), one AC table for an AC scan, none for a DC
    refinement.  A list of uint8 arrays."""
    out = []
    for sc in info['scans']:
        if sc['ss'] == 0:
            keys = [] if sc['ah'] else [(0, td) for _, td, _ in sc['components']]
        else:
            keys = [(1, sc['components'][0][2])]
        parts = []
        for key in keys:
            lut, maxcode, valoff, v = huffman_table(*sc['huffman'][key])
            parts += [lut.view(np.uint8), maxcode.view(np.uint8), valoff.view(np.uint8), v]
        out.append(np.concatenate(parts) if parts else np.zeros(0, np.uint8))
    return out


def scan_block_count(info, sc):
    """(blocks, blocks per restart unit) of a scan: a scan of all components walks the padded MCU grid, a one-component scan only
    the component's true block grid, ceil(ceil(W h / hmax) / 8) by ceil(ceil(H v / vmax) / 8), and its restart interval counts
    blocks"""
    comps = info['components']
    hs, vs = comps[0]['h'], comps[0]['v']
    H, W = info['height'], info['width']
    if len(sc['components']) > 1:
        bpm = hs * vs + len(comps) - 1
        return -(-W // (8 * hs)) * -(-H // (8 * vs)) * bpm, bpm
    c = comps[sc['components'][0][0]]
    return -(-(-(-W * c['h'] // hs)) // 8) * -(-(-(-H * c['v'] // vs)) // 8), 1


def scan_intervals(data, sc):
    """int32 [restart intervals]: the byte of the scan's entropy data at which each restart interval begins ([0] = 0, then the
    byte behind every RSTn marker).  Inside entropy-coded data an FF followed by D0..D7 is always a marker."""
    s, e = sc['entropy']
    raw = np.frombuffer(data, np.uint8, e - s, s)
    at = np.nonzero((raw[:-1] == 0xFF) & (raw[1:] >= 0xD0) & (raw[1:] <= 0xD7))[0] if e - s > 1 else np.zeros(0, np.int64)
    return np.concatenate([[0], at + 2]).astype(np.int32)


def scan_descriptor(info, j, file_index, ent_off, tab_off, level, iv_off=0):
    """the int32 [SCAN_DESC_WORDS] row of csm_jpeg_decode_progressive (include/csm355.h) for scan j of a progressive file that is file
    `file_index` of the call, whose entropy bytes lie at `ent_off` and whose tables (scan_tables) at `tab_off` of the blob; `iv_off`
    is where the blob holds scan_intervals (refinement scans with restart markers)"""
    sc = info['scans'][j]
    d = np.zeros(SCAN_DESC_WORDS, np.int32)
    d[0:7] = (file_index, len(sc['components']), sc['components'][0][0], sc['ss'], sc['se'], sc['ah'], sc['al'])
    d[7:13] = (ent_off, sc['entropy'][1] - sc['entropy'][0], sc['restart_interval'], tab_off, level, iv_off)
    return d
