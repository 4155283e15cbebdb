"""A small progressive-JPEG writer for the tests: quantised coefficients (from the restatement of a PIL file) under a GIVEN scan
script (T.81 G.1.2).  PIL's encoder emits one script only and the parser takes far more; this writes the others.

One fixed Huffman code serves every scan: all symbols at length 9, in ascending order, is a valid JPEG prefix code (the all-ones
code word stays free) and needs no statistics.  A file of this writer is a legitimate test input only because PIL decodes it to the
same pixels as the restatement: the tests assert that for every file they use.

    write(info, coef, script)   bytes of a complete file.  info: probe's description of the frame the coefficients came from
                                (size, components with h / v / tq, qtables); coef: int [blocks, 64], natural order, the block order of
                                jpegdec_restatement; script: a list of dicts {'comps': [component indices], 'ss', 'se', 'ah', 'al'
                                and optionally 'ri': the restart interval from this scan on}.
"""
import struct

import numpy as np

import jpegprog_restatement as P

DC_SYMBOLS = list(range(12))
AC_SYMBOLS = sorted([(r << 4) | s for r in range(16) for s in range(1, 11)] + [r << 4 for r in range(16)])
CODE_BITS = 9


class _Out:
    def __init__(self):
        self.bytes = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, v, k):
        if k == 0:
            return
        self.acc = (self.acc << k) | (v & ((1 << k) - 1))
        self.n += k
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.bytes.append(b)
            if b == 0xFF:
                self.bytes.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)

    def marker(self, m):
        self.flush()
        self.bytes += bytes([0xFF, m])


def _seg(m, payload):
    return bytes([0xFF, m]) + struct.pack('>H', len(payload) + 2) + bytes(payload)


def _dht(cls, tid, symbols):
    bits = [0] * 16
    bits[CODE_BITS - 1] = len(symbols)
    return _seg(0xC4, bytes([cls << 4 | tid]) + bytes(bits) + bytes(symbols))


def _nbits(a):
    return int(a).bit_length()


def _encode_scan(info, coef, sc, ri):
    """the entropy bytes of one scan"""
    comps, ss, se, ah, al = sc['comps'], sc['ss'], sc['se'], sc['ah'], sc['al']
    desc = {'components': [(c, 0, 0) for c in comps]}
    order, comp_of, bpu = P.scan_blocks(info, desc)
    order, comp_of = order.tolist(), comp_of.tolist()
    per = ri * bpu if ri else len(order)
    out = _Out()
    dc_code = {s: i for i, s in enumerate(DC_SYMBOLS)}
    ac_code = {s: i for i, s in enumerate(AC_SYMBOLS)}
    zz = coef[:, P.ZIGZAG]
    st = {'eobrun': 0, 'be': []}

    def emit_eobrun():
        if st['eobrun']:
            n = _nbits(st['eobrun']) - 1
            out.put(ac_code[n << 4], CODE_BITS)
            out.put(st['eobrun'], n)
            st['eobrun'] = 0
        for b in st['be']:
            out.put(b, 1)
        st['be'] = []

    pred = {}
    for i, blk in enumerate(order):
        if i % per == 0:
            if i:
                emit_eobrun()
                out.marker(0xD0 + ((i // per - 1) & 7))
            pred = {c: 0 for c in comps}
        c = comp_of[i]
        row = zz[blk]
        if ss == 0 and ah == 0:
            v = int(row[0]) >> al
            d = v - pred[c]
            pred[c] = v
            n = _nbits(abs(d))
            out.put(dc_code[n], CODE_BITS)
            out.put(d if d >= 0 else d - 1, n)
        elif ss == 0:
            out.put((int(row[0]) >> al) & 1, 1)
        elif ah == 0:
            r = 0
            for k in range(ss, se + 1):
                v = int(row[k])
                a = abs(v) >> al
                if a == 0:
                    r += 1
                    continue
                emit_eobrun()
                while r > 15:
                    out.put(ac_code[0xF0], CODE_BITS)
                    r -= 16
                n = _nbits(a)
                out.put(ac_code[(r << 4) | n], CODE_BITS)
                out.put(a if v >= 0 else ~a, n)
                r = 0
            if r > 0:
                st['eobrun'] += 1
                if st['eobrun'] == 0x7FFF:
                    emit_eobrun()
        else:
            absv = [abs(int(row[k])) >> al for k in range(64)]
            eob = max([k for k in range(ss, se + 1) if absv[k] == 1], default=-1)
            r, br = 0, []
            for k in range(ss, se + 1):
                t = absv[k]
                if t == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    emit_eobrun()
                    out.put(ac_code[0xF0], CODE_BITS)
                    r -= 16
                    for b in br:
                        out.put(b, 1)
                    br = []
                if t > 1:
                    br.append(t & 1)
                    continue
                emit_eobrun()
                out.put(ac_code[(r << 4) | 1], CODE_BITS)
                out.put(0 if row[k] < 0 else 1, 1)
                for b in br:
                    out.put(b, 1)
                br = []
                r = 0
            if r > 0 or br:
                st['eobrun'] += 1
                st['be'] += br
                if st['eobrun'] == 0x7FFF or len(st['be']) > 900:
                    emit_eobrun()
    emit_eobrun()
    out.flush()
    return bytes(out.bytes)


def write(info, coef, script, scan_bytes=None):
    """`scan_bytes(sc, ri)` replaces the entropy coder (the parser's tests write scripts that no coefficients could follow)"""
    comps = info['components']
    coef = None if coef is None else np.asarray(coef, np.int64)
    f = bytearray(b'\xff\xd8')
    f += _seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for tq in sorted({c['tq'] for c in comps}):
        f += _seg(0xDB, bytes([tq]) + bytes(info['qtables'][tq]))
    sof = struct.pack('>BHHB', 8, info['height'], info['width'], len(comps))
    for c in comps:
        sof += bytes([c['id'], c['h'] << 4 | c['v'], c['tq']])
    f += _seg(0xC2, sof)
    ri = 0
    for sc in script:
        if 'ri' in sc and sc['ri'] != ri:
            ri = sc['ri']
            f += _seg(0xDD, struct.pack('>H', ri))
        if sc['ah'] == 0 and sc['ss'] == 0:
            f += _dht(0, 0, DC_SYMBOLS)
        elif sc['ss'] > 0:
            f += _dht(1, 0, AC_SYMBOLS)
        sos = bytes([len(sc['comps'])])
        for c in sc['comps']:
            sos += bytes([comps[c]['id'], 0])
        sos += bytes([sc['ss'], sc['se'], sc['ah'] << 4 | sc['al']])
        f += _seg(0xDA, sos)
        f += scan_bytes(sc, ri) if scan_bytes else _encode_scan(info, coef, sc, ri)
    f += b'\xff\xd9'
    return bytes(f)


# ---- the scripts of the tests (three components unless said otherwise) -----------------------------------------------------------
def _s(comps, ss, se, ah, al, **kw):
    return dict(comps=comps, ss=ss, se=se, ah=ah, al=al, **kw)


SCRIPTS = {
    # as mozjpeg orders a file: one DC scan per component, luminance AC split in three bands, chroma in one
    'mozjpeg_like': [_s([0], 0, 0, 0, 0), _s([1], 0, 0, 0, 0), _s([2], 0, 0, 0, 0), _s([0], 1, 2, 0, 0), _s([0], 3, 9, 0, 0),
                     _s([0], 10, 63, 0, 0), _s([1], 1, 63, 0, 0), _s([2], 1, 63, 0, 0)],
    # a chain of three refinements on the luminance DC and AC
    'chain': [_s([0, 1, 2], 0, 0, 0, 3), _s([0], 1, 63, 0, 3), _s([1], 1, 63, 0, 0), _s([2], 1, 63, 0, 0),
              _s([0, 1, 2], 0, 0, 3, 2), _s([0], 1, 63, 3, 2), _s([0, 1, 2], 0, 0, 2, 1), _s([0], 1, 63, 2, 1),
              _s([0, 1, 2], 0, 0, 1, 0), _s([0], 1, 63, 1, 0)],
    # the restart interval changes between scans: none, then 2, then 5
    'dri_changes': [_s([0, 1, 2], 0, 0, 0, 1), _s([0], 1, 63, 0, 1, ri=2), _s([1], 1, 63, 0, 0), _s([2], 1, 63, 0, 0),
                    _s([0, 1, 2], 0, 0, 1, 0, ri=5), _s([0], 1, 63, 1, 0)],
    # one component: a single first scan over the whole band, then refinements
    'grey_full_band': [_s([0], 0, 0, 0, 0), _s([0], 1, 63, 0, 2), _s([0], 1, 63, 2, 1), _s([0], 1, 63, 1, 0)],
}
