"""numpy / Python restatement of the progressive-JPEG coefficient decode of csrc/jpegprog.hip.

A progressive file (T.81 Annex G, Huffman) brings the quantised coefficients of a frame in several scans; once they are all in, the
pixels are those of jpegdec_restatement.pixels, unchanged.  Integer-exact: the HIP library must return the same bytes.

    decode_coefficients(data, info)              the serial decode of T.81 G.2 (figures G.3 - G.7): int [blocks, 64], natural order, in
                                                 the MCU-interleaved block order of the baseline restatement
    decode_scan(data, info, j, coef)             one scan of it, applied to `coef` in place
    decode_first_scan_subseq(data, info, j, S)   the coefficients of first scan j alone, by the self-synchronising subsequence
                                                 decode of the kernels
    refine_block_positions / refine_block_symbols  one block of an AC refinement scan, position by position as T.81 G.7 draws it,
                                                 and symbol by symbol over a 64-bit mask of the block's history as the kernel does it
    decode(data)                                 probe + decode_coefficients + jpegdec_restatement.pixels

Written for clarity; the entropy decode is a Python loop per symbol.
"""
import numpy as np

import jpegdec_restatement as R
from cartoonsegmentation_amd import jpegcode

ZIGZAG = R.ZIGZAG
_ZZ = ZIGZAG.tolist()


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def scan_blocks(info, sc):
    """(store index of every block of the scan in scan order, component of each, blocks per restart unit).  An interleaved scan
    walks the padded MCU grid, which is the store's own order; a one-component scan walks only the component's true block grid,
    ceil(ceil(W h / hmax) / 8) by ceil(ceil(H v / vmax) / 8), in raster order, and its restart interval counts blocks."""
    g = R.geometry(info)
    comps = info['components']
    if len(sc['components']) > 1:
        return np.arange(g['blocks']), np.tile(np.array(g['comp_of']), g['mx'] * g['my']), g['bpm']
    c = sc['components'][0][0]
    h, v = comps[c]['h'], comps[c]['v']
    bw = -(-(-(-g['W'] * h // g['hs'])) // 8)
    bh = -(-(-(-g['H'] * v // g['vs'])) // 8)
    first = sum(g['nb'][:c])
    by, bx = np.divmod(np.arange(bw * bh), bw)
    idx = ((by // v) * g['mx'] + bx // h) * g['bpm'] + first + (by % v) * h + bx % h
    return idx, np.full(bw * bh, c), 1


def _intervals(raw):
    """the entropy bytes of a scan as one `bytes` per restart interval, stuffed zeros and fill bytes taken out"""
    out, cur = [], bytearray()
    i, n = 0, len(raw)
    while i < n:
        b = raw[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
        elif i + 1 < n and raw[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif i + 1 < n and 0xD0 <= raw[i + 1] <= 0xD7:
            out.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            i += 1                                   # a fill byte
    out.append(bytes(cur))
    return out


class _Bits:
    """MSB-first reader of one restart interval; a read past its end is an error, never padding"""

    def __init__(self, data):
        self.v = int.from_bytes(data, 'big') if data else 0
        self.n = len(data) * 8
        self.p = 0

    def get(self, k):
        if k == 0:
            return 0
        if self.p + k > self.n:
            raise ValueError("a read past the end of the scan's data")
        self.p += k
        return (self.v >> (self.n - self.p)) & ((1 << k) - 1)

    def symbol(self, lut):
        left = self.n - self.p
        k = min(16, left)
        w = ((self.v >> (left - k)) & ((1 << k) - 1)) << (16 - k) if k else 0
        e = lut[w]
        if e == 0 or (e >> 8) > left:
            raise ValueError("invalid Huffman code in the scan's data")
        self.p += e >> 8
        return e & 255


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


# ---- AC refinement of one block (T.81 G.1.2.3, figure G.7) -------------------------------------------------------------------
def refine_block_positions(blk, ss, se, al, bits, lut, eobrun):
    """Position by position.  blk: the block's 64 coefficients in zigzag order (a list, changed in place).  The run field of a
    symbol counts only positions whose coefficient is still zero; every non-zero one that is passed takes one correction bit, and
    the correction moves it by 1 << al away from zero if that bit is still clear.  Returns the EOB run left after this block."""
    p1, m1 = 1 << al, -(1 << al)

    def correct(k):
        if bits.get(1):
            c = blk[k]
            if (abs(c) & p1) == 0:
                blk[k] = c + p1 if c >= 0 else c + m1
    k = ss
    if eobrun == 0:
        while k <= se:
            sym = bits.symbol(lut)
            r, s = sym >> 4, sym & 15
            val = 0
            if s:
                if s != 1:
                    raise ValueError("a refinement symbol with size %d" % s)
                val = p1 if bits.get(1) else m1
            elif r != 15:
                eobrun = (1 << r) + bits.get(r)           # this block included
                break
            while k <= se:
                if blk[k] != 0:
                    correct(k)
                else:
                    r -= 1
                    if r < 0:
                        break
                k += 1
            if s:
                if k > se:
                    raise ValueError("a coefficient placed past the end of the band")
                blk[k] = val
            k += 1
    if eobrun > 0:
        while k <= se:
            if blk[k] != 0:
                correct(k)
            k += 1
        eobrun -= 1
    return eobrun


def history_mask(blk, ss, se):
    return sum(1 << k for k in range(ss, se + 1) if blk[k] != 0)


def _select(free, r):
    """position of the r-th (from 0) set bit of free, or None"""
    for _ in range(r):
        free &= free - 1
    return (free & -free).bit_length() - 1 if free else None


def refine_block_symbols(blk, ss, se, al, bits, lut, eobrun):
    """Symbol by symbol, as the kernel does it: the block's history is a 64-bit mask (bit k: coefficient k was non-zero before this
    scan); a symbol with run r ends at the (r + 1)-th clear bit at or after k, the correction bits in between are as many as the
    mask has set bits there, and only those positions and the one new coefficient are touched."""
    p1, m1 = 1 << al, -(1 << al)
    hist = history_mask(blk, ss, se)
    band = (1 << (se + 1)) - 1

    def corrections(lo, hi):
        """positions lo..hi (hi included)"""
        if hi < lo:
            return
        m = hist & ((1 << (hi + 1)) - 1) & ~((1 << lo) - 1)
        n = bin(m).count('1')
        word = bits.get(n)
        while m:
            k = (m & -m).bit_length() - 1
            m &= m - 1
            n -= 1
            if (word >> n) & 1:
                c = blk[k]
                if (abs(c) & p1) == 0:
                    blk[k] = c + p1 if c >= 0 else c + m1
    k = ss
    if eobrun == 0:
        while k <= se:
            sym = bits.symbol(lut)
            r, s = sym >> 4, sym & 15
            val = 0
            if s:
                if s != 1:
                    raise ValueError("a refinement symbol with size %d" % s)
                val = p1 if bits.get(1) else m1
            elif r != 15:
                eobrun = (1 << r) + bits.get(r)
                break
            target = _select(~hist & band & ~((1 << k) - 1), r)
            if target is None:
                corrections(k, se)
                if s:
                    raise ValueError("a coefficient placed past the end of the band")
                k = se + 1
                break
            corrections(k, target)
            if s:
                blk[target] = val
            k = target + 1
    if eobrun > 0:
        corrections(k, se)
        eobrun -= 1
    return eobrun


# ---- the serial decode ------------------------------------------------------------------------------------------------------
def decode_scan(data, info, j, coef, symbol_stepping=False):
    """scan j of the file applied to coef (int64 [blocks, 64], natural order, store order) in place"""
    sc = info['scans'][j]
    ss, se, ah, al, ri = sc['ss'], sc['se'], sc['ah'], sc['al'], sc['restart_interval']
    order, comp_of, bpu = scan_blocks(info, sc)
    order, comp_of = order.tolist(), comp_of.tolist()
    s, e = sc['entropy']
    ivals = _intervals(bytes(data[s:e]))
    per = ri * bpu if ri else len(order)
    if len(ivals) != max(1, -(-len(order) // per)):
        raise ValueError("scan %d: %d restart intervals for %d blocks" % (j, len(ivals), len(order)))
    tables = {c: (td, ta) for c, td, ta in sc['components']}
    if ah == 0 and ss == 0:
        luts = {c: R._lut16(*sc['huffman'][(0, tables[c][0])]) for c in tables}
    elif ss > 0:
        lut = R._lut16(*sc['huffman'][(1, sc['components'][0][2])])
    refine = refine_block_symbols if symbol_stepping else refine_block_positions
    for iv, raw in enumerate(ivals):
        bits = _Bits(raw)
        blocks = range(iv * per, min((iv + 1) * per, len(order)))
        if ss == 0 and ah == 0:
            pred = {c: 0 for c in tables}
            for i in blocks:
                c = comp_of[i]
                sz = bits.symbol(luts[c])
                if sz > 11:
                    raise ValueError("a DC difference of %d bits" % sz)
                pred[c] += _extend(bits.get(sz), sz)           # predict on the unshifted values, then shift
                coef[order[i], 0] = pred[c] << al
        elif ss == 0:
            for i in blocks:
                if bits.get(1):
                    coef[order[i], 0] = int(coef[order[i], 0]) | (1 << al)           # two's complement, as libjpeg does it
        elif ah == 0:
            eobrun = 0
            for i in blocks:
                if eobrun > 0:
                    eobrun -= 1
                    continue
                k = ss
                while k <= se:
                    sym = bits.symbol(lut)
                    r, sz = sym >> 4, sym & 15
                    if sz:
                        k += r
                        if k > se:
                            raise ValueError("a coefficient placed past the end of the band")
                        coef[order[i], _ZZ[k]] = _extend(bits.get(sz), sz) * (1 << al)
                        k += 1
                    elif r == 15:
                        k += 16
                    else:
                        eobrun = (1 << r) - 1 + bits.get(r)       # further blocks
                        break
        else:
            eobrun = 0
            for i in blocks:
                blk = coef[order[i], ZIGZAG].tolist()
                eobrun = refine(blk, ss, se, al, bits, lut, eobrun)
                coef[order[i], ZIGZAG] = blk
        left = bits.n - bits.p
        if left >= 8 or (left and bits.get(left) != (1 << left) - 1):
            raise ValueError("scan %d: the data do not hold the scan's blocks exactly" % j)


def decode_coefficients(data, info=None, symbol_stepping=False, snapshots=None):
    """serial decode of every scan in file order: int64 [blocks, 64], natural order, the block order of the baseline restatement.
    `snapshots` (a list) receives a copy of the coefficients after every scan."""
    info = info or jpegcode.probe(data, progressive=True)
    coef = np.zeros((R.geometry(info)['blocks'], 64), np.int64)
    for j in range(len(info['scans'])):
        decode_scan(data, info, j, coef, symbol_stepping)
        if snapshots is not None:
            snapshots.append(coef.copy())
    return coef


def decode(data):
    info = jpegcode.probe(data, progressive=True)
    if not info['progressive']:
        return R.decode(data)
    return R.pixels(info, decode_coefficients(data, info))


# ---- first scans by subsequences --------------------------------------------------------------------------------------------
class ScanStream(R.Stream):
    """jpegdec_restatement.Stream over the entropy bytes of one first scan (ah = 0) of a progressive file.  A state is (q, restart
    interval, b, z): logical bit position, block of the restart unit (a DC scan of all components; else 0) and k - ss (an AC
    scan; else 0).  Slots: one per block in a DC scan, se - ss + 1 per block in an AC scan."""

    def __init__(self, info, data, sc):
        s, e = sc['entropy']
        raw = np.frombuffer(bytes(data[s:e]), np.uint8)
        n = raw.size
        prev = np.concatenate([[0], raw[:-1]]).astype(np.int64)
        nxt = np.concatenate([raw[1:], [0xD9]]).astype(np.int64)
        is_ff = raw == 0xFF
        stuffed = (raw == 0) & (prev == 0xFF)
        rst_ff = is_ff & (nxt >= 0xD0) & (nxt <= 0xD7)
        rst_code = (prev == 0xFF) & (raw >= 0xD0) & (raw <= 0xD7)
        fill = is_ff & (nxt == 0xFF)
        keep = ~(stuffed | rst_ff | rst_code | fill)
        self.n = n
        self.raw = raw
        self.L = raw[keep].tobytes()
        self.cum = np.concatenate([[0], np.cumsum(keep)]).tolist()
        self.rawidx = np.concatenate([np.nonzero(keep)[0], [n]]).tolist()
        self.markers = np.nonzero(rst_ff)[0].tolist()
        self.segend = [self.cum[m] for m in self.markers] + [len(self.L)]
        self.end_q = len(self.L) * 8
        self.sc = sc
        self.order, comp_of, self.bpu = scan_blocks(info, sc)
        self.ri = sc['restart_interval']
        self.band = sc['se'] - sc['ss'] + 1
        if sc['ss'] == 0:
            td = {c: t for c, t, _ in sc['components']}
            self.luts = [R._lut16(*sc['huffman'][(0, td[c])]) for c in comp_of[:self.bpu].tolist()]
        else:
            self.luts = [R._lut16(*sc['huffman'][(1, sc['components'][0][2])])]

    def run(self, state, limit, emit=None, slot=0, markers_before=0):
        """as Stream.run.  An EOBn symbol of an AC scan takes the rest of its block plus (run) x band slots at once: the run
        uses no further bits, so it adds nothing to the state."""
        q, k, b, z = state
        L, segend, rawidx = self.L, self.segend, self.rawidx
        bpu, ri, band, dc = self.bpu, self.ri, self.band, self.sc['ss'] == 0
        per_marker = ri * bpu * band
        n_slots, n_mark = 0, 0
        nseg = len(segend)
        while True:
            while True:
                endb = segend[k]
                nreal = endb * 8 - q
                if nreal >= 8:
                    break
                if nreal and (L[q >> 3] & ((1 << nreal) - 1)) != (1 << nreal) - 1:
                    break
                if k + 1 >= nseg:
                    return (self.end_q, k, 0, 0), n_slots, n_mark, True
                k += 1
                q = endb * 8
                b = z = 0
                n_mark += 1
                if emit is not None:
                    slot = (markers_before + n_mark) * per_marker
            if q >= self.end_q or rawidx[q >> 3] * 8 + (q & 7) >= limit:
                return (q, k, b, z), n_slots, n_mark, True
            a = q >> 3
            chunk = L[a:min(a + 5, endb)]
            v = ((int.from_bytes(chunk, 'big') << (8 * (5 - len(chunk)))) >> (8 - (q & 7))) & 0xFFFFFFFF
            e = self.luts[b][v >> 16]
            if e == 0:
                return None, n_slots, n_mark, False
            ln, sym = e >> 8, e & 255
            eob = False
            if dc:
                s = extra = sym
                if s > 11:
                    return None, n_slots, n_mark, False
                adv = 1
            else:
                r, s = sym >> 4, sym & 15
                extra = s
                if s == 0:
                    if r == 15:
                        adv = 16
                    else:
                        eob, extra = True, r
                        adv = 0
                else:
                    if s > 10:
                        return None, n_slots, n_mark, False
                    adv = r + 1
                if z + adv > band:
                    return None, n_slots, n_mark, False
            total = ln + extra
            if total > nreal:
                if k + 1 >= nseg:
                    return (self.end_q, k, 0, 0), n_slots, n_mark, True
                k += 1
                q = endb * 8
                b = z = 0
                n_mark += 1
                if emit is not None:
                    slot = (markers_before + n_mark) * per_marker
                continue
            bitsv = (v >> (32 - total)) & ((1 << extra) - 1) if extra else 0
            if eob:
                adv = (band - z) + ((1 << r) - 1 + bitsv) * band
            elif s and emit is not None:
                emit.append((slot + adv - 1, _extend(bitsv, s)))
            q += total
            slot += adv
            n_slots += adv
            if dc:
                b = b + 1 if b + 1 < bpu else 0
            else:
                z = 0 if eob else (z + adv) % band


def decode_first_scan_subseq(data, info, j, S, group=None, stats=None):
    """The coefficients that first scan j alone gives (int64 [blocks, 64], zero elsewhere) by the subsequence decode: synchronise
    (jpegdec_restatement.subseq_sync), scan the slot and marker counts, decode every subsequence once more from its entry state
    and store; a DC scan then sums the differences per component, restarting at every interval, and shifts."""
    sc = info['scans'][j]
    assert sc['ah'] == 0
    st = ScanStream(info, data, sc)
    states, slots, marks, passes = R.subseq_sync(st, S, group)
    if stats is not None:
        stats['passes'] = passes
    out = []
    slot0, mark0, entry = 0, 0, (0, 0, 0, 0)
    for i in range(len(states)):
        if entry is None:
            raise ValueError("invalid Huffman code in the entropy data")
        st.run(entry, (i + 1) * S * 8, emit=out, slot=slot0, markers_before=mark0)
        slot0 += slots[i]
        mark0 += marks[i]
        entry = states[i]
    order = st.order
    if slot0 != len(order) * st.band:
        raise ValueError("scan %d: the data do not hold the scan's blocks exactly" % j)
    coef = np.zeros((R.geometry(info)['blocks'], 64), np.int64)
    scan_coef = np.zeros((len(order), 64), np.int64)                         # scan order, zigzag order
    if out:
        e = np.array(out, np.int64)
        e = e[(e[:, 0] >= 0) & (e[:, 0] < len(order) * st.band)]
        scan_coef[e[:, 0] // st.band, sc['ss'] + e[:, 0] % st.band] = e[:, 1]
    if sc['ss'] == 0:
        _, comp_of, bpu = scan_blocks(info, sc)
        per = st.ri * bpu if st.ri else len(order)
        for c, _, _ in sc['components']:
            sel = np.nonzero(comp_of == c)[0]
            d = scan_coef[sel, 0]
            seg = sel // per
            total = np.cumsum(d)
            first = np.concatenate([[True], seg[1:] != seg[:-1]])
            start = np.maximum.accumulate(np.where(first, np.arange(d.size), 0))
            scan_coef[sel, 0] = total - (total - d)[start]
    coef[order[:, None], ZIGZAG[None, :]] = scan_coef << sc['al']
    return coef
