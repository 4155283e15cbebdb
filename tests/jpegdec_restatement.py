"""numpy restatement of the baseline-JPEG decoder of csrc/jpegdec.hip.

Integer-exact: the HIP library must return the same bytes.  Three parts:

    decode_coefficients(data)            the serial Huffman decode of T.81 F.2.2: int [blocks, 64], natural order, DC as values
    decode_coefficients_subseq(data, S)  the same coefficients by the self-synchronising subsequence decode of the kernels
                                         (Weissenberger and Schmidt, ICPP 2018): one "lane" per S bytes of entropy data
    pixels(info, coef)                   dequantisation, the 13-bit integer inverse DCT, triangle chroma upsampling and the 16-bit
                                         colour conversion -> uint8 BGR [H, W, 3]
    decode(data)                         probe + decode_coefficients + pixels

Written for clarity; the entropy decode is a Python loop per symbol.
"""
import numpy as np

from cartoonsegmentation_amd import jpegcode

ZIGZAG = np.array(jpegcode.ZIGZAG, np.int64)


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def geometry(info):
    """MCU grid of the (single, interleaved) scan"""
    comps = info['components']
    hs, vs = comps[0]['h'], comps[0]['v']
    H, W = info['height'], info['width']
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    nb = [hs * vs] + [1] * (len(comps) - 1)                # blocks of each component in an MCU
    comp_of = sum(([c] * k for c, k in enumerate(nb)), [])  # component of block b of an MCU
    return {'H': H, 'W': W, 'hs': hs, 'vs': vs, 'mx': mx, 'my': my, 'nb': nb, 'bpm': sum(nb), 'comp_of': comp_of,
            'blocks': mx * my * sum(nb)}


# ---- the entropy-coded segment ---------------------------------------------------------------------------------------------
def _lut16(bits, vals):
    """lut[the next 16 bits] = length << 8 | symbol, 0 = no code"""
    lut = np.zeros(65536, np.int64)
    code, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            lo = code << (16 - ln)
            lut[lo:lo + (1 << (16 - ln))] = (ln << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


class Stream:
    """The entropy bytes of a file with the stuffed zeros, the restart markers and fill bytes taken out ("logical" bytes), and the
    map back to the file's ("raw") positions.  A position is a logical bit index q; raw(q) is the bit position the kernels hold."""

    def __init__(self, info, data):
        s, e = info['entropy']
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
        self.cum = np.concatenate([[0], np.cumsum(keep)]).tolist()             # kept bytes before raw byte i
        self.rawidx = np.concatenate([np.nonzero(keep)[0], [n]]).tolist()
        self.markers = np.nonzero(rst_ff)[0].tolist()                          # raw positions of the RST markers
        self.segend = [self.cum[m] for m in self.markers] + [len(self.L)]      # logical byte where each restart interval ends
        g = geometry(info)
        self.g = g
        self.ri = info['restart_interval']
        huff = info['huffman']
        self.dc = [_lut16(*huff[(0, info['components'][c]['td'])]) for c in g['comp_of']]
        self.ac = [_lut16(*huff[(1, info['components'][c]['ta'])]) for c in g['comp_of']]
        self.end_q = len(self.L) * 8

    def raw_pos(self, q):
        return self.rawidx[q >> 3] * 8 + (q & 7) if q < self.end_q else self.n * 8

    def cold_start(self, byte):
        """logical position of a lane that starts at raw byte `byte`: on the 00 of a stuffed pair or on the second byte of a
        marker it looks one byte back and starts behind the pair"""
        return self.cum[min(byte, self.n)] * 8

    def segment_of(self, byte):
        """restart interval of a lane that starts at raw byte `byte`: the markers that begin before it"""
        return int(np.searchsorted(np.array(self.markers, np.int64), byte, side='left'))

    def run(self, state, limit, emit=None, slot=0, markers_before=0):
        """Decode symbols from `state` = (q, k, b, z) -- logical bit position, restart interval, block of the MCU, zigzag index
        -- while raw(q) < limit.  Returns (state, slots, markers crossed, ok).  ok is False after an invalid code (the state is
        then None: a dead lane).  With `emit` (a list) every non-zero coefficient is appended as (slot, value); `slot` is then
        the absolute coefficient slot of the state and is set from the marker count at every restart marker."""
        q, k, b, z = state
        L, segend, markers, rawidx = self.L, self.segend, self.markers, self.rawidx
        bpm, ri = self.g['bpm'], self.ri
        n_slots, n_mark = 0, 0
        nseg = len(segend)
        while True:
            # a restart marker (or the end of the data) behind nothing but 1-bits of padding is taken at once
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
                    slot = (markers_before + n_mark) * ri * bpm * 64
            if q >= self.end_q or rawidx[q >> 3] * 8 + (q & 7) >= limit:
                return (q, k, b, z), n_slots, n_mark, True
            a = q >> 3
            chunk = L[a:min(a + 5, endb)]
            v = ((int.from_bytes(chunk, 'big') << (8 * (5 - len(chunk)))) >> (8 - (q & 7))) & 0xFFFFFFFF
            e = (self.dc[b] if z == 0 else self.ac[b])[v >> 16]
            if e == 0:
                return None, n_slots, n_mark, False
            ln, sym = e >> 8, e & 255
            if z == 0:
                run_, s = 0, sym
                if s > 11:
                    return None, n_slots, n_mark, False
                adv = 1
            else:
                run_, s = sym >> 4, sym & 15
                if s == 0:
                    if run_ == 15:
                        adv = 16
                    elif run_ == 0:
                        adv = 64 - z
                    else:
                        return None, n_slots, n_mark, False
                else:
                    if s > 10:
                        return None, n_slots, n_mark, False
                    adv = run_ + 1
                if z + adv > 64:
                    return None, n_slots, n_mark, False
            total = ln + s
            if total > nreal:                         # the symbol runs into the marker: not a symbol; take the marker
                if k + 1 >= nseg:
                    return (self.end_q, k, 0, 0), n_slots, n_mark, True
                k += 1
                q = endb * 8
                b = z = 0
                n_mark += 1
                if emit is not None:
                    slot = (markers_before + n_mark) * ri * bpm * 64
                continue
            if s and emit is not None:
                val = (v >> (32 - total)) & ((1 << s) - 1)
                if val < (1 << (s - 1)):
                    val -= (1 << s) - 1
                emit.append((slot + adv - 1, val))
            q += total
            z += adv
            slot += adv
            n_slots += adv
            if z == 64:
                z = 0
                b = b + 1 if b + 1 < bpm else 0


def _blocks_from(emitted, g):
    """[(slot, value)] -> int64 [blocks, 64] in natural order (DC still a difference); slots past the file's blocks are dropped,
    as the kernel's store guard drops them"""
    coef = np.zeros((g['blocks'], 64), np.int64)
    if emitted:
        e = np.array(emitted, np.int64)
        e = e[(e[:, 0] >= 0) & (e[:, 0] < g['blocks'] * 64)]
        coef[e[:, 0] >> 6, ZIGZAG[e[:, 0] & 63]] = e[:, 1]
    return coef


def dc_predict(coef, info):
    """DC differences -> values: a running sum per component that restarts at every restart interval"""
    g = geometry(info)
    ri = info['restart_interval']
    mcus = g['mx'] * g['my']
    c = coef.reshape(mcus, g['bpm'], 64).copy()
    seg = np.arange(mcus) // ri if ri else np.zeros(mcus, np.int64)
    off = 0
    for nb in g['nb']:
        d = c[:, off:off + nb, 0]
        flat = d.reshape(-1)
        s = np.repeat(seg, nb)
        total = np.cumsum(flat)
        first = np.concatenate([[True], s[1:] != s[:-1]])
        start = np.maximum.accumulate(np.where(first, np.arange(flat.size), 0))      # first element of each one's interval
        start_total = (total - flat)[start]
        c[:, off:off + nb, 0] = (total - start_total).reshape(mcus, nb)
        off += nb
    return c.reshape(-1, 64)


def decode_coefficients(data, info=None, predict=True):
    """serial decode: int64 [blocks, 64], natural order, blocks in scan order"""
    info = info or jpegcode.probe(data)
    st = Stream(info, data)
    out = []
    state, _, _, ok = st.run((0, 0, 0, 0), 1 << 62, emit=out)
    if not ok:
        raise ValueError("invalid Huffman code in the entropy data")
    coef = _blocks_from(out, st.g)
    return dc_predict(coef, info) if predict else coef


def subseq_sync(st, S, group=None):
    """The synchronisation of the kernels on subsequences of S raw bytes.  Every lane decodes its own subsequence from a cold
    state (block 0 of an MCU, zigzag index 0), then goes on into its successors from its own end state, and stops where its end
    state equals the one recorded there.  `group` lanes form a workgroup whose lanes stop at its last subsequence; the passes
    between workgroups then carry the end state of each workgroup into the next until nothing changes.  Returns (end states,
    slots, markers) per subsequence and the number of passes between workgroups."""
    nsub = max(1, -(-st.n // S))
    group = group or nsub
    DEAD = None
    states, slots, marks = [DEAD] * nsub, [0] * nsub, [0] * nsub
    cur = [None] * nsub
    # cold decode
    for j in range(nsub):
        start = j * S
        if start > 0 and st.raw[start - 1] == 0xFF and (st.raw[start] == 0 or 0xD0 <= st.raw[start] <= 0xD7):
            start += 1
        q = st.cold_start(start)
        s, n, r, ok = st.run((q, st.segment_of(start), 0, 0), (j + 1) * S * 8)
        states[j], slots[j], marks[j] = s, n, r
        cur[j] = s
    # inside a workgroup: lane i at step k decodes subsequence i + k
    active = [True] * nsub
    step = 1
    while any(active):
        new = {}
        for i in range(nsub):
            j = i + step
            if not active[i]:
                continue
            if j >= nsub or j // group != i // group or cur[i] is None:
                active[i] = False
                continue
            new[i] = st.run(cur[i], (j + 1) * S * 8)
        for i, (s, n, r, ok) in new.items():
            j = i + step
            same = s is not None and states[j] is not None and s[0] == states[j][0] and s[2:] == states[j][2:]
            states[j], slots[j], marks[j] = s, n, r
            cur[i] = s
            if same or s is None:
                active[i] = False
        step += 1
    # between workgroups
    passes = 0
    while True:
        passes += 1
        assert passes <= nsub + 1, "the synchronisation did not settle"
        changed = False
        snapshot = list(states)
        for g0 in range(group, nsub, group):
            s = snapshot[g0 - 1]
            for j in range(g0, min(g0 + group, nsub)):
                if s is None:
                    break
                s2, n, r, ok = st.run(s, (j + 1) * S * 8)
                old = states[j]
                same = s2 is not None and old is not None and s2[0] == old[0] and s2[2:] == old[2:]
                states[j], slots[j], marks[j] = s2, n, r
                if same:
                    break
                changed = True
                s = s2
        if not changed:
            break
    return states, slots, marks, passes


def decode_coefficients_subseq(data, S, info=None, group=None, predict=True):
    """the coefficients by the subsequence decode: synchronise, scan the slot and marker counts, decode every subsequence once
    more from its entry state and store at its position"""
    info = info or jpegcode.probe(data)
    st = Stream(info, data)
    states, slots, marks, passes = subseq_sync(st, S, group)
    nsub = len(states)
    out = []
    slot0, mark0 = 0, 0
    entry = (0, 0, 0, 0)
    for j in range(nsub):
        if entry is None:
            raise ValueError("invalid Huffman code in the entropy data")
        st.run(entry, (j + 1) * S * 8, emit=out, slot=slot0, markers_before=mark0)
        slot0 += slots[j]
        mark0 += marks[j]
        entry = states[j]
    coef = _blocks_from(out, st.g)
    return dc_predict(coef, info) if predict else coef


# ---- pixels -----------------------------------------------------------------------------------------------------------------
_I32 = 2 ** 31


def idct(blocks):
    """The Loeffler-Ligtenberg-Moschytz "accurate integer" inverse DCT on dequantised coefficients int64 [..., 8(v), 8(u)] ->
    samples 0..255 [..., 8(y), 8(x)]: 13-bit constants, two extra bits kept after the column pass, rounding at each descale."""
    def pass_(x, shift, axis):
        x = np.moveaxis(x, axis, -1)
        i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k] for k in range(8))
        z1 = (i2 + i6) * 4433
        t2 = z1 - i6 * 15137
        t3 = z1 + i2 * 6270
        t0 = (i0 + i4) << 13
        t1 = (i0 - i4) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        o0, o1, o2, o3 = i7, i5, i3, i1
        z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
        z5 = (z3 + z4) * 9633
        o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
        out = np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3], -1)
        assert np.abs(out).max(initial=0) + (1 << (shift - 1)) < _I32
        out = (out + (1 << (shift - 1))) >> shift
        return np.moveaxis(out, -1, axis)
    ws = pass_(blocks, 11, -2)                        # columns: descale by CONST_BITS - PASS1_BITS
    px = pass_(ws, 18, -1)                            # rows: descale by CONST_BITS + PASS1_BITS + 3
    return np.clip(px + 128, 0, 255)


def planes(info, coef):
    """the sample plane of every component at its padded size [my * vs * 8, mx * hs * 8]"""
    g = geometry(info)
    comps = info['components']
    mcus = g['mx'] * g['my']
    c = coef.reshape(mcus, g['bpm'], 8, 8)
    out, off = [], 0
    for ci, comp in enumerate(comps):
        h, v = comp['h'], comp['v']
        q = np.zeros(64, np.int64)
        q[ZIGZAG] = info['qtables'][comp['tq']]
        px = idct(c[:, off:off + h * v] * q.reshape(8, 8))                        # [mcus, h*v, 8, 8]
        px = px.reshape(g['my'], g['mx'], v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5)
        out.append(px.reshape(g['my'] * v * 8, g['mx'] * h * 8))
        off += h * v
    return out


def upsample_h(c):
    """2x1 triangle filter over the columns of c [rows, cw] -> [rows, 2 cw]"""
    left = np.concatenate([c[:, :1], c[:, :-1]], 1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out


def upsample_hv(c):
    """2x2 triangle filter of c [ch, cw] -> [2 ch, 2 cw]"""
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), np.int64)
    for par, far in ((0, up), (1, down)):
        t = 3 * c + far
        left = np.concatenate([t[:, :1], t[:, :-1]], 1)
        right = np.concatenate([t[:, 1:], t[:, -1:]], 1)
        out[par::2, 0::2] = (3 * t + left + 8) >> 4
        out[par::2, 1::2] = (3 * t + right + 7) >> 4
    return out


def pixels(info, coef):
    """uint8 BGR [H, W, 3] of the coefficients (DC as values)"""
    g = geometry(info)
    H, W = g['H'], g['W']
    p = planes(info, coef)
    Y = p[0][:H, :W]
    if len(p) == 1:
        return np.repeat(Y[:, :, None], 3, 2).astype(np.uint8)
    cw, ch = -(-W // g['hs']), -(-H // g['vs'])
    ch_planes = []
    for c in p[1:]:
        c = c[:ch, :cw]
        if g['hs'] == 2 and g['vs'] == 2:
            c = upsample_hv(c)
        elif g['hs'] == 2:
            c = upsample_h(c)
        ch_planes.append(c[:H, :W])
    cb, cr = ch_planes[0] - 128, ch_planes[1] - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([B, G, R], -1), 0, 255).astype(np.uint8)


def decode(data):
    info = jpegcode.probe(data)
    return pixels(info, decode_coefficients(data, info))
