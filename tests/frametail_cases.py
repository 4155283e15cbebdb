"""Seeded cases and plain references for the depth-of-field frame tail (csrc/frametail.hip), shared by
tests/test_frametail_references.py (CPU: the oracle, and the path every case exists for) and tests/test_gpu_frametail.py (the HIP
kernels).  numpy only; nothing here comes from the library or from the oracle.  colorize_ref, bokeh_depth_ref, highlight_refs and
yardstick are the ones of imageops_cases.py.  `traversal` restates which element each lane of each wave hands to each
`wave_hist_add` call of the radix select, so that the CPU test can prove which counting path a case reaches."""
import functools

import numpy as np

from imageops_cases import F32, F64, bokeh_depth_ref, colorize_input, colorize_ref, highlight_refs, rng_of, yardstick  # noqa: F401

FLT_MAX = F32(np.finfo(np.float32).max)
K_BLOCK, K_SEL_GRID, K_WIN, K_FINE = 256, 256, 4096, 65536       # frametail.hip: kBlock, kSelGrid, kWin, kFine


def same(a, b):
    """equality by value with NaN equal to NaN (and -0 equal to +0)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def same_bits(a, b):
    """bit equality of two float32 arrays, except that any NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# =====================================================================================================================================
# 1. percentiles
# =====================================================================================================================================
def lerp_sorted(s, q):
    """numpy 1.26's percentile, method 'linear', on an already sorted float32 array: virtual index (n - 1) * (q / 100) in float64, the
    lower and upper neighbours, a + (b - a) t for t < 0.5, else b - (b - a)(1 - t) in float64, rounded to float32"""
    n = s.size
    vi = F64(n - 1) * (F64(q) / F64(100.0))
    lo = int(np.floor(vi))
    hi = min(lo + 1, n - 1)
    x, y, t = F64(s[lo]), F64(s[hi]), vi - F64(lo)
    with np.errstate(invalid='ignore', over='ignore'):
        r = x + (y - x) * t if t < 0.5 else y - (y - x) * (F64(1.0) - t)
        return F32(r)


def percentile_ref(a, q):
    """np.percentile(a, q) of a float32 array as the reference's pinned numpy evaluates it (see lerp_sorted); NaN inputs are outside
    the contract of the kernel and of this reference"""
    return lerp_sorted(np.sort(np.asarray(a, F32).reshape(-1)), q)


def four_ranks(n, q_lo, q_hi):
    """the 0-based ranks (lower, upper) x (q_lo, q_hi) that a call selects"""
    out = []
    for q in (q_lo, q_hi):
        lo = int(np.floor(F64(n - 1) * (F64(q) / F64(100.0))))
        out += [lo, min(lo + 1, n - 1)]
    return out


PCT_LENGTHS = [1, 2, 3, 4, 5, 7, 255, 256, 257, 4095, 4096, 4097, 65539, 1048576, 1048576 + 4099]
PCT_OFFSET_LENGTHS = [1, 3, 4, 5, 257, 4097, 65539, 1048576 + 4099]          # also as a view offset by one float (4-byte aligned only)
PCT_KINDS = ['depth', 'ties', 'constant', 'signed', 'wide', 'top', 'bottom', 'one_prefix', 'one_key24', 'four_prefixes']
PCT_KIND_LENGTHS = [257, 65539]
PCT_PAIRS = [(2.0, 85.0), (0.0, 100.0), (50.0, 99.9), (100.0, 100.0), (0.0, 0.0)]
WIDE_SPECIAL = np.array([0.0, -0.0, 1e-40, -1e-40, FLT_MAX, -FLT_MAX, np.inf, -np.inf, 1.4e-45, -1.4e-45], F32)


@functools.lru_cache(maxsize=None)
def percentile_values(kind, n):
    """float32 [n]; shared, never written to"""
    r = rng_of(71, PCT_KINDS.index(kind), n)
    if kind == 'depth':
        a = r.uniform(200.0, 900.0, n).astype(F32)
    elif kind == 'ties':
        a = np.round(r.uniform(0.0, 8.0, n)).astype(F32)
    elif kind == 'constant':
        a = np.full(n, F32(2.75))
    elif kind == 'signed':
        a = r.normal(0.0, 1.0, n).astype(F32)
    elif kind == 'wide':                                    # signed log-uniform 1e-30 .. 1e30, the specials spread over the plane
        a = (np.where(r.integers(0, 2, n) == 1, -1.0, 1.0) * 10.0 ** r.uniform(-30.0, 30.0, n)).astype(F32)
        k = min(n, len(WIDE_SPECIAL))
        a[(np.arange(k) * (n // k))] = WIDE_SPECIAL[:k]
    elif kind in ('top', 'bottom'):
        # half of the plane within a factor 34 of FLT_MAX (inside the clipped window of a block that starts there), half near 1;
        # the first element of block 0 is +inf, of block 1 (element 1024) FLT_MAX: both windows end past the last key
        big = r.uniform(1e37, 3.4e38, n)
        a = np.where(r.integers(0, 2, n) == 1, big, r.uniform(1.0, 2.0, n)).astype(F32)
        a[0] = np.inf
        if n > 1024:
            a[1024] = FLT_MAX
        if kind == 'bottom':
            a = -a
    elif kind == 'one_prefix':                              # [1, 1 + 2^-7): float bits 0x3F80xxxx
        a = r.uniform(1.0, 1.0078, n).astype(F32)
    elif kind == 'one_key24':                               # only the low byte differs
        a = (np.uint32(0x40490F00) | r.integers(0, 256, n).astype(np.uint32)).view(F32)
    elif kind == 'four_prefixes':                           # finite values of both signs spread evenly over all 65024 16-bit buckets:
        top = np.arange(0x0080, 0x7F80, dtype=np.uint32)    # up to that length every element has a bucket of its own
        top = r.permutation(np.concatenate([top, top | np.uint32(0x8000)]))
        a = ((np.resize(top, n) << np.uint32(16)) | r.integers(0, 65536, n).astype(np.uint32)).view(F32)
    else:
        raise KeyError(kind)
    a = np.ascontiguousarray(a, F32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _sorted_of(kind, n):
    return np.sort(percentile_values(kind, n))


def percentile_cases():
    """-> list of (kind, n, aligned, q_lo, q_hi): every length with 'depth' and 'signed' at (2, 85), a subset of them also offset by one
    float; every kind at two lengths with every pair; n = 3 with q = 25 (virtual index 0.5: t == 0.5 exactly)"""
    out = []
    for kind in ('depth', 'signed'):
        for n in PCT_LENGTHS:
            out.append((kind, n, True, 2.0, 85.0))
        for n in PCT_OFFSET_LENGTHS:
            out.append((kind, n, False, 2.0, 85.0))
    for kind in PCT_KINDS:
        for n in PCT_KIND_LENGTHS:
            for q_lo, q_hi in PCT_PAIRS:
                if (kind, n, True, q_lo, q_hi) not in out:
                    out.append((kind, n, True, q_lo, q_hi))
    out.append(('depth', 3, True, 25.0, 25.0))
    out.append(('signed', 3, False, 25.0, 75.0))
    return out


def percentile_id(c):
    return "%s-%d-%s-%g-%g" % (c[0], c[1], 'a16' if c[2] else 'a4', c[3], c[4])


def percentile_want(c):
    kind, n, _, q_lo, q_hi = c
    return np.array([lerp_sorted(_sorted_of(kind, n), q_lo), lerp_sorted(_sorted_of(kind, n), q_hi)], F32)


def ordered_key(a):
    """the order-preserving uint32 image of float32 values (frametail.hip ordered_key)"""
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def traversal(n, aligned):
    """The element loop of the three selection kernels (for_each_value) for a plane of n floats whose pointer is 16-byte aligned or
    not.  -> dict: grid = min(256, ceil(n / 4096)); n4 (float4s taken by the vector loop, 0 on the scalar route); calls: int64
    [ncalls, 256], the element each thread of a block hands to one wave_hist_add call (-1: not live), rows in the order the block
    issues them; block, trip (outer trip of the vector loop, -1 in the scalar tail), unroll and comp (-1 in the tail) of every row;
    first: the element whose key centres each block's LDS window."""
    grid = min(K_SEL_GRID, max(1, -(-n // (K_BLOCK * 16))))
    n4 = n // 4 if aligned else 0
    stride = grid * K_BLOCK
    tid = np.arange(K_BLOCK, dtype=np.int64)
    rows, blk, trip, unr, comp = [], [], [], [], []
    for b in range(grid):
        t = 0
        base = b * K_BLOCK
        while base < n4:
            for u in range(4):
                i4 = base + u * stride + tid
                for c in range(4):
                    rows.append(np.where(i4 < n4, i4 * 4 + c, -1)); blk.append(b); trip.append(t); unr.append(u); comp.append(c)
            base += stride * 4
            t += 1
        base = n4 * 4 + b * K_BLOCK
        while base < n:
            i = base + tid
            rows.append(np.where(i < n, i, -1)); blk.append(b); trip.append(-1); unr.append(-1); comp.append(-1)
            base += stride
    first = np.array([b * K_BLOCK * 4 if b * K_BLOCK * 4 < n else 0 for b in range(grid)], np.int64)
    return dict(grid=grid, n4=n4, calls=np.stack(rows), block=np.array(blk), trip=np.array(trip), unroll=np.array(unr),
                comp=np.array(comp), first=first)


def window_bases(a, tr):
    """win_base of every block in k_sel_top16: the top 16 key bits of its first element minus half a window, not below 0"""
    d_first = (ordered_key(a[tr['first']]) >> np.uint32(16)).astype(np.int64)
    return np.where(d_first > K_WIN // 2, d_first - K_WIN // 2, 0)


def top16_paths(a, aligned):
    """Which counting path of wave_hist_add every (call, wave) of k_sel_top16 takes -> dict of counts: 'idle' (no live lane),
    'uniform' (one add for the wave), 'mixed' (per-lane atomics), 'leaders' (some digit outside the block's window: the leader
    loop), 'overflow' (more than 8 distinct digits outside it: the per-lane tail of that loop); plus 'clipped_lo' / 'clipped_hi': the
    live elements counted INSIDE the LDS window of a block whose window is clipped at key 0 / at key 65536, and every element is
    visited exactly once ('visited')."""
    tr = traversal(a.size, aligned)
    wb = window_bases(a, tr)
    calls = tr['calls'].reshape(-1, 4, 64)                                    # [call, wave, lane]
    live = calls >= 0
    d = (ordered_key(a)[np.where(live, calls, 0)] >> np.uint32(16)).astype(np.int64)
    base = wb[tr['block']][:, None, None]
    inside = (d - base >= 0) & (d - base < K_WIN)
    out = dict(idle=0, uniform=0, mixed=0, leaders=0, overflow=0)
    dmin = np.where(live, d, 1 << 20).min(-1)
    dmax = np.where(live, d, -1).max(-1)
    any_live = live.any(-1)
    uniform = any_live & (dmin == dmax)
    out['idle'] = int((~any_live).sum())
    out['uniform'] = int(uniform.sum())
    outside = live & ~inside
    has_out = outside.any(-1) & ~uniform
    out['mixed'] = int((any_live & ~uniform & ~has_out).sum())
    out['leaders'] = int(has_out.sum())
    for ci, wi in zip(*np.nonzero(has_out)):
        if np.unique(d[ci, wi][outside[ci, wi]]).size > 8:
            out['overflow'] += 1
    lo_blocks, hi_blocks = (wb == 0), (wb + K_WIN > K_FINE)
    out['clipped_lo'] = int((live & inside & lo_blocks[tr['block']][:, None, None]).sum())
    out['clipped_hi'] = int((live & inside & hi_blocks[tr['block']][:, None, None]).sum())
    seen = np.bincount(tr['calls'][tr['calls'] >= 0], minlength=a.size)
    out['visited'] = bool((seen == 1).all() and seen.size == a.size)
    return out


# =====================================================================================================================================
# 2. colourise + bokeh statistics
# =====================================================================================================================================
def bokeh_stats_ref(bytes_present, focal):
    """{dmax, mn, mx2} of utils/effects.py:146-153 from the byte values that occur; every step one float32 numpy operation"""
    v = np.unique(np.asarray(bytes_present, np.uint8)).astype(F32)
    dmax = v.max()
    t = dmax - np.abs(v - F32(focal))
    mn = t.min()
    mx2 = (t - mn).max()
    return F32(dmax), F32(mn), F32(mx2)


def lut_gray_r():
    return ((1.0 - np.linspace(0.0, 1.0, 256)) * 255).astype(np.uint8)


CS_LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 262144, 262148, 1048576 + 7]
CS_PLANES = ['noise', 'flat', 'spans', 'spans_one', 'ends']
CS_PLANE_LENGTHS = [1025, 262148]
CS_FOCALS = [-1.0, 0.0, 17.25, 100.0, 255.0]
CS_RANGE = (0.5, 3.25)
CS_FLAT = (1.5, 1.5)
CS_SPAN = 256                                               # elements of one wave trip on the vector route: 64 lanes x 4


@functools.lru_cache(maxsize=None)
def colorize_plane(kind, n):
    """-> (value float32 [n], vmin, vmax); shared, never written to"""
    vmin, vmax = CS_FLAT if kind == 'flat' else CS_RANGE
    if kind in ('noise', 'flat'):
        v = colorize_input(n, vmin, vmax)                  # its first elements: vmax, vmin, their neighbours, far under, far over
    elif kind in ('spans', 'spans_one'):
        span = np.arange(n) // CS_SPAN
        v = (vmin + ((span * 37) % 256 + 0.5) / 256.0 * (vmax - vmin)).astype(F32)
        if kind == 'spans_one':
            i = min(n - 1, CS_SPAN * (n // CS_SPAN // 2) + 77)                         # one lane of one wave: byte 0 or 255 among equals
            v[i] = F32(vmax + 1.0) if (i // CS_SPAN * 37) % 256 < 128 else F32(vmin - 1.0)
    elif kind == 'ends':                                    # under -> index 0 -> byte 255; over -> index 255 -> byte 0
        v = np.where(rng_of(72, n).integers(0, 2, n) == 1, F32(vmin - 5.0), F32(vmax + 5.0)).astype(F32)
        v[0], v[-1] = F32(vmax + 5.0), F32(vmin - 5.0)
    else:
        raise KeyError(kind)
    v = np.ascontiguousarray(v, F32)
    v.setflags(write=False)
    return v, F32(vmin), F32(vmax)


@functools.lru_cache(maxsize=None)
def colorize_bytes(kind, n):
    v, vmin, vmax = colorize_plane(kind, n)
    b = colorize_ref(v, vmin, vmax)
    b.setflags(write=False)
    return b


def colorize_grid(n):
    return min(256, -(-(-(-n // 4)) // K_BLOCK))          # cdiv(cdiv(n, 4), kBlock), at most 256


def colorize_wave_uniform(bytes_, n):
    """on the vector route of k_colorize_stats: per (trip, wave, component) whether the 64 lanes share the byte -> bool array over the
    whole spans of the plane (a span = the 256 elements of one wave trip)"""
    whole = (n // CS_SPAN) * CS_SPAN
    b = bytes_[:whole].reshape(-1, 64, 4)
    return (b == b[:, :1, :]).all(1)


# =====================================================================================================================================
# 3. bokeh prep, bokeh depth auto
# =====================================================================================================================================
BP_LENGTHS = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4099, 1048576 + 7]
BP_MISALIGNED = ['d8', 'img', 'dm', 'hi']
BP_LIGHTNESS = [10.0, 2.5, 1.0]
BP_FOCALS = [-1.0, 17.25, 255.0]
BDA_LENGTHS = [1, 15, 16, 17, 4095, 4096, 4097, 262144, 262144 + 21]
BDA_OFFSET_MAX = 4097


@functools.lru_cache(maxsize=None)
def byte_plane(n, single=False, key=0):
    """uint8 [n] with 0 and 255 among its values (from n = 2 on); single: one value everywhere (mx2 == 0)"""
    if single:
        d = np.full(n, 93, np.uint8)
    else:
        d = rng_of(73, n, key).integers(0, 256, n, dtype=np.uint8)
        d[0] = 255
        if n > 1:
            d[-1] = 0
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def byte_image(n):
    im = rng_of(74, n).integers(0, 256, 3 * n, dtype=np.uint8)
    im[0] = 0
    im[-1] = 255
    im.setflags(write=False)
    return im


def bokeh_plane_ref(d8, focal):
    """the bokeh depth plane from the bytes alone -> (plane float32, (dmax, mn, mx2)); a single-valued plane divides 0 by 0: NaN"""
    dmax, mn, mx2 = bokeh_stats_ref(d8, focal)
    with np.errstate(invalid='ignore', divide='ignore'):
        return bokeh_depth_ref(d8, dmax, focal, mn, mx2), (dmax, mn, mx2)


# =====================================================================================================================================
# 4. masked median
# =====================================================================================================================================
MM_LENGTHS = [1, 255, 256, 257, 4096, 4097, 256 * 4096 + 1]
MM_CASES = [(n, 5) for n in MM_LENGTHS] + [(257, 1), (4097, 1), (257, 17), (4097, 17)]
MM_KINDS = ['even', 'empty', 'single', 'odd', 'half', 'all255']
MM_BYTES = np.array([1, 2, 255], np.uint8)


def masked_median_ref(d8, masks):
    """-> float32 [n_inst + 1]: np.median(d8[mask != 0]) per instance (nan for an empty mask), then the largest, -1 if all are empty"""
    out = np.full(masks.shape[0] + 1, np.nan, F32)
    for k, m in enumerate(masks):
        sel = d8[m != 0]
        if sel.size:
            out[k] = F32(np.median(sel))
    out[-1] = F32(-1.0) if np.isnan(out[:-1]).all() else np.nanmax(out[:-1])
    return out


@functools.lru_cache(maxsize=None)
def masked_case(n, n_inst):
    """-> (d8 [n], masks uint8 [n_inst, n], kinds): instance k is of kind MM_KINDS[k % 6] where n has room for it (else 'single');
    non-zero mask bytes are drawn from {1, 2, 255}.  'half': four pixels holding 10, 10, 13, 13 (median 11.5); 'all255': the pixels that hold 255"""
    r = rng_of(75, n, n_inst)
    d8 = r.integers(0, 255, n, dtype=np.uint8)                                # 255 only where planted
    if n >= 16:
        d8[[2, 5]] = 10
        d8[[n - 3, n - 7]] = 13
        d8[[1, n // 2, n - 1]] = 255
    masks = np.zeros((n_inst, n), np.uint8)
    kinds = []
    for k in range(n_inst):
        kind = MM_KINDS[k % len(MM_KINDS)]
        if n < 16 and kind not in ('empty', 'single'):
            kind = 'single'
        if kind == 'single':
            masks[k, n - 1] = 255
        elif kind in ('even', 'odd'):
            sel = r.permutation(n)[:max(2, n // 3)]
            if (sel.size % 2 == 0) != (kind == 'even'):
                sel = sel[:-1]
            masks[k, sel] = MM_BYTES[r.integers(0, 3, sel.size)]
        elif kind == 'half':
            masks[k, [2, 5, n - 3, n - 7]] = [1, 2, 255, 2]
        elif kind == 'all255':
            masks[k, d8 == 255] = 2
        kinds.append(kind)
    d8.setflags(write=False)
    masks.setflags(write=False)
    return d8, masks, tuple(kinds)


# =====================================================================================================================================
# 5. frames for the fused call
# =====================================================================================================================================
# (name, warptile_cases case or None, H, W): 561 pixels (1 mod 4) both ways, 3150 (2 mod 4), 6767 (3 mod 4), and 512 as the aligned control
FRAMES = [('17x33', 'tiny_17x33', 17, 33), ('33x17', 'tiny_33x17', 33, 17), ('45x70', 'seams', 45, 70), ('67x101', None, 67, 101),
          ('16x32', 'tiny_16x32', 16, 32)]
FRAME_DOFS = [(-1.0, 32, 10.0), (117.25, 32, 2.5)]          # (focal plane, samples, lightness); -1: the product's value without an instance


def frame_cloud(name):
    """-> dict(H, W, pts [3, N], rgb [3, N], depth [1, N], shift, focal, baseline)"""
    import warptile_cases as W
    _, case, H, Wd = [f for f in FRAMES if f[0] == name][0]
    if case is not None:
        return W.case(case)
    return W._case(name, H, Wd, *W._grid_cloud(H, Wd, 67), shift=(2.3, -1.1, -3.0))
