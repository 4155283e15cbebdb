"""Case generators and plain references for the Segment Anything kernels of csrc/sam.hip (k_attention_rp, k_xattn_wave / k_xattn_lane,
k_window, k_bcast_add, k_channel_dot, k_sam_preprocess, k_sam_postprocess, k_sam_box_tokens).  Helper module, not collected.

The references are float64 numpy and use nothing from the library; next to each floating-point one stands the PLAIN FLOAT32 EVALUATION of
the same formulas in the straightforward order (dtype=np.float32), whose error against float64 -- e32(case) -- is the yardstick:

    attention_relpos, cross_attention   |got - f64| <= max(4 e32, 8 * 2^-23) * max|v|
    channel_dot, preprocess             |got - f64| <= max(4 e32, 8 * 2^-23) * max|f64|
    window ops, broadcast_add           exact
    box_tokens                          static rows exact, corner rows <= 2^-23 * max(|f64|, 1)
    postprocess                         binary, compared where |f64| > 1e-4 max|f64| of the mask (at most 0.005 of a mask left out)

bound(), ULP, FLOOR and MARGIN are those of tests/tokens_cases.py.  Every reference takes `fault=`: the planted
faults of tests/test_sam_ops_references.py, applied to the reference, never to the kernel.  All generators are seeded.
"""
import functools
import math

import numpy as np

from tokens_cases import FLOOR, MARGIN, ULP, _rng, bound  # noqa: F401


def _err(got, ref, scale, where=None):
    d = np.abs(np.asarray(got, np.float64) - ref)
    if where is not None:
        d = d[np.broadcast_to(where, d.shape)]
    return float('inf') if not np.isfinite(d).all() else float(d.max() / scale)


# ---- attention with the decomposed relative position bias --------------------------------------------------------------------------------
# qkv [n, N, 3 heads d] float32 with q pre-scaled by d^-0.5 (the op's input); rh [2 gh - 1, d], rw [2 gw - 1, d] as a checkpoint has them:
# the bias multiplies the UNSCALED q = q_s sqrt(d).  Token y * gw + x = grid position (y, x).
RP_DS = (32, 64, 80, 128)
RP_GRIDS = ((1, 1), (1, 2), (1, 31), (1, 32), (33, 1), (3, 21), (8, 8), (5, 13), (8, 9), (9, 9), (8, 12), (7, 14), (14, 14), (16, 17),
            (17, 17), (12, 31))
RP_NS = (1, 2, 31, 32, 33, 63, 64, 65, 72, 81, 96, 98, 196, 272, 289, 372)
RP_BIAS_GRIDS = ((3, 21), (7, 14), (12, 31), (14, 14))
RP_FAULTS = ('swap_tables', 'sign_y', 'sign_x', 'gh_for_gw', 'row_off_h', 'row_off_w')
RP_PEAK_GRID = (10, 15)                # N = 150: 5 key tiles, the first half holds tiles 0..2, the second 3 and 4, the last is partial
RP_PEAK_KEYS = dict(key0=0, half1=100, last_tile=130, last=149)
RP_PEAK_NAMES = ['peak_%s' % k for k in RP_PEAK_KEYS] + ['peak_mixed']
RP_MOTION_NAMES = ['max_rising', 'max_falling']
RP_ISOLATION_NAMES = ['isolation_33x1', 'isolation_7x14', 'isolation_head']
RP_REAL_NAMES = ['real_64x64', 'real_windows']
RP_ZERO_NAMES = ['zero_3x21_d32', 'zero_7x14_d64', 'zero_8x9_d128']
PEAK_LEAD = 40.0
MOTION_STEP = 6.0


def rp_indices(gh, gw, fault=None):
    """rows of the stacked table (Rh ; Rw) a (query, key) pair reads: ([N, N], [N, N]).  Faults keep every index inside the table."""
    N, TT = gh * gw, 2 * gh - 1 + 2 * gw - 1
    i = np.arange(N)
    qy, qx = i // gw, i % gw
    ky, kx = i // gw, i % gw
    if fault == 'gh_for_gw':                                              # row / column of the QUERY taken with gh for gw
        qy = i // gh
        qx = i - qy * gh
    dy = qy[:, None] - ky[None, :] if fault != 'sign_y' else ky[None, :] - qy[:, None]
    dx = qx[:, None] - kx[None, :] if fault != 'sign_x' else kx[None, :] - qx[:, None]
    th = dy + gh - 1 + (1 if fault == 'row_off_h' else 0)
    tw = 2 * gh - 1 + dx + gw - 1 + (1 if fault == 'row_off_w' else 0)
    return np.clip(th, 0, TT - 1), np.clip(tw, 0, TT - 1)


def rp_logits(qkv, heads, d, grid, rh, rw, dtype=np.float64, fault=None):
    """q k^T + bias, [n, heads, N, N] in `dtype`"""
    n, N, _ = qkv.shape
    C = heads * d
    x = np.asarray(qkv).astype(dtype)
    q = x[:, :, :C].reshape(n, N, heads, d).transpose(0, 2, 1, 3)
    k = x[:, :, C:2 * C].reshape(n, N, heads, d).transpose(0, 2, 1, 3)
    tab = np.concatenate([rw, rh] if fault == 'swap_tables' else [rh, rw]).astype(dtype)          # [TT, d]
    th, tw = rp_indices(grid[0], grid[1], fault)
    with np.errstate(invalid='ignore'):
        s = q @ k.transpose(0, 1, 3, 2)
        g = (q * np.sqrt(dtype(d))) @ tab.T                               # [n, heads, N, TT]: q_unscaled . R[t]
        s = s + np.take_along_axis(g, np.broadcast_to(th, s.shape), -1) + np.take_along_axis(g, np.broadcast_to(tw, s.shape), -1)
    assert s.dtype == dtype
    return s


def rp_reference(qkv, heads, d, grid, rh, rw, dtype=np.float64, fault=None):
    """softmax(q k^T + bias) v per (sample, head), [n, N, heads d] in `dtype`; dtype=np.float32: fp32 matmuls, add the bias, subtract the
    row maximum, exp, normalise, fp32 matmul"""
    n, N, _ = qkv.shape
    C = heads * d
    s = rp_logits(qkv, heads, d, grid, rh, rw, dtype, fault)
    v = np.asarray(qkv).astype(dtype)[:, :, 2 * C:].reshape(n, N, heads, d).transpose(0, 2, 1, 3)
    with np.errstate(invalid='ignore'):
        p = np.exp(s - s.max(-1, keepdims=True))
        p = p / p.sum(-1, keepdims=True)
        out = (p @ v).transpose(0, 2, 1, 3).reshape(n, N, C)
    assert out.dtype == dtype
    return out


def _rp_case(name, qkv, heads, d, grid, rh, rw, sliced=False, **props):
    n, N, c3 = qkv.shape
    assert qkv.dtype == np.float32 and c3 == 3 * heads * d and N == grid[0] * grid[1]
    assert rh.dtype == np.float32 and rw.dtype == np.float32 and rh.shape == (2 * grid[0] - 1, d) and rw.shape == (2 * grid[1] - 1, d)
    return dict(name=name, qkv=qkv, heads=heads, d=d, grid=grid, rh=rh, rw=rw, sliced=sliced, n=n, N=N, **props)


def _unit_qkv(rng, n, N, heads, d):
    x = rng.normal(0.0, 1.0, (n, N, 3 * heads * d))
    x[:, :, :heads * d] /= math.sqrt(d)
    return x.astype(np.float32)


def _tables(rng, gh, gw, d, sigma):
    """Rh and Rw drawn separately"""
    return rng.normal(0.0, sigma, (2 * gh - 1, d)).astype(np.float32), rng.normal(0.0, sigma, (2 * gw - 1, d)).astype(np.float32)


def rp_sweep_names(grid):
    return ['sweep_%dx%d_d%d_h%d_b%d' % (grid[0], grid[1], d, h, b) for d in RP_DS for h in (1, 3) for b in (1, 2)]


def rp_peak_target(name):
    N = RP_PEAK_GRID[0] * RP_PEAK_GRID[1]
    where = name[len('peak_'):]
    if where == 'mixed':
        return (7 * np.arange(N) + 3) % N                                 # a permutation (gcd(7, 150) = 1): every key leads once
    return np.full(N, RP_PEAK_KEYS[where])


@functools.lru_cache(maxsize=None)
def rp_case(name):
    rng = _rng('attention_relpos', name)
    kind, _, rest = name.partition('_')
    if kind == 'sweep':
        g, d, h, b = rest.split('_')
        gh, gw = (int(t) for t in g.split('x'))
        d, h, b = int(d[1:]), int(h[1:]), int(b[1:])
        rh, rw = _tables(rng, gh, gw, d, 1.0 / math.sqrt(d))              # unit bias next to unit q k^T
        return _rp_case(name, _unit_qkv(rng, b, gh * gw, h, d), h, d, (gh, gw), rh, rw, sliced=b == 2)
    if kind == 'real':
        (gh, gw), n = ((64, 64), 1) if rest == '64x64' else ((14, 14), 25)
        rh, rw = _tables(rng, gh, gw, 80, 1.0 / math.sqrt(80))
        return _rp_case(name, _unit_qkv(rng, n, gh * gw, 1, 80), 1, 80, (gh, gw), rh, rw)
    if kind == 'bias':
        # k = 0: the logits are the bias alone, N(0, 9)
        gh, gw = (int(t) for t in rest.split('x'))
        i = RP_BIAS_GRIDS.index((gh, gw))
        d, h = RP_DS[i], (1, 3)[i % 2]
        qkv = _unit_qkv(rng, 1, gh * gw, h, d)
        qkv[:, :, h * d:2 * h * d] = 0.0
        rh, rw = _tables(rng, gh, gw, d, 3.0 / math.sqrt(d))
        return _rp_case(name, qkv, h, d, (gh, gw), rh, rw)
    if kind == 'peak' or kind == 'max':
        gh, gw = RP_PEAK_GRID
        N = gh * gw
        if kind == 'peak':
            d, h = 64, 1
            k = rng.normal(0.0, 1.0, (N, d))
            k /= np.linalg.norm(k, axis=1, keepdims=True)
            q = 160.0 * k[rp_peak_target(name)] + rng.normal(0.0, 0.5, (N, d))
            x = np.concatenate([q, k, rng.normal(0.0, 1.0, (N, d))], 1)[None]
            sigma = 1.0 / (math.sqrt(d) * 160.0)                          # |q_unscaled| = 8 * 160: a bias of unit size
        else:
            d, h = 32, 3
            tile = np.arange(N) // 32
            level = (tile if rest == 'rising' else tile.max() - tile) * MOTION_STEP
            parts = [[], [], []]
            for _ in range(h):
                u = rng.normal(0.0, 1.0, d)
                u /= np.linalg.norm(u)
                parts[0].append(u + rng.normal(0.0, 0.02, (N, d)))
                parts[1].append(level[:, None] * u + rng.normal(0.0, 0.5, (N, d)))
                parts[2].append(rng.normal(0.0, 1.0, (N, d)))
            x = np.concatenate(parts[0] + parts[1] + parts[2], 1)[None]
            sigma = 0.3 / math.sqrt(d) / math.sqrt(d)                     # |q_unscaled| = sqrt(d): a bias of 0.3
        rh, rw = _tables(rng, gh, gw, d, sigma)
        return _rp_case(name, x.astype(np.float32), h, d, (gh, gw), rh, rw)
    if name == 'offset':
        # k carries a constant component: q[0] k[0] = 1 * 1000 in every logit
        gh, gw, d, h = 8, 12, 32, 3
        qkv = _unit_qkv(rng, 1, gh * gw, h, d)
        for hh in range(h):
            qkv[:, :, hh * d] = 1.0
            qkv[:, :, h * d + hh * d] = 1000.0
        rh, rw = _tables(rng, gh, gw, d, 1.0 / math.sqrt(d) / math.sqrt(d))
        return _rp_case(name, qkv, h, d, (gh, gw), rh, rw)
    if kind == 'isolation':
        d, h = 32, 3
        if rest == 'head':                                                # one sample, head 1 NaN
            gh, gw = 7, 14
            qkv = _unit_qkv(rng, 1, gh * gw, h, d)
            for part in range(3):
                qkv[:, :, part * h * d + d:part * h * d + 2 * d] = np.nan
            fin = np.ones((1, 1, h * d), bool)
            fin[..., d:2 * d] = False
        else:                                                             # batch 2, sample 1 NaN; N = 33: the second key tile holds one key
            gh, gw = (int(t) for t in rest.split('x'))
            qkv = _unit_qkv(rng, 2, gh * gw, h, d)
            qkv[1] = np.nan
            fin = np.ones((2, 1, 1), bool)
            fin[1] = False
        rh, rw = _tables(rng, gh, gw, d, 1.0 / math.sqrt(d))
        return _rp_case(name, qkv, h, d, (gh, gw), rh, rw, finite=fin)
    if kind == 'zero':
        g, d = rest.split('_')
        gh, gw = (int(t) for t in g.split('x'))
        d = int(d[1:])
        return _rp_case(name, _unit_qkv(rng, 2, gh * gw, 2, d), 2, d, (gh, gw), np.zeros((2 * gh - 1, d), np.float32), np.zeros((2 * gw - 1, d), np.float32))
    raise KeyError(name)


def rp_single_sample(case):
    return dict(case, name=case['name'] + '[0]', qkv=np.ascontiguousarray(case['qkv'][:1]), n=1, finite=None, sliced=False)


def attn_vmax(case):
    """largest finite |v| of an attention / cross-attention case"""
    v = case['qkv'][:, :, 2 * case['heads'] * case['d']:] if 'qkv' in case else case['kv'][:, :, case['heads'] * case['d']:]
    return float(np.abs(v[np.isfinite(v)]).max())


@functools.lru_cache(maxsize=None)
def _rp_ref64(name):
    c = rp_case(name)
    return rp_reference(c['qkv'], c['heads'], c['d'], c['grid'], c['rh'], c['rw'])


def rp_ref64(case):
    if case['name'].endswith('[0]'):
        return rp_reference(case['qkv'], case['heads'], case['d'], case['grid'], case['rh'], case['rw'])
    return _rp_ref64(case['name'])


def rp_err(got, ref, case):
    return _err(got, ref, attn_vmax(case), case.get('finite'))


@functools.lru_cache(maxsize=None)
def _rp_e32(name):
    c = rp_case(name)
    return rp_err(rp_reference(c['qkv'], c['heads'], c['d'], c['grid'], c['rh'], c['rw'], np.float32), rp_ref64(c), c)


def rp_e32(case):
    return _rp_e32(case['name'].replace('[0]', ''))


# ---- cross-attention ------------------------------------------------------------------------------------------------------------------------
XA_DS = (2, 4, 8, 16, 32, 64)
XA_NKS = (1, 2, 7, 16, 17, 63, 64, 65, 129, 1000)
XA_NQS = (1, 3, 7, 65)
XA_LANE_MAX = 16                       # launch_xattn_t: Nk <= 16 takes k_xattn_lane, everything longer k_xattn_wave
XA_FAULTS = ('swap_kv', 'v_head_stride', 'l_unscaled')
XA_PEAK_NK = 130
XA_PEAK_KEYS = dict(key0=0, key63=63, key64=64, last=129)
XA_PEAK_NAMES = ['peak_%s' % k for k in XA_PEAK_KEYS]
XA_MOTION_NAMES = ['stride_rising', 'stride_falling', 'lanes_rising', 'lanes_falling', 'lane_kernel_rising', 'lane_kernel_falling']
XA_ISOLATION_NAMES = ['isolation_wave', 'isolation_lane']


def xa_kernel(Nk):
    return 'lane' if Nk <= XA_LANE_MAX else 'wave'


def xa_sweep_names():
    """every d with every Nk, twice: batch 1 plain and batch 2 through slices, Nq and the head count cycling"""
    out = []
    for i, d in enumerate(XA_DS):
        for j, nk in enumerate(XA_NKS):
            out.append('sweep_d%d_k%d_q%d_h%d_b1' % (d, nk, XA_NQS[(i + j) % 4], (1, 3)[(i + j) % 2]))
            out.append('sweep_d%d_k%d_q%d_h%d_b2' % (d, nk, XA_NQS[(i + j + 2) % 4], (3, 1)[(i + j) % 2]))
    return out


def xa_logits(q, kv, heads, d, dtype=np.float64):
    n, Nq, C = q.shape
    Nk = kv.shape[1]
    qq = np.asarray(q).astype(dtype).reshape(n, Nq, heads, d).transpose(0, 2, 1, 3)
    kk = np.asarray(kv).astype(dtype)[:, :, :C].reshape(n, Nk, heads, d).transpose(0, 2, 1, 3)
    with np.errstate(invalid='ignore'):
        return qq @ kk.transpose(0, 1, 3, 2)


def xa_reference(q, kv, heads, d, dtype=np.float64, fault=None):
    """softmax(q k^T) v per (sample, head): q [n, Nq, heads d] pre-scaled, kv [n, Nk, (k: heads d | v: heads d)] -> [n, Nq, heads d]"""
    n, Nq, C = q.shape
    Nk = kv.shape[1]
    kv = np.asarray(kv).astype(dtype)
    if fault == 'swap_kv':
        kv = np.concatenate([kv[:, :, C:], kv[:, :, :C]], 2)
    s = xa_logits(q, kv, heads, d, dtype)
    if fault == 'v_head_stride':                                          # v of head h read D channels behind ITS k, not heads D
        v = np.stack([kv[:, :, (h + 1) * d:(h + 2) * d] for h in range(heads)], 1)
    else:
        v = kv[:, :, C:].reshape(n, Nk, heads, d).transpose(0, 2, 1, 3)
    with np.errstate(invalid='ignore'):
        p = np.exp(s - s.max(-1, keepdims=True))
        if fault == 'l_unscaled':                                         # the 64 lanes' sums added without exp(m_lane - M)
            den = np.zeros(s.shape[:-1] + (1,), dtype)
            for lane in range(min(64, Nk)):
                sl = s[..., lane::64]
                den += np.exp(sl - sl.max(-1, keepdims=True)).sum(-1, keepdims=True)
        else:
            den = p.sum(-1, keepdims=True)
        out = ((p / den) @ v).transpose(0, 2, 1, 3).reshape(n, Nq, C)
    assert out.dtype == dtype
    return out


def _xa_case(name, q, kv, heads, d, sliced=False, **props):
    n, Nq, C = q.shape
    assert q.dtype == np.float32 and kv.dtype == np.float32 and C == heads * d and kv.shape[0] == n and kv.shape[2] == 2 * C
    return dict(name=name, q=q, kv=kv, heads=heads, d=d, n=n, Nq=Nq, Nk=kv.shape[1], sliced=sliced, **props)


def xa_peak_target(name):
    return XA_PEAK_KEYS[name[len('peak_'):]]


@functools.lru_cache(maxsize=None)
def xa_case(name):
    rng = _rng('cross_attention', name)
    kind, _, rest = name.partition('_')
    if kind == 'sweep':
        d, nk, nq, h, b = (int(t[1:]) for t in rest.split('_'))
        q = (rng.normal(0.0, 1.0, (b, nq, h * d)) / math.sqrt(d)).astype(np.float32)
        return _xa_case(name, q, rng.normal(0.0, 1.0, (b, nk, 2 * h * d)).astype(np.float32), h, d, sliced=b == 2)
    if kind == 'peak':
        d, nq, nk = 16, 7, XA_PEAK_NK
        k = rng.normal(0.0, 1.0, (nk, d))
        k /= np.linalg.norm(k, axis=1, keepdims=True)
        q = 160.0 * k[xa_peak_target(name)][None] + rng.normal(0.0, 0.5, (nq, d))
        return _xa_case(name, q[None].astype(np.float32), np.concatenate([k, rng.normal(0.0, 1.0, (nk, d))], 1)[None].astype(np.float32), 1, d)
    if kind in ('stride', 'lanes', 'lane'):
        # the logits follow `level` along the key index: per 64-key stride (a lane's successive keys), per key (across the lanes of the
        # wave kernel), per key of the lane kernel
        rising = rest.endswith('rising')
        d, nq, h = 8, 3, 3
        nk = 16 if kind == 'lane' else 200
        j = np.arange(nk)
        level = (j // 64) * MOTION_STEP if kind == 'stride' else j * (3.0 if kind == 'lane' else 1.0)
        if not rising:
            level = level.max() - level
        qs, ks, vs = [], [], []
        for _ in range(h):
            u = rng.normal(0.0, 1.0, d)
            u /= np.linalg.norm(u)
            qs.append(u + rng.normal(0.0, 0.005, (nq, d)))
            ks.append(level[:, None] * u + rng.normal(0.0, 0.1, (nk, d)))
            vs.append(rng.normal(0.0, 1.0, (nk, d)))
        return _xa_case(name, np.concatenate(qs, 1)[None].astype(np.float32), np.concatenate(ks + vs, 1)[None].astype(np.float32), h, d)
    if kind == 'isolation':
        d, h, nq = 16, 3, 7
        nk = 17 if rest == 'wave' else 7
        q = (rng.normal(0.0, 1.0, (2, nq, h * d)) / math.sqrt(d)).astype(np.float32)
        kv = rng.normal(0.0, 1.0, (2, nk, 2 * h * d)).astype(np.float32)
        q[1], kv[1] = np.nan, np.nan
        fin = np.ones((2, 1, 1), bool)
        fin[1] = False
        return _xa_case(name, q, kv, h, d, finite=fin)
    raise KeyError(name)


def xa_single_sample(case):
    return dict(case, name=case['name'] + '[0]', q=np.ascontiguousarray(case['q'][:1]), kv=np.ascontiguousarray(case['kv'][:1]), n=1, finite=None)


def xa_ref64(case):
    return xa_reference(case['q'], case['kv'], case['heads'], case['d'])


def xa_err(got, ref, case):
    return _err(got, ref, attn_vmax(case), case.get('finite'))


def xa_e32(case):
    return xa_err(xa_reference(case['q'], case['kv'], case['heads'], case['d'], np.float32), xa_ref64(case), case)


# ---- window partition / un-partition (exact) -------------------------------------------------------------------------------------------------
WINDOW_SHAPES = ((1, 1, 1), (7, 7, 3), (9, 9, 4), (14, 14, 14), (5, 13, 4), (13, 5, 4), (3, 5, 7), (15, 1, 4), (23, 23, 14))
WINDOW_FAULTS = ('wy_wx', 't_div_mod', 'crop_padded')
TAIL_COUNTS = (255, 256, 257)


def window_cases():
    """(gh, gw, ws, n, c, with residual, sliced)"""
    out = []
    for i, (gh, gw, ws) in enumerate(WINDOW_SHAPES):
        for n in (1, 2):
            for c in (4, 68):
                for res in (False, True):
                    out.append((gh, gw, ws, n, c, res, (i + n + c // 68 + res) % 2 == 1))
    return out + [(1, cnt, 1, 1, 4, False, False) for cnt in TAIL_COUNTS] + [(1, 257, 1, 1, 4, True, True)]


def window_input(gh, gw, ws, n, c):
    """(map [n, gh, gw, c], windows [n wy wx, ws ws, 1, c], residual [n, gh, gw, c]): independent draws"""
    rng = _rng('window', gh, gw, ws, n, c)
    wy, wx = -(-gh // ws), -(-gw // ws)
    return (rng.normal(0.0, 1.0, (n, gh, gw, c)).astype(np.float32), rng.normal(0.0, 1.0, (n * wy * wx, ws * ws, 1, c)).astype(np.float32),
            rng.normal(0.0, 1.0, (n, gh, gw, c)).astype(np.float32))


def _window_rows(n, gh, gw, ws, fault=None):
    """for every row of the window layout: (sample, y, x) of the map pixel it holds"""
    wy, wx = -(-gh // ws), -(-gw // ws)
    row = np.arange(n * wy * wx * ws * ws)
    t, win = row % (ws * ws), row // (ws * ws)
    if fault == 'wy_wx':
        ix, iy = win % wy, (win // wy) % wx
    else:
        ix, iy = win % wx, (win // wx) % wy
    b = win // (wx * wy)
    ty, tx = (t % ws, t // ws) if fault == 't_div_mod' else (t // ws, t % ws)
    return b, iy * ws + ty, ix * ws + tx


def window_partition_reference(x, ws, fault=None):
    n, gh, gw, c = x.shape
    b, y, xx = _window_rows(n, gh, gw, ws, fault)
    ok = (y < gh) & (xx < gw)
    out = np.zeros((b.size, c), x.dtype)
    out[ok] = x[b[ok], y[ok], xx[ok]]
    return out.reshape(-1, ws * ws, 1, c)


def window_unpartition_reference(xw, ws, shape, res=None, fault=None):
    """shape = (n, gh, gw); float32 in, float32 out: one addition per element"""
    n, gh, gw = shape
    c = xw.shape[-1]
    wy, wx = -(-gh // ws), -(-gw // ws)
    row = np.arange(n * gh * gw)
    if fault == 'crop_padded':                                            # the map rows decoded with the padded width
        x, y, b = row % (wx * ws), (row // (wx * ws)) % gh, row // (gw * gh)
    else:
        x, y, b = row % gw, (row // gw) % gh, row // (gw * gh)
    iy, ix = y // ws, x // ws
    if fault == 'wy_wx':
        src = ((b * wx + iy) * wy + ix)
    else:
        src = ((b * wy + iy) * wx + ix)
    t = (x - ix * ws) * ws + (y - iy * ws) if fault == 't_div_mod' else (y - iy * ws) * ws + (x - ix * ws)
    out = xw.reshape(-1, ws * ws, c)[src % (n * wy * wx), t].reshape(n, gh, gw, c)
    return out if res is None else out + res


# ---- broadcast add (exact against float32 numpy in the order (a + b) + const) ---------------------------------------------------------------
BCAST_POSITIONS = ((1, 1), (1, 5), (7, 7))


def bcast_cases():
    """(n, a.n, b.n or 0, const: None / 'channel' / 'position', (h, w), c, sliced)"""
    out, i = [], 0
    for n in (1, 3):
        for an in sorted({1, n}):
            for bn in sorted({0, 1, n}):
                for const in (None, 'channel', 'position'):
                    for hw in BCAST_POSITIONS:
                        out.append((n, an, bn, const, hw, (4, 68)[i % 2], (i // 2) % 2 == 1))
                        i += 1
    return out


def bcast_input(n, an, bn, const, hw, c):
    rng = _rng('bcast', n, an, bn, str(const), hw[0], hw[1], c)
    a = rng.normal(0.0, 1.0, (an, hw[0], hw[1], c)).astype(np.float32)
    b = rng.normal(0.0, 1.0, (bn, hw[0], hw[1], c)).astype(np.float32) if bn else None
    k = None if const is None else rng.normal(0.0, 1.0, (hw[0], hw[1], c) if const == 'position' else (c,)).astype(np.float32)
    return a, b, k


def bcast_reference(n, a, b, k):
    out = np.broadcast_to(a, (n,) + a.shape[1:]).copy()
    if b is not None:
        out = out + np.broadcast_to(b, out.shape)
    if k is not None:
        out = out + k
    assert out.dtype == np.float32
    return out


# ---- channel dot ----------------------------------------------------------------------------------------------------------------------------
DOT_CS = (4, 8, 32, 68)
DOT_POSITIONS = (1, 255, 256, 257)
DOT_FAULTS = ('h_of_sample_0', 'last_four_dropped')


def dot_input(c, positions, n):
    rng = _rng('dot', c, positions, n)
    return rng.normal(0.0, 1.0, (n, 1, positions, c)).astype(np.float32), rng.normal(0.0, 1.0, (n, 1, 1, c)).astype(np.float32)


def dot_reference(x, h, dtype=np.float64, fault=None):
    """out[b, p] = sum_c x[b, p, c] h[b, c], ascending channels; dtype=np.float32 rounds every product and every partial sum"""
    x, h = x.astype(dtype), h.astype(dtype)
    if fault == 'h_of_sample_0':
        h = np.broadcast_to(h[:1], h.shape)
    c = x.shape[-1] - (4 if fault == 'last_four_dropped' else 0)
    s = np.zeros(x.shape[:-1], dtype)
    for i in range(c):
        s = s + x[..., i] * h[..., i]
    assert s.dtype == dtype
    return s[..., None]


# ---- image -> model input --------------------------------------------------------------------------------------------------------------------
PRE_SHAPES = ((37, 50, 64), (50, 37, 64), (200, 120, 32), (1, 9, 16), (9, 1, 16), (64, 64, 64), (5, 5, 48))
PRE_FAULTS = ('bgr', 'mean_std', 'align_corners', 'scale_from_S')
PRE_MEAN = (123.675, 116.28, 103.53)
PRE_STD = (58.395, 57.12, 57.375)


def preprocess_shape(H, W, S):
    """ResizeLongestSide.get_preprocess_shape"""
    s = S / max(H, W)
    return int(H * s + 0.5), int(W * s + 0.5)


def pre_image(H, W, kind):
    if kind == 'constant':
        return np.full((H, W, 3), 255, np.uint8)
    return _rng('preprocess', H, W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def bilinear_matrix(n_out, n_in, scale, dtype=np.float64, align_corners=False):
    """[n_out, n_in] weights of torch's bilinear resize along one axis; the source coordinate scale (dst + 0.5) - 0.5 and the weights in
    `dtype`.  scale = n_in / n_out unless a caller plants another."""
    dst = np.arange(n_out).astype(dtype)
    scale = dtype(scale)
    if align_corners:
        s = dst * dtype((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    else:
        s = np.maximum(scale * (dst + dtype(0.5)) - dtype(0.5), dtype(0.0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = s - i0.astype(dtype)
    A = np.zeros((n_out, n_in), dtype)
    np.add.at(A, (np.arange(n_out), i0), dtype(1.0) - l1)
    np.add.at(A, (np.arange(n_out), i1), l1)
    assert A.dtype == dtype
    return A


def preprocess_reference(bgr, S, dtype=np.float64, fault=None):
    """uint8 BGR [H, W, 3] -> RGB [3, S, S]: bilinear (align_corners=False, no antialiasing) to nh x nw, (v - mean) / std, zeros beyond.
    dtype=np.float32: the scale float(H) / float(nh), the coordinate, the weights, the four products and the normalisation in float32"""
    H, W = bgr.shape[:2]
    nh, nw = preprocess_shape(H, W, S)
    den_h, den_w = (S, S) if fault == 'scale_from_S' else (nh, nw)
    Ay = bilinear_matrix(nh, H, dtype(H) / dtype(den_h), dtype, fault == 'align_corners')
    Ax = bilinear_matrix(nw, W, dtype(W) / dtype(den_w), dtype, fault == 'align_corners')
    out = np.zeros((3, S, S), dtype)
    for c in range(3):
        ch = c if fault == 'bgr' else 2 - c
        k = (c + 1) % 3 if fault == 'mean_std' else c
        v = Ay @ (bgr[:, :, ch].astype(dtype) @ Ax.T)
        out[c, :nh, :nw] = (v - dtype(PRE_MEAN[k])) / dtype(PRE_STD[k])
    assert out.dtype == dtype
    return out


# ---- low-res logits -> masks -----------------------------------------------------------------------------------------------------------------
POST_SHAPES = ((8, 32, 32, 24, 50, 37), (16, 64, 48, 64, 33, 45), (16, 64, 64, 40, 200, 125), (4, 16, 16, 16, 16, 16), (8, 32, 20, 32, 1, 7),
               (16, 64, 64, 64, 64, 64), (8, 32, 32, 11, 97, 33), (2, 8, 8, 5, 40, 25))
POST_FAULTS = ('xy', 'no_crop', 'scale_from_S')
POST_MARGIN = 1e-4                     # of max|ref| per mask (test_apply_sam_masks_end_to_end)
POST_LEFT_OUT = 0.005
POST_FLIP = 0.01


def post_logits(i):
    L = POST_SHAPES[i][0]
    return np.random.default_rng(500 + i).standard_normal((3, L, L)).astype(np.float32)


def postprocess_reference(low, S, nh, nw, H, W, dtype=np.float64, fault=None):
    """[n, L, L] -> resize to S x S -> crop [nh, nw] -> resize to H x W, align_corners=False: full-size logits [n, H, W]"""
    L = low.shape[-1]
    low = low.astype(dtype)
    if fault == 'xy':
        low = low.transpose(0, 2, 1)
    Uy = Ux = bilinear_matrix(S, L, dtype(L) / dtype(S), dtype)
    if fault == 'no_crop':
        Vy, Vx = bilinear_matrix(H, S, dtype(S) / dtype(H), dtype), bilinear_matrix(W, S, dtype(S) / dtype(W), dtype)
        return Vy @ (Uy @ low @ Ux.T) @ Vx.T
    sy, sx = (dtype(S) / dtype(H), dtype(S) / dtype(W)) if fault == 'scale_from_S' else (dtype(nh) / dtype(H), dtype(nw) / dtype(W))
    Vy, Vx = bilinear_matrix(H, nh, sy, dtype), bilinear_matrix(W, nw, sx, dtype)
    return Vy @ (Uy[:nh] @ low @ Ux[:nw].T) @ Vx.T


def post_sure(ref):
    """the pixels compared: |ref| > 1e-4 max|ref| of their mask"""
    return np.abs(ref) > POST_MARGIN * np.abs(ref).max((1, 2), keepdims=True)


# ---- boxes -> prompt tokens ------------------------------------------------------------------------------------------------------------------
BOX_NS = (1, 3, 300)
BOX_CS = (2, 32, 256)
BOX_STATIC = (0, 5)
BOX_FAULTS = ('corners', 'sin_cos', 'sx_sy', 'no_half')


def box_cases():
    """(n, C, n_static, S, sx, sy)"""
    return [(n, C, ns, (64, 1024)[(i + j + k) % 2], (0.75, 1.6)[(i + k) % 2], (1.25, 0.4)[(i + k) % 2])
            for i, n in enumerate(BOX_NS) for j, C in enumerate(BOX_CS) for k, ns in enumerate(BOX_STATIC)]


def box_input(n, C, n_static, S):
    """boxes [n, 4] float32 (x0, y0, x1, y1): box 0 degenerate, box 1 (n >= 3) with negative coordinates, box 2 beyond the frame;
    consts: [n_static][C] tokens, [2][C] corner embeddings, [2][C / 2] the Gaussian matrix"""
    rng = _rng('boxes', n, C, n_static, S)
    b = np.sort(rng.uniform(0.0, S, (n, 2, 2)), 1).reshape(n, 4)
    b[0] = (0.25 * S, 0.5 * S, 0.25 * S, 0.5 * S)
    if n >= 3:
        b[1] = (-0.3 * S, -7.5, 0.4 * S, 0.2 * S)
        b[2] = (0.6 * S, 0.1 * S, 2.5 * S, 1.75 * S)
    consts = np.concatenate([rng.normal(0.0, 0.5, (n_static + 2) * C), rng.normal(0.0, 1.0, C)]).astype(np.float32)
    return b.astype(np.float32), consts


def box_reference(boxes, sx, sy, S, consts, C, n_static, fault=None):
    """-> float64 [n, C, n_static + 2, 1] (the decoder's NCHW token tensor): rows < n_static the constant tokens, then the two corners:
    sin | cos of 2 pi ((2 (p + 0.5) / S - 1) . gauss) + corner embedding"""
    n, hf = boxes.shape[0], C // 2
    consts = consts.astype(np.float64)
    out = np.zeros((n, n_static + 2, C))
    out[:, :n_static] = consts[:n_static * C].reshape(n_static, C)
    gauss = consts[(n_static + 2) * C:].reshape(2, hf)
    if fault == 'sx_sy':
        sx, sy = sy, sx
    for k in range(2):
        kk = 1 - k if fault == 'corners' else k
        half = 0.0 if fault == 'no_half' else 0.5
        px = 2.0 * ((boxes[:, 2 * kk].astype(np.float64) * sx + half) / S) - 1.0
        py = 2.0 * ((boxes[:, 2 * kk + 1].astype(np.float64) * sy + half) / S) - 1.0
        arg = 2.0 * math.pi * (px[:, None] * gauss[0] + py[:, None] * gauss[1])
        e = np.concatenate([np.cos(arg), np.sin(arg)] if fault == 'sin_cos' else [np.sin(arg), np.cos(arg)], 1)
        out[:, n_static + k] = e + consts[(n_static + k) * C:(n_static + k + 1) * C]
    return out.transpose(0, 2, 1)[..., None]
