"""Case generators, plain references and one-op programs for the layer-program ops of csrc/netops.hip other than the convolutions
on the matrix pipe and their relatives (those, layer by layer against float64, are tests/conv_cases.py): depthwise conv, max pool,
bilinear / nearest resize, the element-wise ops and their activations, the ZoeDepth attractor and log-binomial ops, global average pool
and the NCHW <-> NHWC transposes (csmconv::launch_netop).

The references are numpy float64, or CPU torch float64 for what aten defines (F.conv2d with groups = c, F.max_pool2d, F.interpolate);
nothing comes from the library's kernels or from the oracle.  Where an op rounds more than once the PLAIN FLOAT32 EVALUATION of the same
formula in the straightforward order stands next to the reference; its error against float64 -- e32(case) -- is the yardstick:

    |got - f64| <= max(4 e32, 8 * 2^-23) * scale            

scale = max|ref|, except: bilinear max|x| (a convex blend of the inputs), activations max(|x|, 1) per element.  Ops that round once or
not at all (max pool, nearest, add, scale, copy, relu, prelu, the transposes, a one-hot depthwise kernel) are held to equality.

program(case) lowers a case to a one-op Program (ext NCHW -> NHWC [into a channel slice of a wider buffer] -> op -> NCHW), variant(case)
restates the dispatch conditions of launch_netop and names the kernel the case's shapes select.  tests/test_netops_references.py holds
the oracle to the references on a machine without a GPU and proves what each case exists for; tests/test_gpu_netops.py runs the HIP
kernels on the same cases.  All generators are seeded.
"""
import functools
import inspect

import numpy as np
import torch
import torch.nn.functional as F

from cartoonsegmentation_amd import program as P

ULP = 2.0 ** -23
FLOOR = 8 * ULP
MARGIN = 4.0
f32, f64 = np.float32, np.float64

KERNELS = ('k_dwconv_lds', 'k_dwconv', 'k_maxpool', 'k_bilinear_rows', 'k_bilinear<4>', 'k_bilinear<1>', 'k_nearest',
           'k_eltwise4/0', 'k_eltwise4/1', 'k_eltwise/0', 'k_eltwise/1', 'k_eltwise/2', 'k_eltwise/3', 'k_attractor', 'k_logbinom',
           'k_gavgpool32', 'k_gavgpool', 'k_nchw_to_nhwc', 'k_nchw_to_nhwc_tile', 'k_nhwc_to_nchw', 'k_nhwc_to_nchw_tile')


def bound(e32):
    return max(MARGIN * e32, FLOOR)


def _hash_int(k):
    if isinstance(k, (int, np.integer)):
        return int(k)
    return int.from_bytes(str(k).encode(), 'little') % (2 ** 31)


def _rng(*key):
    return np.random.default_rng([abs(_hash_int(k)) for k in key])


def rel_err(got, ref, scale):
    """largest |got - ref| / scale (scale: a number or an array of ref's shape); inf if anything is not finite"""
    d = np.abs(np.asarray(got, f64) - ref) / scale
    return float(d.max()) if np.isfinite(d).all() else float('inf')


# ---- activations in float64 and in plain float32 -------------------------------------------------------------------------------------
ACTS = ('relu', 'silu', 'prelu', 'hsigmoid', 'sigmoid', 'softplus')
EXACT_ACTS = (None, 'relu', 'prelu')


def act64(y, act, slope=None):
    y = np.asarray(y, f64)
    with np.errstate(over='ignore', invalid='ignore'):
        if act is None:
            return y
        if act == 'relu':
            return np.where(y > 0, y, y * 0.0)                             # (keeps a NaN)
        if act == 'prelu':
            return np.where(y >= 0, y, y * np.asarray(slope, f64))
        if act == 'silu':
            return y / (1.0 + np.exp(-y))
        if act == 'hsigmoid':
            return np.clip(y + 3.0, 0.0, 6.0) / 6.0
        if act == 'sigmoid':
            return 1.0 / (1.0 + np.exp(-y))
        if act == 'softplus':
            return np.logaddexp(0.0, y)
    raise KeyError(act)


def act32(y, act, slope=None):
    """the plain float32 evaluation: torch's definitions, softplus with its threshold of 20"""
    y = np.asarray(y, f32)
    one = f32(1.0)
    with np.errstate(over='ignore', invalid='ignore'):
        if act is None:
            r = y
        elif act == 'relu':
            r = np.where(y > 0, y, y * f32(0.0))
        elif act == 'prelu':
            r = np.where(y >= 0, y, y * np.asarray(slope, f32))
        elif act == 'silu':
            r = y / (one + np.exp(-y))
        elif act == 'hsigmoid':
            r = np.minimum(np.maximum(y + f32(3.0), f32(0.0)), f32(6.0)) / f32(6.0)
        elif act == 'sigmoid':
            r = one / (one + np.exp(-y))
        elif act == 'softplus':
            r = np.where(y > f32(20.0), y, np.log(one + np.exp(np.minimum(y, f32(20.0)))))
        else:
            raise KeyError(act)
    assert r.dtype == f32
    return r


def softplus_without_switch(x):
    """the library's formula with the `v > 20` switch taken out (its expf clamps the argument to 88): only to prove the case"""
    return np.log1p(np.exp(np.minimum(np.asarray(x, f64), 88.0)))


# ---- depthwise conv --------------------------------------------------------------------------------------------------------------------
DW_FRAMES = ((1, 1), (5, 3), (7, 15), (8, 16), (9, 17), (17, 33))      # one pixel, smaller than the kernel, one short of / exactly / one past a tile, several tiles
DW_KS = (3, 5, 7, 9, 11)
DW_ACTS = (None, 'silu', 'prelu')


def dw_lds_bytes(k):
    return (k * k * 32 + (k + 7) * (k + 15) * 32) * 4


def dw_out_size(i, k, stride, pad, dil):
    return (i + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _dw_case(name, k, hw, c, pad, stride=1, dil=1, n=1, sliced=False, bias=True, act=None, nan_sample=False, onehot=None):
    rng = _rng('dwconv', name)
    h, w = hw
    x = rng.normal(0.0, 1.0, (n, h, w, c)).astype(f32)
    if nan_sample:
        x[1] = np.nan
    if onehot is None:
        wt = rng.normal(0.0, 1.0, (c, 1, k, k)).astype(f32)                # different in every channel: a swapped block shows
    else:
        wt = np.zeros((c, k * k), f32)
        wt[np.arange(c), (np.arange(c) + onehot) % (k * k)] = 1.0
        wt = wt.reshape(c, 1, k, k)
        bias, act = False, None
    return dict(kind='dwconv', name=name, x=x, w=wt, b=rng.normal(0.0, 1.0, c).astype(f32) if bias else None, k=k, pad=pad, stride=stride,
                dil=dil, act=act, slope=rng.uniform(0.05, 0.5, c).astype(f32) if act == 'prelu' else None, c=c, n=n,
                in_slice=(4, 8) if sliced else None, out_slice=(8, 4) if sliced else None, onehot=onehot,
                finite_samples=slice(0, 1) if nan_sample else None, exact=onehot is not None)


@functools.lru_cache(maxsize=None)
def dwconv_cases():
    out, i = [], 0
    for k in DW_KS:                                                        # base: pad k // 2, every frame
        for hw in DW_FRAMES:
            out.append(_dw_case('dw_k%d_%dx%d' % (k, hw[0], hw[1]), k, hw, (32, 64)[i % 2], k // 2, n=1 + (i // 2) % 2, sliced=(i // 3) % 2 == 1,
                                bias=i % 5 < 3, act=DW_ACTS[i % 3]))
            i += 1
    for k in (3, 5):                                                       # "valid" and "full"
        for hw in DW_FRAMES:
            for pad, lab in ((0, 'valid'), (k - 1, 'full')):
                if dw_out_size(hw[0], k, 1, pad, 1) < 1 or dw_out_size(hw[1], k, 1, pad, 1) < 1:
                    continue
                out.append(_dw_case('dw_k%d_%s_%dx%d' % (k, lab, hw[0], hw[1]), k, hw, (64, 32)[i % 2], pad, n=2, sliced=i % 2 == 0, bias=i % 3 == 0,
                                    act=DW_ACTS[i % 3]))
                i += 1
    for k in (3, 5):                                                       # the generic kernel by channel count, stride, dilation
        for hw in ((1, 1), (5, 3), (9, 17), (17, 33)):
            for lab, c, stride, dil in (('c36', 36, 1, 1), ('c4', 4, 1, 1), ('s2', 32, 2, 1), ('d2', 64, 1, 2)):
                pad = dil * (k // 2)
                out.append(_dw_case('dw_k%d_%s_%dx%d' % (k, lab, hw[0], hw[1]), k, hw, c, pad, stride, dil, n=2, sliced=i % 2 == 0, bias=i % 3 != 0,
                                    act=DW_ACTS[i % 3]))
                i += 1
    out.append(_dw_case('dw_isolation_lds', 5, (9, 17), 32, 2, n=2, nan_sample=True))
    out.append(_dw_case('dw_isolation_generic', 5, (9, 17), 36, 2, n=2, nan_sample=True, sliced=True))
    return out


@functools.lru_cache(maxsize=None)
def dwconv_onehot_cases():
    """channel ch carries the one-hot kernel of tap (ch + off) % k^2; the offsets 0, c, 2c, ... give every tap its turn"""
    out, i = [], 0
    for k in DW_KS:
        for hw in DW_FRAMES:
            c = (64, 32)[i % 2]
            for off in range(0, k * k, c):
                out.append(_dw_case('dw1hot_k%d_%dx%d_o%d' % (k, hw[0], hw[1], off), k, hw, c, k // 2, n=1 + i % 2, sliced=(i // 2) % 2 == 1, onehot=off))
            i += 1
    for k in (3, 5):
        for pad in (0, k - 1):
            out.append(_dw_case('dw1hot_k%d_p%d' % (k, pad), k, (9, 17), 32, pad, n=2, onehot=0))
    for lab, c, stride, dil in (('c36', 36, 1, 1), ('s2', 32, 2, 1), ('d2', 32, 1, 2)):
        out.append(_dw_case('dw1hot_k5_%s' % lab, 5, (9, 17), c, 2 * dil, stride, dil, n=2, onehot=0))
    return out


def _act_ref(y, k, dtype):
    return (act64 if dtype is f64 else act32)(y, k['act'], k.get('slope'))


def dwconv_reference(k, weights=None):
    """F.conv2d(groups = c) in float64, then the activation"""
    wt = k['w'] if weights is None else weights
    x = torch.from_numpy(k['x'].astype(f64)).permute(0, 3, 1, 2)
    y = F.conv2d(x, torch.from_numpy(wt.astype(f64)), None if k['b'] is None else torch.from_numpy(k['b'].astype(f64)), k['stride'], k['pad'], k['dil'],
                 groups=k['c']).permute(0, 2, 3, 1).numpy()
    return _act_ref(y, k, f64)


def _dw_taps(k):
    """the zero-padded input and, per tap, the strided window the outputs read: (ho, wo, [(ky, kx, window)])"""
    x, pad, s, d, kk = k['x'], k['pad'], k['stride'], k['dil'], k['k']
    n, h, w, c = x.shape
    ho, wo = dw_out_size(h, kk, s, pad, d), dw_out_size(w, kk, s, pad, d)
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, c), f32)
    xp[:, pad:pad + h, pad:pad + w] = x
    return ho, wo, [(ky, kx, xp[:, ky * d:ky * d + (ho - 1) * s + 1:s, kx * d:kx * d + (wo - 1) * s + 1:s]) for ky in range(kk) for kx in range(kk)]


def dwconv_plain32(k):
    """bias, then the taps row by row, each product and each sum rounded to float32"""
    ho, wo, taps = _dw_taps(k)
    acc = np.zeros((k['n'], ho, wo, k['c']), f32) + (k['b'] if k['b'] is not None else f32(0.0))
    with np.errstate(invalid='ignore'):
        for ky, kx, win in taps:
            acc = acc + win * k['w'][:, 0, ky, kx]
    assert acc.dtype == f32
    return _act_ref(acc, k, f32)


def dwconv_onehot_expected(k):
    """the shifted, zero-padded input: channel ch is the window of its own tap"""
    ho, wo, taps = _dw_taps(k)
    out = np.empty((k['n'], ho, wo, k['c']), f32)
    tap = (np.arange(k['c']) + k['onehot']) % (k['k'] ** 2)
    for ch in range(k['c']):
        out[..., ch] = taps[tap[ch]][2][..., ch]
    return out


def dw_shift_centre_tap(wt):
    """planted fault: the centre tap's weight and its right (for a 1-wide kernel: lower) neighbour's exchanged"""
    w2 = wt.copy()
    k = wt.shape[-1]
    w2[:, 0, k // 2, k // 2], w2[:, 0, k // 2, k // 2 + 1] = wt[:, 0, k // 2, k // 2 + 1], wt[:, 0, k // 2, k // 2]
    return w2


def dw_swap_blocks(wt):
    """planted fault: the weights of channel blocks 0 and 1 exchanged"""
    return np.concatenate([wt[32:64], wt[:32], wt[64:]])


# ---- max pool --------------------------------------------------------------------------------------------------------------------------
POOL_CFGS = ((2, 2, 0, True), (2, 2, 0, False), (3, 2, 1, False), (3, 2, 0, True), (5, 1, 2, False), (2, 2, 1, True))
POOL_SIZES = ((1, 1), (3, 3), (4, 5), (21, 18))


def pool_out_size(i, k, stride, pad, ceil):
    """torch's pooling_output_shape: with ceil_mode the last window must start inside the input or its left padding"""
    num = i + 2 * pad - k
    o = (-(-num // stride) if ceil else num // stride) + 1
    if ceil and (o - 1) * stride >= i + pad:
        o -= 1
    return o


@functools.lru_cache(maxsize=None)
def maxpool_cases():
    out, i = [], 0
    for cfg in POOL_CFGS:
        for hw in POOL_SIZES:
            k, s, pad, ceil = cfg
            if pool_out_size(hw[0], k, s, pad, ceil) < 1 or pool_out_size(hw[1], k, s, pad, ceil) < 1:
                continue                                               # no output: torch refuses 1 x 1 under (2, 2, 0, floor) and (3, 2, 0, ceil)
            for c in (4, 36):
                name = 'pool_k%ds%dp%d%s_%dx%d_c%d' % (k, s, pad, 'ceil' if ceil else 'floor', hw[0], hw[1], c)
                x = -np.abs(_rng('maxpool', name).normal(0.0, 1.0, (2, hw[0], hw[1], c))).astype(f32) - f32(0.01)      # strictly negative
                out.append(dict(kind='maxpool', name=name, x=x, k=k, stride=s, pad=pad, ceil=ceil, in_slice=(4, 8) if i % 2 else None,
                                out_slice=(8, 4) if i % 2 else None, exact=True))
                i += 1
    return out


def maxpool_reference(k, zero_pad=False):
    x = torch.from_numpy(k['x'].astype(f64)).permute(0, 3, 1, 2)
    if zero_pad:                                                           # planted fault: the padding counts as 0
        h, w = x.shape[2:]
        ho, wo = (pool_out_size(i, k['k'], k['stride'], k['pad'], k['ceil']) for i in (h, w))
        hi = [max((o - 1) * k['stride'] + k['k'] - k['pad'] - i, 0) for o, i in ((ho, h), (wo, w))]
        xp = F.pad(x, (k['pad'], hi[1], k['pad'], hi[0]), value=0.0)
        y = F.max_pool2d(xp, k['k'], k['stride'], 0)[:, :, :ho, :wo]
    else:
        y = F.max_pool2d(x, k['k'], k['stride'], k['pad'], ceil_mode=k['ceil'])
    return y.permute(0, 2, 3, 1).numpy()


# ---- bilinear --------------------------------------------------------------------------------------------------------------------------
# (in size, out size, channels): every pair runs with align_corners both ways; c / 4 in {1, 3, 5, 7, 9, 25} for the row kernel's division
BILINEAR_PAIRS = (((23, 23), (45, 45), 4), ((45, 45), (90, 90), 12), ((12, 12), (23, 23), 100), ((45, 45), (23, 23), 20), ((7, 7), (1, 1), 28),
                  ((1, 1), (5, 7), 36), ((5, 7), (1, 1), 4), ((9, 12), (9, 23), 12), ((12, 9), (23, 9), 20), ((6, 7), (6, 7), 28),
                  ((4, 128), (7, 256), 4), ((4, 100), (7, 257), 4), ((23, 12), (45, 23), 36), ((3, 40), (5, 64), 100))


def _bil_case(name, n, in_hw, out_hw, c, align, in_slice=None, out_slice=None, act=None):
    rng = _rng('bilinear', name)
    return dict(kind='bilinear', name=name, x=rng.normal(0.0, 1.0, (n, in_hw[0], in_hw[1], c)).astype(f32), size=tuple(out_hw), align=align, act=act,
                slope=rng.uniform(0.05, 0.5, c).astype(f32) if act == 'prelu' else None, in_slice=in_slice, out_slice=out_slice, exact=False,
                align_matters=any(i != o and i > 1 for i, o in zip(in_hw, out_hw)))


@functools.lru_cache(maxsize=None)
def bilinear_cases():
    out = []
    for i, (ihw, ohw, c) in enumerate(BILINEAR_PAIRS):
        for align in (False, True):
            j = 2 * i + align
            out.append(_bil_case('bil_%dx%d_%dx%d_c%d_a%d' % (ihw + ohw + (c, align)), 1 + j % 2, ihw, ohw, c, align, (4, 8) if j % 3 == 1 else None,
                                 (8, 4) if j % 3 else None, 'prelu' if j % 4 == 2 else None))
    for align in (False, True):
        # the two grid limits of the row kernel: more than 65535 output rows, more than 65535 samples
        out.append(_bil_case('bil_tall_a%d' % align, 1, (3, 1), (65536, 1), 4, align, act='prelu' if align else None))
        out.append(_bil_case('bil_batch_a%d' % align, 65536, (1, 1), (2, 2), 4, align))
        # one and two channels at a base that is not 16-byte aligned
        out.append(_bil_case('bil_c1_a%d' % align, 2, (5, 7), (9, 13), 1, align, (1, 2), (3, 0), 'prelu' if align else None))
        out.append(_bil_case('bil_c2_a%d' % align, 2, (9, 13), (5, 7), 2, align, (1, 1), None, None if align else 'prelu'))
    return out


def bilinear_reference(k, dtype=f64, align=None):
    """F.interpolate on the CPU in `dtype`, then the fused activation"""
    align = k['align'] if align is None else align
    x = torch.from_numpy(k['x'].astype(dtype)).permute(0, 3, 1, 2)
    y = F.interpolate(x, size=k['size'], mode='bilinear', align_corners=align).permute(0, 2, 3, 1).numpy()
    assert y.dtype == dtype
    return _act_ref(y, k, dtype)


# ---- nearest ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nearest_cases():
    out, i = [], 0
    for f in (1, 2, 4):
        for hw in ((1, 1), (3, 5)):
            for c in (4, 36):
                name = 'nearest_f%d_%dx%d_c%d' % (f, hw[0], hw[1], c)
                out.append(dict(kind='nearest', name=name, x=_rng('nearest', name).normal(0.0, 1.0, (2, hw[0], hw[1], c)).astype(f32), factor=f,
                                in_slice=(4, 8) if i % 2 else None, out_slice=(8, 4) if i % 2 else None, exact=True))
                i += 1
    return out


def nearest_reference(k):
    return np.repeat(np.repeat(k['x'].astype(f64), k['factor'], 1), k['factor'], 2)


# ---- element-wise ----------------------------------------------------------------------------------------------------------------------
ELT_FRAMES = ((3, 5), (7, 37))                                             # 15 and 259 pixels: one block, and the thread tail of a later one
WIDE4 = dict(c=36, slice=(4, 8))                                           # 16-byte aligned slice: the float4 kernel
NARROW = dict(c=2, slice=(1, 1))                                           # 2 channels at an odd offset: the generic kernel


@functools.lru_cache(maxsize=None)
def eltwise_cases():
    out = []

    def case(op, name, shape, **kw):
        rng = _rng('eltwise', name)
        d = dict(kind='eltwise', op=op, name=name, x=rng.normal(0.0, 1.0, shape).astype(f32), act=None, slope=None, in_slice=None, in1_slice=None,
                 out_slice=None, exact=True)
        d.update(kw)
        out.append(d)
        return d, rng

    for h, w in ELT_FRAMES:
        for lab, geo in (('wide', WIDE4), ('narrow', NARROW)):
            c, sl = geo['c'], geo['slice']
            for sliced in (False, True):
                if lab == 'narrow' and not sliced:
                    continue                                           # a 2-channel buffer of its own is not what the lowering produces
                s = sl if sliced else None
                tag = '%s%s_%dx%d' % (lab, '_sl' if sliced else '', h, w)
                for act in (None, 'relu'):
                    d, rng = case('add', 'add_%s_%s' % (tag, act), (2, h, w, c), act=act, in_slice=s, in1_slice=s, out_slice=s)
                    d['y'] = rng.normal(0.0, 1.0, (2, h, w, c)).astype(f32)
                d, rng = case('scale', 'scale_%s' % tag, (2, h, w, c), in_slice=s, in1_slice=s, out_slice=s)
                d['y'] = rng.normal(0.0, 1.0, (2, 1, 1, c)).astype(f32)                   # a scale vector per sample
                case('copy', 'copy_%s' % tag, (2, h, w, c), in_slice=s, out_slice=sl)     # copy and act always write into a slice
                d, rng = case('act', 'actrelu_%s' % tag, (2, h, w, c), act='relu', in_slice=s, out_slice=sl)
                d, rng = case('act', 'actprelu_%s' % tag, (2, h, w, c), act='prelu', in_slice=s, out_slice=sl)
                d['slope'] = rng.uniform(0.05, 0.5, c).astype(f32)
        for dh, dw in ((1, 0), (0, 1), (1, 1)):                            # the first operand one row / one column / both larger
            for c, s in ((4, None), (36, (4, 8))):
                d, rng = case('add', 'addcrop_%d%d_%dx%d_c%d' % (dh, dw, h, w, c), (2, h + dh, w + dw, c), in_slice=s, in1_slice=s, crop=(dh, dw))
                d['y'] = rng.normal(0.0, 1.0, (2, h, w, c)).astype(f32)
    return out


def eltwise_reference(k, fault=None):
    """float64; add and scale round once, so the float32 rounding of this is what the kernel must give.  fault: 'pitch' reads the cropped
    operand with the output's pitch, 'sample0' applies sample 0's scale vector to every sample (both only to prove the cases)"""
    x = k['x'].astype(f64)
    if k['op'] == 'add':
        n, h, w, c = k['y'].shape
        a = x[:, :h, :w] if fault != 'pitch' else x.reshape(-1, c)[:n * h * w].reshape(n, h, w, c)
        r = a + k['y'].astype(f64)
    elif k['op'] == 'scale':
        s = k['y'].astype(f64)
        r = x * (s if fault != 'sample0' else s[:1])
    else:
        r = x
    return act64(r, k['act'], k['slope'])


# ---- activations -----------------------------------------------------------------------------------------------------------------------
def activation_points():
    """+-0, +-denormal, +-2^-20 .. +-16 in powers of two, +-3 and 20 with their float32 neighbours, +-87, 88, 89, 100, 1e4, and 4096 seeded
    N(0, 3) values; a multiple of 4 long"""
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    dn = lambda v: np.nextafter(f32(v), f32(-np.inf))
    pos = [0.0, 1e-40, 2.0 ** -140] + [2.0 ** e for e in range(-20, 5)] + [dn(3.0), 3.0, up(3.0), 87.0, 88.0, 89.0, 100.0, 1e4]
    sp = np.asarray([s * f32(v) for v in pos for s in (1.0, -1.0)] + [dn(20.0), 20.0, up(20.0)], f32)
    x = np.concatenate([sp, _rng('activation_points').normal(0.0, 3.0, 4096).astype(f32)])
    return np.concatenate([x, np.zeros((-x.size) % 4, f32)])


@functools.lru_cache(maxsize=None)
def activation_cases():
    out = []
    x = activation_points()
    for act in ACTS:
        for lab, c, sl in (('c4', 4, None), ('c2', 2, (1, 1))):
            name = 'act_%s_%s' % (act, lab)
            out.append(dict(kind='eltwise', op='act', name=name, x=x.reshape(1, -1, 1, c).copy(), act=act,
                            slope=_rng('activations', name).uniform(0.05, 0.5, c).astype(f32) if act == 'prelu' else None,
                            in_slice=sl, out_slice=sl, exact=act in EXACT_ACTS, per_element=True))
    return out


# ---- ZoeDepth attractor ----------------------------------------------------------------------------------------------------------------
ATTRACTOR_PIXELS = (1, 257)


@functools.lru_cache(maxsize=None)
def attractor_cases():
    out, i = [], 0
    for na in (1, 8, 16):
        for bins in (1, 16, 64):
            for typ in ('exp', 'inv'):
                for agg in ('mean', 'sum'):
                    for alpha in (300.0, 1000.0):
                        name = 'attr_a%d_b%d_%s_%s_%d' % (na, bins, typ, agg, alpha)
                        rng = _rng('attractor', name)
                        h, w = ATTRACTOR_PIXELS
                        b = np.sort(rng.uniform(0.1, 10.0, (1, h, w, bins)), -1).astype(f32)
                        # every attractor sits on a centre, near one (alpha dx^2 of order 1) or far from all (alpha dx^2 > 100)
                        at = np.take_along_axis(b, rng.integers(0, bins, (1, h, w, na)), -1).astype(f64)
                        mode = rng.integers(0, 3, (1, h, w, na))
                        A = np.where(mode == 0, at, np.where(mode == 1, at + rng.normal(0.0, 0.05, at.shape), at + rng.choice([-1.0, 1.0], at.shape) * rng.uniform(0.7, 3.0, at.shape)))
                        out.append(dict(kind='attractor', name=name, x=A.astype(f32), y=b, alpha=alpha, typ=typ, agg=agg,
                                        in_slice=(4, 4) if i % 2 or na % 4 else None, in1_slice=(8, 4) if i % 2 or bins % 4 else None, out_slice=None,
                                        exact=False))
                        i += 1
    return out


def attractor_reference(k, dtype=f64):
    """out_k = b_k + agg_i dist(A_i - b_k): dist = exp(-alpha dx^2) dx or dx / (1 + alpha dx^2); the sum over i in order"""
    A, b = k['x'].astype(dtype), k['y'].astype(dtype)
    alpha = dtype(k['alpha'])
    delta = np.zeros(b.shape, dtype)
    for i in range(A.shape[-1]):
        dx = A[..., i:i + 1] - b
        delta = delta + (np.exp(-alpha * (dx * dx)) * dx if k['typ'] == 'exp' else dx / (dtype(1.0) + alpha * (dx * dx)))
    if k['agg'] == 'mean':
        delta = delta / dtype(A.shape[-1])
    out = b + delta
    assert out.dtype == dtype
    return out


# ---- log-binomial ----------------------------------------------------------------------------------------------------------------------
LOGBINOM_KS = (1, 2, 64, 256)
P_EPS = 1e-4


def shipped_temperatures():
    """(min_temp, max_temp) of the project's ZoeDepth head"""
    from cartoonsegmentation_amd.nets import zoedepth_head
    sig = inspect.signature(zoedepth_head.build_zoe_head).parameters
    return float(sig['min_temp'].default), float(sig['max_temp'].default)


def log_binom_table(K):
    """log C(K - 1, k) by Stirling's leading terms with eps = 1e-7, in float32 as ZoeDepth registers it (an INPUT of the op)"""
    eps = f32(1e-7)
    n = f32(K - 1) + eps
    k = np.arange(K).astype(f32) + eps
    return (n * np.log(n) - k * np.log(k) - (n - k) * np.log(n - k + eps)).astype(f32)


@functools.lru_cache(maxsize=None)
def logbinom_cases():
    out = []
    for family, temps in (('shipped', shipped_temperatures()), ('warm', (1.0, shipped_temperatures()[1]))):
        for K in LOGBINOM_KS:
            name = 'logbinom_%s_K%d' % (family, K)
            rng = _rng('logbinom', name)
            npx = 257
            pt = rng.uniform(0.05, 3.0, (1, 1, npx, 4))                    # softplus outputs: positive
            q = np.arange(npx) % 8                                         # p to both clamps, the temperature to both ends, in every pairing
            pt[0, 0, q % 4 == 1, :2] = (0.0, 30.0)                         # p = eps / (30 + 2 eps) < 1e-4
            pt[0, 0, q % 4 == 2, :2] = (30.0, 0.0)                         # 1 - p < 1e-4
            pt[0, 0, q // 4 == 1, 2] = 0.0                                 # t -> min_temp
            pt[0, 0, np.arange(npx) % 16 >= 12, 2:] = (40.0, 0.0)          # t -> max_temp
            pt[0, 0, np.arange(npx) % 16 == 11, 2:] = (0.0, 40.0)          # t = min_temp to the last bit but eps
            cen = np.cumsum(rng.uniform(0.02, 0.3, (1, 1, npx, K)), -1)
            out.append(dict(kind='logbinom', name=name, family=family, x=pt.astype(f32), y=cen.astype(f32), K=K, p_eps=P_EPS, min_temp=temps[0],
                            max_temp=temps[1], table=log_binom_table(K), in_slice=(0, 4), in1_slice=(4, 4) if K != 64 else None, out_slice=None,
                            exact=False))
    return out


def logbinom_reference(k, dtype=f64, clamps=True):
    """ConditionalLogBinomial's tail and the expectation over the bins: p, t from the four softplus outputs, y_k = (log C(K-1, k) +
    k log p + (K-1-k) log(1-p)) / t with p and 1 - p clamped to [1e-4, 1], out = sum_k softmax(y)_k centre_k.  All parameters are float32
    values (the op's parameter block); clamps=False only to prove the cases"""
    q, cen = k['x'].astype(dtype), k['y'].astype(dtype)
    pe, tmin, tmax, eps = (dtype(f32(v)) for v in (k['p_eps'], k['min_temp'], k['max_temp'], 1e-4))
    lb = k['table'].astype(dtype)
    K = k['K']
    p0, p1, t0, t1 = (q[..., i:i + 1] + pe for i in range(4))
    p = p0 / (p0 + p1)
    t = (tmax - tmin) * (t0 / (t0 + t1)) + tmin
    one = dtype(1.0)
    x, omx = (np.clip(p, eps, one), np.clip(one - p, eps, one)) if clamps else (p, one - p)
    kk = np.arange(K).astype(dtype)
    y = (lb + kk * np.log(x) + (dtype(K - 1) - kk) * np.log(omx)) / t
    e = np.exp(y - y.max(-1, keepdims=True))
    num, den = np.zeros(p.shape, dtype), np.zeros(p.shape, dtype)
    for j in range(K):                                                     # in order
        den = den + e[..., j:j + 1]
        num = num + e[..., j:j + 1] * cen[..., j:j + 1]
    out = num / den
    assert out.dtype == dtype
    return out


# ---- global average pool ---------------------------------------------------------------------------------------------------------------
GAP_FRAMES = ((1, 1), (1, 7), (15, 17), (16, 16), (1, 257), (25, 40))      # 1, 7, 255, 256, 257, 1000 pixels


@functools.lru_cache(maxsize=None)
def gavgpool_cases():
    out = []
    for h, w in GAP_FRAMES:
        for c, sl in ((32, None), (64, None), (36, None), (4, None), (32, (4, 4))):
            for offset in (0.0, 1000.0) if (h, w) in ((1, 257), (25, 40)) else (0.0,):
                name = 'gap_%dx%d_c%d%s%s' % (h, w, c, '_sl' if sl else '', '_off' if offset else '')
                x = (_rng('gavgpool', name).normal(0.0, 1.0, (2, h, w, c)) + offset).astype(f32)
                out.append(dict(kind='gavgpool', name=name, x=x, in_slice=sl, out_slice=None, exact=False))
    return out


def gavgpool_reference(k, dtype=f64):
    """mean over the pixels; float32: one running sum per channel over the pixels in order, then the division"""
    x = k['x'].astype(dtype)
    n, h, w, c = x.shape
    if dtype is f64:
        return x.mean((1, 2), keepdims=True)
    s = np.zeros((n, c), f32)
    for px in x.reshape(n, h * w, c).transpose(1, 0, 2):
        s = s + px
    return (s / f32(h * w)).reshape(n, 1, 1, c)


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
LAYOUT_CS = (1, 3, 4, 7, 8, 9, 64, 69, 240, 241)
LAYOUT_FRAMES = ((1, 1), (7, 9), (8, 8), (5, 13), (10, 13))                # 1, 63, 64, 65, 130 pixels


@functools.lru_cache(maxsize=None)
def layout_cases():
    """an NCHW tensor of distinct values to NHWC and back.  'pad': into a buffer of the lowering's padded width (channels rounded up to 4,
    the padding written as zeros) and back out whole; 'slice': into csrc channels of a wider buffer and back out of that slice"""
    out = []
    for c in LAYOUT_CS:
        for h, w in LAYOUT_FRAMES:
            for mode in ('pad', 'slice'):
                x = np.arange(2 * c * h * w, dtype=f32).reshape(2, c, h, w) + f32(1.0)         # NCHW here
                out.append(dict(kind='layout', name='layout_c%d_%dx%d_%s' % (c, h, w, mode), x=x, mode=mode, c=c, exact=True,
                                in_slice=None, out_slice=(5, 3) if mode == 'slice' else None))
    return out


def layout_reference(k, transposed=False):
    """the NCHW result: the input itself, zero channels appended in 'pad' mode.  transposed: the element (c, pixel) taken from (pixel, c)
    (planted fault)"""
    x = k['x'].astype(f64)
    n, c, h, w = x.shape
    if transposed:
        x = x.reshape(n, h * w, c).transpose(0, 2, 1).reshape(n, c, h, w)
    if k['mode'] == 'pad':
        x = np.concatenate([x, np.zeros((n, (-c) % 4, h, w))], 1)
    return x


# ---- all cases -------------------------------------------------------------------------------------------------------------------------
FAMILIES = dict(dwconv=dwconv_cases, dwconv_onehot=dwconv_onehot_cases, maxpool=maxpool_cases, bilinear=bilinear_cases, nearest=nearest_cases,
                eltwise=eltwise_cases, activations=activation_cases, attractor=attractor_cases, logbinom=logbinom_cases, gavgpool=gavgpool_cases,
                layout=layout_cases)
_REF, _E32 = {}, {}


def all_cases():
    return [k for f in FAMILIES.values() for k in f()]


def reference(k):
    """float64, in the layout the program returns (NHWC; NCHW for the layout cases), computed once per case"""
    if k['name'] not in _REF:
        kind = k['kind']
        if kind == 'dwconv':
            r = dwconv_onehot_expected(k).astype(f64) if k['onehot'] is not None else dwconv_reference(k)
        elif kind == 'eltwise':
            r = eltwise_reference(k)
        else:
            r = dict(maxpool=maxpool_reference, bilinear=bilinear_reference, nearest=nearest_reference, attractor=attractor_reference,
                     logbinom=logbinom_reference, gavgpool=gavgpool_reference, layout=layout_reference)[kind](k)
        r.setflags(write=False)
        _REF[k['name']] = r
    return _REF[k['name']]


def plain32(k):
    kind = k['kind']
    if kind == 'dwconv':
        return dwconv_plain32(k)
    if kind == 'eltwise':
        return act32(k['x'], k['act'], k['slope'])
    return dict(bilinear=bilinear_reference, attractor=attractor_reference, logbinom=logbinom_reference, gavgpool=gavgpool_reference)[kind](k, f32)


def compared(k, a):
    """the part of a result that is compared: the finite samples of an isolation case"""
    return a if k.get('finite_samples') is None else a[k['finite_samples']]


def scale(k):
    if k.get('per_element'):
        return np.maximum(np.abs(k['x'].astype(f64)), 1.0)
    if k['kind'] == 'bilinear':
        return float(np.abs(k['x']).max())
    return float(np.abs(compared(k, reference(k))).max())


def error(k, got):
    """the distance of a result from the reference in units of the case's scale"""
    return rel_err(compared(k, got), compared(k, reference(k)), scale(k))


def e32(k):
    if k['name'] not in _E32:
        _E32[k['name']] = error(k, plain32(k))
    return _E32[k['name']]


# ---- one-op programs -------------------------------------------------------------------------------------------------------------------
def nchw(x):
    """[n, h, w, c] -> contiguous [n, c, h, w]"""
    return np.ascontiguousarray(np.asarray(x, f32).transpose(0, 3, 1, 2))


def nhwc(y):
    return y.transpose(0, 2, 3, 1)


class Built:
    """a lowered case: the program, its ext inputs (NCHW), the ext output's shape, the views of the op under test and -- when the op
    writes a channel slice -- (the whole buffer, the slice)"""
    def __init__(self, prog, ext_in, out_shape, views, guard, aux=()):
        self.prog, self.ext_in, self.out_shape, self.views, self.guard, self.aux = prog, ext_in, out_shape, views, guard, aux


def _source(p, x, sl):
    """the NHWC copy of an ext tensor: a buffer of its own, or channels lead .. lead + c of one `lead + tail` channels wider"""
    n, h, w, c = x.shape
    ext = p.ext_nchw(n, c, h, w)
    if sl is None:
        assert c % 4 == 0
        return p.to_nhwc(ext)
    v = p.buffer(n, h, w, c + sl[0] + sl[1]).slice(sl[0], sl[0] + c)
    p.to_nhwc_into(ext, v)
    return v


def _target(p, shape, sl):
    if sl is None:
        return None, None
    n, h, w, c = shape
    wide = p.buffer(n, h, w, c + sl[0] + sl[1])
    return wide.slice(sl[0], sl[0] + c), wide


def _aux(p, a):
    return (-1, -1) if a is None else p._w(a, a)


def program(k):
    kind = k['kind']
    p = P.Program(k['name'])
    if kind == 'layout':
        n, c, h, w = k['x'].shape
        x_ext = p.ext_nchw(n, c, h, w)
        if k['mode'] == 'pad':
            v, wide = p.to_nhwc(x_ext), None
        else:
            v, wide = _target(p, (n, h, w, c), k['out_slice'])
            p.to_nhwc_into(x_ext, v)
        y_ext = p.ext_nchw(n, v.c, h, w)
        p.to_nchw(v, y_ext)
        return Built(p, [k['x']], (n, v.c, h, w), (x_ext, None, v), (wide, v) if wide is not None else None)
    x = _source(p, k['x'], k['in_slice'])
    ext_in = [nchw(k['x'])]
    y = None
    if 'y' in k:
        y = _source(p, k['y'], k.get('in1_slice'))
        ext_in.append(nchw(k['y']))
    ref_shape = reference(k).shape
    out, wide = _target(p, ref_shape, k['out_slice'])
    if kind == 'dwconv':
        if k['act'] != 'prelu':
            r = p.dwconv(x, k['w'], k['b'], k['stride'], k['pad'], k['dil'], k['act'], out=out)
        else:                                                              # the op as Program.dwconv emits it, with a slope vector
            if out is None:
                out = p.buffer(*ref_shape)
            c, kk = k['c'], k['k']
            w_h, w_n = p._w(k['w'].reshape(c, kk * kk).T, k['w'])
            b_h, b_n = _aux(p, k['b'])
            a_h, a_n = _aux(p, k['slope'])
            r = p._emit(P.OP_DWCONV, x, None, out, kh=kk, kw=kk, stride=k['stride'], pad=k['pad'], dil=k['dil'], act=P.ACT['prelu'], w_off=w_h,
                        b_off=b_h, aux_off=a_h, nat=dict(w_off=w_n, b_off=b_n, aux_off=a_n))
    elif kind == 'maxpool':
        r = p.maxpool(x, k['k'], k['stride'], k['pad'], k['ceil'], out=out)
    elif kind == 'bilinear':
        r = p.bilinear(x, k['size'], k['align'], out=out, act=k['act'], slope=k['slope'])
    elif kind == 'nearest':
        r = p.nearest(x, k['factor'], out=out)
    elif kind == 'eltwise':
        op = k['op']
        if op == 'add':
            r = p.add(x, y, k['act'], out=out)
        elif op == 'scale':
            r = p.scale(x, y, out=out)
        elif op == 'copy':
            r = p.copy(x, out)
        else:
            r = p.act(x, k['act'], out=out, slope=k['slope'])
    elif kind == 'attractor':
        r = p.attractor(x, y, k['alpha'], k['typ'], k['agg'])
    elif kind == 'logbinom':
        r = p.logbinom(x, y, k['p_eps'], k['min_temp'], k['max_temp'], k['table'])
    elif kind == 'gavgpool':
        r = p.gavgpool(x)
    else:
        raise KeyError(kind)
    assert r.shape == ref_shape, (k['name'], r.shape, ref_shape)
    for v, sl in ((x, k['in_slice']), (y, k.get('in1_slice')), (r, k['out_slice'])):
        assert v is None or (v.buf.c != v.c) == (sl is not None) or kind == 'logbinom'          # ld != c exactly where the case says so
    y_ext = p.ext_nchw(r.n, r.c, r.h, r.w)
    p.to_nchw(r, y_ext)
    return Built(p, ext_in, (r.n, r.c, r.h, r.w), (x, y, r), (wide, r) if wide is not None else None)


# ---- which kernel a case selects (a restatement of csmconv::launch_netop) -----------------------------------------------------------
def _ld(v):
    return v.buf.c


def _aligned16(v):
    """the workspace base is at least 256-byte aligned: a view is 16-byte aligned when its float offset is a multiple of 4"""
    return (v.buf.offset + v.coff) % 4 == 0


def _eltwise4_ok(out, *ins):
    return all(_aligned16(v) and _ld(v) % 4 == 0 for v in ins + (out,)) and out.c % 4 == 0


def variant(k):
    """the kernel(s) the case runs for the op under test; the layout cases name both directions"""
    b = program(k)
    b.prog.plan()
    x, y, out = b.views
    kind = k['kind']
    if kind == 'layout':
        return ('k_nchw_to_nhwc_tile' if 8 <= out.c <= 240 else 'k_nchw_to_nhwc', 'k_nhwc_to_nchw_tile' if 8 <= out.c <= 240 else 'k_nhwc_to_nchw')
    if kind == 'dwconv':
        lds = k['stride'] == 1 and k['dil'] == 1 and out.c % 32 == 0 and dw_lds_bytes(k['k']) <= 65536
        return ('k_dwconv_lds' if lds else 'k_dwconv',)
    if kind == 'bilinear':
        vec = out.c % 4 == 0 and _ld(x) % 4 == 0 and _ld(out) % 4 == 0 and _aligned16(x) and _aligned16(out)
        return ('k_bilinear_rows' if vec and out.h <= 65535 and out.n <= 65535 else 'k_bilinear<4>' if vec else 'k_bilinear<1>',)
    if kind == 'eltwise':
        if k['op'] == 'scale':
            return ('k_eltwise/2',)
        if k['op'] == 'add':
            if (x.h, x.w) != (out.h, out.w):
                return ('k_eltwise/3',)
            return ('k_eltwise4/1' if _eltwise4_ok(out, x, y) else 'k_eltwise/1',)
        return ('k_eltwise4/0' if _eltwise4_ok(out, x) else 'k_eltwise/0',)       # (a slope vector starts a multiple of 4 floats into the weights)
    if kind == 'gavgpool':
        return ('k_gavgpool32' if x.c % 32 == 0 and _ld(x) % 4 == 0 and _aligned16(x) else 'k_gavgpool',)
    return (dict(maxpool='k_maxpool', nearest='k_nearest', attractor='k_attractor', logbinom='k_logbinom')[kind],)
