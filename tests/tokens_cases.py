"""Case generators and plain references for the transformer ops of csrc/tokens.hip (k_attention, k_layernorm, k_tokens,
k_depth_to_space) and the GELU epilogue of the convolution engine (csm_conv.h).

The references are float64 numpy and use nothing from the library or the oracle; next to each stands the PLAIN FLOAT32 EVALUATION of the
same formulas in the straightforward order, whose error against float64 -- e32(case) -- is the yardstick of the tolerances:

    attention    |got - f64| <= max(4 e32, 8 * 2^-23) * max|v|
    layernorm    |got - f64| <= max(4 e32, 8 * 2^-23) * max|f64|
    gelu         |got - f64| <= 3.2e-7 * max(|x|, 1)

(4 = the margin for another, equally legitimate summation order and the running-max rescales; 8 ulp = the per-output rounding chain beyond
the sums.  DESIGN.md 6.2.)  tests/test_tokens_references.py holds the oracle (oracle/nets_oracle.c) against the references on a machine
without a GPU and asserts that every case has the property it exists for; tests/test_gpu_tokens.py holds the HIP kernels against the same
references and against the oracle.  All generators are seeded.
"""
import functools
import math

import numpy as np

ULP = 2.0 ** -23
FLOOR = 8 * ULP
MARGIN = 4.0


def bound(e32):
    return max(MARGIN * e32, FLOOR)


# ---- attention -----------------------------------------------------------------------------------------------------------------------
def relative_position_index(gh, gw):
    """timm's gen_relative_position_index((gh, gw)) written out: [N, N] entries into a table of T = (2gh-1)(2gw-1) + 3 rows, class
    token first; T-3 class -> patch, T-2 patch -> class, T-1 class -> class"""
    T = (2 * gh - 1) * (2 * gw - 1) + 3
    coords = np.stack(np.meshgrid(np.arange(gh), np.arange(gw), indexing='ij')).reshape(2, -1)          # [2, P]
    rel = (coords[:, :, None] - coords[:, None, :]).transpose(1, 2, 0).copy()                          # [P, P, 2]
    rel[:, :, 0] += gh - 1
    rel[:, :, 1] += gw - 1
    rel[:, :, 0] *= 2 * gw - 1
    idx = np.zeros((gh * gw + 1, gh * gw + 1), np.int64)
    idx[1:, 1:] = rel.sum(-1)
    idx[0, 0:] = T - 3
    idx[0:, 0] = T - 2
    idx[0, 0] = T - 1
    return idx


def attention_logits(qkv, heads, d, table=None, grid=None, index=None, dtype=np.float64):
    """q k^T + bias, [n, heads, N, N] in `dtype` (table [T, heads]; index: an [N, N] index map instead of the grid's own)"""
    n, N, _ = qkv.shape
    C = heads * d
    x = qkv.astype(dtype)
    out = np.empty((n, heads, N, N), dtype)
    bias = None
    if table is not None:
        bias = np.asarray(table).astype(dtype)[relative_position_index(*grid) if index is None else index]   # [N, N, heads]
    with np.errstate(invalid='ignore'):
        for b in range(n):
            for h in range(heads):
                s = x[b, :, h * d:(h + 1) * d] @ x[b, :, C + h * d:C + (h + 1) * d].T
                out[b, h] = s if bias is None else s + bias[:, :, h]
    return out


def attention_reference(qkv, heads, d, table=None, grid=None, index=None, dtype=np.float64):
    """softmax(q k^T + bias) v per (batch, head), [n, N, heads * d] in `dtype`.  dtype=np.float32 is the plain float32 evaluation:
    fp32 matmul, add bias, subtract the row maximum, exp, normalise, fp32 matmul."""
    n, N, _ = qkv.shape
    C = heads * d
    s = attention_logits(qkv, heads, d, table, grid, index, dtype)
    v = qkv.astype(dtype)[:, :, 2 * C:]
    out = np.empty((n, N, C), dtype)
    with np.errstate(invalid='ignore'):
        for b in range(n):
            for h in range(heads):
                p = np.exp(s[b, h] - s[b, h].max(1, keepdims=True))
                p = p / p.sum(1, keepdims=True)
                out[b, :, h * d:(h + 1) * d] = p @ v[b, :, h * d:(h + 1) * d]
    assert out.dtype == dtype
    return out


def attention_vmax(case):
    v = case['qkv'][:, :, 2 * case['heads'] * case['d']:]
    return float(np.abs(v[np.isfinite(v)]).max())


def attention_err(got, ref, case, samples=None):
    """largest |got - ref| over the samples compared, in units of the case's largest |v|"""
    sl = slice(None) if samples is None else samples
    return float(np.abs(np.asarray(got, np.float64)[sl] - ref[sl]).max() / attention_vmax(case))


def attention_e32(case):
    samples = case.get('finite_samples')
    return attention_err(attention_reference(case['qkv'], case['heads'], case['d'], case['table'], case['grid'], dtype=np.float32),
                         attention_ref64(case), case, samples)


@functools.lru_cache(maxsize=None)
def _ref64(name):
    c = attention_case(name)
    return attention_reference(c['qkv'], c['heads'], c['d'], c['table'], c['grid'])


def attention_ref64(case):
    return _ref64(case['name'])


def _rng(*key):
    return np.random.default_rng([abs(hash_int(k)) for k in key])


def hash_int(k):
    if isinstance(k, (int, np.integer)):
        return int(k)
    return int.from_bytes(str(k).encode(), 'little') % (2 ** 31)


def _unit_qkv(rng, n, N, heads, d, scale=1.0):
    """q ~ N(0, scale^2 / d), k, v ~ N(0, 1): logits ~ N(0, scale^2)"""
    x = rng.normal(0.0, 1.0, (n, N, 3 * heads * d))
    x[:, :, :heads * d] *= scale / math.sqrt(d)
    return x.astype(np.float32)


def _table(rng, gh, gw, heads, sigma=1.0):
    return rng.normal(0.0, sigma, ((2 * gh - 1) * (2 * gw - 1) + 3, heads)).astype(np.float32)


def _case(name, qkv, heads, d, grid=None, table=None, in_slice=False, **props):
    n, N, c3 = qkv.shape
    assert c3 == 3 * heads * d and qkv.dtype == np.float32
    if table is not None:
        assert table.dtype == np.float32 and table.shape == ((2 * grid[0] - 1) * (2 * grid[1] - 1) + 3, heads) and N == grid[0] * grid[1] + 1
    return dict(name=name, qkv=qkv, heads=heads, d=d, grid=grid, table=table, in_slice=in_slice, n=n, N=N, **props)


# shape sweep without a table: one key tile (second key half empty); two; an odd tile count (second half one tile short); partial last
# tile; partial last query block
SWEEP_NS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 129)
SWEEP_DS = (32, 64, 128)
SWEEP_HEADS = (1, 3)
SWEEP_BATCH = (1, 2)


def sweep_names(N):
    return ['sweep_N%d_d%d_h%d_b%d' % (N, d, h, b) for d in SWEEP_DS for h in SWEEP_HEADS for b in SWEEP_BATCH]


# grids with a table (N = gh gw + 1)
GRIDS = ((1, 1), (1, 31), (1, 32), (3, 21), (8, 8), (8, 16), (33, 1), (7, 2), (3, 50), (12, 31), (16, 16))


def _grid_shape(i):
    return SWEEP_DS[i % 3], SWEEP_HEADS[i % 2], SWEEP_BATCH[(i // 2) % 2]


GRID_NAMES = ['grid_%dx%d' % g for g in GRIDS]
BIAS_NAMES = ['bias_%dx%d' % g for g in GRIDS]
CLS_BIAS = (5.0, -5.0, 3.0)            # class -> patch, patch -> class, class -> class in the bias-only cases

# peaked softmax: N = 150 = 5 key tiles, the first key half holds tiles 0..2, the second tiles 3 and 4 (keys >= 96), the last tile is
# partial (keys 128..149)
PEAK_N = 150
PEAK_KEYS = dict(key0=0, tile0=17, half1=100, last_tile=130, last=149)
PEAK_NAMES = ['peak_%s' % k for k in PEAK_KEYS] + ['peak_mixed']
PEAK_LEAD = 40.0

MOTION_NAMES = ['max_rising', 'max_falling']
MOTION_STEP = 6.0
OFFSET_NAMES = ['offset_table', 'offset_table_q0', 'offset_qk']
OTHER_NAMES = ['wide_spread']
ISOLATION_NAMES = ['isolation', 'isolation_table']
TABLE_NAMES = GRID_NAMES + BIAS_NAMES + ['offset_table', 'offset_table_q0', 'isolation_table']       # run on both bias paths


def peak_target(name):
    """the key every query of a peaked case leads with, [N]"""
    where = name[len('peak_'):]
    if where == 'mixed':
        return (7 * np.arange(PEAK_N) + 3) % PEAK_N                       # a permutation (gcd(7, 150) = 1): every key leads once
    return np.full(PEAK_N, PEAK_KEYS[where])


@functools.lru_cache(maxsize=None)
def attention_case(name):
    rng = _rng('attention', name)
    kind, _, rest = name.partition('_')
    if kind == 'sweep':
        N, d, h, b = (int(t[1:]) for t in rest.split('_'))
        return _case(name, _unit_qkv(rng, b, N, h, d), h, d, in_slice=b == 2)
    if kind in ('grid', 'bias'):
        gh, gw = (int(t) for t in rest.split('x'))
        i = GRIDS.index((gh, gw))
        d, h, b = _grid_shape(i)
        qkv = _unit_qkv(rng, b, gh * gw + 1, h, d)
        if kind == 'grid':
            return _case(name, qkv, h, d, (gh, gw), _table(rng, gh, gw, h), in_slice=i % 2 == 1)
        # bias only: q = 0, the logits ARE the table entries; N(0, 3) with the three class-token entries far apart
        qkv[:, :, :h * d] = 0.0
        table = _table(rng, gh, gw, h, 3.0)
        table[-3:] = np.asarray(CLS_BIAS, np.float32)[:, None]
        return _case(name, qkv, h, d, (gh, gw), table, in_slice=i % 2 == 0)
    if kind == 'peak':
        N, d, h = PEAK_N, 64, 1
        k = rng.normal(0.0, 1.0, (N, d))
        k /= np.linalg.norm(k, axis=1, keepdims=True)
        q = 160.0 * k[peak_target(name)] + rng.normal(0.0, 0.5, (N, d))
        v = rng.normal(0.0, 1.0, (N, d))
        return _case(name, np.concatenate([q, k, v], 1)[None].astype(np.float32), h, d)
    if kind == 'max':
        # every query's logits grow (fall) by about MOTION_STEP from one key tile to the next
        N, d, h = PEAK_N, 32, 3
        tile = np.arange(N) // 32
        level = (tile if rest == 'rising' else tile.max() - tile) * MOTION_STEP
        parts = [[], [], []]
        for _ in range(h):
            u = rng.normal(0.0, 1.0, d)
            u /= np.linalg.norm(u)
            parts[0].append(u + rng.normal(0.0, 0.02, (N, d)))
            parts[1].append(level[:, None] * u + rng.normal(0.0, 0.5, (N, d)))
            parts[2].append(rng.normal(0.0, 1.0, (N, d)))
        return _case(name, np.concatenate(parts[0] + parts[1] + parts[2], 1)[None].astype(np.float32), h, d)
    if name in ('offset_table', 'offset_table_q0'):
        gh, gw, d, h = 8, 16, 32, 3
        qkv = _unit_qkv(rng, 1, gh * gw + 1, h, d)
        if name.endswith('q0'):
            qkv[:, :, :h * d] = 0.0                                           # the logits are exactly the (rounded) table entries
        table = (_table(rng, gh, gw, h).astype(np.float64) + 1000.0).astype(np.float32)
        return _case(name, qkv, h, d, (gh, gw), table)
    if name == 'offset_qk':
        # integer q and k: every dot product is an exact integer near 3000 in any summation order, the competing keys a few units apart
        N, d, h = 129, 32, 1
        q = rng.integers(-1, 2, (N, d)).astype(np.float64)
        k = rng.integers(-1, 2, (N, d)).astype(np.float64)
        q[:, 0], k[:, 0] = 50.0, 60.0
        return _case(name, np.concatenate([q, k, rng.normal(0.0, 1.0, (N, d))], 1)[None].astype(np.float32), h, d)
    if name == 'wide_spread':
        # integer q and k in -5..5 (exact dot products, |.| <= 1600): logits of standard deviation 80, most probabilities underflow
        N, d, h = 129, 64, 3
        q = rng.integers(-5, 6, (2, N, h * d)).astype(np.float64)
        k = rng.integers(-5, 6, (2, N, h * d)).astype(np.float64)
        return _case(name, np.concatenate([q, k, rng.normal(0.0, 1.0, (2, N, h * d))], 2).astype(np.float32), h, d, in_slice=True)
    if kind == 'isolation':
        # sample 1 entirely NaN; N = 33: the second key tile holds one key, its 31 padded rows lie in sample 1 without the clamp
        d, h = 32, 3
        grid = (1, 32) if rest == 'table' else None
        qkv = _unit_qkv(rng, 2, 33, h, d)
        qkv[1] = np.nan
        return _case(name, qkv, h, d, grid, _table(rng, 1, 32, h) if grid else None, finite_samples=slice(0, 1))
    raise KeyError(name)


def single_sample(case):
    """sample 0 of a batched case as a case of its own"""
    return dict(case, name=case['name'] + '[0]', qkv=np.ascontiguousarray(case['qkv'][:1]), n=1)


def shifted_indices(gh, gw):
    """index maps a wrong window row / column / class-token entry would produce: {label: [N, N] index map}, only those that differ
    from the true map.  Patch -> patch entries moved by +-1 (a column) and +-(2 gw - 1) (a row) inside the table, and the three
    class-token entries exchanged pairwise."""
    idx = relative_position_index(gh, gw)
    T = (2 * gh - 1) * (2 * gw - 1) + 3
    out = {}
    for lab, s in (('col+1', 1), ('col-1', -1), ('row+1', 2 * gw - 1), ('row-1', -(2 * gw - 1))):
        m = idx.copy()
        m[1:, 1:] = np.clip(idx[1:, 1:] + s, 0, T - 4)
        if (m != idx).any():
            out[lab] = m
    for a, b in ((T - 3, T - 2), (T - 3, T - 1), (T - 2, T - 1)):
        m = idx.copy()
        m[idx == a], m[idx == b] = b, a
        out['swap%d,%d' % (a - T, b - T)] = m
    return out


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------
LN_CS = (4, 8, 252, 256, 260, 1024, 1028)
LN_ROWS = (1, 3, 4, 5, 257)
LN_EPS = (1e-6, 1e-5, 1e-12)


def layernorm_reference(x, gamma, beta, eps, dtype=np.float64, one_pass=False):
    """(x - mean) / sqrt(var + eps) * gamma + beta over the last axis, biased variance.  dtype=np.float32: the plain two-pass
    evaluation (mean, centred second moment); one_pass: var = E[x^2] - mean^2 (only to prove the cases)"""
    x, gamma, beta = (np.asarray(a).astype(dtype) for a in (x, gamma, beta))
    c = dtype(x.shape[-1])
    mean = x.sum(-1, keepdims=True) / c
    d = x - mean
    with np.errstate(invalid='ignore'):
        var = (x * x).sum(-1, keepdims=True) / c - mean * mean if one_pass else (d * d).sum(-1, keepdims=True) / c
        out = d / np.sqrt(var + dtype(eps)) * gamma + beta
    assert out.dtype == dtype
    return out


def layernorm_err(got, ref):
    d = np.abs(np.asarray(got, np.float64) - ref)
    return float('inf') if not np.isfinite(d).all() else float(d.max() / np.abs(ref).max())


def _ln_params(rng, c):
    gamma = rng.normal(0.0, 1.0, c).astype(np.float32)
    gamma[::7] = 0.0
    gamma[1::5] = -np.abs(gamma[1::5]) - 0.1
    return gamma, rng.normal(0.0, 1.0, c).astype(np.float32)


@functools.lru_cache(maxsize=None)
def layernorm_case(c, rows, eps):
    """rows of their own scale (0.5 .. 3) and shift (-2 .. 2); gamma with zero and negative entries"""
    rng = _rng('layernorm', c, rows, int(round(-math.log10(eps))))
    x = rng.normal(0.0, 1.0, (rows, c)) * rng.uniform(0.5, 3.0, (rows, 1)) + rng.uniform(-2.0, 2.0, (rows, 1))
    gamma, beta = _ln_params(rng, c)
    return dict(x=x.astype(np.float32), gamma=gamma, beta=beta, eps=eps, c=c, rows=rows, sliced=rows % 2 == 1)


@functools.lru_cache(maxsize=None)
def layernorm_constant_case(c):
    """every entry 3.0: x - mean is exactly 0, the output exactly beta"""
    rng = _rng('layernorm_constant', c)
    gamma, beta = _ln_params(rng, c)
    return dict(x=np.full((5, c), 3.0, np.float32), gamma=gamma, beta=beta, eps=1e-6, c=c, rows=5, sliced=False)


@functools.lru_cache(maxsize=None)
def layernorm_offset_case():
    """mean 1000, sigma 0.9 (mean / sigma >= 1e3), c = 1028, 64 rows (the largest error over 64 x 1028 outputs is a stable yardstick, one
    row's is a matter of luck): E[x^2] - mean^2 loses everything in fp32 (1e6 +- 1 at an ulp of 0.06), the two-pass form does not"""
    rng = _rng('layernorm_offset')
    c = 1028
    gamma, beta = _ln_params(rng, c)
    return dict(x=rng.normal(1000.0, 0.9, (64, c)).astype(np.float32), gamma=gamma, beta=beta, eps=1e-6, c=c, rows=64, sliced=False)


# ---- token plumbing, depth to space ------------------------------------------------------------------------------------------------
TOKEN_GRIDS = ((1, 1), (3, 5), (7, 2))
TOKEN_CS = (4, 68)
TOKEN_NS = (1, 2)
TAIL_COUNTS = (255, 256, 257)           # float4s of a launch: the thread tail of the last 256-thread block
D2S_KS = (1, 2, 4)
D2S_MAPS = ((1, 1), (3, 5))


def token_input(mode, n, c, grid, seed=0):
    """mode 0: patch embedding [n, gh, gw, c] and class token [c]; modes 1 / 2: tokens [n, gh gw + 1, 1, c]"""
    rng = _rng('tokens', mode, n, c, grid[0], grid[1], seed)
    gh, gw = grid
    if mode == 0:
        return rng.normal(0.0, 1.0, (n, gh, gw, c)).astype(np.float32), rng.normal(0.0, 1.0, c).astype(np.float32)
    return rng.normal(0.0, 1.0, (n, gh * gw + 1, 1, c)).astype(np.float32), None


def tokens_reference(mode, x, grid, cls=None):
    n, c = x.shape[0], x.shape[-1]
    gh, gw = grid
    if mode == 0:                                                        # assemble: row 0 = class token, row 1 + i = patch i
        return np.concatenate([np.broadcast_to(cls, (n, 1, c)), x.reshape(n, gh * gw, c)], 1)[:, :, None, :]
    tok = x[:, 1:, 0, :].reshape(n, gh, gw, c)
    if mode == 2:                                                        # readout "ignore": drop the class token
        return tok
    return np.concatenate([tok, np.broadcast_to(x[:, :1, :, :], (n, gh, gw, c))], -1)      # "project": (token | class token)


def depth_to_space_input(n, h, w, k, c, seed=0):
    return _rng('d2s', n, h, w, k, c, seed).normal(0.0, 1.0, (n, h, w, k * k * c)).astype(np.float32)


def depth_to_space_reference(x, k):
    """out[n, y k + ky, x k + kx, c] = in[n, y, x, (ky k + kx) C + c]"""
    n, h, w, ckk = x.shape
    c = ckk // (k * k)
    return x.reshape(n, h, w, k, k, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h * k, w * k, c)


# ---- GELU ------------------------------------------------------------------------------------------------------------------------------
GELU_C = 64
GELU_REL = 3.2e-7                      # 2 x the oracle's measured 1.6e-7 max(|x|, 1) (the 2 x: another libm erf on the test machine)
GELU_SPECIALS = (0.0, 1e-30, 1e-40, 20.0, 87.0, 100.0, 1e4, 3e38)


def gelu_points():
    """12 000 points on [-12, 12] and the special values with both signs, zero-padded to a multiple of GELU_C; float32 [rows, GELU_C]"""
    sp = np.asarray([s * v for v in GELU_SPECIALS for s in (1.0, -1.0)], np.float64)
    x = np.concatenate([np.linspace(-12.0, 12.0, 12000), sp]).astype(np.float32)
    x = np.concatenate([x, np.zeros((-x.size) % GELU_C, np.float32)])
    return x.reshape(-1, GELU_C)


def gelu_reference(x):
    """0.5 x (1 + erf(x / sqrt 2)) in float64 on the float32 points"""
    x = np.asarray(x, np.float64)
    return np.asarray([0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0))) for v in x.reshape(-1)]).reshape(x.shape)


def gelu_bound(x):
    return GELU_REL * np.maximum(np.abs(np.asarray(x, np.float64)), 1.0)
