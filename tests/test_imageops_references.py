"""CPU: the oracle of the image glue (oracle/post_oracle.c, oracle/kenburns.py) against the plain float64 references of
tests/imageops_cases.py on every case the GPU tests use, and for every case list the property it exists for (widths on both sides of
256, tail lengths, ties, identity cases, both paths of the tiled kernels, every stated condition on the inputs).  Runs without a GPU.
The figures printed here (run with -s) are the ones DESIGN.md 6.3 records."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imageops_cases as C  # noqa: E402

from oracle import kenburns as okb, segment as oseg  # noqa: E402

ci, cf, _p = ctypes.c_int, ctypes.c_float, oseg._p
F32, F64 = np.float32, np.float64


# ---- oracle wrappers (shared with the GPU file) --------------------------------------------------------------------------------------
def orc_resize_u8_linear(src, h, w):
    H, W, Cn = src.shape
    out = np.empty((h, w, Cn), np.uint8)
    oseg.lib().orc_resize_u8_linear(_p(src), ci(H), ci(W), ci(Cn), ci(h), ci(w), _p(out))
    return out


def orc_resize_f32_linear(src, h, w):
    H, W, Cn = src.shape
    out = np.empty((h, w, Cn), F32)
    oseg.lib().orc_resize_f32_linear(_p(src), ci(H), ci(W), ci(Cn), ci(h), ci(w), _p(out))
    return out


def orc_lanczos(src, H, W):
    h, w = src.shape
    out = np.empty((H, W), F32)
    oseg.lib().orc_resize_u8_lanczos4_to_f32(_p(src), ci(h), ci(w), ci(H), ci(W), _p(out))
    return out


def orc_area(src, H, W):
    h, w = src.shape
    out = np.empty((H, W), F32)
    oseg.lib().orc_resize_u8_to_f32(_p(src), ci(h), ci(w), ci(H), ci(W), _p(out))
    return out


def orc_leres_input(img, h, w):
    H, W = img.shape[:2]
    out = np.empty((3, h, w), F32)
    oseg.lib().orc_leres_input(_p(img), ci(H), ci(W), ci(h), ci(w), _p(out))
    return out


def orc_crop(frame, ph, pw, cx, cy):
    H, W = frame.shape[:2]
    out = np.empty_like(frame)
    oseg.lib().orc_crop_resize_u8(_p(frame), ci(H), ci(W), ci(ph), ci(pw), cf(cx), cf(cy), _p(out))
    return out


def orc_quantize(d, mn, mx):
    out = np.empty(d.shape, np.uint8)
    oseg.lib().orc_leres_quantize(_p(d), ctypes.c_int64(d.size), cf(float(mn)), cf(float(mx)), _p(out))
    return out


def orc_bokeh_pass(img, depth, ns, dx, dy):
    H, W = depth.shape
    out = np.empty_like(img)
    oseg.lib().orc_bokeh_pass(_p(img), _p(depth), _p(out), ci(H), ci(W), ci(ns), cf(dx), cf(dy))
    return out


# ---- checks shared with the GPU file ---------------------------------------------------------------------------------------------------
def leres_back(out):
    """[3, h, w] normalised RGB -> grey levels (out * std + mean) * 255 in float64, [h, w, 3] in RGB order"""
    return ((out.astype(F64) * C.LERES_STD[:, None, None] + C.LERES_MEAN[:, None, None]) * 255.0).transpose(1, 2, 0)


def check_leres(out, img):
    """the levels are integers to 1e-3, and each lies strictly within 1 of the float64 bilinear of the swapped channel"""
    h, w = out.shape[1:]
    lv = leres_back(out)
    q = np.rint(lv)
    assert np.abs(lv - q).max() <= 1e-3
    d = np.abs(q - C.bilinear_ref(img[..., ::-1], h, w)).max()
    assert d < 1.0, d
    return d


def f32_linear_bound(src, h, w):
    """-> (ref64, absolute bound): max(4 e32, 8 * 2^-23) * max|src| with e32 the plain numpy float32 two-pass blend"""
    ref = C.bilinear_ref(src, h, w)
    scale = float(np.abs(src).max())
    e32 = float(np.abs(C.bilinear_ref(src, h, w, F32).astype(F64) - ref).max()) / scale
    return ref, C.yardstick(e32) * scale, e32


def crop_kinds_of(frame_hw):
    return [(k,) + C.crop_case(frame_hw, k) for k in C.CROP_KINDS]


WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


# =====================================================================================================================================
# 1. row resamplers
# =====================================================================================================================================
def test_resize_pair_lists_have_their_widths():
    ws = [p[1][1] for p in C.RESIZE_PAIRS]
    assert {1, 9, 256, 257, 258, 259, 514} <= set(ws)                     # one block / x >= w guard / blockIdx.x > 0 / three blocks
    assert any(p[0] == p[1] for p in C.RESIZE_PAIRS)                      # the copy / `same` branch
    assert any(p[1][0] == 2 * p[0][0] and p[1][1] == 2 * p[0][1] for p in C.RESIZE_PAIRS)
    assert any(p[0][0] == p[1][0] and p[0][1] != p[1][1] or p[0][1] == p[1][1] and p[0][0] != p[1][0] for p in C.RESIZE_PAIRS)
    # the 3x5 -> 17x259 enlargement has clamped taps at every border
    for n_in, n_out in ((3, 17), (5, 259)):
        i0, i1, f = C.cv_taps(n_in, n_out)
        assert 0.5 * n_in / n_out - 0.5 < 0 and i0[0] == 0 and f[0] == 0 and i0[-1] == i1[-1] == n_in - 1 and f[-1] == 0
    for (h, w), (H, W) in C.AREA_PAIRS:
        assert H >= h and W >= w
    assert {1, 200, 257, 260, 300} <= {p[1][1] for p in C.AREA_PAIRS}
    assert set(C.RESIZE_PAIRS) < set(C.LANCZOS_PAIRS) and ((608, 416), (600, 400)) in C.LANCZOS_PAIRS


@pytest.mark.parametrize("pair", C.RESIZE_PAIRS, ids=C.pair_id)
def test_oracle_resize_u8_linear_within_one_level_of_float64(pair):
    (H, W), (h, w) = pair
    for Cn in C.LINEAR_CHANNELS:
        src = C.image_u8((H, W, Cn), 1, H, W, Cn)
        got = orc_resize_u8_linear(src, h, w)
        d = np.abs(got.astype(F64) - C.bilinear_ref(src, h, w)).max()
        _note('u8_linear', d)
        assert d < 1.0, (pair, Cn, d)
        if (H, W) == (h, w):
            assert np.array_equal(got, src)
    const = np.full((H, W, 3), 77, np.uint8)
    assert (orc_resize_u8_linear(const, h, w) == 77).all()
    print("u8_linear worst |orc - f64| = %.4f" % WORST['u8_linear'])


@pytest.mark.parametrize("pair", C.RESIZE_PAIRS, ids=C.pair_id)
def test_oracle_resize_f32_linear_within_the_float32_yardstick(pair):
    (H, W), (h, w) = pair
    for Cn in C.LINEAR_CHANNELS:
        src = C.image_f32((H, W, Cn), 2, H, W, Cn)
        got = orc_resize_f32_linear(src, h, w)
        ref, bound, e32 = f32_linear_bound(src, h, w)
        d = float(np.abs(got.astype(F64) - ref).max())
        _note('f32_linear_rel', d / np.abs(src).max())
        assert d <= bound, (pair, Cn, d, bound)
    const = np.full((H, W, 1), F32(0.3))                                  # (1 - f) is rounded, so a constant is kept to the bound, not to the bit
    assert np.abs(orc_resize_f32_linear(const, h, w).astype(F64) - float(F32(0.3))).max() <= 8 * C.EPS32 * 0.3
    print("f32_linear worst |orc - f64| / max|src| = %.3g" % WORST['f32_linear_rel'])


def test_float32_coordinate_matters_for_the_f32_reference():
    """300 -> 257: the coordinate kept in double moves the reference by far more than the bound, which is why cv_taps rounds it"""
    src = C.image_f32((7, 300, 1), 2, 7, 300, 1)
    d = np.arange(257, dtype=F64)
    fx = (d + 0.5) * (300 / 257) - 0.5
    sx = np.floor(fx).astype(np.int64)
    f = fx - sx
    keep = (sx >= 0) & (sx < 299)
    tx = (np.clip(sx, 0, 299), np.minimum(np.clip(sx, 0, 299) + 1, 299), np.where(keep, f, 0.0))
    dbl = C.blend2(src, C.cv_taps(7, 5), tx)
    ref, bound, _ = f32_linear_bound(src, 5, 257)
    assert np.abs(dbl - ref).max() > 4 * bound


@pytest.mark.parametrize("pair", C.AREA_PAIRS, ids=C.pair_id)
def test_oracle_area_enlargement_within_one_level_of_float64(pair):
    (h, w), (H, W) = pair
    src = C.image_u8((h, w), 3, h, w)
    got = orc_area(src, H, W)
    assert np.array_equal(got, np.rint(got)) and got.min() >= 0 and got.max() <= 255
    d = np.abs(got.astype(F64) - C.area_ref(src, H, W)).max()
    _note('area', d)
    assert d < 1.0, (pair, d)
    if (h, w) == (H, W):
        assert np.array_equal(got, src.astype(F32))
    assert (orc_area(np.full((h, w), 201, np.uint8), H, W) == 201).all()
    print("area worst |orc - f64| = %.4f" % WORST['area'])


@pytest.mark.parametrize("pair", C.LANCZOS_PAIRS, ids=C.pair_id)
def test_oracle_lanczos_within_one_level_of_float64(pair):
    (h, w), (H, W) = pair
    src = C.image_u8((h, w), 4, h, w)
    got = orc_lanczos(src, H, W)
    d = np.abs(got.astype(F64) - C.lanczos_ref(src, H, W)).max()
    _note('lanczos', d)
    assert d < 1.0, (pair, d)
    assert np.abs(orc_lanczos(np.full((h, w), 130, np.uint8), H, W) - 130).max() <= 1
    print("lanczos worst |orc - f64| = %.4f" % WORST['lanczos'])


@pytest.mark.parametrize("pair", C.RESIZE_PAIRS, ids=C.pair_id)
def test_oracle_leres_input_swaps_and_normalises(pair):
    (H, W), (h, w) = pair
    img = C.leres_image(H, W)
    assert img[..., 0].max() + 8 <= img[..., 1].min() and img[..., 1].max() + 8 <= img[..., 2].min()
    out = orc_leres_input(img, h, w)
    _note('leres', check_leres(out, img))
    with pytest.raises(AssertionError):                                   # the unswapped image fails the same check
        check_leres(out, np.ascontiguousarray(img[..., ::-1]))
    print("leres_input worst |level - f64| = %.4f" % WORST['leres'])


def test_exact_2x_of_a_ramp_is_monotone_in_the_oracle():
    src = C.ramp_u8(31, 257, 3)
    assert (np.diff(src[0, :, 0].astype(int)) >= 0).all() and src[0, 0, 0] == 0 and src[0, -1, 0] == 255
    got = orc_resize_u8_linear(src, 62, 514)
    assert (np.diff(got.astype(int), axis=1) >= 0).all()
    gf = orc_resize_f32_linear(src.astype(F32), 62, 514)
    assert (np.diff(gf, axis=1) >= 0).all()


# =====================================================================================================================================
# 2. crop + resize
# =====================================================================================================================================
def test_crop_case_list_takes_the_window_path_the_fallback_and_both_in_one_launch():
    window = fallback = mixed = 0
    for hw in C.CROP_FRAMES:
        for kind, ph, pw, cx, cy in crop_kinds_of(hw):
            fits = C.crop_fits(hw, ph, pw)
            window += bool(fits.all()); fallback += bool((~fits).all()); mixed += bool(fits.any() and (~fits).any())
            ox, oy = cx - (pw - 1) * 0.5, cy - (ph - 1) * 0.5
            assert float(F32(ox)) == ox and float(F32(oy)) == oy          # the kernel's float32 origin is exact
            if kind == 'same_int':
                assert ox == 0 and oy == 0 and (ph, pw) == hw
            if kind == 'twice' and hw[1] >= 63:
                assert not fits.all()                                     # shrinking: the window does not fit
            if kind == 'tall' and hw[0] >= 4:
                assert pw <= hw[1] and ph == 2 * hw[0] and not fits[:hw[0] // 4].any()   # fits in x; a full tile does not in y
            if kind == 'half':
                assert fits.all()
    assert window >= 6 and fallback >= 3 and mixed >= 3, (window, fallback, mixed)
    assert {hw[1] for hw in C.CROP_FRAMES} >= {1, 63, 64, 65, 257} and {hw[0] for hw in C.CROP_FRAMES} >= {1, 3, 4, 5}


@pytest.mark.parametrize("hw", C.CROP_FRAMES, ids=lambda v: "%dx%d" % v)
def test_oracle_crop_resize_within_the_float64_chain(hw):
    frame = C.image_u8(hw + (3,), 5, *hw)
    for kind, ph, pw, cx, cy in crop_kinds_of(hw):
        got = orc_crop(frame, ph, pw, cx, cy)
        d = np.abs(got.astype(F64) - C.crop_ref(frame, ph, pw, cx, cy)).max()
        _note('crop', d)
        assert d < 1.5, (hw, kind, d)
        if kind == 'same_int':
            assert np.array_equal(got, frame)
        if kind == 'outside':
            assert (got == frame[0, 0]).all()
    print("crop_resize worst |orc - f64| = %.4f" % WORST['crop'])


# =====================================================================================================================================
# 3. reductions
# =====================================================================================================================================
def test_reduction_lengths_cover_the_vector_body_the_tail_and_the_grid_switch():
    L = C.REDUCE_LENGTHS
    assert {n % 4 for n in L} == {0, 1, 2, 3} and {1, 2, 3} <= set(L)                           # no float4 at all
    assert {2 ** 18 - 1, 2 ** 18} <= set(L)                                                       # last of (n + 1023) / 1024 blocks, first of 256 / 512
    assert any(n > 2 ** 18 and n % 4 for n in L) and {1023, 1024, 1025} <= set(L)               # one block / two blocks
    for n in L:
        pos = C.minmax_positions(n)
        assert ('tail' in pos) == (n % 4 != 0) and ('last_vec' in pos) == (n >= 4)
        for where, p in pos.items():
            x = C.minmax_case(n, where)
            assert x[p] == 7.0 == x.max() and (n == 1 or x.min() == -9.0)
    for n in (1, 5, 257):
        v = C.minmax_value_cases(n)
        assert (v['signed_zeros'] == 0).all() and (n == 1 or np.signbit(v['signed_zeros']).any())
        assert np.isinf(v['inf']).any() and not np.isnan(v['inf']).any()


@pytest.mark.parametrize("kind", C.FILL_KINDS)
def test_fill_cases_hold_what_they_are_named_for(kind):
    for n in (1, 2, 5, 257, 1025):
        x = C.fill_case(n, kind)
        ref = C.fill_reference(x)
        if n < 5:
            continue
        z, pos = (x == 0), (x > 0)
        if kind == 'neg_zero':
            assert np.signbit(x[z]).any() and pos.any() and (ref[z] == x[pos].min()).all()
        if kind == 'negatives':
            assert (x < 0).any() and z.any() and np.array_equal(ref[x < 0], x[x < 0])
        if kind == 'subnormal':
            assert x[pos].min() == F32(1e-40) and 0 < float(x[pos].min()) < np.finfo(F32).tiny and (ref[z] == F32(1e-40)).all() and z.any()
        if kind == 'last_positive':
            assert pos.sum() == 1 and pos[-1] and z.any() and (ref[z] == F32(0.625)).all()
        if kind == 'no_zero':
            assert not z.any() and np.array_equal(ref, x)
        if kind == 'nothing_positive':
            assert not pos.any() and z.any() and np.array_equal(ref, x)


def test_mean_std_bound_has_its_binding_term_at_mean_1e4_sigma():
    for ratio in C.MEAN_STD_RATIOS:
        x = C.mean_std_case(1025, ratio)
        m64, s64, bm, bs = C.mean_std_bounds(x)
        assert abs(m64 - 0.5 * ratio) < 0.1 and abs(s64 - 0.5) < 0.05
        second = C.ulp32(m64) ** 2 / (8 * s64)
        assert (second > C.ulp32(s64)) == (ratio == 1e4)
    assert C.mean_std_bounds(np.full(100, F32(3.3)))[1] == 0.0


@pytest.mark.parametrize("name", C.STATS_CASES)
def test_stats_cases_hold_what_they_are_named_for(name):
    d, y0, x0, ch, cw = C.stats_case(name)
    H, W = d.shape
    c = d[y0:y0 + ch, x0:x0 + cw]
    assert c.shape == (ch, cw)
    if name == 'large':
        assert ch * cw > 256 * 256
    if name == 'ties':
        mn_at, mx_at = np.flatnonzero(c.reshape(-1) == c.min()), np.flatnonzero(c.reshape(-1) == c.max())
        assert len(mn_at) == 3 and len(mx_at) == 3
        assert len(set(mn_at // 256)) == 3 and len(set(mx_at // 256)) == 3                       # different blocks' ranges
    if name == 'negative':
        assert c.max() < 0
    if name == 'edge':
        assert y0 + ch == H and x0 + cw == W and np.argmin(c) == ch * cw - 1 and np.argmax(c) // cw == ch - 1
    if name != 'whole':
        assert d.min() < c.min() and d.max() > c.max()                                           # the crop, not the plane


@pytest.mark.parametrize("name", C.ADJUST_CASES)
def test_oracle_depth_adjustment_equals_the_numpy_statement(name):
    disp, mask, span = C.adjust_case(name)
    ref = C.adjust_reference(disp, mask)
    got = okb.depth_adjustment(mask.astype(bool)[None], disp[None, None].copy())[0, 0]
    assert np.array_equal(got, ref)
    if span is None:
        assert mask.any() and np.array_equal(ref, disp) and not (disp * mask).any()
        return
    top, bot = span
    plane = disp * mask
    rows = np.flatnonzero(plane.max(1) > 0)
    assert (rows[0], rows[-1]) == span
    r0 = int(round(top + 0.97 * (bot - top)))
    assert (ref[mask != 0] == plane[r0:].max()).all() and np.array_equal(ref[mask == 0], disp[mask == 0])
    if r0 > top:
        assert plane[r0:].max() < plane.max()                                                    # a wrong r0 (0, say) changes the value
    if name in ('half_even', 'half_odd'):
        v = top + 0.97 * (bot - top)
        assert v - np.floor(v) == 0.5 and r0 % 2 == 0 and r0 == (48 if name == 'half_even' else 50)
        assert plane[r0 - 1:].max() > plane[r0:].max() > plane[r0 + 1:].max()                   # one row off either way shows
    if name == 'one_row':
        assert top == bot == r0
    H, W = disp.shape
    assert {'w1': W == 1, 'w255': W == 255, 'w256': W == 256, 'w257': W == 257, 'h1': H == 1, 'h255': H == 255,
            'h257': H == 257}.get(name, True)


# =====================================================================================================================================
# 4. aten-defined operations
# =====================================================================================================================================
def test_area_mask_cases_have_every_tie_and_the_reference_equals_aten():
    kinds = set()
    for pair in C.AREA_MASK_PAIRS:
        for n in (1, 3):
            m, planted = C.area_mask_case(n, *pair)
            ref, ties = C.area_mask_reference(m, pair[1])
            for kh, kw, oy, ox in planted:
                assert ties[0, oy, ox]
                kinds.add((kh, kw))
            # torch's own float64 adaptive pooling agrees wherever the window is not exactly 30 % set
            t = torch.nn.functional.interpolate(torch.from_numpy((m != 0).astype(F64))[None], size=pair[1], mode='area')[0].numpy() > 0.3
            assert np.array_equal(t[~ties], ref.astype(bool)[~ties])
            if n == 3:
                assert np.array_equal(C.area_mask_reference(m[:1], pair[1])[0][0], ref[0])
                assert not np.array_equal(ref[0], ref[1])
    assert kinds == {(2, 5), (4, 5), (20, 3)}
    # the float32 sequence at a 30 % window: 3 / 2 / 5 and 6 / 4 / 5 round to 0.3f itself, 18 / 20 / 3 to the float below it: none is > 0.3f,
    # which is also what the integer rule's strict > gives -- a kernel that compares >= or rounds the quotient up sets these pixels
    assert not (F32(3) / F32(2) / F32(5) > F32(0.3)) and not (F32(6) / F32(4) / F32(5) > F32(0.3)) and not (F32(18) / F32(20) / F32(3) > F32(0.3))
    wins = {C._area_window(o, 250, 400)[1] - C._area_window(o, 250, 400)[0] for o in range(400)}
    assert wins == {1, 2}


def test_zoe_case_lists_hold_their_branches():
    Cs = C.ZOE_PREP_CASES
    B, H, W, ph, pw, nh, nw = Cs['pad0_same']
    assert ph == pw == 0 and (nh, nw) == (H, W)
    B, H, W, ph, pw, nh, nw = Cs['pad_max']
    assert ph == H - 1 and pw == W - 1
    B, H, W, ph, pw, nh, nw = Cs['padded_same']
    assert (nh, nw) == (H + 2 * ph, W + 2 * pw) and ph > 0
    assert Cs['b2'][0] == 2 and Cs['nh1'][5] == 1 and Cs['tiny'][1:3] == (2, 2)
    assert Cs['pipeline'][3:5] == (int((96 / 2) ** 0.5 * 3), int((130 / 2) ** 0.5 * 3)) == (20, 24)
    img = C.zoe_image(2, 33, 47)
    assert not np.array_equal(img[0], img[1])
    Z = C.ZOE_CROP_CASES
    B, h, w, ph, pw, H, W = Z['copy']
    assert (h, w) == (H + 2 * ph, W + 2 * pw)
    B, h, w, ph, pw, H, W = Z['up3_clamped']
    assert (H + 2 * ph, W + 2 * pw) == (3 * h, 3 * w)
    B, h, w, ph, pw, H, W = Z['reduce']
    assert h > H + 2 * ph and w > W + 2 * pw
    assert Z['b2'][0] == 2 and Z['pad0'][3:5] == (0, 0)
    assert {c[6] % 2 for c in Z.values()} == {0, 1}                                              # unflip on an odd and an even W


# =====================================================================================================================================
# 5. single-rounding chains
# =====================================================================================================================================
@pytest.mark.parametrize("name", C.QUANT_CASES)
def test_oracle_quantize_inside_a_bracket_that_is_a_single_value_almost_everywhere(name):
    d, mn, mx = C.quant_case(name)
    lo, hi = C.quant_bracket(d, mn, mx)
    assert (lo == hi).mean() >= 0.98, (name, (lo == hi).mean())
    got = orc_quantize(d, mn, mx).astype(np.int64)
    assert ((lo <= got) & (got <= hi)).all()
    if name == 'constant':
        assert (got == 255).all()
    if name == 'two_valued':
        assert set(got.tolist()) == {0, 255} and (got[d == mx] == 0).all()
    if name == 'tiny_range':
        assert 0 < float(mx) - float(mn) < 2.2e-16 and (got == 255).all()
    assert (got[d == mx] == (255 if name in ('constant', 'tiny_range') else 0)).all()            # the element equal to mx
    print("%s: bracket single-valued on %.2f %%" % (name, 100 * (lo == hi).mean()))


def test_chain_inputs_hold_their_special_values():
    x = C.denormalise_input(257)
    std, mean = F32(0.25) - F32(0.0000001), F32(0.5)
    assert std + F32(0.0000001) == F32(0.25)
    v = C.denormalise_ms_ref(x, mean, std, 0)
    assert v[0] == 0.0 and v[1] == 1.0 and v[2] > 0 > v[3] and v[4] > 1
    z = C.denormalise_ms_ref(x, F32(-0.0), std, 0)
    assert z[5] == 0 and np.signbit(z[5])                                                         # -0.0 * 0.25 + -0.0 = -0.0
    d = C.zoe_disp_input(257)
    with np.errstate(all='ignore'):
        raw = (F32(1.0) / (d + F32(0.00001))) * F32(12.5)
    assert np.isposinf(raw[0]) and np.isnan(raw[1]) and raw[2] == 0 and np.isfinite(raw[3]) and np.isfinite(raw[4])
    ref = C.zoe_disp_ref(d, 12.5)
    assert ref[0] == 0 and ref[1] == 0 and np.isfinite(ref).all() and ref[3] == F32(F32(1.0) / F32(0.00001)) * F32(12.5)
    for hw in (1, 255, 257):
        assert C.bytes_image(hw).shape == (hw, 3)
    assert all(len(set(C.bytes_image(257)[:, c].tolist())) == 256 for c in range(3))


def test_colorize_cases_reach_every_branch_and_the_oracle_agrees():
    """the inputs of the csm_colorize_gray_r test: vmax itself (256 -> 255), both clamps, the truncation of (-1, 0) to 0, vmin == vmax;
    oracle/kenburns.py colorize_gray_r (which takes its own percentiles) equals the reference evaluated at those percentiles"""
    vmin, vmax = C.COLORIZE_CASES['range']
    for n in C.CHAIN_LENGTHS:
        v = C.colorize_input(n, vmin, vmax)
        ref = C.colorize_ref(v, vmin, vmax)
        assert v[0] == F32(vmax) and ref[0] == 0 and ref.shape == (n,) and ref.dtype == np.uint8
        if n > 1:
            x = (v - F32(vmin)) / (F32(vmax) - F32(vmin)) * F32(256)
            assert v[1] == F32(vmin) and ref[1] == 255
            assert x[2] < 256 and ref[2] == 0 and x[3] > 256 and ref[3] == 0               # next to vmax: index 255 from both sides
            assert -1 < x[4] < 0 and ref[4] == 255                                         # truncated toward zero, not floored to under
            assert x[5] < -1 and ref[5] == 255 and x[6] > 256 and ref[6] == 0              # under and over
            assert (v < F32(vmin)).sum() > 20 and (v > F32(vmax)).sum() > 20 and len(set(ref.tolist())) > 100
            k = np.clip((x.astype(F32)).astype(np.int64), 0, 255)
            assert ((ref.astype(int) != 255 - k) & (x > 0) & (x < 255)).sum() >= 5         # table entries that are not 255 - k are hit
        flat = C.COLORIZE_CASES['flat']
        assert flat[0] == flat[1] and (C.colorize_ref(C.colorize_input(n, *flat), *flat) == 255).all()
        if n > 1:
            lo, hi = okb._percentile(v, 2), okb._percentile(v, 85)
            assert lo < hi and np.array_equal(okb.colorize_gray_r(v), C.colorize_ref(v, lo, hi))


def test_pow_yardsticks():
    """numpy float32 against float64 on the inputs of the GPU tests: e32 of the highlight power and the exact-match share of the uint8
    finish (the GPU test requires HIP to reach that share minus 2 percentage points)"""
    img = C.image_u8((9, 257, 3), 56)
    for lf in C.POW_LIGHTNESS:
        ref, e32 = C.highlight_refs(img, lf)
        assert e32 < 1e-6
        a = np.power(img.astype(F32) / F32(255), F32(lf)).reshape(-1)
        b = a[::-1].copy()
        u64, u32 = C.finish_refs(a, b, lf)
        share, worst = C.pow_share(u32, u64)
        assert worst <= 1 and share > 0.9
        print("lightness %g: e32 highlight %.3g, numpy float32 finish exact share %.4f" % (lf, e32, share))


# =====================================================================================================================================
# 6. bokeh pass
# =====================================================================================================================================
def test_bokeh_cases_select_every_template_and_both_out_of_window_branches():
    R = {c[0]: C.bokeh_template(c[1], c[2], c[3]) for c in C.BOKEH_CASES}
    assert (R['r9'], R['r16'], R['r20']) == (9, 16, 20)
    assert all(R[n] == 9 for n in ('5x7', '8x32', '9x33', '50x70', 'far_interior', 'far_border', 'zero_region'))
    assert not C.bokeh_interior_blocks(5, 7, 9).any() and not C.bokeh_interior_blocks(9, 33, 9).any()
    assert not C.bokeh_interior_blocks(70, 70, 9).any()
    assert not C.bokeh_interior_blocks(50, 70, 9).any()                                            # 70 < 32 + 32 + 2 * 9: border tiles only
    assert C.bokeh_interior_blocks(50, 70, 2)[1:5, 1].all()                                        # ... interior only for a small R
    for R_, rows in ((9, slice(2, 10)), (16, slice(2, 10)), (20, slice(3, 9))):                    # 96x128: tiles x = 32 / 64
        inter = C.bokeh_interior_blocks(96, 128, R_)
        assert inter[rows, 1:3].all() and inter.sum() == 2 * (rows.stop - rows.start)
    for name in ('far_interior', 'far_border'):
        img, depth, ns = C.bokeh_case(name)
        for dx, dy in C.BOKEH_DIRS:
            assert C.bokeh_leaves_window(depth, ns, dx, dy, 9) > 0
    # ... inside an interior block too
    img, depth, ns = C.bokeh_case('far_interior')
    assert depth.shape == (96, 128)
    sub = np.zeros_like(depth); sub[16:80, 32:96] = 1                                              # the interior blocks at R = 9
    ox, oy = C.bokeh_offsets(depth, ns, *C.BOKEH_DIRS[0])
    assert ((np.abs(oy) > 9) & (sub[..., None] > 0)).any()
    for name in ('50x70', 'r9', 'r16', 'r20'):
        img, depth, ns = C.bokeh_case(name)
        assert C.bokeh_leaves_window(depth, ns, *C.BOKEH_DIRS[1], R[name]) == 0
    img, depth, ns = C.bokeh_case('zero_region')
    ref = C.bokeh_pass_ref(img, depth, ns, *C.BOKEH_DIRS[0])
    assert (depth[20:50, 30:90] == 0).all() and np.array_equal(ref[35, 60], img[35, 60].astype(F64))
    assert (depth[:5] > 0).all()


def bokeh_bound(img, depth, ns, dx, dy):
    """-> (ref64, absolute bound) with e32 the numpy float32 evaluation of the same sample loop"""
    ref = C.bokeh_pass_ref(img, depth, ns, dx, dy)
    e32 = float(np.abs(C.bokeh_pass_ref(img, depth, ns, dx, dy, F32).astype(F64) - ref).max() / np.abs(ref).max())
    return ref, C.yardstick(e32) * float(np.abs(ref).max()), e32


@pytest.mark.parametrize("name", [c[0] for c in C.BOKEH_CASES])
def test_oracle_bokeh_pass_within_the_float32_yardstick(name):
    img, depth, ns = C.bokeh_case(name)
    for dx, dy in C.bokeh_dirs(name):
        got = orc_bokeh_pass(img, depth, ns, dx, dy)
        ref, bound, e32 = bokeh_bound(img, depth, ns, dx, dy)
        d = float(np.abs(got.astype(F64) - ref).max())
        assert d <= bound, (name, d, bound, e32)
