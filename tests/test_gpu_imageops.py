"""GPU: the image-glue kernels one by one (csrc/imageops.hip, csrc/zoedepth.hip), each entry point called through ctypes, against the
plain float64 references of tests/imageops_cases.py and, where one exists, bit for bit against the oracle.  Every output buffer is
pre-filled with a sentinel and over-allocated by a few elements; the slack must still hold the sentinel afterwards.
tests/test_imageops_references.py proves the same cases (and the property each exists for) on the CPU; DESIGN.md 6.3 has the rules."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imageops_cases as C  # noqa: E402
import test_imageops_references as R  # noqa: E402

CSM_ERR_ARG = 1
SLACK = 8
SENT = {torch.uint8: 0xA5, torch.float32: float('nan'), torch.float64: float('nan'), torch.int32: -7, torch.int64: -7}
F32, F64 = np.float32, np.float64


def _L():
    from cartoonsegmentation_amd import _lib
    return _lib.load()


def _a():
    from cartoonsegmentation_amd._lib import check, f32, i32, i64, ptr, stream_ptr
    return check, f32, i32, i64, ptr, stream_ptr


_ALIVE = []


@pytest.fixture(autouse=True)
def _inputs_live_until_the_test_ends():
    """a tensor made inline as `ptr(_dev(a))` would go back to the caching allocator at once and the next upload could take its block
    before the kernel has read it: every upload is held until the test is over"""
    yield
    torch.cuda.synchronize()
    del _ALIVE[:]


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _ALIVE.append(t)
    return t


def _buf(n, dtype=torch.float32):
    """output buffer of n elements + SLACK, filled with the type's sentinel"""
    return torch.full((int(n) + SLACK,), SENT[dtype], dtype=dtype, device='cuda')


def _untouched(t):
    a = t.cpu().numpy()
    return bool(np.isnan(a).all()) if t.dtype.is_floating_point else bool((a == SENT[t.dtype]).all())


def _take(buf, shape):
    """the first prod(shape) elements; the slack behind them must still hold the sentinel"""
    n = int(np.prod(shape))
    assert _untouched(buf[n:]), "written past the output"
    return buf[:n].cpu().numpy().reshape(shape)


# =====================================================================================================================================
# 1. row resamplers
# =====================================================================================================================================
def _hip_linear(src, h, w):
    check, f32, i32, i64, ptr, sp = _a()
    H, W, Cn = src.shape
    u8 = src.dtype == np.uint8
    out = _buf(h * w * Cn, torch.uint8 if u8 else torch.float32)
    fn = _L().csm_resize_u8_linear if u8 else _L().csm_resize_f32_linear
    check(fn(ptr(_dev(src)), i32(H), i32(W), i32(Cn), i32(h), i32(w), ptr(out), sp()), "resize_linear")
    return _take(out, (h, w, Cn))


@pytest.mark.parametrize("pair", C.RESIZE_PAIRS, ids=C.pair_id)
def test_resize_u8_linear(pair):
    """k_resize_u8_linear: bit-equal to the oracle, strictly within one level of the float64 bilinear (the result is one of the two
    integers around the exact value); a constant image stays constant; the identical size returns the input bytes"""
    (H, W), (h, w) = pair
    for Cn in C.LINEAR_CHANNELS:
        src = C.image_u8((H, W, Cn), 1, H, W, Cn)
        got = _hip_linear(src, h, w)
        assert np.array_equal(got, R.orc_resize_u8_linear(src, h, w)), (pair, Cn)
        assert np.abs(got.astype(F64) - C.bilinear_ref(src, h, w)).max() < 1.0
        if (H, W) == (h, w):
            assert np.array_equal(got, src)
    assert (_hip_linear(np.full((H, W, 3), 77, np.uint8), h, w) == 77).all()


@pytest.mark.parametrize("pair", C.RESIZE_PAIRS, ids=C.pair_id)
def test_resize_f32_linear(pair):
    """k_resize_f32_linear: bit-equal to the oracle; |got - f64| <= max(4 e32, 8 * 2^-23) max|src| with the coordinate rounded to float32;
    a constant image stays constant within 8 * 2^-23 of its value (OpenCV's float32 blend does not keep it to the bit: DESIGN.md 6.3)"""
    (H, W), (h, w) = pair
    for Cn in C.LINEAR_CHANNELS:
        src = C.image_f32((H, W, Cn), 2, H, W, Cn)
        got = _hip_linear(src, h, w)
        assert np.array_equal(got, R.orc_resize_f32_linear(src, h, w)), (pair, Cn)
        ref, bound, _ = R.f32_linear_bound(src, h, w)
        assert np.abs(got.astype(F64) - ref).max() <= bound
        if (H, W) == (h, w):
            assert np.array_equal(got, src)
    const = np.full((H, W, 1), F32(0.3))                # s0 * (1 - f) + s1 * f rounds (1 - f): a constant is kept to the bound, not to the bit
    got = _hip_linear(const, h, w)
    assert np.array_equal(got, R.orc_resize_f32_linear(const, h, w))
    assert np.abs(got.astype(F64) - float(F32(0.3))).max() <= 8 * C.EPS32 * 0.3


def test_resize_linear_exact_2x_of_a_ramp_is_monotone():
    src = C.ramp_u8(31, 257, 3)
    assert (np.diff(_hip_linear(src, 62, 514).astype(int), axis=1) >= 0).all()
    assert (np.diff(_hip_linear(src.astype(F32), 62, 514), axis=1) >= 0).all()


@pytest.mark.parametrize("Cn", [0, 5])
def test_resize_linear_refuses_a_channel_count_without_a_launch(Cn):
    check, f32, i32, i64, ptr, sp = _a()
    for fn, dt in ((_L().csm_resize_u8_linear, torch.uint8), (_L().csm_resize_f32_linear, torch.float32)):
        src = torch.zeros(8 * 8 * 5, dtype=dt, device='cuda')
        out = _buf(4 * 4 * 5, dt)
        assert fn(ptr(src), i32(8), i32(8), i32(Cn), i32(4), i32(4), ptr(out), sp()) == CSM_ERR_ARG
        torch.cuda.synchronize()
        assert _untouched(out)


@pytest.mark.parametrize("pair", C.AREA_PAIRS, ids=C.pair_id)
def test_resize_u8_to_f32_area_enlargement(pair):
    """k_resize_u8_to_f32 (INTER_AREA when enlarging): bit-equal to the oracle, integral, strictly within one level of float64"""
    check, f32, i32, i64, ptr, sp = _a()
    (h, w), (H, W) = pair

    def run(src):
        out = _buf(H * W)
        check(_L().csm_resize_u8_to_f32(ptr(_dev(src)), i32(h), i32(w), i32(H), i32(W), ptr(out), sp()), "resize_u8_to_f32")
        return _take(out, (H, W))
    src = C.image_u8((h, w), 3, h, w)
    got = run(src)
    assert np.array_equal(got, R.orc_area(src, H, W))
    assert np.array_equal(got, np.rint(got)) and np.abs(got.astype(F64) - C.area_ref(src, H, W)).max() < 1.0
    if (h, w) == (H, W):
        assert np.array_equal(got, src.astype(F32))
    assert (run(np.full((h, w), 201, np.uint8)) == 201).all()


@pytest.mark.parametrize("pair", C.LANCZOS_PAIRS, ids=C.pair_id)
def test_resize_u8_lanczos4(pair):
    """k_resize_u8_lanczos4: bit-equal to the oracle, strictly within one level of the float64 normalised 8-tap Lanczos; constant +-1"""
    check, f32, i32, i64, ptr, sp = _a()
    (h, w), (H, W) = pair

    def run(src):
        out = _buf(H * W)
        check(_L().csm_resize_u8_lanczos4_to_f32(ptr(_dev(src)), i32(h), i32(w), i32(H), i32(W), ptr(out), sp()), "lanczos4")
        return _take(out, (H, W))
    src = C.image_u8((h, w), 4, h, w)
    got = run(src)
    assert np.array_equal(got, R.orc_lanczos(src, H, W))
    assert np.abs(got.astype(F64) - C.lanczos_ref(src, H, W)).max() < 1.0
    assert np.abs(run(np.full((h, w), 130, np.uint8)) - 130).max() <= 1


@pytest.mark.parametrize("pair", C.RESIZE_PAIRS, ids=C.pair_id)
def test_leres_input(pair):
    """k_leres_input: bit-equal to the oracle; mapped back through (out * std + mean) * 255 an integer to 1e-3, which lies strictly
    within one level of the float64 bilinear of the SWAPPED channel (the planes differ by >= 8 levels)"""
    check, f32, i32, i64, ptr, sp = _a()
    (H, W), (h, w) = pair
    img = C.leres_image(H, W)
    out = _buf(3 * h * w)
    check(_L().csm_leres_input(ptr(_dev(img)), i32(H), i32(W), i32(h), i32(w), ptr(out), sp()), "leres_input")
    got = _take(out, (3, h, w))
    assert np.array_equal(got, R.orc_leres_input(img, h, w))
    R.check_leres(got, img)
    if (H, W) == (h, w):
        assert np.array_equal(np.rint(R.leres_back(got)).astype(np.uint8), img[..., ::-1])


# =====================================================================================================================================
# 2. crop + resize
# =====================================================================================================================================
@pytest.mark.parametrize("hw", C.CROP_FRAMES, ids=lambda v: "%dx%d" % v)
def test_crop_resize_u8(hw):
    """k_crop_resize_tile on the LDS-window path, on the direct fallback and with blocks of both kinds in one launch (which case takes
    which is asserted on the CPU): bit-equal to the oracle, |got - f64 chain| < 1.5; the integer-origin same-size patch returns the
    frame, a centre far outside the replicated corner colour"""
    check, f32, i32, i64, ptr, sp = _a()
    H, W = hw
    frame = C.image_u8(hw + (3,), 5, *hw)
    d_frame = _dev(frame)
    for kind, ph, pw, cx, cy in R.crop_kinds_of(hw):
        out = _buf(H * W * 3, torch.uint8)
        check(_L().csm_crop_resize_u8(ptr(d_frame), i32(H), i32(W), i32(ph), i32(pw), f32(cx), f32(cy), ptr(out), sp()), "crop_resize")
        got = _take(out, (H, W, 3))
        assert np.array_equal(got, R.orc_crop(frame, ph, pw, cx, cy)), (hw, kind)
        assert np.abs(got.astype(F64) - C.crop_ref(frame, ph, pw, cx, cy)).max() < 1.5, (hw, kind)
        if kind == 'same_int':
            assert np.array_equal(got, frame)
        if kind == 'outside':
            assert (got == frame[0, 0]).all()


# =====================================================================================================================================
# 3. reductions
# =====================================================================================================================================
def _hip_minmax(x_d, n, ptr_override=None):
    check, f32, i32, i64, ptr, sp = _a()
    out = _buf(2)
    scratch = torch.empty(512, device='cuda')
    rc = _L().csm_minmax(ptr(x_d) if ptr_override is None else ptr_override, i64(n), ptr(out), ptr(scratch), sp())
    return rc, out


@pytest.mark.parametrize("n", C.REDUCE_LENGTHS)
def test_minmax_is_exact(n):
    """k_minmax_partial / k_minmax_final == numpy with the extreme first, last, in the last full float4 and in the scalar tail; all-equal
    input, +-0 only (the values compare equal; the sign is not asserted), +-inf present"""
    cases = [C.minmax_case(n, where) for where in C.minmax_positions(n)] + list(C.minmax_value_cases(n).values())
    for x in cases:
        x_d = _dev(x)
        assert x_d.data_ptr() % 16 == 0
        rc, out = _hip_minmax(x_d, n)
        assert rc == 0
        got = _take(out, (2,))
        assert got[0] == x.min() and got[1] == x.max(), (n, got, x.min(), x.max())


def test_minmax_refuses_a_pointer_that_is_only_4_byte_aligned():
    x_d = _dev(C.minmax_case(1025, 'first'))
    rc, out = _hip_minmax(x_d, 1024, ctypes.c_void_p(x_d.data_ptr() + 4))
    torch.cuda.synchronize()
    assert rc == CSM_ERR_ARG and _untouched(out)


@pytest.mark.parametrize("kind", C.FILL_KINDS)
def test_fill_zero_min_positive_is_exact(kind):
    """k_minpos_scan / k_minpos_apply == `d[d == 0] = d[d > 0].min()` bit for bit; the scratch is NOT zeroed by the caller"""
    check, f32, i32, i64, ptr, sp = _a()
    for n in C.REDUCE_LENGTHS:
        x = C.fill_case(n, kind)
        buf = _buf(n)
        buf[:n] = _dev(x)
        scratch = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
        check(_L().csm_fill_zero_min_positive(ptr(buf), i64(n), ptr(scratch), sp()), "fill_zero")
        got = _take(buf, (n,))
        ref = C.fill_reference(x)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (kind, n)


@pytest.mark.parametrize("ratio", C.MEAN_STD_RATIOS)
def test_mean_std_within_the_derived_bound(ratio):
    """k_sum_partial / k_sum_final against numpy float64: |mean - m64| <= 1 ulp32(m64), |std - s64| <= 1 ulp32(s64) + ulp32(m64)^2 / (8 s64)
    (the mean is rounded to float32 and the second pass is centred on it); a constant gives std == 0 exactly"""
    check, f32, i32, i64, ptr, sp = _a()
    L = _L()
    worst = 0.0
    for n in C.REDUCE_LENGTHS:
        for x in (C.mean_std_case(n, ratio), np.full(n, F32(3.3) + F32(ratio))):
            out = _buf(2)
            scratch = torch.empty(L.csm_mean_std_scratch_bytes(), dtype=torch.uint8, device='cuda')
            check(L.csm_mean_std(ptr(_dev(x)), i64(n), ptr(out), ptr(scratch), sp()), "mean_std")
            got = _take(out, (2,)).astype(F64)
            m64, s64, bm, bs = C.mean_std_bounds(x)
            assert abs(got[0] - m64) <= bm, (n, ratio, got[0], m64)
            assert abs(got[1] - s64) <= bs, (n, ratio, got[1], s64, bs)
            if s64 == 0.0:
                assert got[1] == 0.0
            else:
                worst = max(worst, abs(got[1] - s64) / bs)
    print("mean/sigma %g: worst |std - s64| / bound = %.3f" % (ratio, worst))


def _hip_stats(d_d, H, W, y0, x0, ch, cw, mm, scale):
    check, f32, i32, i64, ptr, sp = _a()
    out6 = _buf(6, torch.float64)
    keys = torch.full((2,), 0x5A5A5A5A, dtype=torch.int64, device='cuda')
    rc = _L().csm_depth_range_stats(ptr(_dev(np.asarray(mm, F32))), f32(scale), ptr(d_d), i32(H), i32(W), i32(y0), i32(x0), i32(ch), i32(cw),
                                    ptr(keys), ptr(out6), sp())
    return rc, out6


@pytest.mark.parametrize("name", C.STATS_CASES)
def test_depth_range_stats_is_exact(name):
    """k_crop_minmaxloc / k_stats_pack: values and FIRST row-major positions of the crop's extremes, the normalised raw min / max"""
    d, y0, x0, ch, cw = C.stats_case(name)
    H, W = d.shape
    rc, out6 = _hip_stats(_dev(d), H, W, y0, x0, ch, cw, (0.5, 4.0), 40.0)
    assert rc == 0
    assert _take(out6, (6,)).tolist() == C.stats_reference(d, y0, x0, ch, cw, (0.5, 4.0), 40.0)


def test_depth_range_stats_refuses_a_crop_outside_the_plane():
    d_d = _dev(np.ones((20, 30), F32))
    for y0, x0, ch, cw in ((15, 0, 6, 30), (0, 25, 20, 6), (-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, 0, 5)):
        rc, out6 = _hip_stats(d_d, 20, 30, y0, x0, ch, cw, (1.0, 2.0), 1.0)
        torch.cuda.synchronize()
        assert rc == CSM_ERR_ARG and _untouched(out6), (y0, x0, ch, cw)


@pytest.mark.parametrize("name", C.ADJUST_CASES)
def test_depth_adjust_instance_is_exact(name):
    """k_adjust_rows / k_adjust_pick / k_adjust_apply == oracle == the numpy statement of kenburns_effect.py:68-78, bit for bit"""
    from oracle import kenburns as okb
    check, f32, i32, i64, ptr, sp = _a()
    disp, mask, _ = C.adjust_case(name)
    H, W = disp.shape
    buf = _buf(H * W)
    buf[:H * W] = _dev(disp).reshape(-1)
    scratch = torch.full((2 * H + 2 + SLACK,), float('nan'), device='cuda')
    check(_L().csm_depth_adjust_instance(ptr(buf), ptr(_dev(mask)), i32(H), i32(W), ptr(scratch), sp()), "depth_adjust")
    got = _take(buf, (H, W))
    assert np.isnan(scratch[2 * H + 2:].cpu().numpy()).all()
    assert np.array_equal(got, C.adjust_reference(disp, mask))
    assert np.array_equal(got, okb.depth_adjustment(mask.astype(bool)[None], disp[None, None].copy())[0, 0])


# =====================================================================================================================================
# 4. aten-defined operations
# =====================================================================================================================================
def _rel_bound(ref64, ref32, scale):
    return C.yardstick(float(np.abs(ref32.astype(F64) - ref64).max()) / scale) * scale


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("pair", C.PLANES_PAIRS, ids=C.pair_id)
def test_resize_bilinear_planes(pair, align):
    """k_bilinear_planes against F.interpolate in float64 on the CPU: max(4 e32, 8 * 2^-23) max|x| with e32 torch's CPU float32 call,
    on a smooth plane and on white noise, 1 and 3 planes; the identical size returns the input"""
    check, f32, i32, i64, ptr, sp = _a()
    (H, W), (h, w) = pair
    for planes in (1, 3):
        for kind in ('smooth', 'noise'):
            x = C.planes_input(planes, (H, W), kind)
            out = _buf(planes * h * w)
            check(_L().csm_resize_bilinear_planes(ptr(_dev(x)), i32(planes), i32(H), i32(W), i32(h), i32(w), i32(align), ptr(out), sp()), "planes")
            got = _take(out, (planes, h, w))
            ref = C.interp_bilinear(x, (h, w), align, torch.float64)
            bound = _rel_bound(ref, C.interp_bilinear(x, (h, w), align, torch.float32), float(np.abs(x).max()))
            assert np.abs(got.astype(F64) - ref).max() <= bound, (pair, align, planes, kind)
            if (H, W) == (h, w):
                assert np.array_equal(got, x)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("pair", C.AREA_MASK_PAIRS, ids=C.pair_id)
def test_mask_area_resize_threshold_equals_the_integer_rule(pair, n):
    """k_mask_area_threshold == 10 * count > 3 * kh * kw over the integer window, with the float32 bit at exactly 30 %; instance 0 of
    the three-instance call equals the same mask run alone"""
    check, f32, i32, i64, ptr, sp = _a()
    (H, W), (h, w) = pair
    m, _ = C.area_mask_case(n, (H, W), (h, w))
    out = _buf(n * h * w, torch.uint8)
    check(_L().csm_mask_area_resize_threshold(ptr(_dev(m)), i32(n), i32(H), i32(W), i32(h), i32(w), f32(C.AREA_THR), ptr(out), sp()), "mask_area")
    got = _take(out, (n, h, w))
    ref, _ = C.area_mask_reference(m, (h, w))
    assert np.array_equal(got, ref)                 # the instances have different densities: a leak from one into another shows
    if n > 1:
        alone = _buf(h * w, torch.uint8)
        check(_L().csm_mask_area_resize_threshold(ptr(_dev(m[:1])), i32(1), i32(H), i32(W), i32(h), i32(w), f32(C.AREA_THR), ptr(alone), sp()),
              "mask_area")
        assert np.array_equal(_take(alone, (1, h, w))[0], got[0])


def _hip_zoe_prep(img, pad_h, pad_w, flip, nh, nw):
    check, f32, i32, i64, ptr, sp = _a()
    B, _, H, W = img.shape
    out = _buf(B * 3 * nh * nw)
    check(_L().csm_zoe_pad_prep(ptr(_dev(img)), i32(B), i32(H), i32(W), i32(pad_h), i32(pad_w), i32(flip), i32(nh), i32(nw), ptr(out), sp()),
          "zoe_pad_prep")
    return _take(out, (B, 3, nh, nw))


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("name", list(C.ZOE_PREP_CASES))
def test_zoe_pad_prep(name, flip):
    """k_zoe_pad_prep against flip -> F.pad(reflect) -> F.interpolate(bilinear, align_corners=True) -> (v - 0.5) / 0.5 in float64; the
    flipped output of a left-right symmetric image equals the unflipped one bit for bit"""
    B, H, W, pad_h, pad_w, nh, nw = C.ZOE_PREP_CASES[name]
    img = C.zoe_image(B, H, W)
    got = _hip_zoe_prep(img, pad_h, pad_w, flip, nh, nw)
    ref = C.zoe_prep_ref(img, pad_h, pad_w, flip, nh, nw, torch.float64)
    bound = _rel_bound(ref, C.zoe_prep_ref(img, pad_h, pad_w, flip, nh, nw, torch.float32), float(np.abs(img).max()))
    assert np.abs(got.astype(F64) - ref).max() <= bound, (name, flip)
    if flip:
        sym = np.ascontiguousarray(np.concatenate([img[..., :(W + 1) // 2], img[..., :W // 2][..., ::-1]], -1))
        assert np.array_equal(sym, sym[..., ::-1])
        assert np.array_equal(_hip_zoe_prep(sym, pad_h, pad_w, 1, nh, nw), _hip_zoe_prep(sym, pad_h, pad_w, 0, nh, nw))


def test_zoe_pad_prep_refuses_a_pad_as_large_as_the_image():
    check, f32, i32, i64, ptr, sp = _a()
    img = torch.zeros((1, 3, 7, 9), device='cuda')
    out = _buf(3 * 8 * 8)
    for pad_h, pad_w in ((7, 0), (0, 9)):
        assert _L().csm_zoe_pad_prep(ptr(img), i32(1), i32(7), i32(9), i32(pad_h), i32(pad_w), i32(0), i32(8), i32(8), ptr(out), sp()) == CSM_ERR_ARG
    torch.cuda.synchronize()
    assert _untouched(out)


def _hip_zoe_crop(d, pad_h, pad_w, H, W, unflip, mode=0, prev=None):
    check, f32, i32, i64, ptr, sp = _a()
    B, _, h, w = d.shape
    out = _buf(B * H * W)
    if prev is not None:
        out[:B * H * W] = _dev(prev).reshape(-1)
    check(_L().csm_zoe_resize_crop(ptr(_dev(d)), i32(B), i32(h), i32(w), i32(pad_h), i32(pad_w), i32(H), i32(W), i32(unflip), i32(mode), ptr(out),
                                   sp()), "zoe_resize_crop")
    return _take(out, (B, 1, H, W))


@pytest.mark.parametrize("unflip", [0, 1])
@pytest.mark.parametrize("name", list(C.ZOE_CROP_CASES))
def test_zoe_resize_crop(name, unflip):
    """k_zoe_resize_crop against F.interpolate(bicubic, align_corners=False) -> crop -> flip in float64, max(4 e32, 8 * 2^-23) max|d|;
    mode 1 gives (previous + v) / 2 to the bit"""
    B, h, w, pad_h, pad_w, H, W = C.ZOE_CROP_CASES[name]
    d = C.zoe_depth(B, h, w)
    got = _hip_zoe_crop(d, pad_h, pad_w, H, W, unflip)
    ref = C.zoe_crop_ref(d, pad_h, pad_w, H, W, unflip, torch.float64)
    bound = _rel_bound(ref, C.zoe_crop_ref(d, pad_h, pad_w, H, W, unflip, torch.float32), float(np.abs(d).max()))
    assert np.abs(got.astype(F64) - ref).max() <= bound, (name, unflip)
    if (h, w) == (H + 2 * pad_h, W + 2 * pad_w):
        assert np.array_equal(got, ref.astype(F32))
    prev = C.rng_of(45, B, H, W).uniform(1.0, 5.0, (B, 1, H, W)).astype(F32)
    assert np.array_equal(_hip_zoe_crop(d, pad_h, pad_w, H, W, unflip, 1, prev), ((prev + got) / F32(2.0)).astype(F32))


def test_zoe_resize_crop_keeps_a_constant_plane_within_4_ulp():
    """A constant plane comes back constant within 4 ulp, because the cubic weights sum to 1"""
    worst = {}
    for name, (B, h, w, pad_h, pad_w, H, W) in C.ZOE_CROP_CASES.items():
        const = _hip_zoe_crop(np.full((B, 1, h, w), F32(2.7)), pad_h, pad_w, H, W, 0)
        worst[name] = float(np.abs(const.astype(F64) - float(F32(2.7))).max() / C.ulp32(2.7))
        print("constant 2.7 through %s: %.1f ulp" % (name, worst[name]))
    assert max(worst.values()) <= 4.0, worst


# =====================================================================================================================================
# 5. single-rounding chains: exact bits (the library is built with -ffp-contract=off)
# =====================================================================================================================================
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("n", C.CHAIN_LENGTHS)
def test_normalise_and_denormalise_chains_are_bit_exact(n):
    check, f32, i32, i64, ptr, sp = _a()
    L = _L()
    x = C.chain_input(n, 1)
    mm = np.array([x.min(), x.max()], F32)
    out, nmax = _buf(n), _buf(1)
    check(L.csm_normalise_disparity(ptr(_dev(x)), i64(n), ptr(_dev(mm)), f32(40.0), ptr(out), ptr(nmax), sp()), "normalise")
    ref, ref_max = C.normalise_disparity_ref(x, mm[1], 40.0)
    assert np.array_equal(_bits(_take(out, (n,))), _bits(ref)) and _take(nmax, (1,))[0] == ref_max == ref.max()
    out = _buf(n)
    check(L.csm_normalise_disparity(ptr(_dev(x)), i64(n), ptr(_dev(mm)), f32(40.0), ptr(out), ptr(None), sp()), "normalise")
    assert np.array_equal(_bits(_take(out, (n,))), _bits(ref))
    ms = np.array([0.37, 1.9], F32)
    out = _buf(n)
    check(L.csm_normalise_mean_std(ptr(_dev(x)), i64(n), ptr(_dev(ms)), ptr(out), sp()), "normalise_ms")
    assert np.array_equal(_bits(_take(out, (n,))), _bits(C.normalise_ms_ref(x, ms[0], ms[1])))
    xd = C.denormalise_input(n)
    for mean in (F32(0.5), F32(-0.0)):
        ms = np.array([mean, F32(0.25) - F32(0.0000001)], F32)
        for mode in (0, 1, 2):
            out = _buf(n)
            check(L.csm_denormalise_mean_std(ptr(_dev(xd)), i64(n), ptr(_dev(ms)), i32(mode), ptr(out), sp()), "denormalise_ms")
            got, ref = _take(out, (n,)), C.denormalise_ms_ref(xd, ms[0], ms[1], mode)
            if mode == 0:
                assert np.array_equal(_bits(got), _bits(ref))
            else:                       # the sign of a zero that leaves clip / threshold is not defined by the reference; every other bit is
                assert np.array_equal(got, ref) and np.array_equal(_bits(got)[ref != 0], _bits(ref)[ref != 0])
    out = _buf(n)
    assert L.csm_denormalise_mean_std(ptr(_dev(xd)), i64(n), ptr(_dev(ms)), i32(3), ptr(out), sp()) == CSM_ERR_ARG
    torch.cuda.synchronize()
    assert _untouched(out)


@pytest.mark.parametrize("hw", [(1, 1), (5, 51), (1, 257)], ids=lambda v: "%dx%d" % v)
def test_u8_hwc_to_f32_chw_is_bit_exact(hw):
    check, f32, i32, i64, ptr, sp = _a()
    H, W = hw
    img = C.bytes_image(H * W).reshape(H, W, 3)
    out = _buf(3 * H * W)
    check(_L().csm_u8_hwc_to_f32_chw(ptr(_dev(img)), i32(H), i32(W), ptr(out), sp()), "u8_hwc_to_f32_chw")
    assert np.array_equal(_bits(_take(out, (3, H, W))), _bits(C.u8_to_chw_ref(img)))


@pytest.mark.parametrize("n", C.CHAIN_LENGTHS)
def test_bokeh_depth_and_zoe_disparity_are_bit_exact(n):
    check, f32, i32, i64, ptr, sp = _a()
    d8 = C.image_u8((n,), 57, n)
    out = _buf(n)
    check(_L().csm_bokeh_depth(ptr(_dev(d8)), ptr(out), i64(n), f32(251.0), f32(100.5), f32(17.0), f32(203.5), sp()), "bokeh_depth")
    assert np.array_equal(_bits(_take(out, (n,))), _bits(C.bokeh_depth_ref(d8, 251.0, 100.5, 17.0, 203.5)))
    d = C.zoe_disp_input(n)
    out = _buf(n)
    check(_L().csm_zoe_depth_to_disparity(ptr(_dev(d)), i64(n), f32(12.5), ptr(out), sp()), "zoe_disparity")
    got = _take(out, (n,))
    assert np.array_equal(_bits(got), _bits(C.zoe_disp_ref(d, 12.5))), (got[:10], C.zoe_disp_ref(d, 12.5)[:10])


@pytest.mark.parametrize("n", C.CHAIN_LENGTHS)
@pytest.mark.parametrize("name", list(C.COLORIZE_CASES))
def test_colorize_gray_r_is_bit_exact(name, n):
    """k_colorize_gray_r == the numpy float32 chain (v - vmin) / (vmax - vmin) * 256 -> 256 to 255 -> clip -> int -> gray_r byte table:
    vmax itself, both clamps, the truncation of (-1, 0), vmin == vmax (all 255); with the oracle's percentiles as vmin / vmax it equals
    the oracle; a null pointer and n = 0 are refused without a launch"""
    check, f32, i32, i64, ptr, sp = _a()
    vmin, vmax = C.COLORIZE_CASES[name]
    v = C.colorize_input(n, vmin, vmax)

    def run(lo, hi):
        out = _buf(n, torch.uint8)
        check(_L().csm_colorize_gray_r(ptr(_dev(v)), ptr(out), i64(n), f32(lo), f32(hi), sp()), "colorize_gray_r")
        return _take(out, (n,))
    got = run(vmin, vmax)
    assert np.array_equal(got, C.colorize_ref(v, vmin, vmax))
    if name == 'flat':
        assert (got == 255).all()
    elif n > 1:
        lo, hi = R.okb._percentile(v, 2), R.okb._percentile(v, 85)
        assert np.array_equal(run(lo, hi), R.okb.colorize_gray_r(v))
    out = _buf(n, torch.uint8)
    assert _L().csm_colorize_gray_r(ptr(_dev(v)), ptr(out), i64(0), f32(vmin), f32(vmax), sp()) == CSM_ERR_ARG
    assert _L().csm_colorize_gray_r(ptr(None), ptr(out), i64(n), f32(vmin), f32(vmax), sp()) == CSM_ERR_ARG
    torch.cuda.synchronize()
    assert _untouched(out)


@pytest.mark.parametrize("name", C.QUANT_CASES)
def test_leres_quantize_inside_the_bracket(name):
    """k_leres_quantize: bit-equal to the oracle; between the float64 evaluations of truncate / scale / round / invert at
    o64 (1 -+ 2^-20) (a single value for >= 98 % of every case, asserted on the CPU)"""
    check, f32, i32, i64, ptr, sp = _a()
    d, mn, mx = C.quant_case(name)
    out = _buf(d.size, torch.uint8)
    check(_L().csm_leres_quantize(ptr(_dev(d)), i64(d.size), ptr(_dev(np.array([mn, mx], F32))), ptr(out), sp()), "leres_quantize")
    got = _take(out, d.shape)
    assert np.array_equal(got, R.orc_quantize(d, mn, mx))
    lo, hi = C.quant_bracket(d, mn, mx)
    assert ((lo <= got) & (got <= hi)).all()
    if name in ('constant', 'tiny_range'):
        assert (got == 255).all()
    else:
        assert (got[d == mx] == 0).all() and (got[d == mn] == 255).all()


@pytest.mark.parametrize("lf", C.POW_LIGHTNESS)
def test_bokeh_highlight_and_finish(lf):
    """k_bokeh_highlight within max(4 e32, 8 * 2^-23) of (img / 255) ^ lf in float64 (e32: numpy's float32 power); k_bokeh_finish within
    one level of the float64 uint8, and exact on at least numpy float32's own share minus 2 percentage points"""
    check, f32, i32, i64, ptr, sp = _a()
    img = C.image_u8((9, 257, 3), 56)
    n = img.size
    out = _buf(n)
    check(_L().csm_bokeh_highlight(ptr(_dev(img)), ptr(out), i64(n), f32(lf), sp()), "bokeh_highlight")
    hi = _take(out, (n,))
    ref, e32 = C.highlight_refs(img, lf)
    err = float(np.abs(hi.astype(F64) - ref.reshape(-1)).max() / np.abs(ref).max())
    assert err <= C.yardstick(e32), (err, e32)
    a = np.power(img.astype(F32) / F32(255), F32(lf)).reshape(-1)
    b = a[::-1].copy()
    out8 = _buf(n, torch.uint8)
    check(_L().csm_bokeh_finish(ptr(_dev(a)), ptr(_dev(b)), ptr(out8), i64(n), f32(lf), sp()), "bokeh_finish")
    got = _take(out8, (n,))
    u64, u32 = C.finish_refs(a, b, lf)
    share_np, _ = C.pow_share(u32, u64)
    share, worst = C.pow_share(got, u64)
    print("lightness %g: highlight err %.3g (e32 %.3g); finish exact share HIP %.4f, numpy float32 %.4f" % (lf, err, e32, share, share_np))
    assert worst <= 1 and share >= share_np - 0.02


@pytest.mark.parametrize("factor", [1, 2, 3])
@pytest.mark.parametrize("focal", [None, 100.5])
@pytest.mark.parametrize("is_u8", [1, 0])
def test_bokeh_depth_general(is_u8, focal, factor):
    """k_bokeh_depth_pre / csm_minmax / k_bokeh_depth_post: factors 1 and 2 (v * v) bit-equal to the numpy float32 chain, factor 3 (powf)
    within max(4 e32, 8 * 2^-23) of the float64 chain, relative to the output's range 0.0005"""
    check, f32, i32, i64, ptr, sp = _a()
    for n in (1023, 2 ** 18 + 5):
        depth = C.bokeh_general_input(n, is_u8)
        tmp, out = _buf(n + 4 - n % 4), _buf(n)
        mm4, scratch = _buf(4), torch.empty(512, device='cuda')
        assert tmp.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
        check(_L().csm_bokeh_depth_general(ptr(_dev(depth)), i32(is_u8), i64(n), i32(0 if focal is None else 1), f32(focal or 0.0), f32(factor),
                                           ptr(tmp), ptr(mm4), ptr(scratch), ptr(out), sp()), "bokeh_depth_general")
        got = _take(out, (n,))
        assert _untouched(tmp[n:])
        ref, r32, e32 = C.bokeh_general_refs(depth, focal, factor)
        if factor != 3:
            assert np.array_equal(_bits(got), _bits(r32)), (is_u8, focal, factor, n)
        assert np.abs(got.astype(F64) - ref).max() / 0.0005 <= C.yardstick(e32)


# =====================================================================================================================================
# 6. bokeh pass: every template and path
# =====================================================================================================================================
@pytest.mark.parametrize("name", [c[0] for c in C.BOKEH_CASES])
def test_bokeh_pass_and_fused_finish(name):
    """k_bokeh_pass_tile<9 / 16 / 20, false / true> (which template, which blocks are interior and where samples leave the staged window
    is asserted on the CPU): the pass bit-equal to the oracle and within max(4 e32, 8 * 2^-23) of the float64 accumulation over the
    reference's float32 sample positions; the fused finish bit-equal to pass + csm_bokeh_finish"""
    check, f32, i32, i64, ptr, sp = _a()
    L = _L()
    img, depth, ns = C.bokeh_case(name)
    H, W = depth.shape
    img_d, depth_d = _dev(img), _dev(depth)
    for dx, dy in C.bokeh_dirs(name):
        out = _buf(H * W * 3)
        check(L.csm_bokeh_pass(ptr(img_d), ptr(depth_d), ptr(out), i32(H), i32(W), i32(ns), f32(dx), f32(dy), sp()), "bokeh_pass")
        got = _take(out, (H, W, 3))
        assert np.array_equal(got, R.orc_bokeh_pass(img, depth, ns, dx, dy)), (name, dx, dy)
        ref, bound, _ = R.bokeh_bound(img, depth, ns, dx, dy)
        assert np.abs(got.astype(F64) - ref).max() <= bound
        two, fused = _buf(H * W * 3, torch.uint8), _buf(H * W * 3, torch.uint8)
        check(L.csm_bokeh_finish(ptr(img_d), ptr(out), ptr(two), i64(H * W * 3), f32(2.5), sp()), "bokeh_finish")
        check(L.csm_bokeh_pass_finish(ptr(img_d), ptr(depth_d), ptr(fused), i32(H), i32(W), i32(ns), f32(dx), f32(dy), f32(2.5), sp()),
              "bokeh_pass_finish")
        assert np.array_equal(_take(fused, (H, W, 3)), _take(two, (H, W, 3)))
