"""GPU: the kernels of the depth-of-field frame tail one by one (csrc/frametail.hip), each entry point called through ctypes, against
the plain references of tests/frametail_cases.py.  Every comparison is equality (NaN equal to NaN); the one exception is the
highlight plane of csm_bokeh_prep, which is bit-equal to csm_bokeh_highlight and, like that kernel in test_gpu_imageops.py, within
max(4 e32, 8 * 2^-23) of the float64 power.  Output buffers carry a sentinel in front of and behind the part a call may write; the
counting tables and tickets that a call must leave zeroed are read back after it.  tests/test_frametail_references.py proves on the
CPU which path each case reaches."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frametail_cases as C  # noqa: E402

CSM_ERR_ARG = 1
SLACK = 8
SENT = {torch.uint8: 0xA5, torch.float32: float('nan')}
F32, F64 = np.float32, np.float64
PCT_CASES = C.percentile_cases()


def _L():
    from cartoonsegmentation_amd import _lib
    return _lib.load()


def _a():
    from cartoonsegmentation_amd._lib import check, f32, f64, i32, i64, ptr, stream_ptr
    return check, f32, f64, i32, i64, ptr, stream_ptr


_ALIVE = []


@pytest.fixture(autouse=True)
def _inputs_live_until_the_test_ends():
    """every upload is held until the test is over (the caching allocator could hand its block to the next upload before the kernel has
    read it)"""
    yield
    torch.cuda.synchronize()
    del _ALIVE[:]


def _dev(a, off=0):
    """upload; off > 0: as a view that starts `off` elements into a fresh allocation (the pointer is aligned to the element only)"""
    a = np.concatenate([np.zeros(off, a.dtype), a.reshape(-1)]) if off else np.array(a, order='C')     # a copy: the cases are read-only
    t = torch.from_numpy(a).cuda()
    _ALIVE.append(t)
    return t[off:] if off else t


class _Out:
    """output of n elements that starts `off` elements into its allocation, with SLACK sentinel elements on both sides"""

    def __init__(self, n, dtype=torch.float32, off=0):
        assert off < SLACK
        self.n, self.lead = int(n), SLACK + off              # the allocation is 256-byte aligned and SLACK elements are a multiple of 16 bytes
        self.buf = torch.full((self.lead + self.n + SLACK,), SENT[dtype], dtype=dtype, device='cuda')
        self.view = self.buf[self.lead:self.lead + self.n]
        align = 16 if dtype == torch.float32 else 4
        assert (self.view.data_ptr() % align == 0) == (off == 0)

    def take(self):
        a = self.buf.cpu().numpy()
        edge = np.concatenate([a[:self.lead], a[self.lead + self.n:]])
        assert np.isnan(edge).all() if a.dtype.kind == 'f' else (edge == 0xA5).all(), "written outside the output"
        return a[self.lead:self.lead + self.n]


def _lut():
    return (ctypes.c_uint8 * 256)(*[int(x) for x in C.lut_gray_r()])


# =====================================================================================================================================
# 1. csm_percentile_pair
# =====================================================================================================================================
@pytest.fixture(scope="module")
def sel():
    """ONE scratch, zeroed once, for the whole parametrised run: every call must leave what the next one needs cleared"""
    return torch.zeros(_L().csm_percentile_scratch_bytes(), dtype=torch.uint8, device='cuda')


def _sel_is_clean(sel):
    """the counting tables (everything behind the 64-byte state) and the ticket and poison words of the state"""
    return not bool(sel[64:].any()) and not bool(sel[32:40].any())


def _percentile_input(kind, n, aligned):
    d = _dev(C.percentile_values(kind, n), 0 if aligned else 1)
    assert d.data_ptr() % 16 == (0 if aligned else 4)
    return d


@pytest.mark.parametrize("case", PCT_CASES, ids=C.percentile_id)
def test_percentile_pair_equals_the_sorted_reference(case, sel):
    check, f32, f64, i32, i64, ptr, sp = _a()
    kind, n, aligned, q_lo, q_hi = case
    d = _percentile_input(kind, n, aligned)
    out = _Out(2)
    check(_L().csm_percentile_pair(ptr(d), i64(n), f64(q_lo), f64(q_hi), ptr(out.view), ptr(sel), sp()), "percentile_pair")
    got, want = out.take(), C.percentile_want(case)
    assert C.same(got, want), (case, got, want)
    assert _sel_is_clean(sel), "the call left a table, the ticket or the poison flag set"


def test_percentile_scratch_is_clean_after_the_run(sel):
    """after the last case of the run above (or on the fresh scratch when run alone)"""
    assert _sel_is_clean(sel)


def test_two_percentile_calls_queued_back_to_back(sel):
    """different inputs, different outputs, one stream, no synchronisation in between: the second call's first pass starts on the tables
    the first call's last block has just re-zeroed"""
    check, f32, f64, i32, i64, ptr, sp = _a()
    cases = [('signed', 65539, True, 2.0, 85.0), ('depth', 1048576 + 4099, True, 50.0, 99.9), ('top', 65539, True, 0.0, 100.0),
             ('four_prefixes', 65539, True, 2.0, 85.0), ('ties', 257, True, 2.0, 85.0)]
    ins = [_percentile_input(c[0], c[1], c[2]) for c in cases]
    outs = [_Out(2) for _ in cases]
    torch.cuda.synchronize()
    for c, d, o in zip(cases, ins, outs):
        check(_L().csm_percentile_pair(ptr(d), i64(c[1]), f64(c[3]), f64(c[4]), ptr(o.view), ptr(sel), sp()), "percentile_pair")
    torch.cuda.synchronize()
    for c, o in zip(cases, outs):
        assert C.same(o.take(), C.percentile_want(c)), c
    assert _sel_is_clean(sel)


def test_percentile_refusals_launch_nothing():
    check, f32, f64, i32, i64, ptr, sp = _a()
    L = _L()
    scratch = torch.zeros(L.csm_percentile_scratch_bytes(), dtype=torch.uint8, device='cuda')
    d = _dev(C.percentile_values('depth', 257))
    out = _Out(2)
    ok = dict(v=ptr(d), n=257, lo=2.0, hi=85.0, o=ptr(out.view), s=ptr(scratch))
    bad = [dict(n=0), dict(n=1 << 32), dict(n=-1), dict(lo=-0.1), dict(hi=-0.1), dict(lo=100.1), dict(hi=100.1), dict(lo=float('nan')),
           dict(hi=float('nan')), dict(v=ptr(None)), dict(o=ptr(None)), dict(s=ptr(None))]
    for b in bad:
        k = dict(ok, **b)
        rc = L.csm_percentile_pair(k['v'], i64(k['n']), f64(k['lo']), f64(k['hi']), k['o'], k['s'], sp())
        assert rc == CSM_ERR_ARG, (sorted(b), rc)
    torch.cuda.synchronize()
    assert np.isnan(out.take()).all() and not bool(scratch.any())
    check(L.csm_percentile_pair(ok['v'], i64(257), f64(2.0), f64(85.0), ok['o'], ok['s'], sp()), "percentile_pair")       # and the accepted form
    assert C.same(out.take(), C.percentile_want(('depth', 257, True, 2.0, 85.0)))


def test_percentile_tables_that_count_too_little_give_nan():
    """The poisoned state from the other side (test_gpu_kenburns.py plants a count too MANY): a scratch that was not zeroed can make
    the coarse bins add up to LESS than n, and then no bin holds the top ranks.  Planted: -3 in the coarse bin of XCD copy 0 that
    holds the largest values, q = (0, 100).  The call answers NaN, keeps doing so, and recovers once the scratch is zeroed; the bucket
    index of a rank that was not found must stay inside the tables (it was read uninitialised before)."""
    check, f32, f64, i32, i64, ptr, sp = _a()
    L = _L()
    case = ('depth', 65539, True, 0.0, 100.0)
    a = C.percentile_values('depth', 65539)
    top = int(C.ordered_key(a).max() >> 24)
    assert int((C.ordered_key(a) >> 24 == top).sum()) >= 3                   # so the planted bin reads true count - 3, without a wrap
    scratch = torch.zeros(L.csm_percentile_scratch_bytes(), dtype=torch.uint8, device='cuda')
    d = _percentile_input(*case[:3])
    scratch.view(torch.int32)[16 + top] = -3                                  # the tables follow the 64-byte state: coarse bins first
    for call in (1, 2):
        out = _Out(2)
        check(L.csm_percentile_pair(ptr(d), i64(case[1]), f64(0.0), f64(100.0), ptr(out.view), ptr(scratch), sp()), "percentile_pair")
        assert np.isnan(out.take()).all(), call
        assert not bool(scratch[64:].any()) and bool(scratch[36:40].any()) and not bool(scratch[32:36].any())     # tables cleared, poison kept
    scratch.zero_()
    out = _Out(2)
    check(L.csm_percentile_pair(ptr(d), i64(case[1]), f64(0.0), f64(100.0), ptr(out.view), ptr(scratch), sp()), "percentile_pair")
    assert C.same(out.take(), C.percentile_want(case)) and _sel_is_clean(scratch)


# =====================================================================================================================================
# 2. csm_colorize_stats
# =====================================================================================================================================
@pytest.fixture(scope="module")
def bsc():
    """ONE csm_bokeh_depth_scratch_bytes() buffer, zeroed once, for every csm_colorize_stats call of the module"""
    return torch.zeros(_L().csm_bokeh_depth_scratch_bytes(), dtype=torch.uint8, device='cuda')


def _colorize_stats(kind, n, v_off, o_off, focal, bsc, calls=2):
    """csm_colorize_stats on the plane (value pointer offset by v_off floats, output by o_off bytes) -> checks everything"""
    check, f32, f64, i32, i64, ptr, sp = _a()
    L = _L()
    v, vmin, vmax = C.colorize_plane(kind, n)
    want = C.colorize_bytes(kind, n)
    stats_want = np.array(C.bokeh_stats_ref(want, focal), F32)
    d = _dev(v, v_off)
    assert d.data_ptr() % 16 == 4 * v_off
    vmm = _dev(np.array([vmin, vmax], F32))
    lut = _lut()
    for call in range(calls):                                # the second call runs on the scratch the first one left, not re-zeroed
        out = _Out(n, torch.uint8, o_off)
        bsc[:12] = 0xFF                                      # the three statistics are outputs: NaN before the call
        check(L.csm_colorize_stats(ptr(d), ptr(out.view), i64(n), ptr(vmm), lut, f32(focal), ptr(bsc), sp()), "colorize_stats")
        got = out.take()
        assert np.array_equal(got, want), (kind, n, v_off, o_off, call, int((got != want).sum()))
        stats = bsc[:12].cpu().numpy().view(F32)
        assert C.same_bits(stats, stats_want), (kind, n, v_off, o_off, focal, call, stats, stats_want)
        assert not bool(bsc[12:].any()), "ticket or histogram not zero after the call"
    plain = _Out(n, torch.uint8)
    check(L.csm_colorize_gray_r_dev(ptr(d), ptr(plain.view), i64(n), ptr(vmm), lut, sp()), "colorize_gray_r_dev")
    assert np.array_equal(plain.take(), want)


@pytest.mark.parametrize("n", C.CS_LENGTHS)
def test_colorize_stats_lengths_and_alignments(n, bsc):
    """bytes == colorize_ref == csm_colorize_gray_r_dev, stats3 == bokeh_stats_ref bit for bit, tables and ticket zero after the call,
    twice on one scratch; value pointer 16-byte aligned and offset by 4 bytes, output 4-byte aligned and offset by 1 byte"""
    for v_off in (0, 1):
        for o_off in (0, 1):
            _colorize_stats('noise', n, v_off, o_off, 17.25, bsc)


@pytest.mark.parametrize("n", C.CS_PLANE_LENGTHS)
@pytest.mark.parametrize("kind", C.CS_PLANES)
def test_colorize_stats_planes_and_focal_planes(kind, n, bsc):
    """a flat plane (one byte present, mx2 == 0), planes constant per wave span (the wave-uniform add) with and without one odd lane,
    bytes 0 and 255 only; every focal plane, -1 (no instance) among them; vector and scalar route"""
    for focal in C.CS_FOCALS:
        for v_off in (0, 1):
            _colorize_stats(kind, n, v_off, 0, focal, bsc, calls=1)


# =====================================================================================================================================
# 3. csm_bokeh_prep
# =====================================================================================================================================
def _bokeh_prep(n, d8, img, focal, lf, mis):
    check, f32, f64, i32, i64, ptr, sp = _a()
    L = _L()
    dm_want, stats = C.bokeh_plane_ref(d8, focal)
    dm = _Out(n, torch.float32, 1 if mis == 'dm' else 0)
    hi = _Out(3 * n, torch.float32, 1 if mis == 'hi' else 0)
    d8_d, img_d = _dev(d8, 1 if mis == 'd8' else 0), _dev(img, 1 if mis == 'img' else 0)
    assert d8_d.data_ptr() % 4 == (1 if mis == 'd8' else 0) and img_d.data_ptr() % 4 == (1 if mis == 'img' else 0)
    check(L.csm_bokeh_prep(ptr(d8_d), ptr(img_d), ptr(dm.view), ptr(hi.view), i64(n), f32(focal), ptr(_dev(np.array(stats, F32))), f32(lf), sp()),
          "bokeh_prep")
    assert C.same_bits(dm.take(), dm_want), (n, focal, lf, mis)
    plain = _Out(3 * n)
    check(L.csm_bokeh_highlight(ptr(_dev(img)), ptr(plain.view), i64(3 * n), f32(lf), sp()), "bokeh_highlight")
    got = hi.take()
    assert C.same_bits(got, plain.take()), (n, focal, lf, mis)
    ref, e32 = C.highlight_refs(img, lf)
    err = float(np.abs(got.astype(F64) - ref).max() / np.abs(ref).max())
    assert err <= C.yardstick(e32), (n, lf, err, e32)
    return stats


@pytest.mark.parametrize("n", C.BP_LENGTHS)
def test_bokeh_prep_depth_plane_and_highlights(n):
    """dm bit-equal to bokeh_depth_ref on the statistics of the reference (a single-valued plane gives mx2 == 0 and a NaN plane); hi
    bit-equal to csm_bokeh_highlight and within the yardstick of the float64 power; each of the four pointers misaligned in turn"""
    d8, img = C.byte_plane(n), C.byte_image(n)
    combos = list(zip(C.BP_LIGHTNESS, C.BP_FOCALS))
    for lf, focal in combos[:1] if n > 4099 else combos:
        stats = _bokeh_prep(n, d8, img, focal, lf, None)
        assert stats[2] > 0 or n == 1
    assert _bokeh_prep(n, C.byte_plane(n, True), img, 17.25, 10.0, None)[2] == 0.0
    if n <= 4099:
        for mis in C.BP_MISALIGNED:
            _bokeh_prep(n, d8, img, 17.25, 2.5, mis)


def test_new_entry_points_refuse_bad_arguments(bsc):
    check, f32, f64, i32, i64, ptr, sp = _a()
    L = _L()
    n = 257
    v, vmin, vmax = C.colorize_plane('noise', n)
    d, vmm, lut = _dev(v), _dev(np.array([vmin, vmax], F32)), _lut()
    out = _Out(n, torch.uint8)
    ok = [ptr(d), ptr(out.view), n, ptr(vmm), lut, ptr(bsc)]
    for i, bad in ((0, ptr(None)), (1, ptr(None)), (2, 0), (2, -5), (3, ptr(None)), (4, None), (5, ptr(None))):
        a = list(ok)
        a[i] = bad
        assert L.csm_colorize_stats(a[0], a[1], i64(a[2]), a[3], a[4], f32(17.25), a[5], sp()) == CSM_ERR_ARG, i
    d8, img = _dev(C.byte_plane(n)), _dev(C.byte_image(n))
    dm, hi, st = _Out(n), _Out(3 * n), _dev(np.array([255.0, 17.25, 230.5], F32))
    ok = [ptr(d8), ptr(img), ptr(dm.view), ptr(hi.view), n, ptr(st)]
    for i, bad in ((0, ptr(None)), (1, ptr(None)), (2, ptr(None)), (3, ptr(None)), (4, 0), (4, -1), (5, ptr(None))):
        a = list(ok)
        a[i] = bad
        assert L.csm_bokeh_prep(a[0], a[1], a[2], a[3], i64(a[4]), f32(17.25), a[5], f32(2.5), sp()) == CSM_ERR_ARG, i
    torch.cuda.synchronize()
    assert (out.take() == 0xA5).all() and np.isnan(dm.take()).all() and np.isnan(hi.take()).all() and not bool(bsc[12:].any())


# =====================================================================================================================================
# 4. csm_bokeh_depth_auto
# =====================================================================================================================================
@pytest.mark.parametrize("n", C.BDA_LENGTHS)
def test_bokeh_depth_auto_equals_the_reference(n):
    """k_u8_hist / k_bokeh_stats / k_bokeh_depth_dev: bit-equal to bokeh_depth_ref fed with bokeh_stats_ref; bytes 0 and 255 present,
    a single-valued plane (NaN), the 16-byte route, its tail and the byte route (pointer offset by 1); the per-block partial
    histograms are fully rewritten by every call, so the scratch starts as 0xFF bytes"""
    check, f32, f64, i32, i64, ptr, sp = _a()
    L = _L()
    scratch = torch.full((L.csm_bokeh_depth_scratch_bytes(),), 0xFF, dtype=torch.uint8, device='cuda')
    for single in (False, True):
        d8 = C.byte_plane(n, single)
        for off in (0, 1) if n <= C.BDA_OFFSET_MAX else (0,):
            d = _dev(d8, off)
            assert d.data_ptr() % 16 == off
            for focal in (-1.0, 17.25, 255.0) if not single else (100.0,):
                out = _Out(n)
                check(L.csm_bokeh_depth_auto(ptr(d), ptr(out.view), i64(n), f32(focal), ptr(scratch), sp()), "bokeh_depth_auto")
                want, stats = C.bokeh_plane_ref(d8, focal)
                assert C.same_bits(out.take(), want), (n, single, off, focal)
                assert C.same_bits(scratch[:12].cpu().numpy().view(F32), np.array(stats, F32))


# =====================================================================================================================================
# 5. csm_masked_u8_median_max
# =====================================================================================================================================
@pytest.mark.parametrize("n,n_inst", C.MM_CASES)
def test_masked_median_max_equals_numpy(n, n_inst):
    """every instance and the maximum; mask bytes 0 / 1 / 2 / 255; empty, single, even, odd, a .5 median, an all-255 selection; the
    histogram scratch pre-filled with 0xFF bytes (the call zeroes it); all-empty -> -1"""
    check, f32, f64, i32, i64, ptr, sp = _a()
    L = _L()
    d8, masks, kinds = C.masked_case(n, n_inst)
    dd = _dev(d8)
    for m in (masks, np.zeros((min(n_inst, 2), n), np.uint8)):
        k = m.shape[0]
        hist = torch.full((k * 256 + SLACK,), -1, dtype=torch.int32, device='cuda')
        out = _Out(k + 1)
        check(L.csm_masked_u8_median_max(ptr(dd), ptr(_dev(m)), i32(k), i64(n), ptr(hist), ptr(out.view), sp()), "masked_u8_median_max")
        got, want = out.take(), C.masked_median_ref(d8, m)
        assert C.same(got, want), (n, n_inst, kinds, got, want)
        assert bool((hist[k * 256:] == -1).all())
        cnt = hist[:k * 256].cpu().numpy().reshape(k, 256)
        assert np.array_equal(cnt, np.stack([np.bincount(d8[mk != 0], minlength=256) for mk in m]))
    assert want[-1] == -1.0


# =====================================================================================================================================
# 6. the fused frame at odd pixel counts
# =====================================================================================================================================
@pytest.mark.parametrize("name", [f[0] for f in C.FRAMES])
def test_fused_frame_equals_the_chain_of_single_calls(name):
    """csm_kenburns_frame through WarpFrame.frame_into, where the depth plane render + 3 * H * W is 16-byte aligned only when H * W is a
    multiple of 4 (the scalar routes of the select and of k_colorize_stats, the word tails of k_bokeh_prep) == the chain of single
    calls, each tested above, on ALIGNED copies of the call's own render[3] and warp output"""
    from cartoonsegmentation_amd import ops
    check, f32, f64, i32, i64, ptr, sp = _a()
    L = _L()
    c = C.frame_cloud(name)
    H, W = c['H'], c['W']
    P = H * W
    pts, rgb, dep = _dev(c['pts'][None]), _dev(c['rgb'][None]), _dev(c['depth'][None])
    ph, pw = max(1, int(0.9 * H)), max(1, int(0.93 * W))
    lut = _lut()
    PI = math.pi
    for dof in C.FRAME_DOFS:
        fp, ns, lf = dof
        wf = ops.WarpFrame(H, W, torch.device('cuda'), keep_render=True, path='tiled')
        got = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device='cuda')
        for call in (1, 2):                                  # the scratch re-arms itself
            wf.frame_into(got, pts, rgb, dep, c['focal'], c['baseline'], list(c['shift']), ph, pw, W / 2.0, H / 2.0, dof)
        torch.cuda.synchronize()
        assert wf.render.data_ptr() % 16 == 0                # so its fourth plane is 16-byte aligned exactly when P % 4 == 0
        rdepth, frame = wf.render[0, 3].clone().reshape(-1), wf.frame.clone()
        assert rdepth.data_ptr() % 16 == 0 and frame.data_ptr() % 16 == 0
        vmm, sel = _Out(2), torch.zeros(L.csm_percentile_scratch_bytes(), dtype=torch.uint8, device='cuda')
        bsc = torch.zeros(L.csm_bokeh_depth_scratch_bytes(), dtype=torch.uint8, device='cuda')
        d8, dm, hi = _Out(P, torch.uint8), _Out(P), _Out(3 * P)
        pa, pb, blurred = _Out(3 * P), _Out(3 * P), _Out(3 * P, torch.uint8)
        want = _Out(3 * P, torch.uint8)
        check(L.csm_percentile_pair(ptr(rdepth), i64(P), f64(2.0), f64(85.0), ptr(vmm.view), ptr(sel), sp()), "percentile_pair")
        check(L.csm_colorize_stats(ptr(rdepth), ptr(d8.view), i64(P), ptr(vmm.view), lut, f32(fp), ptr(bsc), sp()), "colorize_stats")
        check(L.csm_bokeh_prep(ptr(d8.view), ptr(frame), ptr(dm.view), ptr(hi.view), i64(P), f32(fp), ptr(bsc), f32(lf), sp()), "bokeh_prep")
        check(L.csm_bokeh_pass(ptr(hi.view), ptr(dm.view), ptr(pa.view), i32(H), i32(W), i32(ns), f32(0.0), f32(1.0), sp()), "bokeh_pass")
        check(L.csm_bokeh_pass(ptr(pa.view), ptr(dm.view), ptr(pb.view), i32(H), i32(W), i32(ns), f32(math.cos(-PI / 6)), f32(math.sin(-PI / 6)),
                               sp()), "bokeh_pass")
        check(L.csm_bokeh_pass_finish(ptr(pb.view), ptr(dm.view), ptr(blurred.view), i32(H), i32(W), i32(ns), f32(math.cos(-PI * 5 / 6)),
                                      f32(math.sin(-PI * 5 / 6)), f32(lf), sp()), "bokeh_pass_finish")
        check(L.csm_crop_resize_u8(ptr(blurred.view), i32(H), i32(W), i32(ph), i32(pw), f32(W / 2.0), f32(H / 2.0), ptr(want.view), sp()),
              "crop_resize_u8")
        w = want.take().reshape(H, W, 3)
        g = got.cpu().numpy()
        assert np.array_equal(g, w), (name, dof, int((g != w).sum()))
        # the links of the chain against the references, on this frame's own planes
        r = rdepth.cpu().numpy()
        lo, hi_ = C.percentile_ref(r, 2.0), C.percentile_ref(r, 85.0)
        assert C.same(vmm.take(), np.array([lo, hi_], F32))
        b = C.colorize_ref(r, lo, hi_)
        assert np.array_equal(d8.take(), b)
        plane, stats = C.bokeh_plane_ref(b, fp)
        assert C.same_bits(bsc[:12].cpu().numpy().view(F32), np.array(stats, F32)) and C.same_bits(dm.take(), plane)
        assert len(np.unique(w)) > 8                         # a picture, not a constant
