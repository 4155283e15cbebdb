"""GPU: the batched depth glue (csrc/frameglue.hip: csm_frame_glue_batch, csm_leres_post_batch) called through the C ABI, BITWISE
against today's single-frame entry points called frame by frame (both compile csrc/csm_glue.h), and the batched configuration
against per-frame _config_from.  No nets run.  The glue frames are 258 x 259 and 301 x 262: the [128:-128, 128:-128] crop needs
sides > 256, so these are the smallest shapes at which it exists (odd W; H * W no multiple of 4, so the block outputs are padded)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
FOCAL, BASE, EPS = 130.0, 40.0, 0.00001


def _abi():
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import check, f32, f64, i32, i64, ptr, stream_ptr
    return _lib.load(), check, f32, f64, i32, i64, ptr, stream_ptr


def _bits(t):
    """bit pattern of a float tensor (NaN-safe equality)"""
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _disparity(kind, H, W, rng):
    """kind 0: exact zeros in a random plane; 1: a constant plane (min == max, every location ties); 2: the extremes sit on the
    border of the [128:-128, 128:-128] crop (first row / last pixel); 3: a plain random plane; 4: 100 + uniform noise of +-1, whose
    Laplacian over the maximum is spread densely around the +-0.03 threshold of `valid` (the only way the Laplacian reaches an output)"""
    if kind == 1:
        return np.full((H, W), 37.0, F32)
    if kind == 4:
        return (100.0 + rng.uniform(-1, 1, (H, W))).astype(F32)
    d = np.floor(rng.uniform(1, 200, (H, W))).astype(F32) + F32(0.25)
    if kind == 0:
        d[rng.uniform(size=d.shape) < 0.1] = 0
    elif kind == 2:
        d[128, 128 + (W - 256) // 2] = 250.0           # largest disparity = smallest depth, on the crop's first row
        d[H - 129, W - 129] = 0.5                      # smallest disparity = largest depth, on the crop's last pixel
    return d


def _masks(n, k, H, W):
    """n == 3: an all-zero mask (adjustment skipped), a mask that touches the last row, and one that overlaps it (order matters);
    n == 1: one box that moves with the frame index"""
    m = np.zeros((n, H, W), np.bool_)
    if n == 3:
        m[1, 100:H, 40:200] = True
        m[2, 60:180, 120:250] = True
    elif n == 1:
        m[0, 20 + 3 * k:150 + 2 * k, 30 + k:140 + 5 * k] = True
    return m


def _glue_inputs(B, H, W):
    rng = np.random.default_rng(1000 * B + H)
    frames, coarse, masks = [], [], []
    for k in range(B):
        frames.append(torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda())
        coarse.append(torch.from_numpy(_disparity((k + B) % 5, H, W, rng)).cuda().view(1, 1, H, W))
        n = (3, 0, 1)[k % 3]                          # ragged instance counts
        masks.append(torch.from_numpy(_masks(n, k, H, W)).cuda().view(torch.uint8) if n else None)
    return frames, coarse, masks


def _glue_per_frame(frame, coarse, masks, H, W):
    """today's single-frame entry points in the order of _config_from / _finish_config"""
    L, check, f32, f64, i32, i64, ptr, sp = _abi()
    n, dev = H * W, frame.device
    img = torch.empty((1, 3, H, W), device=dev)
    check(L.csm_u8_hwc_to_f32_chw(ptr(frame), i32(H), i32(W), ptr(img), sp()))
    raw = coarse
    if masks is not None:
        raw = coarse.clone()
        sc = torch.empty(2 * H + 2, device=dev)
        for j in range(masks.shape[0]):
            check(L.csm_depth_adjust_instance(ptr(raw), ptr(masks[j]), i32(H), i32(W), ptr(sc), sp()))
    mm, nmax, part = torch.empty(2, device=dev), torch.empty(1, device=dev), torch.empty(512, device=dev)
    check(L.csm_minmax(ptr(raw), i64(n), ptr(mm), ptr(part), sp()))
    disp = torch.empty_like(raw)
    check(L.csm_normalise_disparity(ptr(raw), i64(n), ptr(mm), f32(BASE), ptr(disp), ptr(nmax), sp()))
    depth, valid = torch.empty_like(disp), torch.empty_like(disp)
    pts, un = torch.empty((1, 3, H, W), device=dev), torch.empty((1, 3, H, W), device=dev)
    check(L.csm_disparity_to_points(ptr(disp), ptr(nmax), i32(H), i32(W), f64(FOCAL), f64(BASE), f32(EPS), ptr(depth), ptr(valid), ptr(pts),
                                    ptr(un), sp()))
    keys, out6 = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(6, dtype=torch.float64, device=dev)
    check(L.csm_depth_range_stats(ptr(mm), f32(BASE), ptr(depth), i32(H), i32(W), i32(128), i32(128), i32(H - 256), i32(W - 256), ptr(keys),
                                  ptr(out6), sp()))
    return {'image': img, 'disparity': disp, 'depth': depth, 'valid': valid, 'points': pts, 'unaltered': un, 'nmax': nmax, 'stats': out6}


# ---- csm_frame_glue_batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("H,W", [(258, 259), (301, 262)])
def test_frame_glue_batch_is_the_per_frame_path_bit_for_bit(H, W, B):
    L, check, f32, f64, i32, i64, ptr, sp = _abi()
    frames, coarse, masks = _glue_inputs(B, H, W)
    n = H * W
    s1, s3 = (n + 3) & ~3, (3 * n + 3) & ~3
    nan = float('nan')
    blk = {k: torch.full((B, s3 if k in ('image', 'points', 'unaltered') else s1), nan, device='cuda')
           for k in ('image', 'disparity', 'depth', 'valid', 'points', 'unaltered')}
    nmax = torch.full((B,), nan, device='cuda')
    stats = torch.full((B, 6), nan, dtype=torch.float64, device='cuda')
    scratch = torch.empty(L.csm_frame_glue_scratch_bytes(i32(B), i32(H), i32(W)), dtype=torch.uint8, device='cuda')
    VP = ctypes.c_void_p * B
    counts = [0 if m is None else int(m.shape[0]) for m in masks]
    check(L.csm_frame_glue_batch(i32(B), i32(H), i32(W), VP(*[f.data_ptr() for f in frames]), VP(*[c.data_ptr() for c in coarse]),
                                 VP(*[None if m is None else m.data_ptr() for m in masks]), (ctypes.c_int * B)(*counts), f64(FOCAL), f64(BASE),
                                 f32(EPS), ptr(blk['image']), ptr(blk['disparity']), ptr(blk['depth']), ptr(blk['valid']), ptr(blk['points']),
                                 ptr(blk['unaltered']), i64(s1), i64(s3), ptr(nmax), ptr(stats), ptr(scratch), sp()), "frame_glue_batch")
    kinds = set()
    for k in range(B):
        ref = _glue_per_frame(frames[k], coarse[k], masks[k], H, W)
        for name, t in blk.items():
            ln = 3 * n if t.shape[1] == s3 else n
            assert _same(t[k, :ln], ref[name].reshape(-1)), (name, k)
            assert bool(torch.isnan(t[k, ln:]).all()), ("written into the padding", name, k)
        assert _same(nmax[k:k + 1], ref['nmax']), k
        assert _same(stats[k], ref['stats']), (k, stats[k].tolist(), ref['stats'].tolist())
        kinds.add((k + B) % 5)
    if B == 17:
        assert kinds == {0, 1, 2, 3, 4} and set(counts) == {0, 1, 3}
        # what the cases exist for: a constant plane ties everywhere (first position wins), the border extremes are found
        for k in range(B):
            cw = W - 256
            if (k + B) % 5 == 1:
                assert stats[k, 4].item() == 0.0 and stats[k, 5].item() == 0.0
            if (k + B) % 5 == 2 and masks[k] is None:
                assert int(stats[k, 4].item()) == (W - 256) // 2 and int(stats[k, 5].item()) == (H - 257) * cw + cw - 1
            if (k + B) % 5 == 4 and masks[k] is None:                         # both sides of the Laplacian threshold are populated
                assert 0.2 < float(blk['valid'][k, :n].mean().item()) < 0.8


def test_frame_glue_batch_refuses_bad_arguments():
    L, check, f32, f64, i32, i64, ptr, sp = _abi()
    one = (ctypes.c_void_p * 1)(8)
    cnt = (ctypes.c_int * 1)(0)
    t = torch.empty(64, device='cuda')
    for H, W in ((256, 300), (300, 256)):                                    # no crop
        assert L.csm_frame_glue_batch(i32(1), i32(H), i32(W), one, one, one, cnt, f64(FOCAL), f64(BASE), f32(EPS), ptr(t), ptr(t), ptr(t), ptr(t),
                                      ptr(t), ptr(t), i64(H * W), i64(3 * H * W), ptr(t), ptr(t), ptr(t), sp()) == 1
    assert L.csm_frame_glue_batch(i32(1), i32(300), i32(300), one, one, one, cnt, f64(FOCAL), f64(BASE), f32(EPS), ptr(t), ptr(t), ptr(t), ptr(t),
                                  ptr(t), ptr(t), i64(300 * 300 - 1), i64(3 * 300 * 300), ptr(t), ptr(t), ptr(t), sp()) == 1      # stride < plane


# ---- csm_leres_post_batch ---------------------------------------------------------------------------------------------------------
def _net_output(kind, h, w, rng):
    """kind 0: all zero; 1: constant; 2: a mix with exact zeros and a plateau of maxima (which quantise to the zeros the fix rewrites)"""
    if kind == 0:
        return np.zeros((h, w), F32)
    if kind == 1:
        return np.full((h, w), 3.5, F32)
    y = rng.normal(0, 2, (h, w)).astype(F32)
    y[rng.uniform(size=y.shape) < 0.1] = 0
    y[h // 3:h // 3 + 4, w // 4:w // 4 + 9] = 9.0
    return y


def _leres_post_per_frame(y, h, w, H, W):
    L, check, f32, f64, i32, i64, ptr, sp = _abi()
    dev = y.device
    mm, part = torch.empty(2, device=dev), torch.empty(512, device=dev)
    check(L.csm_minmax(ptr(y), i64(h * w), ptr(mm), ptr(part), sp()))
    q = torch.empty((h, w), dtype=torch.uint8, device=dev)
    check(L.csm_leres_quantize(ptr(y), i64(h * w), ptr(mm), ptr(q), sp()))
    depth = torch.empty((H, W), device=dev)
    if h / H > 1:
        check(L.csm_resize_u8_lanczos4_to_f32(ptr(q), i32(h), i32(w), i32(H), i32(W), ptr(depth), sp()))
    else:
        check(L.csm_resize_u8_to_f32(ptr(q), i32(h), i32(w), i32(H), i32(W), ptr(depth), sp()))
    st = torch.empty(2, dtype=torch.int32, device=dev)
    check(L.csm_fill_zero_min_positive(ptr(depth), i64(H * W), ptr(st), sp()))
    return depth


@pytest.mark.parametrize("kinds", [(0,), (1,), (2,), (2, 0, 1)])
@pytest.mark.parametrize("h,w,H,W", [(32, 64, 32, 64), (32, 64, 40, 80), (64, 96, 60, 90)])       # same size, area route, Lanczos route
def test_leres_post_batch_is_the_per_frame_path_bit_for_bit(h, w, H, W, kinds):
    L, check, f32, f64, i32, i64, ptr, sp = _abi()
    B = len(kinds)
    rng = np.random.default_rng(7 * h + H + B)
    y = torch.from_numpy(np.stack([_net_output(k, h, w, rng) for k in kinds])).cuda().view(B, 1, h, w)
    stride = H * W + 4                                                          # padded frames: the padding stays untouched
    out = torch.full((B, stride), float('nan'), device='cuda')
    scratch = torch.empty(L.csm_leres_post_scratch_bytes(i32(B), i32(h), i32(w)), dtype=torch.uint8, device='cuda')
    check(L.csm_leres_post_batch(ptr(y), i32(B), i32(h), i32(w), i32(H), i32(W), ptr(out), i64(stride), ptr(scratch), sp()), "leres_post_batch")
    for k in range(B):
        ref = _leres_post_per_frame(y[k], h, w, H, W)
        assert _same(out[k, :H * W], ref.reshape(-1)), (k, kinds[k])
        assert bool(torch.isnan(out[k, H * W:]).all()), k
        if kinds[k] == 2:
            assert float(ref.min().item()) > 0.0                                # the plateau's zeros were rewritten
    from cartoonsegmentation_amd import ops
    views = ops.leres_post_batch(y, H, W)                                       # the Python entry: views [1,1,H,W] of one block
    assert all(v.shape == (1, 1, H, W) and v.is_contiguous() and v.data_ptr() % 16 == 0 for v in views)
    assert all(_same(v.reshape(-1), out[k, :H * W]) for k, v in enumerate(views))


# ---- generate_kenburns_configs' batched glue against per-frame _config_from -------------------------------------------------------
def test_batched_configs_are_the_per_frame_configs():
    from cartoonsegmentation_amd.anime_instances import AnimeInstances
    from cartoonsegmentation_amd.kenburns import KenBurnsConfig, KenBurnsPipeline
    H, W, B = 258, 259, 3

    class _Upload:
        @staticmethod
        def _upload(img):
            return img.contiguous()
    pipe = KenBurnsPipeline.__new__(KenBurnsPipeline)                           # the glue only: no detector, no depth net
    pipe.cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', refine_crf=False, focal=FOCAL, baseline=BASE)
    pipe.device, pipe.animeinsseg = torch.device('cuda', torch.cuda.current_device()), _Upload()
    frames, coarse, masks = _glue_inputs(B, H, W)

    def instances():
        out = []
        for m in masks:
            if m is None:
                out.append(AnimeInstances())
            else:
                n = int(m.shape[0])
                out.append(AnimeInstances(masks=m.view(torch.bool).clone(), bboxes=torch.tensor([[1, 2, 30, 40]] * n, device='cuda'),
                                          scores=torch.ones(n, device='cuda')))
        return out
    assert pipe._glue_batchable(frames, coarse, False) and not pipe._glue_batchable(frames, coarse, True)
    batched = pipe._configs_batched(frames, instances(), coarse, frames)
    for k, (kb, inst) in enumerate(zip(batched, instances())):
        ks = pipe._config_from(frames[k], inst, coarse[k], False, frame_dev=frames[k])
        for name in ('tenRawImage', 'tenRawDisparity', 'tenRawDepth', 'tenRawPoints', 'tenRawUnaltered', 'tenInpaDisparity', 'tenInpaDepth',
                     'tenInpaPoints'):
            a, b = kb[name], ks[name]
            assert a.shape == b.shape and a.is_contiguous() and _same(a, b), (name, k)
        assert _same(kb.inpainted_img, ks.inpainted_img) and kb.inpainted_img.shape == (1, 3, H * W)
        assert kb['objDepthrange'] == ks['objDepthrange'] and (kb['fltDispmin'], kb['fltDispmax']) == (ks['fltDispmin'], ks['fltDispmax'])
        assert (kb.int_height, kb.int_width) == (H, W) and kb.original_img_nparray is frames[k]
        assert len(kb.instances) == len(ks.instances)
        if len(kb.instances):
            assert torch.equal(kb.instances.masks, ks.instances.masks)
