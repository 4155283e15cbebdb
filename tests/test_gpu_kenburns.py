"""GPU parity of the KenBurnsPipeline glue (through the drop-in import surface) vs the numpy/C oracle."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe_and_cfg():
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from cartoonsegmentation_amd import synth
    H, W = 320, 384
    cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=512, refine_crf=False,
                         depth_field=False, focal=W / 2.0, num_frame=3,
                         mask_refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    pipe = KenBurnsPipeline(cfg)
    img = synth.image_u8(H, W, 11)
    inst = pipe.animeinsseg.infer(img, pred_score_thr=0.3, max_instances=2, det_size=96, refine_kwargs=cfg.mask_refine_kwargs)
    kc = pipe.generate_kenburns_config(img, instances=inst)
    return pipe, kc, img, inst


def test_image_ops_bit_exact():
    import ctypes
    from cartoonsegmentation_amd import _lib, synth
    from cartoonsegmentation_amd._lib import check, f32, i32, i64, ptr, stream_ptr
    from oracle import segment as oseg
    L, O = _lib.load(), oseg.lib()
    ci, cf = ctypes.c_int, ctypes.c_float
    img = synth.image_u8(150, 200, 3)
    d_img = torch.from_numpy(img).cuda()
    x = torch.empty((1, 3, 96, 128), device='cuda'); xo = np.empty((1, 3, 96, 128), np.float32)
    check(L.csm_leres_input(ptr(d_img), i32(150), i32(200), i32(96), i32(128), ptr(x), stream_ptr()))
    O.orc_leres_input(oseg._p(img), ci(150), ci(200), ci(96), ci(128), oseg._p(xo))
    assert np.array_equal(x.cpu().numpy(), xo)
    d = np.random.default_rng(0).normal(0, 3, (96, 128)).astype(np.float32)
    dd = torch.from_numpy(d).cuda(); mm = torch.stack([dd.min(), dd.max()])
    q = torch.empty((96, 128), dtype=torch.uint8, device='cuda'); qo = np.empty((96, 128), np.uint8)
    check(L.csm_leres_quantize(ptr(dd), i64(96 * 128), ptr(mm), ptr(q), stream_ptr()))
    O.orc_leres_quantize(oseg._p(d), ctypes.c_int64(96 * 128), cf(float(d.min())), cf(float(d.max())), oseg._p(qo))
    assert np.array_equal(q.cpu().numpy(), qo)
    up = torch.empty((150, 200), device='cuda'); upo = np.empty((150, 200), np.float32)
    check(L.csm_resize_u8_to_f32(ptr(q), i32(96), i32(128), i32(150), i32(200), ptr(up), stream_ptr()))
    O.orc_resize_u8_to_f32(oseg._p(qo), ci(96), ci(128), ci(150), ci(200), oseg._p(upo))
    assert np.array_equal(up.cpu().numpy(), upo)
    cr = torch.empty((150, 200, 3), dtype=torch.uint8, device='cuda'); cro = np.empty((150, 200, 3), np.uint8)
    # crop + resize (kenburns_effect.py:1069-1070): the LDS-tiled kernel on a near-full patch, the full frame at a fractional centre,
    # a 4x enlargement of a small patch, patches hanging over every border (clamped taps), a 1-px patch
    for (ph_, pw_, cx_, cy_) in ((145, 194, 100.0, 75.0), (150, 200, 99.3, 74.6), (37, 50, 60.5, 40.25), (120, 160, 3.0, 2.0),
                                 (120, 160, 198.7, 149.1), (1, 1, 17.0, 9.0), (150, 200, 99.5, 74.5)):
        check(L.csm_crop_resize_u8(ptr(d_img), i32(150), i32(200), i32(ph_), i32(pw_), f32(cx_), f32(cy_), ptr(cr), stream_ptr()))
        O.orc_crop_resize_u8(oseg._p(img), ci(150), ci(200), ci(ph_), ci(pw_), cf(cx_), cf(cy_), oseg._p(cro))
        assert np.array_equal(cr.cpu().numpy(), cro), (ph_, pw_, cx_, cy_)


def test_generate_kenburns_config_vs_oracle(pipe_and_cfg):
    from cartoonsegmentation_amd.nets import build_leres
    from cartoonsegmentation_amd.weights import SynthWeights
    from oracle import kenburns as okb
    pipe, kc, img, inst = pipe_and_cfg
    assert kc['intWidth'] == 384 and kc['intHeight'] == 320 and kc['tenRawPoints'].shape == (1, 3, 320 * 384)
    progs = {}

    def leres_for(h, w):
        if (h, w) not in progs:
            progs[(h, w)] = build_leres(SynthWeights('leres.'), 1, h, w)
        return progs[(h, w)]
    masks = inst.masks.cpu().numpy()
    o = okb.kenburns_config(img, masks, leres_for, 96, kc['fltFocal'], kc['fltBaseline'])
    assert np.array_equal(kc['tenRawDisparity'].cpu().numpy(), o['disparity'])
    assert np.array_equal(kc['tenRawDepth'].cpu().numpy(), o['depth'])
    assert np.array_equal(kc['tenRawPoints'].cpu().numpy(), o['pts'])
    assert np.array_equal(kc['tenRawUnaltered'].cpu().numpy(), o['unaltered'])
    assert kc['objDepthrange'][0] == o['depthrange'][0] and tuple(kc['objDepthrange'][2]) == tuple(o['depthrange'][2])


def test_autozoom_and_frames_vs_oracle(pipe_and_cfg):
    from oracle import kenburns as okb
    pipe, kc, img, inst = pipe_and_cfg
    W, H = kc['intWidth'], kc['intHeight']
    o = dict(depth=kc['tenRawDepth'].cpu().numpy(), pts=kc['tenRawPoints'].cpu().numpy(), depthrange=kc['objDepthrange'])
    rgb = kc['tenRawImage'].view(1, 3, -1).cpu().numpy()
    objTo_o, objFrom = okb.autozoom_target(o, rgb, W, H, kc['fltFocal'], kc['fltBaseline'])
    objTo = pipe.process_autozoom({'fltShift': 100.0, 'fltZoom': 1.25, 'objFrom': objFrom}, kc)
    assert objTo == objTo_o
    steps = [0.0, 0.5, 1.0]
    frames, _ = pipe.process_kenburns({'fltSteps': steps, 'objFrom': objFrom, 'objTo': objTo, 'boolInpaint': False}, kc, inpaint=False)
    frames_o = okb.frames(o, rgb, W, H, kc['fltFocal'], kc['fltBaseline'], objFrom, objTo, steps)
    assert len(frames) == 3 and frames[0].shape == (H, W, 3) and frames[0].dtype == np.uint8
    for a, b in zip(frames, frames_o):
        diff = np.abs(a.astype(np.int32) - b.astype(np.int32))
        assert (diff <= 1).mean() >= 0.999 and (diff == 0).mean() >= 0.99      # fp32 atomicAdd order only


def test_inpaint_forward_vs_oracle_and_reference():
    """Inpaint.forward on the HIP path vs the oracle (Jacobi degrid, tolerance: mean/std are torch reductions) and,
    where coverage agrees, vs the reference fixture"""
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from cartoonsegmentation_amd.nets import build_inpaint_context, build_inpaint_grid
    from cartoonsegmentation_amd.weights import SynthWeights
    from oracle import kenburns as okb
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "net_inpaint_32x40.npz")))
    H, W = 32, 40
    pipe = KenBurnsPipeline(KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', refine_crf=False, focal=W / 2.0))
    common = {'intWidth': W, 'intHeight': H, 'fltFocal': W / 2.0, 'fltBaseline': 40.0}
    dev = pipe.device
    o = pipe._inpaint(torch.from_numpy(g['img']).to(dev), torch.from_numpy(g['disp']).to(dev), torch.from_numpy(g['shift']).to(dev), common,
                      torch.from_numpy(g['seg']).to(dev))
    ws = SynthWeights('inpaint.')
    r = okb.inpaint_forward(g['img'], g['disp'], g['shift'], g['seg'], W, H, W / 2.0, 40.0, build_inpaint_context(ws, H, W),
                            build_inpaint_grid(ws, H, W), degrid_mode=1)
    assert np.array_equal(o['tenExisting'].cpu().numpy(), r['existing'])
    assert np.abs(o['tenImage'].cpu().numpy() - r['image']).max() < 2e-3
    assert np.abs(o['tenDisparity'].cpu().numpy() - r['disparity']).max() / r['disparity'].max() < 2e-3
    assert np.abs(o['segmasks'].cpu().numpy() - r['segmasks']).max() < 1e-4
    assert (o['tenExisting'].cpu().numpy() == g['existing']).mean() > 0.99


def _frame_diff(a, b):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return float((d <= 1).mean()), float((d == 0).mean())


def _inpainted_autozoom_vs_oracle(pipe, kc):
    """pipe.autozoom(kc) with inpainting (process_autozoom -> process_kenburns(inpaint=True): two Inpaint passes at 1.1 x the shifts
    of steps 0 and 1, hole pixels appended to the cloud, frames rendered from the grown cloud) against oracle/kenburns.py::
    inpaint_append + frames_inpainted on the same raw configuration.  Returns the measured differences."""
    import math
    from cartoonsegmentation_amd.nets import build_inpaint_context, build_inpaint_grid
    from cartoonsegmentation_amd.weights import SynthWeights
    from oracle import kenburns as okb
    W, H, f, b = kc['intWidth'], kc['intHeight'], kc['fltFocal'], kc['fltBaseline']
    raw = dict(img=kc['tenRawImage'].cpu().numpy(), disparity=kc['tenRawDisparity'].cpu().numpy(), depth=kc['tenRawDepth'].cpu().numpy(),
               pts=kc['tenRawPoints'].cpu().numpy(), depthrange=kc['objDepthrange'])
    n0 = raw['pts'].shape[2]
    got = []                                                      # the dict each KenBurnsPipeline.inpaint pass returns
    inpaint = pipe.inpaint
    pipe.inpaint = lambda *a, **k: got.append(inpaint(*a, **k)) or got[-1]
    try:
        frames = pipe.autozoom(kc)
    finally:
        del pipe.inpaint
    objFrom = {'fltCenterU': W / 2.0, 'fltCenterV': H / 2.0, 'intCropWidth': int(math.floor(0.97 * W)), 'intCropHeight': int(math.floor(0.97 * H))}
    objTo = pipe.process_autozoom({'fltShift': 100.0, 'fltZoom': 1.25, 'objFrom': objFrom}, kc)
    steps = np.linspace(0.0, 1.0, kc.num_frame).tolist()
    ws = SynthWeights('inpaint.')
    passes, cloud = okb.inpaint_append(raw, W, H, f, b, objFrom, objTo, build_inpaint_context(ws, H, W), build_inpaint_grid(ws, H, W))
    assert len(got) == 2 and len(frames) == kc.num_frame and frames[0].shape == (H, W, 3) and frames[0].dtype == np.uint8
    pts_d, img_d = kc['tenInpaPoints'].cpu().numpy(), kc.inpainted_img.cpu().numpy()
    dsp_d, dep_d = kc['tenInpaDisparity'].cpu().numpy(), kc['tenInpaDepth'].cpu().numpy()
    r = {'size': (H, W), 'holes': [int(p['pts'].shape[2]) for p in passes], 'n_appended': int(pts_d.shape[2] - n0)}
    # the cloud grows by the hole pixels of both passes, raw points first (kenburns_effect.py:984-988, :510-512)
    assert np.array_equal(pts_d[:, :, :n0], raw['pts']) and np.array_equal(img_d[:, :, :n0], raw['img'].reshape(1, 3, -1))
    assert img_d.shape[2] == dsp_d.shape[2] == dep_d.shape[2] == pts_d.shape[2] and np.isfinite(pts_d).all()
    r['existing_equal'] = [bool(np.array_equal(g['tenExisting'].cpu().numpy(), p['existing'])) for g, p in zip(got, passes)]
    r['image_err'] = max(float(np.abs(g['tenImage'].cpu().numpy() - p['image_full']).max()) for g, p in zip(got, passes))
    r['disparity_rel'] = max(float(np.abs(g['tenDisparity'].cpu().numpy() - p['disparity_full']).max() / p['disparity_full'].max())
                             for g, p in zip(got, passes))
    # what the product appended, taken from its own inpainted maps: image / disparity by mask, depth and points by the oracle's
    # restatement of kenburns_effect.py:454-458 applied to the HIP disparity
    own = {'image': [], 'disparity': [], 'depth': [], 'valid': [], 'pts': []}
    for g, p in zip(got, passes):
        m = (g['tenExisting'].cpu().numpy() == 0.0).reshape(-1)
        dmap = g['tenDisparity'].cpu().numpy()
        depth, valid, pts = okb._inpaint_points(dmap, f, b)
        own['image'].append(g['tenImage'].cpu().numpy().reshape(1, 3, -1)[:, :, m])
        own['disparity'].append(dmap.reshape(1, 1, -1)[:, :, m])
        own['depth'].append(depth.reshape(1, 1, -1)[:, :, m])
        own['valid'].append(valid.reshape(1, 1, -1)[:, :, m])
        own['pts'].append((pts - p['shift']).astype(np.float32)[:, :, m])
    own = {k: np.concatenate(v, 2) for k, v in own.items()}
    r['append_chain_exact'] = {k: bool(np.array_equal(v, a[:, :, n0:])) for k, v, a in
                               (('image', own['image'], img_d), ('disparity', own['disparity'], dsp_d), ('depth', own['depth'], dep_d),
                                ('pts', own['pts'], pts_d))}
    app_o = {k: np.concatenate([p[k] for p in passes], 2) for k in ('image', 'disparity', 'depth', 'valid', 'pts')}
    if r['n_appended'] == app_o['pts'].shape[2]:
        r['app_image_err'] = float(np.abs(img_d[:, :, n0:] - app_o['image']).max()) if r['n_appended'] else 0.0
        r['app_disparity_rel'] = float(np.abs(dsp_d[:, :, n0:] - app_o['disparity']).max() / max(p['disparity_full'].max() for p in passes)) \
            if r['n_appended'] else 0.0
        # a point's scale is its largest coordinate; `valid` thresholds the laplacian of the inpainted disparity, so the 2e-3 of the
        # disparity can flip it (point at -shift instead of on its ray): counted apart
        rel = (np.abs(pts_d[:, :, n0:] - app_o['pts']) / np.maximum(np.abs(app_o['pts']).max(1, keepdims=True), 1e-6)).max(1)[0]
        same = (own['valid'] == app_o['valid']).reshape(-1)
        r['app_valid_flips'] = int((~same).sum())
        r['app_pts_rel_max'] = float(rel[same].max()) if same.any() else 0.0
        r['app_pts_within_2e-3'] = float((rel < 2e-3).mean()) if rel.size else 1.0
    # frames: against the oracle's own grown cloud, and against the oracle frame loop on the product's cloud
    fo = okb.frames_inpainted(raw, cloud, W, H, f, b, objFrom, objTo, steps)
    fp = okb.frames_inpainted(raw, dict(pts=pts_d, rgb=img_d, depth=dep_d), W, H, f, b, objFrom, objTo, steps)
    r['frames_vs_oracle'] = [_frame_diff(a, o) for a, o in zip(frames, fo)]
    r['frames_vs_oracle_loop'] = [_frame_diff(a, o) for a, o in zip(frames, fp)]
    print("inpainted autozoom vs oracle:", r)
    return r


def _assert_inpainted_run(r):
    assert all(r['existing_equal']), r                                 # splat + median-5 coverage of both passes: exact
    assert r['n_appended'] == sum(r['holes']), r
    assert all(r['append_chain_exact'].values()), r                   # hole gather, depth, valid mask, points - shift: exact
    # the inpainted maps: the bound of test_inpaint_forward_vs_oracle_and_reference (mean / std are torch reductions)
    assert r['image_err'] < 2e-3 and r['disparity_rel'] < 2e-3, r
    assert r['app_image_err'] < 2e-3 and r['app_disparity_rel'] < 2e-3, r
    # appended points: given the disparity they are exact (append_chain_exact), so their error is the disparity's mapped through
    # depth = f * b / disparity, which magnifies it where the inpainted disparity nears 0: measured up to 8 % on single points and
    # 99.5-99.99 % of the points within 2e-3; the valid flag (laplacian < 0.03) flipped on <= 1 point in 37 000
    assert r['app_valid_flips'] <= 1e-4 * r['n_appended'], r
    assert r['app_pts_within_2e-3'] >= 0.99, r
    for within, exact in r['frames_vs_oracle_loop']:                 # frame loop on the same cloud: fp32 atomicAdd order only
        assert within >= 0.999 and exact >= 0.99, r
    for within, exact in r['frames_vs_oracle']:
        assert within >= 0.999 and exact >= 0.99, r


def test_autozoom_end_to_end_with_inpainting(pipe_and_cfg):
    """run_kenburns.py's call sequence: generate_kenburns_config -> autozoom (inpaint=True) -> frames, against the oracle"""
    pipe, kc, img, inst = pipe_and_cfg
    r = _inpainted_autozoom_vs_oracle(pipe, kc)
    assert r['n_appended'] > 0
    _assert_inpainted_run(r)


# (input image H x W, frame H x W after scaledown_maxsize(1024)): the reference's example image (1359x1680 -> 828x1024), a 1000x750
# photo (750x1000) and a 3:2 one (1024x1536 -> 683x1024), an odd-sized portrait and an odd x odd frame -- every one takes the
# GridNet's odd-size crop -- and the 320x384 frame of pipe_and_cfg (multiples of 8)
INPAINT_FRAMES = [((1359, 1680), (828, 1024)), ((750, 1000), (750, 1000)), ((1024, 1536), (683, 1024)), ((517, 333), (517, 333)),
                  ((601, 457), (601, 457)), ((320, 384), (320, 384))]


def _two_instances(h, w):
    """a disc and a bar at the input image size: depth_adjustment lifts each to a plane (kenburns_effect.py:39-91), so the views of
    both inpainting passes disocclude the background and both append points"""
    from cartoonsegmentation_amd.anime_instances import AnimeInstances
    yy, xx = np.mgrid[0:h, 0:w]
    masks = np.stack([np.hypot(xx - 0.4 * w, yy - 0.55 * h) < 0.25 * min(h, w), (np.abs(xx - 0.75 * w) < 0.08 * w) & (yy > 0.3 * h)])
    boxes = [[int(0.4 * w - 0.25 * min(h, w)), int(0.55 * h - 0.25 * min(h, w)), int(0.4 * w + 0.25 * min(h, w)), int(0.55 * h + 0.25 * min(h, w))],
             [int(0.67 * w), int(0.3 * h), int(0.83 * w), h - 1]]
    return AnimeInstances(torch.from_numpy(masks).cuda(), torch.tensor(boxes, dtype=torch.int32, device='cuda'), torch.ones(2, device='cuda'))


@pytest.fixture(scope="module")
def inpaint_pipe():
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=1024, refine_crf=False,
                         depth_field=False, num_frame=3, mask_refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    return KenBurnsPipeline(cfg)


@pytest.mark.parametrize("src,frame", INPAINT_FRAMES, ids=["%dx%d" % f for _, f in INPAINT_FRAMES])
def test_inpainted_autozoom_vs_oracle_at_frame_sizes(inpaint_pipe, src, frame):
    """the inpainted Ken Burns path at the frame sizes photos produce (not multiples of 8), with two instances lifted to planes:
    coverage of both passes, the appended cloud and the frames rendered from it"""
    from cartoonsegmentation_amd import synth
    pipe = inpaint_pipe
    pipe.cfg.focal = frame[1] / 2.0
    img = synth.image_u8(src[0], src[1], 31 + src[0])
    kc = pipe.generate_kenburns_config(img, instances=_two_instances(*src))
    assert (kc['intHeight'], kc['intWidth']) == frame
    r = _inpainted_autozoom_vs_oracle(pipe, kc)
    assert min(r['holes']) > 0, r
    _assert_inpainted_run(r)


def test_refine_depth_vs_reference_fixture():
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "net_refine_48x64.npz")))
    pipe = KenBurnsPipeline(KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', refine_crf=False, default_depth_refine=True))
    y = pipe.refine_depth(torch.from_numpy(g['img']).to(pipe.device), torch.from_numpy(g['dsp']).to(pipe.device)).cpu().numpy()
    assert np.abs(y - g['y']).max() / np.abs(g['y']).max() < 1e-4          # reference Refine module, fp32 tolerance


def test_bokeh_and_colorize_vs_oracle_and_reference():
    from cartoonsegmentation_amd import ops
    from oracle import kenburns as okb
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "bokeh_240x320.npz")))
    d8 = ops.colorize_gray_r(torch.from_numpy(g['depth_f']).cuda()).cpu().numpy()
    assert np.array_equal(d8, okb.colorize_gray_r(g['depth_f']))                  # == oracle (numpy-1.26 percentile rule)
    dd = np.abs(d8.astype(np.int32) - g['depth_u8'].astype(np.int32))
    assert dd.max() <= 1 and (dd == 0).mean() > 0.98                              # reference colorize under numpy 2.2
    from cartoonsegmentation_amd._lib import load, ptr, stream_ptr, i32, i64, f32, check
    imf = torch.from_numpy((g['img'].astype(np.float32) / 255)).cuda().contiguous()
    dn = torch.from_numpy(g['dn']).cuda()
    one = torch.empty_like(imf)
    check(load().csm_bokeh_pass(ptr(imf), ptr(dn), ptr(one), i32(240), i32(320), i32(32), f32(np.cos(-np.pi / 6)), f32(np.sin(-np.pi / 6)),
                                stream_ptr()))
    assert np.array_equal(one.cpu().numpy(), g['one_pass'])                      # kernel_bokeh: bit-exact vs the reference text
    # the fused third pass (csm_bokeh_pass_finish) == csm_bokeh_pass followed by csm_bokeh_finish, byte for byte
    two = torch.empty_like(imf); sep = torch.empty((240, 320, 3), dtype=torch.uint8, device='cuda'); fus = torch.empty_like(sep)
    ddx, ddy = f32(np.cos(-np.pi * 5 / 6)), f32(np.sin(-np.pi * 5 / 6))
    check(load().csm_bokeh_pass(ptr(one), ptr(dn), ptr(two), i32(240), i32(320), i32(32), ddx, ddy, stream_ptr()))
    check(load().csm_bokeh_finish(ptr(one), ptr(two), ptr(sep), i64(240 * 320 * 3), f32(13.0), stream_ptr()))
    check(load().csm_bokeh_pass_finish(ptr(one), ptr(dn), ptr(fus), i32(240), i32(320), i32(32), ddx, ddy, f32(13.0), stream_ptr()))
    assert torch.equal(sep, fus)
    for tag, fp in (("fp100", 100.0), ("fp17", 17.25)):
        out = ops.bokeh_blur(torch.from_numpy(g['img']).cuda(), torch.from_numpy(g['depth_u8']).cuda(), 32, 13, depth_factor=1,
                             use_cuda=True, focal_plane=fp).cpu().numpy()
        ref = okb.bokeh_blur(g['img'], g['depth_u8'], 32, 13, fp)
        for other in (ref, g['blur_' + tag]):
            diff = np.abs(out.astype(np.int32) - other.astype(np.int32))
            # un-blurred pixels go v/255 -> ^13 -> ^(1/13) -> *255 -> floor and land within ulps of an integer, so the last
            # ulp of powf (device libm vs numpy's) decides between v and v-1: +-1 level, measured 5-9 % of values
            assert diff.max() <= 1 and (diff == 0).mean() > 0.85


def test_bokeh_blur_with_the_reference_defaults():
    """`from utils.effects import bokeh_blur; bokeh_blur(img, depth)` -- float depth, depth_factor = 2, lightness 10, no focal plane
    (utils/effects.py:143) -- and the other call forms (focal plane on a float map, uint8 depth with depth_factor 3) against fixtures
    made by the reference function (its kernel_bokeh branch; tests/golden/make_golden_bokeh.py): uint8 within +-1 (last ulp of powf)"""
    from utils.effects import bokeh_blur
    from oracle import kenburns as okb
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "bokeh_defaults_96x128.npz")))
    img, depth = g['img'], g['depth']
    cases = (('blur_defaults', depth, {}), ('blur_focal_f2', depth, dict(num_samples=32, lightness_factor=10, depth_factor=2, focal_plane=3.0)),
             ('blur_u8_f3', (depth * 60).astype(np.uint8), dict(num_samples=16, lightness_factor=8, depth_factor=3)))
    for tag, d, kw in cases:
        out = bokeh_blur(img, d, **kw)                                   # numpy in (uploaded), device tensor out
        out = out.cpu().numpy() if hasattr(out, 'cpu') else out
        diff = np.abs(out.astype(np.int32) - g[tag].astype(np.int32))
        assert out.shape == img.shape and diff.max() <= 1 and (diff == 0).mean() > 0.85, (tag, diff.max(), (diff == 0).mean())
        ref = okb.bokeh_blur(img, d, kw.get('num_samples', 32), kw.get('lightness_factor', 10), kw.get('focal_plane'), kw.get('depth_factor', 2))
        assert np.abs(out.astype(np.int32) - ref.astype(np.int32)).max() <= 1, tag
    # the same through device tensors and a float64 depth array
    out = bokeh_blur(torch.from_numpy(img).cuda(), torch.from_numpy(depth.astype(np.float64)).cuda())
    assert np.abs(out.cpu().numpy().astype(np.int32) - g['blur_defaults'].astype(np.int32)).max() <= 1


def test_shipped_yaml_configuration_runs_end_to_end(pipe_and_cfg):
    """depth_field=True + inpainting = configs/3dkenburns.yaml's frame loop"""
    pipe, kc, img, inst = pipe_and_cfg
    kc.depth_field, kc.num_frame = True, 4
    frames = pipe.autozoom(kc)
    kc.depth_field = False
    assert len(frames) == 4 and frames[0].shape == (kc.int_height, kc.int_width, 3)
    assert all(np.isfinite(f.astype(np.float32)).all() for f in frames)


def test_overlapped_depth_equals_sequential():
    """seg || LeReS on two HIP streams must give exactly the sequential result"""
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from cartoonsegmentation_amd import synth
    img = synth.image_u8(320, 320, 21)
    cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=512, refine_crf=False, focal=160.0,
                         mask_refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    pipe = KenBurnsPipeline(cfg)
    pipe.max_instances = 2
    pipe.animeinsseg.set_detect_size(96)
    outs = []
    for ov in (True, False, True):
        pipe.overlap_depth = ov
        kc = pipe.generate_kenburns_config(img)
        torch.cuda.synchronize()
        outs.append((kc['tenRawPoints'].clone(), kc['tenRawDepth'].clone(), kc.instances.masks.clone()))
    for a, b in ((0, 1), (1, 2)):
        assert all(torch.equal(x, y) for x, y in zip(outs[a], outs[b]))


def test_batched_configs_match_single_frame_path():
    """generate_kenburns_configs (batched detector / refine / LeReS) vs the per-image reference order: BITWISE the same instances,
    depth and point clouds -- csm_op.ksplit follows the per-sample shape, so the batch a frame runs in does not touch its bits"""
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from cartoonsegmentation_amd import synth
    imgs = [synth.image_u8(320, 320, 31 + k) for k in range(3)]
    cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=512, refine_crf=False, focal=160.0,
                         mask_refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    pipe = KenBurnsPipeline(cfg)
    pipe.max_instances, pipe.overlap_depth = 2, False
    pipe.animeinsseg.set_detect_size(96)
    batched = pipe.generate_kenburns_configs(imgs)
    for im, kb in zip(imgs, batched):
        ks = pipe.generate_kenburns_config(im)
        assert len(ks.instances) == len(kb.instances) and torch.equal(ks.instances.bboxes, kb.instances.bboxes)
        assert torch.equal(ks.instances.masks, kb.instances.masks) and torch.equal(ks.instances.scores, kb.instances.scores)
        assert torch.equal(ks['tenRawDepth'], kb['tenRawDepth']) and torch.equal(ks['tenRawPoints'], kb['tenRawPoints'])
        assert ks['objDepthrange'] == kb['objDepthrange']


def test_depth_glue_ops_vs_numpy():
    """csm_minmax / csm_fill_zero_min_positive / csm_depth_adjust_instance / csm_normalise_disparity / csm_depth_range_stats
    against numpy restatements of the reference lines (leres/__init__.py:143-145, kenburns_effect.py:68-78, :928, :935),
    including the branches the pipeline tests do not reach: zeros present, empty mask, ties in the depth crop."""
    import ctypes
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import check, f32, i32, i64, ptr, stream_ptr
    from oracle import kenburns as okb
    L = _lib.load()
    _mm_scratch = lambda t: torch.empty(512, dtype=torch.float32, device=t.device)
    rng = np.random.default_rng(5)
    H, W = 300, 333
    # -- min/max
    x = rng.normal(0, 3, (H, W)).astype(np.float32)
    xd = torch.from_numpy(x).cuda(); mm = torch.empty(2, device='cuda')
    check(L.csm_minmax(ptr(xd), i64(x.size), ptr(mm), ptr(_mm_scratch(xd)), stream_ptr()))
    assert mm.cpu().numpy().tolist() == [float(x.min()), float(x.max())]
    # -- zero fill: zeros + positives, no zeros, nothing positive
    for case in ("zeros", "nozero", "nopos"):
        d = np.floor(rng.uniform(0, 255, (H, W))).astype(np.float32)
        if case == "zeros":
            d[rng.uniform(size=d.shape) < 0.05] = 0
        elif case == "nozero":
            d[d == 0] = 7
        else:
            d[:] = 0
        ref = d.copy()
        if (ref > 0).any():
            ref[ref == 0] = ref[ref > 0].min()
        dd = torch.from_numpy(d).cuda(); sc = torch.empty(2, dtype=torch.int32, device='cuda')
        check(L.csm_fill_zero_min_positive(ptr(dd), i64(d.size), ptr(sc), stream_ptr()))
        assert np.array_equal(dd.cpu().numpy(), ref), case
    # -- depth adjustment: two overlapping instances, one empty mask, one touching the bottom row
    disp = rng.uniform(1, 255, (1, 1, H, W)).astype(np.float32)
    masks = np.zeros((4, H, W), bool)
    masks[0, 40:200, 50:180] = True
    masks[1, 150:H, 100:300] = True            # reaches the last row, overlaps instance 0
    masks[3, 10:13, 5:9] = True                # tiny: top == r0 region
    ref = okb.depth_adjustment(list(masks), disp)
    dd = torch.from_numpy(disp.copy()).cuda()
    sc = torch.empty(2 * H + 2, device='cuda')
    for m in masks:
        md = torch.from_numpy(m).cuda()
        check(L.csm_depth_adjust_instance(ptr(dd), ptr(md.view(torch.uint8)), i32(H), i32(W), ptr(sc), stream_ptr()))
    assert np.array_equal(dd.cpu().numpy(), ref)
    # -- normalise + depth-range statistics with ties (a constant plateau inside the crop)
    raw = ref.astype(np.float32)
    raw[0, 0, 140:160, 140:170] = raw.max()           # many equal maxima of the disparity -> equal minima of the depth
    base = np.float32(40.0)
    norm = (raw / raw.max() * base).astype(np.float32)
    rd = torch.from_numpy(raw).cuda(); mm = torch.empty(2, device='cuda'); nd = torch.empty_like(rd); nmax = torch.empty(1, device='cuda')
    check(L.csm_minmax(ptr(rd), i64(raw.size), ptr(mm), ptr(_mm_scratch(rd)), stream_ptr()))
    check(L.csm_normalise_disparity(ptr(rd), i64(raw.size), ptr(mm), f32(float(base)), ptr(nd), ptr(nmax), stream_ptr()))
    assert np.array_equal(nd.cpu().numpy(), norm) and float(nmax.item()) == float(norm.max())
    depth = ((np.float32(1.0) / (norm + np.float32(1e-5))) * np.float32(100.0)).astype(np.float32)
    dd = torch.from_numpy(depth).cuda()
    keys = torch.empty(2, dtype=torch.int64, device='cuda'); out6 = torch.empty(6, dtype=torch.float64, device='cuda')
    check(L.csm_depth_range_stats(ptr(mm), f32(float(base)), ptr(dd), i32(H), i32(W), i32(128), i32(128), i32(H - 256), i32(W - 256),
                                  ptr(keys), ptr(out6), stream_ptr()))
    crop = depth[0, 0, 128:-128, 128:-128]
    got = out6.cpu().numpy()
    assert got[0] == float(norm.min()) and got[1] == float(norm.max())
    assert got[2] == float(crop.min()) and got[3] == float(crop.max())
    assert int(got[4]) == int(crop.argmin()) and int(got[5]) == int(crop.argmax())      # first row-major occurrence, like numpy / cv2


def test_bench_two_ranks_end_to_end(tmp_path):
    """bench.py's multi-rank path as the driver launches it (torch.distributed.run, 2 ranks), on ONE GPU over gloo (a logic check,
    not a measurement): rank 1 builds with placeholder weights and rank 0's tile table, receives the weights through the
    broadcast, the uint8 outputs are gathered, one JSON line comes out with global_batch = 2 x batch."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CSM_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", CSM_SYNTHETIC_WEIGHTS="1",
               CSM_BENCH_WATCHDOG="500")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(root, "bench.py"), "--gpus", "2", "--batch", "2", "--size", "320", "--steps", "1",
           "--warmup", "0", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 4 and d["config"]["frames_per_gpu_step"] == 2
    assert d["weights_broadcast_bytes"] > 1e8 and d["weights_equal_after_broadcast"] is True
    assert d["value"] > 0 and d["scaling"] == "weak" and "roofline" in d
    # rank 0's tuned tile table reaches the other ranks through the process group (broadcast_object_list), not through a shared file
    assert d["tile_table"]["entries"] > 0 and "broadcast_object_list" in d["tile_table"]["how"]
    # every rank's output records (uint8 frame + bit-packed instance masks + count) reach rank 0 and unpack
    g = d["gather"]
    assert g["records_ok"] is True and g["masks_in_first_frames"] >= 2 and g["record_bytes"] == 320 * 320 * 3 + 2 * (320 * 320 // 8) + 8


def test_bench_process_group_path_on_rccl_with_one_rank():
    """the same start-up with the measured backend: ONE rank (this box has one GPU) launched by torch.distributed.run with
    CSM_BENCH_FORCE_DIST=1, so init_process_group("nccl", device_id=...), broadcast_object_list, the weight broadcasts, the MAX / MIN
    all-reduces, the asynchronous gather on the communicator's stream and destroy_process_group all execute on RCCL (what a 1-GPU box
    can show of SURVEY 8e; the 2-rank logic is the gloo test above)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CSM_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29543", CSM_SYNTHETIC_WEIGHTS="1",
               CSM_BENCH_WATCHDOG="500", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("CSM_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", "29543", os.path.join(root, "bench.py"), "--gpus", "1", "--batch", "2", "--size", "320", "--steps", "2",
           "--warmup", "1", "--no-variants", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    assert d["process_group"] == {"backend": "nccl", "world_size": 1} and d["n_gpus"] == 1
    assert d["weights_broadcast_bytes"] > 1e8 and d["weights_equal_after_broadcast"] is True
    assert d["gather"]["records_ok"] is True and d["value"] > 0


def test_bench_plain_run_prints_the_headline_only(tmp_path):
    """bench.py without --full: set-up, warm-up, the timed steps, --dump-outputs and the headline line -- none of the items that
    rerun the workload or the oracle (roofline, CPU baseline, mask IoU, variants) is measured or reported"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CSM_SYNTHETIC_WEIGHTS="1", CSM_BENCH_WATCHDOG="500")
    env.pop("CSM_BENCH_FORCE_DIST", None)
    dump = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--batch", "2", "--size", "320", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(d)
    assert d["value"] > 0 and d["steps"] == 2 and d["warmup"] == 1 and d["config"]["frames_per_gpu_step"] == 2
    assert not {"roofline", "cpu_baseline", "mask_iou_vs_oracle", "variants", "batch1"} & set(d)
    assert sorted(os.listdir(dump)) == sorted(k + ".npy" for k in d["dumped_outputs"]["arrays"])


def test_default_depth_estimator_pipeline():
    """depth_est='default' + default_depth_refine (the commented 'original 3dkenburns' block of configs/3dkenburns.yaml):
    VGG19-BN semantics + Disparity GridNet at <= 512, depth adjustment through the resize branch, Refine back to the frame size"""
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from cartoonsegmentation_amd import synth
    img = synth.image_u8(320, 384, 51)
    cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='default', default_depth_refine=True, max_size=512, refine_crf=False, focal=192.0,
                         num_frame=2, mask_refine_kwargs={'refine_method': 'none'})
    pipe = KenBurnsPipeline(cfg)
    pipe.max_instances = 2
    pipe.animeinsseg.set_detect_size(96)
    coarse = pipe._depth_est(None, torch.from_numpy(img).cuda())
    assert coarse.shape == (1, 1, 213, 256) and float(coarse.min()) >= 0.0 and torch.isfinite(coarse).all()
    kc = pipe.generate_kenburns_config(img)
    assert kc['tenRawDisparity'].shape == (1, 1, 320, 384) and torch.isfinite(kc['tenRawPoints']).all()
    frames = pipe.autozoom(kc, inpaint=False)
    assert len(frames) == 2 and frames[0].shape == (320, 384, 3)
    # a PORTRAIT frame: 680 x 400 -> the estimator runs at 512 x 301, whose feature maps are odd in width on the way down (the
    # reference's [0,-1] column crops, disparity_estimation.py:172-173; bit-checked against the reference modules in test_gpu_nets)
    img = synth.image_u8(680, 400, 52)
    coarse = pipe._depth_est(None, torch.from_numpy(img).cuda())
    assert coarse.shape == (1, 1, 256, 151) and float(coarse.min()) >= 0.0 and torch.isfinite(coarse).all()
    kc = pipe.generate_kenburns_config(img)
    assert kc["tenRawDisparity"].shape == (1, 1, 512, 301) and torch.isfinite(kc["tenRawPoints"]).all()      # max_size 512 scales the frame


def test_device_percentiles_and_bokeh_stats_are_exact():
    """csm_percentile_pair (3-pass 16 + 8 + 8 bit radix select in three launches, no sort, no host sync; one scratch re-used by every
    call: each call must leave its counting tables cleared) == the order statistics of the sorted array for awkward inputs (negatives, signed zeros,
    heavy ties, tiny / huge magnitudes, two far-apart clusters, a constant plane, a smooth ramp, an unaligned plane), and
    csm_bokeh_depth_auto == csm_bokeh_depth fed with the
    host-side reductions"""
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import check, f32, f64, i64, ptr, stream_ptr
    from oracle import kenburns as okb
    L = _lib.load()
    rng = np.random.default_rng(12)
    sel = torch.zeros(L.csm_percentile_scratch_bytes(), dtype=torch.uint8, device='cuda')       # zeroed ONCE (the contract)
    out2 = torch.empty(2, device='cuda')
    yy, xx = np.mgrid[0:720, 0:1280]
    cases = [rng.normal(0, 1, 100003).astype(np.float32),
             np.concatenate([np.zeros(5000, np.float32), -np.zeros(5000, np.float32), rng.uniform(-1e-30, 1e30, 777).astype(np.float32)]),
             np.round(rng.uniform(0, 8, 1 << 20)).astype(np.float32),                    # heavy ties
             rng.uniform(200, 900, 1024 * 1024).astype(np.float32),                      # like a render depth plane
             np.array([3.0], np.float32), np.array([2.0, -7.5], np.float32),
             np.concatenate([rng.normal(1.0, 0.01, 300000), rng.normal(-5e4, 10.0, 200001)]).astype(np.float32),   # two clusters, far apart in key space
             np.full(70001, 2.75, np.float32),                                           # constant plane
             (3.0 + 0.002 * yy + 0.0005 * xx + 0.3 * np.sin(xx / 90.0)).astype(np.float32).ravel(),   # smooth depth ramp (the frame loop's case)
             rng.uniform(1, 2, 4099).astype(np.float32)]
    for ci, a in enumerate(cases):
        for q_lo, q_hi in ((2.0, 85.0), (0.0, 100.0), (50.0, 99.9)):
            d = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), a])).cuda()[1:] if ci == len(cases) - 1 else torch.from_numpy(a).cuda()   # last: 4-byte aligned only
            check(L.csm_percentile_pair(ptr(d), i64(a.size), f64(q_lo), f64(q_hi), ptr(out2), ptr(sel), stream_ptr()))
            got = out2.cpu().numpy()
            assert got[0] == okb._percentile(a, q_lo) and got[1] == okb._percentile(a, q_hi), (a.size, q_lo, q_hi, got)
    # poisoned state (what an aborted launch could leave behind): a stale count in a pass-1 table -> the selection does not return a
    # plausible wrong number, it returns NaN, and keeps doing so until the caller re-zeroes the scratch (the documented start state)
    a = rng.normal(0, 1, 50000).astype(np.float32)
    d = torch.from_numpy(a).cuda()
    sel.view(torch.int32)[16 + 7] += 3                                # a coarse bin of XCD copy 0 (the tables follow the 64-byte state)
    check(L.csm_percentile_pair(ptr(d), i64(a.size), f64(2.0), f64(85.0), ptr(out2), ptr(sel), stream_ptr()))
    assert torch.isnan(out2).all()
    check(L.csm_percentile_pair(ptr(d), i64(a.size), f64(2.0), f64(85.0), ptr(out2), ptr(sel), stream_ptr()))
    assert torch.isnan(out2).all()                                    # sticky
    sel.zero_()
    check(L.csm_percentile_pair(ptr(d), i64(a.size), f64(2.0), f64(85.0), ptr(out2), ptr(sel), stream_ptr()))
    got = out2.cpu().numpy()
    assert got[0] == okb._percentile(a, 2.0) and got[1] == okb._percentile(a, 85.0)
    d8 = rng.integers(3, 250, (300, 400)).astype(np.uint8)
    dd = torch.from_numpy(d8).cuda()
    for fp in (0.0, 100.0, 17.25, 255.0):
        df = dd.float()
        dmax = float(df.max().item()); t = dmax - (df - fp).abs(); mn = float(t.min().item()); mx2 = float((t - mn).max().item())
        ref, got = torch.empty((300, 400), device='cuda'), torch.empty((300, 400), device='cuda')
        check(L.csm_bokeh_depth(ptr(dd), ptr(ref), i64(d8.size), f32(dmax), f32(fp), f32(mn), f32(mx2), stream_ptr()))
        sc = torch.zeros(L.csm_bokeh_depth_scratch_bytes(), dtype=torch.uint8, device="cuda")         # the completion counter starts at 0
        check(L.csm_bokeh_depth_auto(ptr(dd), ptr(got), i64(d8.size), f32(fp), ptr(sc), stream_ptr()))
        assert torch.equal(ref, got), fp


def test_lanczos4_resize_back_and_small_frames():
    """frames whose 32-aligned LeReS size exceeds the frame (600 x 400 -> 608 x 416, k > 1): the reference resizes the uint8 depth
    back with INTER_LANCZOS4 (kenburns_effect.py:571-573).  HIP == oracle restatement bit for bit [EXT, unpinned]; a constant map
    stays constant (the Q11 coefficients of every phase sum to 2048 +- rounding, checked to +-1); the pipeline runs."""
    import ctypes
    from cartoonsegmentation_amd import _lib, synth
    from cartoonsegmentation_amd._lib import check, i32, ptr, stream_ptr
    from oracle import segment as oseg
    L, O = _lib.load(), oseg.lib()
    rng = np.random.default_rng(3)
    for (h, w, H, W) in ((608, 416, 600, 400), (64, 96, 50, 90), (32, 32, 31, 17)):
        src = rng.integers(0, 256, (h, w)).astype(np.uint8)
        d = torch.from_numpy(src).cuda()
        out = torch.empty((H, W), device='cuda'); ref = np.empty((H, W), np.float32)
        check(L.csm_resize_u8_lanczos4_to_f32(ptr(d), i32(h), i32(w), i32(H), i32(W), ptr(out), stream_ptr()))
        O.orc_resize_u8_lanczos4_to_f32(oseg._p(src), ctypes.c_int(h), ctypes.c_int(w), ctypes.c_int(H), ctypes.c_int(W), oseg._p(ref))
        assert np.array_equal(out.cpu().numpy(), ref)
        flat = torch.full((h, w), 200, dtype=torch.uint8, device='cuda')
        check(L.csm_resize_u8_lanczos4_to_f32(ptr(flat), i32(h), i32(w), i32(H), i32(W), ptr(out), stream_ptr()))
        assert float((out - 200).abs().max()) <= 1.0
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', depth_est_size=640, max_size=720, refine_crf=False, focal=200.0,
                         num_frame=2, mask_refine_kwargs={'refine_method': 'none'})
    pipe = KenBurnsPipeline(cfg)
    pipe.max_instances = 1
    pipe.animeinsseg.set_detect_size(96)
    os.environ["CSM_AUTOTUNE"] = "0"
    try:
        kc = pipe.generate_kenburns_config(synth.image_u8(600, 400, 8))            # default max_size 720 >= image: no frame scaling
    finally:
        os.environ.pop("CSM_AUTOTUNE", None)
    assert kc['tenRawDepth'].shape == (1, 1, 600, 400) and torch.isfinite(kc['tenRawPoints']).all()


def test_io_utils_float_masks_and_large_frame_fallback():
    """utils.io_utils.scaledown_maxsize / resize_pad take float masks like the reference's callers
    (prepare_refine_batch, animeinsseg/__init__.py:47) -- HIP == the oracle restatement of cv2's float INTER_LINEAR [EXT] -- and
    WarpFrame falls back to the global-atomic chain for frames beyond the tiled path's 8192-tile limit instead of raising"""
    import ctypes
    from cartoonsegmentation_amd import ops, synth
    from oracle import segment as oseg
    from utils.io_utils import resize_pad, scaledown_maxsize
    rng = np.random.default_rng(2)
    m = (rng.uniform(size=(300, 212)) > 0.5).astype(np.float32)
    out = scaledown_maxsize(m, 128)
    assert out.shape == (128, 90) and out.dtype == np.float32
    ref = np.empty((128, 90), np.float32)
    oseg.lib().orc_resize_f32_linear(oseg._p(m), ctypes.c_int(300), ctypes.c_int(212), ctypes.c_int(1), ctypes.c_int(128), ctypes.c_int(90),
                                     oseg._p(ref))
    assert np.array_equal(out, ref) and 0.0 <= out.min() and out.max() <= 1.0 and 0.3 < out.mean() < 0.7
    padded, pads = resize_pad(m, 128, 0)
    assert padded.shape == (128, 128) and pads == (0, 0, 0, 38) and np.array_equal(padded[:, :90], ref) and not padded[:, 90:].any()
    img3 = rng.uniform(0, 1, (64, 200, 3)).astype(np.float32)
    o3 = scaledown_maxsize(torch.from_numpy(img3).cuda(), 100)
    r3 = np.empty((32, 100, 3), np.float32)
    oseg.lib().orc_resize_f32_linear(oseg._p(img3), ctypes.c_int(64), ctypes.c_int(200), ctypes.c_int(3), ctypes.c_int(32), ctypes.c_int(100),
                                     oseg._p(r3))
    assert o3.is_cuda and np.array_equal(o3.cpu().numpy(), r3)
    with pytest.raises(TypeError):
        scaledown_maxsize(m > 0.5, 128)
    # 2176 x 2048 = 64 x 136 = 8704 tiles of 32 x 16 > 8192
    H, W = 2176, 2048
    wf = ops.WarpFrame(H, W, torch.device('cuda'))
    assert wf.path == 'atomics'
    sc = synth.warp_scene(H, W, 3)
    disp = torch.from_numpy(sc['disp']).cuda()
    disp = disp / disp.max() * sc['baseline']
    depth, _, pts, _ = ops.disparity_to_points(disp, sc['focal'], sc['baseline'])
    frame, _ = wf(pts.view(1, 3, -1), torch.from_numpy(sc['rgb']).cuda(), depth.view(1, 1, -1), sc['focal'], sc['baseline'], [3.0, -2.0, -5.0])
    torch.cuda.synchronize()
    assert frame.shape == (H, W, 3) and float(frame.float().mean()) > 1.0


def test_frame_streams_and_lanes_give_the_serial_results():
    """MI355X scheduling additions are invisible in the results: (i) process_kenburns with consecutive frames on 3 HIP streams ==
    the one-stream loop, byte for byte, with and without the bokeh tail; (ii) FrameLanes (frames in flight on several host threads,
    each with its own pipeline object) == the serial per-frame loop"""
    os.environ["CSM_SYNTHETIC_WEIGHTS"] = "1"
    from anime_3dkenburns import KenBurnsConfig, KenBurnsPipeline
    from cartoonsegmentation_amd import synth
    from cartoonsegmentation_amd.lanes import FrameLanes

    def make():
        cfg = KenBurnsConfig(det_ckpt='synthetic', depth_est='leres', depth_est_size=96, max_size=512, refine_crf=False, focal=160.0,
                             num_frame=7, mask_refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
        p = KenBurnsPipeline(cfg)
        p.max_instances = 2
        p.animeinsseg.set_detect_size(96)
        return p
    pipe = make()
    img = synth.image_u8(320, 352, 61)
    res = {}
    for dof in (False, True):
        for ns in (1, 3):
            pipe.frame_streams = ns
            kc = pipe.generate_kenburns_config(img)
            kc.depth_field = dof
            res[(dof, ns)] = np.stack(pipe.autozoom(kc, inpaint=False))
        assert np.array_equal(res[(dof, 1)], res[(dof, 3)]), dof
    assert not np.array_equal(res[(False, 1)], res[(True, 1)])
    imgs = [synth.image_u8(320, 352, 70 + k) for k in range(5)]

    def one(p, im):
        kc = p.generate_kenburns_config(im)
        return (kc['tenRawPoints'].clone(), kc.instances.masks.clone(), kc['objDepthrange'])
    serial = [one(pipe, im) for im in imgs]

    def make_worker(i):
        p = make()
        return lambda im: one(p, im)
    fl = FrameLanes(make_worker, lanes=2)
    try:
        par = fl.map(imgs)
    finally:
        fl.close()
    for a, b in zip(serial, par):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


def test_device_focal_plane_median_matches_numpy():
    """csm_masked_u8_median_max == max_k np.median(depth_u8[mask_k]) (kenburns_effect.py:1045-1056) for odd / even counts, a single
    pixel, an empty mask (skipped: np.median gives nan) and all-empty (-1, the reference's initial focalplane_end)"""
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import check, i32, i64, ptr, stream_ptr
    L = _lib.load()
    rng = np.random.default_rng(4)
    H, W = 123, 211
    d8 = rng.integers(0, 256, (H, W)).astype(np.uint8)
    d8[:40] = (d8[:40] // 64) * 3                                   # heavy ties in one region
    masks = np.zeros((5, H, W), bool)
    masks[0, 10:60, 20:91] = True                                   # 50 x 71 = 3550 (even)
    masks[1, 0:33, 0:33] = True                                     # 1089 (odd), inside the tie region
    masks[2, 100, 200] = True                                       # one pixel
    masks[4] = rng.uniform(size=(H, W)) > 0.7
    def run(m):
        md = torch.from_numpy(m).cuda().view(torch.uint8)
        hist = torch.empty(m.shape[0] * 256, dtype=torch.int32, device='cuda')
        out = torch.empty(m.shape[0] + 1, device='cuda')
        check(L.csm_masked_u8_median_max(ptr(torch.from_numpy(d8).cuda()), ptr(md), i32(m.shape[0]), i64(H * W), ptr(hist), ptr(out), stream_ptr()))
        return out.cpu().numpy()
    got = run(masks)
    want = [np.median(d8[m]) if m.any() else np.nan for m in masks]
    for k in range(5):
        assert (np.isnan(got[k]) and np.isnan(want[k])) or got[k] == np.float32(want[k]), (k, got[k], want[k])
    assert got[5] == np.float32(np.nanmax(want))
    assert run(np.zeros((2, H, W), bool))[2] == -1.0


def test_hand_written_glue_kernels_match_torch():
    """the kernels that replaced torch ops on the product path (round 3): mean / std (double accumulation), normalise / de-normalise
    with clip and threshold, aten bilinear on planes, adaptive-area mask resize + 0.3 threshold (AnimeInstances.resize)"""
    from cartoonsegmentation_amd import ops
    from cartoonsegmentation_amd.anime_instances import AnimeInstances
    F = torch.nn.functional
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randn((1, 3, 301, 417), device='cuda', generator=g) * 3 + 0.7
    ms = ops.mean_std(x)
    ref = torch.stack([x.double().mean(), x.double().std(unbiased=False)]).float()
    assert torch.allclose(ms, ref, rtol=1e-6, atol=0)
    n = ops.normalise(x, ms)
    assert torch.allclose(n, (x - ms[0]) / (ms[1] + 0.0000001), rtol=1e-6, atol=1e-7)
    for mode, fn in ((1, lambda t: t.clip(0.0, 1.0)), (2, lambda t: F.threshold(t, 0.0, 0.0)), (0, lambda t: t)):
        assert torch.allclose(ops.denormalise(n, ms, mode), fn(n * (ms[1] + 0.0000001) + ms[0]), rtol=1e-6, atol=1e-6)
    # torch's device kernel is built with FMA contraction: its source coordinate scale * (dst + 0.5) - 0.5 can differ from the
    # unfused evaluation (aten's CPU order, which libcsm355 follows) by one ulp of a coordinate ~ 400, i.e. 3e-5 in the interpolation
    # weight -> compare a SMOOTH plane tightly (weight noise x small gradient) and white noise at the weight-noise level
    yy, xx = torch.meshgrid(torch.arange(301, device='cuda'), torch.arange(417, device='cuda'), indexing='ij')
    smooth = (torch.sin(xx / 40.0) * torch.cos(yy / 55.0))[None, None].float().expand(1, 3, -1, -1).contiguous()
    for (h, w, ac) in ((150, 200, False), (640, 333, False), (77, 91, True), (301, 417, False)):
        for src, tol in ((smooth, 1e-5), (x, 2e-3)):
            got, want = ops.resize_bilinear(src, h, w, align_corners=ac), F.interpolate(src, size=(h, w), mode='bilinear', align_corners=ac)
            assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-5, atol=tol), (h, w, ac, tol)
        cpu = F.interpolate(x.cpu(), size=(h, w), mode='bilinear', align_corners=ac)
        assert (ops.resize_bilinear(x, h, w, align_corners=ac).cpu() - cpu).abs().max() <= 2e-3
    masks = torch.rand((3, 250, 310), device='cuda', generator=g) > 0.6
    masks[1, :, :100] = True
    for (h, w) in ((125, 155), (100, 123), (400, 512), (250, 311), (83, 31)):
        inst = AnimeInstances(masks.clone(), torch.tensor([[10, 20, 30, 40]] * 3, dtype=torch.int32, device='cuda'), torch.ones(3, device='cuda'))
        inst.resize(h, w)
        want = F.interpolate(masks.float().unsqueeze(1), (h, w), mode='area').squeeze(1) > 0.3
        assert inst.masks.dtype == torch.bool and torch.equal(inst.masks, want), (h, w)


def test_fused_frame_call_equals_the_separate_calls():
    """csm_kenburns_frame (one library call per output frame) == WarpFrame() + colorize_gray_r + bokeh_blur + csm_crop_resize_u8, byte
    for byte, with and without the depth-of-field tail"""
    from cartoonsegmentation_amd import _lib, ops, synth
    from cartoonsegmentation_amd._lib import check, f32, i32, ptr, stream_ptr
    L = _lib.load()
    H, W = 200, 264
    sc = synth.warp_scene(H, W, 9)
    disp = torch.from_numpy(sc['disp']).cuda()
    disp = disp / disp.max() * sc['baseline']
    depth, _, pts, _ = ops.disparity_to_points(disp, sc['focal'], sc['baseline'])
    pts, dep, rgb = pts.view(1, 3, -1).contiguous(), depth.view(1, 1, -1).contiguous(), torch.from_numpy(sc['rgb']).cuda()
    ph, pw = int(0.9 * H), int(0.93 * W)
    for dof in (None, (117.25, 32, 13)):
        for shift in ([3.0, -2.0, -6.0], [-1.5, 0.25, 2.0]):
            a = ops.WarpFrame(H, W, torch.device('cuda'), keep_render=True)
            frame, render = a(pts, rgb, dep, sc['focal'], sc['baseline'], shift)
            if dof is not None:
                d8 = ops.colorize_gray_r(render[0, 3])
                frame = ops.bokeh_blur(frame, d8, dof[1], dof[2], focal_plane=dof[0], use_cuda=True, depth_factor=1)
            want = torch.empty((H, W, 3), dtype=torch.uint8, device='cuda')
            check(L.csm_crop_resize_u8(ptr(frame), i32(H), i32(W), i32(ph), i32(pw), f32(W / 2.0), f32(H / 2.0), ptr(want), stream_ptr()))
            b = ops.WarpFrame(H, W, torch.device('cuda'), keep_render=True)
            got = torch.empty((H, W, 3), dtype=torch.uint8, device='cuda')
            b.frame_into(got, pts, rgb, dep, sc['focal'], sc['baseline'], shift, ph, pw, W / 2.0, H / 2.0, dof)
            b.frame_into(got, pts, rgb, dep, sc['focal'], sc['baseline'], shift, ph, pw, W / 2.0, H / 2.0, dof)     # scratch re-arms itself
            assert torch.equal(got, want), (dof, shift)


def test_frame_lanes_collect_every_result_before_raising():
    """FrameLanes.map: an item that raises does not leave the other results of the call in the queue for the next call, and the
    tensors it hands over are registered with the caller's stream"""
    from cartoonsegmentation_amd.lanes import FrameLanes

    def make_worker(i):
        def fn(item):
            if item == 'boom':
                raise ValueError('boom')
            return {'v': torch.full((1024,), float(item), device='cuda'), 'lane': i}
        return fn
    fl = FrameLanes(make_worker, lanes=2)
    try:
        with pytest.raises(ValueError):
            fl.map([1, 'boom', 3, 4, 5])
        out = fl.map([5, 6, 7])
        assert [float(o['v'][0]) for o in out] == [5.0, 6.0, 7.0] and [o['lane'] for o in out] == [0, 1, 0]
        assert float(sum(o['v'].sum() for o in out)) == 1024.0 * 18
    finally:
        fl.close()
