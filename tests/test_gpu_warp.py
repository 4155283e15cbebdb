"""GPU parity: libcsm355 warp kernels (through the C ABI / ops.py)  vs  oracle + golden fixtures.

Bit-exact where the algorithm is order independent (z-buffer, degrid, fill, point-wise);
fp32 atomicAdd accumulation order is not deterministic on any GPU (nor in the reference),
so accumulators/renders use north_star's 1e-3 relative tolerance.
"""
import glob
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import warp as orc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
RENDER_CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "warp_*.npz")) if not p.endswith("_fast.npz"))
IDS = [os.path.basename(p)[:-4] for p in RENDER_CASES]


def cases(keep):
    """(paths, ids) of the render fixtures whose file name passes `keep` (the name only: the checkout's directory may hold any text)"""
    sel = [(p, i) for p, i in zip(RENDER_CASES, IDS) if keep(i)]
    return dict(argvalues=[p for p, _ in sel], ids=[i for _, i in sel])


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from cartoonsegmentation_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close_frac(a, b, rtol=1e-3, atol=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) <= atol + rtol * np.abs(b)).mean())


@pytest.mark.parametrize("path", RENDER_CASES, ids=IDS)
def test_stages_vs_golden_and_oracle(ops, path):
    g = dict(np.load(path))
    H, W, C = int(g['H']), int(g['W']), int(g['C'])
    focal, baseline = float(g['focal']), float(g['baseline'])
    # process_shift: bit exact vs the reference
    ps = ops.shift_points(dev(g['pts']), [float(v) for v in g['shift']])
    assert np.array_equal(ps.cpu().numpy(), g['pts_shift'])
    # z-buffer: bit exact vs the reference (atomic min is order independent)
    zee = ops.pointrender_update_zee(ps, W, H, focal, baseline)
    assert np.array_equal(zee.cpu().numpy(), g['zee_after_zee'])
    # degrid: bit exact vs the oracle's Jacobi form
    zd = ops.pointrender_degrid(zee)
    zd_o = orc.degrid(g['zee_after_zee'], 1)
    assert np.array_equal(zd.cpu().numpy(), zd_o)
    # accumulate: same z-buffer as the fixture -> compare with the reference accumulators
    zin = dev(g['zee_after_degrid_inplace'])
    acc = ops.pointrender_update_output(ps, dev(g['data']), zin, focal, baseline).cpu().numpy()
    data1 = np.concatenate([g['data'], np.ones_like(g['data'][:, :1])], 1)
    acc_o = orc.update_output(g['pts_shift'], data1, g['zee_after_degrid_inplace'], focal, baseline)
    assert np.array_equal(acc != 0, acc_o != 0)          # same coverage decisions
    assert close_frac(acc, acc_o, 1e-4, 1e-5) == 1.0
    if 'accum' in g:
        assert close_frac(acc, g['accum'], 1e-4, 1e-5) == 1.0


@pytest.mark.parametrize("how", ["tiled", "atomics"])
@pytest.mark.parametrize("path", RENDER_CASES, ids=IDS)
def test_render_pointcloud(ops, path, how):
    """both executions of the operator (destination tiles + LDS fixed point / global float atomics; batches always take the latter)"""
    g = dict(np.load(path))
    H, W = int(g['H']), int(g['W'])
    focal, baseline = float(g['focal']), float(g['baseline'])
    render, existing = ops.render_pointcloud(dev(g['pts_shift']), dev(g['data']), W, H, focal, baseline, path=how)
    render, existing = render.cpu().numpy(), existing.cpu().numpy()
    r1, e1 = orc.render_pointcloud(g['pts_shift'], g['data'], W, H, focal, baseline, degrid_mode=1)
    assert np.array_equal(existing > 0, e1 > 0)
    assert close_frac(existing, e1, 1e-4, 1e-6) == 1.0
    assert close_frac(render, r1) >= 0.999
    # against the reference fixture (in-place racy degrid): wherever the two degrid semantics agree
    r0, e0 = orc.render_pointcloud(g['pts_shift'], g['data'], W, H, focal, baseline, degrid_mode=0)
    agree = np.broadcast_to((e0 == e1), r0.shape) & (np.abs(r0 - r1) <= 1e-6 + 1e-5 * np.abs(r1))
    assert agree.mean() > 0.9
    ok = np.abs(render - g['render']) <= 1e-5 + 1e-3 * np.abs(g['render'])
    assert ok[agree].mean() >= 0.999


@pytest.mark.parametrize("path", **cases(lambda i: 'c4' in i))
def test_fill_disocclusion_bit_exact(ops, path):
    g = dict(np.load(path))
    out = ops.fill_disocclusion(dev(g['render']), dev(g['fill_depth'])).cpu().numpy()
    assert np.array_equal(out, g['filled'])


def test_discfill_synthetic_holes(ops):
    g = dict(np.load(os.path.join(GOLDEN, "discfill_48x40.npz")))
    out = ops.fill_disocclusion(dev(g['img']), dev(g['depth'])).cpu().numpy()
    assert np.array_equal(out, g['out'])


def test_pointwise(ops):
    g = dict(np.load(os.path.join(GOLDEN, "pointwise_72x56.npz")))
    focal, baseline = float(g['focal']), float(g['baseline'])
    depth, valid, pts, un = [t.cpu().numpy() for t in ops.disparity_to_points(dev(g['disp']), focal, baseline)]
    d_o, dep_o, val_o, pts_o, un_o = orc.disparity_to_points(g['disp_raw'], focal, baseline)
    assert np.array_equal(depth, dep_o) and np.array_equal(valid, val_o)
    assert np.array_equal(pts, pts_o) and np.array_equal(un, un_o)
    assert np.array_equal(depth, g['depth']) and np.array_equal(un, g['unaltered'])
    nd = g['disp'] / g['disp'].max()
    lap = ops.spatial_filter(dev(nd), 'laplacian').cpu().numpy()
    assert np.array_equal(lap, orc.spatial_filter_laplacian(nd))
    assert np.abs(lap - g['lap']).max() < 2e-6
    p2 = ops.depth_to_points(dev(g['depth']), focal).cpu().numpy()
    assert np.array_equal(p2, g['unaltered'])
    m = (np.random.default_rng(3).uniform(0, 1, (2, 1, 37, 41)) > 0.4).astype(np.float32)
    assert np.array_equal(ops.spatial_filter(dev(m), 'median-5').cpu().numpy(), orc.spatial_filter_median5(m))
    f = np.random.default_rng(4).normal(0, 1, (1, 2, 19, 23)).astype(np.float32)
    assert np.array_equal(ops.spatial_filter(dev(f), 'median-5').cpu().numpy(), orc.spatial_filter_median5(f))
    # 'median-3' / 'median-5' against the reference function's own output (models/utils.py:26-36), and the oracle on a 2 x 2 map
    pm = np.load(os.path.join(GOLDEN, "pin_spatial_filter_median.npz"))
    assert np.array_equal(ops.spatial_filter(dev(pm['x']), 'median-3').cpu().numpy(), pm['median3'])
    assert np.array_equal(ops.spatial_filter(dev(pm['x']), 'median-5').cpu().numpy(), pm['median5'])
    tiny = np.array([[[[1.0, 5.0], [3.0, 2.0]]]], np.float32)
    assert np.array_equal(ops.spatial_filter(dev(tiny), 'median-3').cpu().numpy(), orc.spatial_filter_median3(tiny))
    with pytest.raises(ValueError):
        ops.spatial_filter(dev(tiny), 'median-7')


def _frame_case(ops, H, W, seed, extra=0):
    from cartoonsegmentation_amd import synth
    sc = synth.warp_scene(H, W, seed)
    disp_o, depth_o, valid_o, pts_o, un_o = orc.disparity_to_points(sc['disp'], sc['focal'], sc['baseline'])
    dmin = float(depth_o.min()); loc = np.unravel_index(int(depth_o.argmin()), (H, W))
    settings, common = synth.shift_request(sc, dmin, (loc[1], loc[0]))
    shift = ops.shift_vector(settings, common)
    assert np.array_equal(np.asarray(shift, np.float32), orc.shift_vector(settings, common))
    pts = pts_o.reshape(1, 3, -1); rgb = sc['rgb']; dep = depth_o.reshape(1, 1, -1)
    if extra:
        g = np.random.default_rng(seed)
        idx = g.integers(0, H * W, extra)
        pts = np.concatenate([pts, un_o.reshape(1, 3, -1)[:, :, idx] + g.normal(0, 2, (1, 3, extra)).astype(np.float32)], 2)
        rgb = np.concatenate([rgb, rgb[:, :, idx]], 2); dep = np.concatenate([dep, dep[:, :, idx]], 2)
    return sc, pts, rgb, dep, shift


@pytest.mark.parametrize("path", ["tiled", "atomics"])
@pytest.mark.parametrize("H,W,extra", [(96, 128, 0), (250, 333, 5000), (1024, 1024, 0), (1024, 1024, 600000)])
def test_warp_frame_fused_vs_oracle(ops, H, W, extra, path):
    """both frame paths (tile-binned LDS splat / global-atomic chain) against the oracle frame; the second call re-uses the
    scratch (the tile counters must be re-armed by the first)"""
    sc, pts, rgb, dep, shift = _frame_case(ops, H, W, 1234, extra)
    wf = ops.WarpFrame(H, W, 'cuda', keep_render=True, path=path)
    d_pts, d_rgb, d_dep = dev(pts), dev(rgb), dev(dep)
    wf(d_pts, d_rgb, d_dep, sc['focal'], sc['baseline'], [0.5 * v for v in shift])
    frame, render = wf(d_pts, d_rgb, d_dep, sc['focal'], sc['baseline'], shift)
    frame, render = frame.cpu().numpy(), render.cpu().numpy()
    filled_o, existing_o, frame_o = orc.warp_frame(pts, np.concatenate([rgb, dep], 1), H, W, sc['focal'], sc['baseline'],
                                                   np.asarray(shift, np.float32), degrid_mode=1)
    assert (existing_o == 0).mean() > 0.001, "scene must contain disocclusions"
    assert close_frac(render, filled_o) >= 0.999
    diff = np.abs(frame.astype(np.int32) - frame_o.astype(np.int32))
    assert (diff <= 1).mean() >= 0.999 and (diff == 0).mean() >= 0.99
    # unfused operators give the same frame as the fused path
    ps = ops.shift_points(dev(pts), shift)
    r, e = ops.render_pointcloud(ps, dev(np.concatenate([rgb, dep], 1)), W, H, sc['focal'], sc['baseline'])
    f2 = ops.fill_disocclusion(r, r[:, 3:4] * (e > 0.0).float())
    assert close_frac(f2.cpu().numpy(), render, 1e-3, 1e-5) >= 0.9995


def test_tiled_frame_edge_cases(ops):
    """tile path: empty cloud, clouds entirely outside the image / behind the camera, image sizes that are not multiples of the
    32 x 32 tile, a cloud that piles onto a few pixels (one tile gets every entry)"""
    from cartoonsegmentation_amd import synth
    H, W = 45, 70
    wf = ops.WarpFrame(H, W, 'cuda', keep_render=True, path='tiled')
    z3, z1 = torch.zeros(1, 3, 0, device='cuda'), torch.zeros(1, 1, 0, device='cuda')
    frame, render = wf(z3, z3, z1, 35.0, 40.0, [0.0, 0.0, 0.0])
    assert int(frame.max()) == 0 and float(render.abs().max()) == 0.0
    pts = torch.tensor([[[0.0, 1e4, -1e4, 0.0, 3.0], [0.0, 0.0, 0.0, 0.0, 1e5], [-5.0, 10.0, 10.0, 0.0005, 20.0]]], device='cuda')
    frame, render = wf(pts, torch.ones(1, 3, 5, device='cuda'), torch.ones(1, 1, 5, device='cuda'), 35.0, 40.0, [0.0, 0.0, 0.0])
    assert int(frame.max()) == 0
    sc, p, rgb, dep, shift = _frame_case(ops, H, W, 77)
    for path in ('tiled', 'atomics'):
        w2 = ops.WarpFrame(H, W, 'cuda', keep_render=True, path=path)
        fr, rn = w2(dev(p), dev(rgb), dev(dep), sc['focal'], sc['baseline'], shift)
        fo, eo, fro = orc.warp_frame(p, np.concatenate([rgb, dep], 1), H, W, sc['focal'], sc['baseline'], np.asarray(shift, np.float32), 1)
        assert close_frac(rn.cpu().numpy(), fo) >= 0.999, path
        assert (np.abs(fr.cpu().numpy().astype(np.int32) - fro.astype(np.int32)) <= 1).mean() >= 0.999, path
    # pile-up: 20000 points within a 3 x 3 px neighbourhood
    g = np.random.default_rng(5)
    n = 20000
    z = g.uniform(30, 60, n).astype(np.float32)
    xy = g.uniform(-0.02, 0.02, (2, n)).astype(np.float32) * z
    pp = np.stack([xy[0], xy[1], z])[None].astype(np.float32)
    cc = g.uniform(0, 1, (1, 3, n)).astype(np.float32)
    dd = z[None, None].copy()
    fr, rn = wf(dev(pp), dev(cc), dev(dd), 35.0, 40.0, [0.0, 0.0, 0.0])
    fo, eo, fro = orc.warp_frame(pp, np.concatenate([cc, dd], 1), H, W, 35.0, 40.0, np.zeros(3, np.float32), 1)
    assert close_frac(rn.cpu().numpy(), fo, 1e-3, 1e-4) >= 0.999
    assert (np.abs(fr.cpu().numpy().astype(np.int32) - fro.astype(np.int32)) <= 1).mean() >= 0.999
    # the pile-up overflows the tile's fixed-capacity segment (entries go through the spill list): the frame must be reproducible
    # bit for bit (order-free fixed-point sums), and the next, ordinary frame on the same scratch must not see stale spill entries
    fr1, rn1 = fr.clone(), rn.clone()
    fr, rn = wf(dev(pp), dev(cc), dev(dd), 35.0, 40.0, [0.0, 0.0, 0.0])
    assert torch.equal(fr, fr1) and torch.equal(rn, rn1)
    fr, rn = wf(dev(p), dev(rgb), dev(dep), sc['focal'], sc['baseline'], shift)
    w2 = ops.WarpFrame(H, W, 'cuda', keep_render=True, path='tiled')
    fr2, rn2 = w2(dev(p), dev(rgb), dev(dep), sc['focal'], sc['baseline'], shift)
    assert torch.equal(fr, fr2) and torch.equal(rn, rn2)


def test_properties_full_size(ops):
    """size independent properties at BASELINE's 1024x1024: identity warp, linearity in the data,
    z-buffer determinism."""
    H = W = 1024
    sc, pts, rgb, dep, _ = _frame_case(ops, H, W, 4321)
    dpts, drgb = dev(pts), dev(rgb)
    f, b = sc['focal'], sc['baseline']
    r0, e0 = ops.render_pointcloud(dpts, drgb, W, H, f, b)       # no shift: every valid point lands on its own pixel
    valid = (dpts[:, 2:3] > 0).view(1, 1, H, W)
    img = drgb.view(1, 3, H, W)
    m = valid.expand_as(img) & (e0 > 0.999).expand_as(img)
    assert m.float().mean() > 0.5
    assert torch.allclose(r0[m], img[m], rtol=1e-3, atol=2e-3)
    ps = ops.shift_points(dpts, [11.0, -7.0, -3.0])
    z1 = ops.pointrender_update_zee(ps, W, H, f, b); z2 = ops.pointrender_update_zee(ps, W, H, f, b)
    assert torch.equal(z1, z2)
    d2 = torch.rand_like(drgb)
    ra, ea = ops.render_pointcloud(ps, drgb, W, H, f, b)
    rb, eb = ops.render_pointcloud(ps, d2, W, H, f, b)
    rc, ec = ops.render_pointcloud(ps, 0.25 * drgb + 0.5 * d2, W, H, f, b)
    assert torch.equal(ea > 0, ec > 0)
    assert torch.allclose(rc, 0.25 * ra + 0.5 * rb, rtol=1e-3, atol=1e-4)


def test_edge_cases(ops):
    H, W = 20, 30
    empty = torch.zeros(1, 3, 0, device='cuda'); edata = torch.zeros(1, 4, 0, device='cuda')
    r, e = ops.render_pointcloud(empty, edata, W, H, 15.0, 40.0)
    assert float(r.abs().max()) == 0.0 and float(e.abs().max()) == 0.0
    out = ops.fill_disocclusion(r, r[:, 3:4])        # all-hole image: nothing to march to -> unchanged
    assert torch.equal(out, r)
    # points behind the camera / outside the image are skipped (models/utils.py:82, bounds checks)
    pts = torch.tensor([[[0.0, 1e4, -1e4, 0.0], [0.0, 0.0, 0.0, 0.0], [-5.0, 10.0, 10.0, 0.0005]]], device='cuda')
    r, e = ops.render_pointcloud(pts, torch.ones(1, 2, 4, device='cuda'), W, H, 15.0, 40.0)
    assert float(e.sum()) == 0.0
    with pytest.raises(Exception):
        ops.render_pointcloud(torch.zeros(1, 3, 4), torch.zeros(1, 2, 4), W, H, 15.0, 40.0)   # CPU tensors: no fallback


@pytest.mark.parametrize("path", **cases(lambda i: 'c4' in i and 'b2' not in i))
def test_frame_inside_fma_bracket(ops, path):
    """the fused frame kernel vs BOTH ends of the FMA-contraction bracket (fixtures built with -ffp-contract=off and =fast):
    the z-buffer equals both bit for bit, every uint8 value is within one level of one of them wherever the degrid orders agree"""
    g, f = dict(np.load(path)), dict(np.load(path[:-4] + "_fast.npz"))
    H, W = int(g['H']), int(g['W'])
    focal, baseline = float(g['focal']), float(g['baseline'])
    ps = ops.shift_points(dev(g['pts']), [float(v) for v in g['shift']])
    zee = ops.pointrender_update_zee(ps, W, H, focal, baseline).cpu().numpy()
    assert np.array_equal(zee, g['zee_after_zee']) and np.array_equal(zee, f['zee_after_zee'])
    wf = ops.WarpFrame(H, W, torch.device('cuda'), keep_render=False)
    frame, _ = wf(dev(g['pts']), dev(g['data'][:, :3]), dev(g['data'][:, 3:4]), focal, baseline, [float(v) for v in g['shift']])
    fr = frame.cpu().numpy().astype(np.int32)
    near = (np.abs(fr - g['frame'].astype(np.int32)) <= 1) | (np.abs(fr - f['frame'].astype(np.int32)) <= 1)
    # pixels where the Jacobi and the in-place degrid pass differ are the reference's own race; bound them like test_render_pointcloud
    assert near.mean() >= 0.9
    zj = orc.degrid(g['zee_after_zee'], 1)
    same = (zj == g['zee_after_degrid_inplace'])[0, 0]
    r0, e0 = orc.render_pointcloud(g['pts_shift'], g['data'], W, H, focal, baseline, degrid_mode=0)
    r1, e1 = orc.render_pointcloud(g['pts_shift'], g['data'], W, H, focal, baseline, degrid_mode=1)
    agree = same & np.all(np.abs(r0 - r1) <= 1e-6, axis=1)[0] & (g['fill_depth'][0, 0] > 0)
    assert near[agree].mean() >= 0.999



def test_render_pointcloud_68_channels_tiled_vs_atomics_and_oracle(ops):
    """the splat of Inpaint.forward (68 feature channels, pointcloud_inpainting.py:135) on the tile path: same coverage, values
    within float-atomic noise of the global-atomic path and of the oracle, deterministic, scratch re-usable; ragged sizes"""
    rng = np.random.default_rng(5)
    for (H, W, C) in ((96, 130, 68), (41, 57, 13)):
        sc, pts, rgb, dep, _ = _frame_case(ops, H, W, 99 + H)
        ps = ops.shift_points(dev(pts), [3.0, -2.0, -1.5])
        data = dev(rng.normal(0, 3, (1, C, pts.shape[2])).astype(np.float32))
        rt, et = ops.render_pointcloud(ps, data, W, H, sc['focal'], sc['baseline'], path='tiled')
        ra, ea = ops.render_pointcloud(ps, data, W, H, sc['focal'], sc['baseline'], path='atomics')
        assert torch.equal(et > 0, ea > 0)
        assert torch.allclose(et, ea, rtol=1e-5, atol=1e-6)
        assert float(((rt - ra).abs() <= 1e-5 + 1e-4 * ra.abs()).float().mean()) >= 0.9999
        ro, eo = orc.render_pointcloud(ps.cpu().numpy(), data.cpu().numpy(), W, H, sc['focal'], sc['baseline'], degrid_mode=1)
        assert np.array_equal(et.cpu().numpy() > 0, eo > 0)
        assert close_frac(rt.cpu().numpy(), ro) >= 0.999
        rt2, et2 = ops.render_pointcloud(ps, data, W, H, sc['focal'], sc['baseline'], path='tiled')      # same scratch again
        assert torch.equal(rt, rt2) and torch.equal(et, et2)


def test_multi_frame_call_is_bitwise_the_per_frame_calls(ops):
    """csm_warp_frames_tiled: K frames of one cloud dealt onto 1 / 2 / 3 internal streams in ONE call == K csm_warp_frame_tiled calls, bit
    for bit, also when the call is repeated on the same scratch (headers re-armed by every frame) and when K is not a multiple of the
    lane count; K = 0 is a no-op"""
    from cartoonsegmentation_amd import synth
    H, W = 304, 416
    sc = synth.warp_scene(H, W, 77)
    disp = dev(sc['disp']); disp = disp / disp.max() * sc['baseline']
    depth, _, pts, _ = ops.disparity_to_points(disp, sc['focal'], sc['baseline'])
    pts, dep, rgb = pts.view(1, 3, -1).contiguous(), depth.view(1, 1, -1).contiguous(), dev(sc['rgb'])
    shifts = [(3.0 * k - 9.0, 1.5 * k, 0.25 * k) for k in range(7)]
    wf = ops.WarpFrame(H, W, 'cuda', path='tiled')
    ref = torch.stack([wf(pts, rgb, dep, sc['focal'], sc['baseline'], s)[0].clone() for s in shifts])
    assert not torch.equal(ref[0], ref[6])
    for lanes in (1, 2, 3):
        wm = ops.WarpFrame(H, W, 'cuda', path='tiled')
        for rep in range(3):
            got = wm.frames(pts, rgb, dep, sc['focal'], sc['baseline'], shifts, lanes=lanes)
            torch.cuda.synchronize()
            assert torch.equal(got, ref), (lanes, rep)
        assert wm.frames(pts, rgb, dep, sc['focal'], sc['baseline'], [], lanes=lanes).shape[0] == 0
        one = wm.frames(pts, rgb, dep, sc['focal'], sc['baseline'], shifts[2:3], lanes=lanes)
        assert torch.equal(one[0], ref[2])


def test_multi_frame_call_after_the_cloud_changed_size(ops):
    """WarpFrame.frames() keeps its multi-lane scratch for any N up to the capacity, and the library carves the lanes by the CURRENT N:
    after N changes (inpainting appends points) the headers of lanes 1.. lie in bytes the previous call used as storage and must be
    cleared.  N1 -> N2 < N1 -> N1 on one WarpFrame, each bitwise equal to per-frame calls"""
    from cartoonsegmentation_amd import synth
    H, W = 208, 272
    sc = synth.warp_scene(H, W, 5)
    disp = dev(sc['disp']); disp = disp / disp.max() * sc['baseline']
    depth, _, pts, _ = ops.disparity_to_points(disp, sc['focal'], sc['baseline'])
    pts, dep, rgb = pts.view(1, 3, -1).contiguous(), depth.view(1, 1, -1).contiguous(), dev(sc['rgb']).view(1, 3, -1)
    shifts = [(2.5 * k - 6.0, 1.0 * k, 0.2 * k) for k in range(5)]
    wm = ops.WarpFrame(H, W, 'cuda', path='tiled')
    for n_pts in (H * W, H * W - 4001, H * W - 977, H * W):
        p, d, c = pts[:, :, :n_pts].contiguous(), dep[:, :, :n_pts].contiguous(), rgb[:, :, :n_pts].contiguous()
        wf = ops.WarpFrame(H, W, 'cuda', path='tiled')
        ref = torch.stack([wf(p, c, d, sc['focal'], sc['baseline'], s)[0].clone() for s in shifts])
        got = wm.frames(p, c, d, sc['focal'], sc['baseline'], shifts, lanes=3)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), n_pts
