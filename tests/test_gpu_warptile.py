"""GPU: the tiled point-cloud renderer (csrc/warptile.hip) is bit for bit its numpy restatement (tests/warptile_restatement.py) on
the cases of tests/warptile_cases.py -- through WarpFrame.__call__, WarpFrame.frames and render_pointcloud(path='tiled') -- and the
float-atomic path (csrc/warp.hip) takes the same decisions and stays, pixel by pixel, within the bound derived in warptile_cases.
No assertion here is a fraction of pixels."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warptile_cases as K  # noqa: E402

NAMES = list(K.CASES)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from cartoonsegmentation_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(got, want, what):
    """every element equal bit for bit; the message names how many differ and the first one"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%s: %d of %d values differ, first at %s: got %r, want %r" % (what, int(bad.sum()), bad.size, i, got[i], want[i]))


def _cloud(c):
    return dev(c['pts'][None]), dev(c['rgb'][None]), dev(c['depth'][None])


def _frame(wf, c, shift=None):
    frame, render = wf(*_cloud(c), c['focal'], c['baseline'], list(c['shift'] if shift is None else shift))
    return frame.cpu().numpy(), render.cpu().numpy()[0]


# ---- a. frame path -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_frame_is_the_restatement(ops, name):
    c, rs = K.case(name), K.restated(name)
    wf = ops.WarpFrame(c['H'], c['W'], 'cuda', keep_render=True, path='tiled')
    for call in (1, 2):                                      # the second call runs on the scratch the first one left
        frame, render = _frame(wf, c)
        same_bits(render, rs['render_filled'], "%s render, call %d" % (name, call))
        same_bits(frame, rs['frame'], "%s frame, call %d" % (name, call))
    if name == 'spill':                                      # an ordinary frame after the one that went through the spill list
        c2, r2 = K.case('seams'), K.restated('seams')
        frame, render = _frame(wf, c2)
        same_bits(render, r2['render_filled'], "seams render after spill")
        same_bits(frame, r2['frame'], "seams frame after spill")


# ---- b. multi-frame call -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2, 3])
@pytest.mark.parametrize("name", ['seams', 'patched_grid'])
def test_frames_call_is_the_restatement_of_every_shift(ops, name, lanes):
    c = K.case(name)
    wf = ops.WarpFrame(c['H'], c['W'], 'cuda', path='tiled')
    for call in (1, 2):
        got = wf.frames(*_cloud(c), c['focal'], c['baseline'], [list(s) for s in K.MULTI_SHIFTS], lanes=lanes).cpu().numpy()
        assert got.shape[0] == len(K.MULTI_SHIFTS)
        for k, s in enumerate(K.MULTI_SHIFTS):
            same_bits(got[k], K.restated(name, s)['frame'], "%s frame %d of the call, lanes %d, call %d" % (name, k, lanes, call))


# ---- c. channel path ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", K.CHANNEL_COUNTS)
@pytest.mark.parametrize("name", K.CHANNEL_CASES)
def test_channel_render_is_the_restatement(ops, name, C):
    """signed data, channel groups of 8 with C not a multiple of 8, one saturating contribution in channel 0"""
    c, rs = K.case(name), K.restated_channels(name, C, True)
    ps, data = dev(K.shifted_points(name)[None]), dev(K.channel_data(name, True)[None, :C])
    for call in (1, 2):
        render, existing = ops.render_pointcloud(ps, data, c['W'], c['H'], c['focal'], c['baseline'], path='tiled')
        same_bits(existing.cpu().numpy()[0, 0], rs['existing'], "%s existing, C %d, call %d" % (name, C, call))
        same_bits(render.cpu().numpy()[0], rs['render'], "%s render, C %d, call %d" % (name, C, call))


# ---- d. float-atomic path ----------------------------------------------------------------------------------------------------------

def within(got, rs, what, planes=None):
    """every value within the derived bound of the exact quotient"""
    q, b = K.exact_quotient(rs), K.float_bound(rs)
    if planes is not None:
        q, b = q[planes], b[planes]
    off = np.abs(got.astype(np.float64) - q)
    bad = ~(off <= b)
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%s: %d values beyond the bound, first at %s: got %r, exact %r, bound %r" % (what, int(bad.sum()), i, got[i], q[i], b[i]))


@pytest.mark.parametrize("name", NAMES)
def test_atomic_frame_path_is_held_to_the_exact_sums(ops, name):
    c, rs = K.case(name), K.restated(name)
    H, W = c['H'], c['W']
    # decisions, through the operator: coverage and the set of holes
    rgbd = np.concatenate([c['rgb'], c['depth']])
    r, e = ops.render_pointcloud(dev(K.shifted_points(name)[None]), dev(rgbd[None]), W, H, c['focal'], c['baseline'], path='atomics')
    r, e = r.cpu().numpy()[0], e.cpu().numpy()[0, 0]
    assert np.array_equal(e > 0, rs['existing'] > 0)
    assert np.array_equal((r[3] * (e > 0).astype(np.float32)).astype(np.float64) > 0.0, rs['valid'])
    within(r, rs, name + " render_pointcloud(atomics)")
    n = np.where(rs['nz'] > 1, rs['nz'], 0)
    assert np.all(np.abs(e.astype(np.float64) - rs['S'][4]) <= n * 2.0 ** -23 * rs['S'][4])
    # the fused frame
    wf = ops.WarpFrame(H, W, 'cuda', keep_render=True, path='atomics')
    frame, render = _frame(wf, c)
    h = rs['holes']; h = h[h[:, 6] >= 0]
    own = np.ones((H, W), bool); own[h[:, 0], h[:, 1]] = False         # pixels that carry their own sums: valid ones and kept holes
    q, b = K.exact_quotient(rs), K.float_bound(rs)
    off = np.abs(render.astype(np.float64) - q)
    assert np.all(off[:, own] <= b[:, own]), (name, float((off - b)[:, own].max()))
    lo, hi = K.u8_levels(rs)
    fr = frame.transpose(2, 0, 1)
    assert np.all((fr >= lo)[:, own] & (fr <= hi)[:, own])
    # a filled hole carries the path's own values at the source the restatement chose
    same_bits(render[:, h[:, 0], h[:, 1]], render[:, h[:, 6], h[:, 7]], name + " filled holes, render")
    same_bits(frame[h[:, 0], h[:, 1]], frame[h[:, 6], h[:, 7]], name + " filled holes, frame")


@pytest.mark.parametrize("C", K.CHANNEL_COUNTS)
@pytest.mark.parametrize("name", K.CHANNEL_CASES)
def test_atomic_channel_path_is_held_to_the_exact_sums(ops, name, C):
    """the same data without the saturating contribution (the float path keeps IEEE semantics there)"""
    c, rs = K.case(name), K.restated_channels(name, C, False)
    ps, data = dev(K.shifted_points(name)[None]), dev(K.channel_data(name, False)[None, :C])
    render, existing = ops.render_pointcloud(ps, data, c['W'], c['H'], c['focal'], c['baseline'], path='atomics')
    e = existing.cpu().numpy()[0, 0]
    assert np.array_equal(e > 0, rs['existing'] > 0)
    within(render.cpu().numpy()[0], rs, "%s render_pointcloud(atomics), C %d" % (name, C))
    n = np.where(rs['nz'] > 1, rs['nz'], 0)
    assert np.all(np.abs(e.astype(np.float64) - rs['S'][-1]) <= n * 2.0 ** -23 * rs['S'][-1])
