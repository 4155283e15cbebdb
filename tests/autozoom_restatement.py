"""Exact numpy restatement of the autozoom coverage count (csrc/autozoom.hip) -- TEST INFRASTRUCTURE ONLY.

numpy only; nothing from the library or from oracle/.  The count of one candidate shift is `(tenExisting > 0).sum()` of
render_pointcloud(process_shift(points, shift)) with a ones channel (anime_3dkenburns/common.py:110-126): the z-buffer starts at
1e6 (models/utils.py:59), every point puts its fltError on its arg-max corner (:101-147), the z-buffer is degridded in Jacobi form
(:152-212), and a corner adds `1.0 * weight` to `existing` iff `(double)fltError <= (double)zee + 1.0` (:268-310).  The weights
are products of two non-negative factors, so `existing > 0` iff some passing corner has a weight > 0.

What is restated is the reference's statement and nothing of the kernels' organisation: no "certain pixel" shortcut, no fp32
thresholds, no row bands, no candidate groups.  Every decision is exact (one rounding per operation, like warp_device.h built with
-ffp-contract=off), so a count is an integer that has to be met exactly.

The steps are small functions taken as keyword arguments, so that tests/test_autozoom_references.py can swap one of them for a
deliberately wrong one and show that the cases notice.
"""
import numpy as np

from warptile_restatement import D, F, argmax_corner, corner_weights, degrid, process_shift, project


def ztest(err, zd):
    """models/utils.py:269: the mixed-precision z-test of one corner"""
    return err.astype(D) <= zd.astype(D) + 1.0


def positive(w):
    """the ones channel: atomicAdd(existing, 1.0 * w), then existing > 0"""
    return F(1.0) * w > F(0.0)


def keep_all(fx, fy):
    return np.ones(fx.shape, bool)


def zbuffer(pts, shift, H, W, focal, baseline, argmax=argmax_corner, keep=keep_all):
    """updateZee: the z-buffer float32 [H, W] before the degrid, and the geometry (x0, y0, w [4, n], err) of the points it saw"""
    pts = np.asarray(pts, F).reshape(3, -1)
    x, y, z = process_shift(pts, [F(v) for v in shift])
    ok, fx, fy, err = project(x, y, z, H, W, focal, baseline)
    # a NaN coordinate gives four NaN weights (no arg-max branch fires, no weight is > 0) and an infinite one corners outside every
    # image: such points add nothing, and floor() of them is not asked for
    ok &= np.isfinite(fx) & np.isfinite(fy)
    ok &= keep(fx, fy)
    fx, fy, err = fx[ok], fy[ok], err[ok]
    x0, y0, w = corner_weights(fx, fy)
    zee = np.full(H * W, F(1000000.0))                           # models/utils.py:59
    sel = argmax(w)
    cx, cy = x0 + (sel & 1), y0 + (sel >> 1)
    m = (sel >= 0) & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
    np.minimum.at(zee, cy[m] * W + cx[m], err[m])                # :137-147, float atomicMin
    return zee.reshape(H, W), (x0, y0, w, err)


def coverage_mask(pts, shift, H, W, focal, baseline, degrid=degrid, argmax=argmax_corner, ztest=ztest, positive=positive, keep=keep_all):
    """bool [H, W]: the pixels with `existing > 0` for the cloud pts [3, N] moved by shift (sx, sy, sz)"""
    zee, (x0, y0, w, err) = zbuffer(pts, shift, H, W, focal, baseline, argmax=argmax, keep=keep)
    zd = degrid(zee).ravel()
    mask = np.zeros(H * W, bool)
    for k in range(4):                                           # NW, NE, SW, SE (:268-310)
        cx, cy = x0 + (k & 1), y0 + (k >> 1)
        inimg = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        pix = np.where(inimg, cy * W + cx, 0)
        take = inimg & ztest(err, zd[pix]) & positive(w[k])
        mask[pix[take]] = True
    return mask.reshape(H, W)


def count_mask(mask):
    return int(mask.sum())


def coverage_counts(pts, shifts, H, W, focal, baseline, count=count_mask, **steps):
    """the K counts of ops.autozoom_coverage as Python ints; shifts are rounded to fp32 like FloatTensor(shift) (common.py:74)"""
    s32 = np.asarray([[float(v) for v in s] for s in shifts], D).reshape(-1, 3).astype(F)
    return [count(coverage_mask(pts, s, H, W, focal, baseline, **steps)) for s in s32]
