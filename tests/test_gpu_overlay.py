"""GPU: instance overlays drawn on the device (csrc/overlay.hip) against tests/overlay_restatement.py on every byte;
the reference's own picture (tests/golden/pin_draw_instances.npz); the argument checks of the
C ABI; and the surfaces: ops.draw_instances(_many), AnimeInstances.draw_instances(on_device=True) / save_visualization,
AnimeInsSeg.save_visualization and _infer_save_annotations(save_visualization_only=True)."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_restatement as R  # noqa: E402
from overlay_cases import CASES, case  # noqa: E402
from test_overlay import fixture  # noqa: E402

CSM_OK, CSM_ERR_ARG = 0, 1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _want(img, masks, boxes, kw):
    kw = dict(kw)
    return R.draw(img, masks, boxes, line_width_=kw.pop('line_width', None), **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_restatement(name):
    from cartoonsegmentation_amd import ops
    img, masks, boxes, kw = case(name)
    want = _want(img, masks, boxes, kw)
    got = ops.draw_instances(_dev(img), _dev(masks), _dev(boxes), **kw)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == img.shape
    assert np.array_equal(got.cpu().numpy(), want)
    again = ops.draw_instances(img, _dev(masks.astype(np.uint8)), boxes, **kw)       # a host frame and boxes, 0 / 1 uint8 masks
    assert torch.equal(again, got)
    if name == 'no-indices' or name == 'n0':
        assert np.array_equal(want, img)
    # pixels outside every listed mask and every listed band are the frame's
    idx = kw.get('indices', range(len(masks)))
    touched = np.zeros(img.shape[:2], bool)
    for i in idx:
        touched |= masks[i] | R.band(img.shape[0], img.shape[1], boxes[i], kw.get('line_width', R.line_width(*img.shape[:2])))
    assert np.array_equal(got.cpu().numpy()[~touched], img[~touched])


def test_device_equals_the_references_picture():
    from cartoonsegmentation_amd import ops
    from cartoonsegmentation_amd.anime_instances import AnimeInstances
    img, masks, boxes, drawn, order, drawn_order = fixture()
    assert np.array_equal(ops.draw_instances(_dev(img), _dev(masks), _dev(boxes), draw_bbox=False).cpu().numpy(), drawn)
    assert np.array_equal(ops.draw_instances(_dev(img), _dev(masks), _dev(boxes), draw_bbox=False, indices=order).cpu().numpy(), drawn_order)
    for inst in (AnimeInstances(masks=masks, bboxes=boxes), AnimeInstances(masks=_dev(masks), bboxes=_dev(boxes))):
        got = inst.draw_instances(img, draw_bbox=False, mask_alpha=0.4, draw_tags=True, on_device=True)   # alpha is 0.75 whatever is asked
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), drawn)
        assert np.array_equal(inst.draw_instances(_dev(img), on_device=True).cpu().numpy(), R.draw(img, masks, boxes))
    assert np.array_equal(AnimeInstances().draw_instances(img, on_device=True).cpu().numpy(), img)


def test_many_frames_of_different_sizes_equal_each_frame_alone():
    from cartoonsegmentation_amd import ops
    names = ['5x7', '64x256-tiles', '33x61', 'n0']
    data = [case(nm) for nm in names]
    frames = [_dev(d[0]) for d in data]
    insts = [(_dev(d[1]), _dev(d[2])) for d in data]
    indices = [None, [6, 0, 3, 3], None, None]
    colors = [None, None, np.arange(27, dtype=np.uint8).reshape(9, 3), None]
    for kw in ({}, {'draw_ins_contour': True, 'mask_alpha': 0.3, 'line_width': 3}):
        many = ops.draw_instances_many(frames, insts, indices=indices, colors=colors, **kw)
        again = ops.draw_instances_many(frames, insts, indices=indices, colors=colors, **kw)
        assert len(many) == 4
        for k, d in enumerate(data):
            alone = ops.draw_instances(frames[k], *insts[k], indices=indices[k], colors=colors[k], **kw)
            assert torch.equal(many[k], alone) and torch.equal(again[k], alone), names[k]
            assert np.array_equal(alone.cpu().numpy(), R.draw(d[0], d[1], d[2], colors=colors[k], indices=indices[k],
                                                              draw_ins_contour=kw.get('draw_ins_contour', False),
                                                              mask_alpha=kw.get('mask_alpha', 0.75), line_width_=kw.get('line_width')))
    assert ops.draw_instances_many([], []) == []


def test_python_refusals():
    from cartoonsegmentation_amd import ops
    img, masks, boxes, _ = case('33x61')
    with pytest.raises(ValueError, match=r"cv2\.resize\(INTER_AREA\)"):
        ops.draw_instances(_dev(img[:30]), _dev(masks), _dev(boxes))
    for bad in ([9], [-1], [0, 3, 12]):
        with pytest.raises(ValueError, match="indices"):
            ops.draw_instances(_dev(img), _dev(masks), _dev(boxes), indices=bad)
    with pytest.raises(ValueError):
        ops.draw_instances(_dev(img), _dev(masks), _dev(boxes), colors=np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError):
        ops.draw_instances(_dev(img), _dev(masks), _dev(boxes), line_width=0)
    with pytest.raises(ValueError):
        ops.draw_instances_many([_dev(img)], [])


def test_c_abi_refuses_bad_arguments():
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import f32, i32, ptr, stream_ptr
    L = _lib.load()
    words = L.csm_overlay_job_words()
    assert words == 16
    img, masks, boxes, _ = case('33x61')
    H, W, n = 33, 61, len(masks)
    im, m, b, out = _dev(img), _dev(masks.view(np.uint8)), _dev(boxes), torch.zeros((H, W, 3), dtype=torch.uint8, device='cuda')
    ent = np.array([0, 8, 2], np.int32)
    ent_d, col_d = _dev(ent), _dev(np.full((3, 3), 9, np.uint8))
    i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)

    def table(**kw):
        row = dict(img=im.data_ptr(), out=out.data_ptr(), masks=m.data_ptr(), boxes=b.data_ptr(), H=H, W=W, n=n, k=3, first=0, line=2)
        row.update(kw)
        return np.array([[row[key] for key in ('img', 'out', 'masks', 'boxes', 'H', 'W', 'n', 'k', 'first', 'line')] + [0] * 6], np.int64)

    def plan(jobs, n_jobs=1, n_entries=3):
        return L.csm_overlay_plan(None if jobs is None else jobs.ctypes.data_as(i64p), i32(n_jobs), i32(n_entries))

    def draw(jobs, entries=ent, n_jobs=1, n_entries=3, flags=3, jobs_dev=True, entries_dev=True):
        jd = _dev(good if jobs is None else jobs) if jobs_dev else None
        rc = L.csm_draw_instances(None if jobs is None else jobs.ctypes.data_as(i64p), ptr(jd), i32(n_jobs),
                                  None if entries is None else entries.ctypes.data_as(i32p), ptr(ent_d if entries_dev else None), ptr(col_d),
                                  i32(n_entries), i32(flags), f32(0.75), f32(0.25), stream_ptr())
        torch.cuda.synchronize()
        return rc

    good = table()
    assert plan(good) == 5 and draw(good) == CSM_OK and out.any()                     # 33 x 61: one tile across, five down
    out.zero_()
    assert plan(None) == 0 and plan(good, n_jobs=0) == 0 and plan(good, n_entries=-1) == 0
    for kw in (dict(img=0), dict(out=0), dict(masks=0), dict(boxes=0), dict(H=0), dict(W=-61), dict(n=-1), dict(k=-3), dict(first=-1),
               dict(first=1), dict(k=4), dict(line=0), dict(out=im.data_ptr())):      # first / k: a draw list outside the entry table
        assert plan(table(**kw)) == 0, kw
        bad = good.copy()
        bad[0, :10] = table(**kw)[0, :10]
        assert draw(bad) == CSM_ERR_ARG, kw
    assert draw(table()) == CSM_ERR_ARG                                               # a table that csm_overlay_plan has not filled
    assert draw(good, n_jobs=-1) == CSM_ERR_ARG and draw(good, n_entries=-1) == CSM_ERR_ARG and draw(good, flags=8) == CSM_ERR_ARG
    assert draw(None) == CSM_ERR_ARG and draw(good, jobs_dev=False) == CSM_ERR_ARG
    assert draw(good, entries=None) == CSM_ERR_ARG and draw(good, entries_dev=False) == CSM_ERR_ARG
    for outside in ([0, 9, 2], [0, -1, 2]):                                           # an entry outside its frame's masks
        assert draw(good, entries=np.array(outside, np.int32)) == CSM_ERR_ARG
    small = plan(table(n=2))                                                          # fewer masks than the entries name
    assert small > 0 and draw(np.concatenate([table(n=2)[:, :10], good[:, 10:]], 1)) == CSM_ERR_ARG
    assert not out.any()                                                              # nothing was launched by a refused call
    assert draw(good, n_jobs=0) == CSM_OK and not out.any()
    assert draw(good) == CSM_OK
    assert np.array_equal(out.cpu().numpy(), R.draw(img, masks, boxes, indices=[0, 8, 2], colors=[(9, 9, 9)] * 3))


# ---- end to end, synthetic weights at a small detector size -------------------------------------------------------------------------
def _read_bgr(path_or_bytes):
    from PIL import Image
    im = Image.open(io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, bytes) else str(path_or_bytes))
    return np.asarray(im.convert('RGB'))[..., ::-1]


@pytest.fixture(scope='module')
def net_and_frames():
    from animeinsseg import AnimeInsSeg
    from cartoonsegmentation_amd import synth
    os.environ['CSM_DET_BATCH'] = '2'
    try:
        net = AnimeInsSeg('synthetic', default_det_size=96, refine_kwargs={'refine_method': 'refinenet_isnet', 'refine_size': 64})
    finally:
        del os.environ['CSM_DET_BATCH']
    assert net.det_batch == 2
    net.set_max_instance(3)
    return net, [synth.image_u8(160, 192, 50 + k) for k in range(2)] + [synth.image_u8(120, 136, 52)]


def test_save_visualization_files(net_and_frames, tmp_path):
    from cartoonsegmentation_amd import ops
    from utils.io_utils import imwrite
    net, imgs = net_and_frames
    inst = net.infer(imgs[0], pred_score_thr=0.0, max_instances=3)
    assert len(inst) >= 1 and inst.is_cuda
    drawn = inst.draw_instances(imgs[0], on_device=True)
    assert np.array_equal(drawn.cpu().numpy(), R.draw(imgs[0], inst.masks.cpu().numpy(), inst.bboxes.cpu().numpy()))
    assert not np.array_equal(drawn.cpu().numpy(), imgs[0])
    png, jpg, webp = (str(tmp_path / "sub" / ("v" + s)) for s in ('.png', '.jpg', '.webp'))
    for p in (png, jpg, webp):
        net.save_visualization(p, imgs[0], inst)
    assert np.array_equal(_read_bgr(png), drawn.cpu().numpy()) and np.array_equal(_read_bgr(webp), drawn.cpu().numpy())
    assert open(jpg, 'rb').read() == ops.jpeg_encode(drawn, quality=95, subsampling='420')[0]
    assert inst.save_visualization(_dev(imgs[0]), str(tmp_path / "again.png")) is True
    assert open(str(tmp_path / "again.png"), 'rb').read() == open(png, 'rb').read()
    with pytest.raises(ValueError):
        net.save_visualization(str(tmp_path / "v.bmp"), imgs[0], inst)
    assert not (tmp_path / "v.bmp").exists()
    assert imwrite(drawn, str(tmp_path / "direct.png")) and open(str(tmp_path / "direct.png"), 'rb').read() == open(png, 'rb').read()


def test_save_visualization_only(net_and_frames, tmp_path):
    from PIL import Image
    net, imgs = net_and_frames
    src = tmp_path / "src"
    src.mkdir()
    names = ['b.png', 'a.png', 'c.png']
    for nm, im in zip(names, imgs):
        Image.fromarray(im[..., ::-1]).save(str(src / nm))
    paths = [str(src / nm) for nm in names]
    before = {nm: (src / nm).read_bytes() for nm in names}
    sd, js = tmp_path / "sd", tmp_path / "pred.json"
    assert net._infer_save_annotations(paths, 0.0, str(sd), str(js), -1, -1, None, save_visualization_only=True) is None
    assert sorted(os.listdir(str(sd))) == sorted(names) and not js.exists()
    differs = 0
    for nm, p, im in zip(names, paths, imgs):
        one = tmp_path / ("one_" + nm[0])
        net._infer_save_annotations([p], 0.0, str(one), str(js), -1, -1, None, save_visualization_only=True)
        assert os.listdir(str(one)) == [nm] and (one / nm).read_bytes() == (sd / nm).read_bytes()
        inst = net.infer(p, pred_score_thr=0.0, max_instances=3)
        assert np.array_equal(_read_bgr(sd / nm), inst.draw_instances(im, on_device=True).cpu().numpy())
        differs += not np.array_equal(_read_bgr(sd / nm), im)
    assert differs >= 1 and not js.exists()
    # arrays are named by their position, as in the annotation export
    arr = tmp_path / "arr"
    net._infer_save_annotations(imgs[:1], 0.0, str(arr), str(js), -1, -1, None, save_visualization_only=True)
    assert os.listdir(str(arr)) == ['%012d.jpg' % 0]
    # a save_dir that is the images' own directory: refused before anything is written
    for same in (str(src), str(src) + os.sep + '.'):
        with pytest.raises(ValueError):
            net._infer_save_annotations(paths, 0.0, same, str(js), -1, -1, None, save_visualization_only=True)
    assert {nm: (src / nm).read_bytes() for nm in names} == before and sorted(os.listdir(str(src))) == sorted(names)
    with pytest.raises(NotImplementedError):
        net.infer(paths[0], save_visualization=True)
