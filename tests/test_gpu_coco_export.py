"""GPU: COCO RLE on the device (csm_mask_rle_measure / _write, ops.mask_rle_encode, utils.io_utils.mask2rle) byte-exact against
the restatement of pycocotools' rleEncode + rleToString, and AnimeInsSeg.infer(save_annotation=...) equal, as text, to the file
the reference's _infer_save_annotations (animeinsseg/__init__.py:506-621) builds from infer() results with that restatement."""
import json
import os

import numpy as np
import pytest

from test_coco_export import rle_counts_ref, rle_decode_ref, rle_encode_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _device_rle(masks_u8):
    """the raw C ABI: (strings, info [n,4])"""
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd._lib import check, i32, ptr, stream_ptr
    L = _lib.load()
    m = torch.from_numpy(np.ascontiguousarray(masks_u8, dtype=np.uint8)).cuda()
    n, H, W = m.shape
    info = torch.full((n, 4), -7, dtype=torch.int64, device='cuda')
    scratch = torch.empty(L.csm_mask_rle_scratch_bytes(i32(n), i32(H), i32(W)), dtype=torch.uint8, device='cuda')
    check(L.csm_mask_rle_measure(ptr(m), i32(n), i32(H), i32(W), ptr(info), ptr(scratch), stream_ptr()), "measure")
    ih = info.cpu().numpy()
    total = int(ih[-1, 3] + ih[-1, 1])
    out = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device='cuda')       # guard bytes behind the strings
    check(L.csm_mask_rle_write(ptr(m), i32(n), i32(H), i32(W), ptr(info), ptr(out), ptr(scratch), stream_ptr()), "write")
    oh = out.cpu().numpy()
    assert (oh[total:] == 0xEE).all()
    blob = oh[:total].tobytes()
    assert all(48 <= b < 112 for b in blob)
    return [blob[o:o + b].decode() for o, b in zip(ih[:, 3], ih[:, 1])], ih


def _check(masks):
    strs, ih = _device_rle(masks)
    off = 0
    for k, m in enumerate(masks):
        cnts = rle_counts_ref(m)
        want = rle_encode_ref(m)
        assert strs[k] == want, (k, m.shape, strs[k][:80], want[:80])
        assert ih[k, 0] == len(cnts) and ih[k, 1] == len(want) and ih[k, 2] == int((m > 0).sum()) and ih[k, 3] == off
        off += len(want)


def _patterns(H, W, rng):
    ms = [np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)]
    first = np.zeros((H, W), np.uint8)
    first[0, 0] = 1
    ms.append(first)
    for d in (0.01, 0.5, 0.99):
        ms.append(((rng.random((H, W)) < d) * int(rng.choice([1, 255]))).astype(np.uint8))
    hb = np.zeros((H, W), np.uint8)
    hb[(np.arange(H) // 3) % 2 == 1] = 1
    vb = np.zeros((H, W), np.uint8)
    vb[:, (np.arange(W) // 5) % 2 == 0] = 7
    late = np.zeros((H, W), np.uint8)                               # empty for most columns: carries cross hundreds of columns
    late[:, (3 * W) // 4:] = rng.random((H, W - (3 * W) // 4)) < 0.3
    late[H // 2, W // 3] = 1
    return ms + [hb, vb, late]


@pytest.mark.parametrize("H,W", [(1, 1), (1, 300), (300, 1), (37, 53), (517, 333), (750, 1000), (1024, 1024)])
def test_device_rle_is_byte_exact(H, W):
    _check(np.stack(_patterns(H, W, np.random.default_rng(H * 7 + W))))


def test_checkerboard_and_long_counts():
    y, x = np.mgrid[:1024, :1024]
    cb = ((y + x) % 2).astype(np.uint8)
    strs, ih = _device_rle(cb[None])
    assert ih[0, 0] == len(rle_counts_ref(cb)) > 1_000_000 and strs[0] == rle_encode_ref(cb)
    # counts above 2^20: multi-character values and large negative deltas
    big = np.zeros((3, 1100, 1000), np.uint8)
    big[0, 1, 2] = big[0, 1099, 999] = big[0, 500, 3] = 1
    big[1, -1, -1] = 1
    big[2, :, 990:] = 1
    big[2, 7, 0] = 1
    _check(big)
    assert max(rle_counts_ref(big[1])) > 2 ** 20


def test_many_instances_in_one_call():
    rng = np.random.default_rng(3)
    for n in (1, 2, 100):
        ms = (rng.random((n, 61, 47)) < rng.random((n, 1, 1))).astype(np.uint8)
        ms[::7] = 0
        ms[1::9, :, :20] = 0
        _check(ms)


def test_ops_and_mask2rle():
    from cartoonsegmentation_amd import ops
    from utils.io_utils import mask2rle
    rng = np.random.default_rng(4)
    m = ((rng.random((90, 70)) < 0.4) * 255).astype(np.uint8)
    want = rle_encode_ref(m)
    assert mask2rle(m) == {'size': [90, 70], 'counts': want}
    assert list(mask2rle(m).keys()) == ['size', 'counts']
    assert mask2rle(m, decode_for_json=False) == {'size': [90, 70], 'counts': want.encode()}
    t = torch.from_numpy(m > 0).cuda()
    assert mask2rle(t) == {'size': [90, 70], 'counts': want}
    counts, areas = ops.mask_rle_encode(torch.stack([t, ~t]))
    assert counts == [want, rle_encode_ref(m == 0)] and areas.tolist() == [int((m > 0).sum()), int((m == 0).sum())]
    assert ops.mask_rle_encode(torch.zeros((0, 5, 5), dtype=torch.bool, device='cuda'))[0] == []
    from cartoonsegmentation_amd._lib import CsmError
    with pytest.raises(CsmError):
        ops.mask_rle_encode(torch.from_numpy(m))


# ---- infer(save_annotation=...) ------------------------------------------------------------------------------------------

def restated_export(net, imgs, infer_kw, obj_id_start=-1, img_id_start=-1, names=None, ids=None):
    """reference _infer_save_annotations (:547-621) over infer() results, with the CPU RLE; imgs: BGR arrays in file order"""
    from utils.constants import CATEGORIES
    from utils.io_utils import NumpyEncoder
    results = net.infer(list(imgs), **infer_kw)
    image_meta, det_annotations = [], []
    obj_id, image_id = obj_id_start + 1, img_id_start + 1
    for ii, (img, instances) in enumerate(zip(imgs, results)):
        img_name = names[ii] if names is not None else f'{ii}'.zfill(12) + '.jpg'
        if ids is not None:
            image_id = ids[ii]
        im_h, im_w = img.shape[:2]
        image_meta.append({"id": image_id, "height": im_h, "width": im_w, "file_name": img_name, "id": image_id})  # noqa: F601
        for k in range(len(instances)):
            segmentation = instances.masks[k].squeeze().cpu().numpy().astype(np.uint8)
            area = segmentation.sum()
            segmentation *= 255
            score = instances.scores[k]
            if isinstance(score, torch.Tensor):
                score = score.item()
            score = float(score)
            bbox = instances.bboxes[k].cpu().numpy().astype(np.float32).tolist()
            rle = {'size': list(segmentation.shape), 'counts': rle_encode_ref(segmentation)}
            det_annotations.append({'id': obj_id, 'category_id': 0, 'iscrowd': 0, 'score': score, 'segmentation': rle,
                                    'image_id': image_id, 'area': area, 'tag_string': instances.tags[k],
                                    'tag_string_character': instances.character_tags[k], 'bbox': bbox})
            obj_id += 1
        image_id += 1
    d = {"info": {}, "licenses": [], "images": image_meta, "annotations": det_annotations, "categories": CATEGORIES}
    return json.dumps(d, ensure_ascii=False, cls=NumpyEncoder), results


def _check_file(path, want_txt, results):
    txt = open(path, encoding='utf-8').read()
    assert txt == want_txt
    d = json.loads(txt)
    anns = iter(d['annotations'])
    for res in results:
        for k in range(len(res)):
            a = next(anns)
            h, w = a['segmentation']['size']
            assert np.array_equal(rle_decode_ref(a['segmentation']['counts'], h, w), res.masks[k].cpu().numpy().astype(np.uint8))
    return d


def _net(method):
    from animeinsseg import AnimeInsSeg
    kw = {'none': {'refine_method': 'none'}, 'refinenet_isnet': {'refine_method': 'refinenet_isnet', 'refine_size': 48},
          'animeseg': {'refine_method': 'animeseg', 'refine_size': 64}}[method]
    return AnimeInsSeg('synthetic', default_det_size=64, refine_kwargs=kw)


def _thr_kw(net):
    """equal-size synthetic frames and a score threshold at which some of them keep instances and at least one keeps none: the
    threshold lies between the two lowest best-scores of the frames"""
    from cartoonsegmentation_amd import synth
    cands = [synth.image_u8(64, 96, 50 + k) for k in range(24)] + [np.zeros((64, 96, 3), np.uint8), np.full((64, 96, 3), 200, np.uint8)]
    res = net.infer(cands, pred_score_thr=0.0, max_instances=3, output_type='numpy')
    top = [float(r.scores.max()) if len(r) else -1.0 for r in res]
    levels = sorted(set(top))
    for lo, hi in zip(levels, levels[1:]):
        thr = float(np.float32((max(lo, 0.0) + hi) / 2))
        full = [c for c, t in zip(cands, top) if np.float32(t) > np.float32(thr)]
        empty = [c for c, t in zip(cands, top) if not np.float32(t) > np.float32(thr)]
        if len(full) >= 4 and empty:
            return dict(pred_score_thr=thr, max_instances=3), full, empty
    raise AssertionError("no threshold splits the synthetic frames into empty and non-empty ones: %s" % top)


@pytest.mark.parametrize("method", ['none', 'refinenet_isnet', 'animeseg'])
def test_export_of_an_array_list_matches_the_reference(tmp_path, method):
    from cartoonsegmentation_amd import synth
    net = _net(method)
    kw, full, empty = _thr_kw(net)
    odd = synth.image_u8(64, 130, 9)                          # detector masks 2 px narrower than the frame (ceil(S / scale))
    imgs = [full[0], empty[0], odd, full[1], synth.image_u8(134, 66, 4)]
    want, results = restated_export(net, imgs, kw, obj_id_start=41, img_id_start=1000)
    assert any(len(r) == 0 for r in results) and sum(len(r) for r in results) >= 2
    if method == 'none' and len(results[2]):
        assert tuple(results[2].masks.shape[1:]) == (64, 128)
    out = tmp_path / 'pred.json'
    sd = tmp_path / 'sd'
    assert net.infer(imgs, save_annotation=str(out), save_dir=str(sd), obj_id_start=41, img_id_start=1000, **kw) is None
    assert sd.is_dir()
    d = _check_file(out, want, results)
    assert d['images'][0]['id'] == 1001 and d['annotations'][0]['id'] == 42
    assert d['images'][1]['file_name'] == '000000000001.jpg'
    assert list(d['annotations'][0].keys()) == ['id', 'category_id', 'iscrowd', 'score', 'segmentation', 'image_id', 'area',
                                                'tag_string', 'tag_string_character', 'bbox']
    # default ids; equally sized frames take the batched detector / refine path
    want, results = restated_export(net, full[:3] + empty[:1], kw)
    net.infer(full[:3] + empty[:1], save_annotation=str(out), save_dir=str(sd), **kw)
    assert _check_file(out, want, results)['images'][0]['id'] == 0


def test_export_of_a_directory_a_txt_list_and_coco_json(tmp_path, monkeypatch):
    from PIL import Image
    from utils.io_utils import find_all_imgs, imread
    net = _net('refinenet_isnet')
    kw, full, empty = _thr_kw(net)
    root = tmp_path / 'ds'
    (root / 'val').mkdir(parents=True)
    (root / 'annotations').mkdir()
    names = ['b.png', 'a.png', 'c.png', 'z.png']
    for im, nm in zip(full[:3] + empty[:1], names):
        Image.fromarray(im[..., ::-1]).save(str(root / 'val' / nm))
    # a directory: target_dir = the directory, save_dir = <dir>/<ckpt name> (created)
    order = find_all_imgs(str(root / 'val'), abs_path=True)
    want, res = restated_export(net, [imread(p) for p in order], kw, names=[os.path.basename(p) for p in order])
    out = tmp_path / 'dir.json'
    assert net.infer(str(root / 'val'), save_annotation=str(out), **kw) is None
    _check_file(out, want, res)
    assert (root / 'val' / 'synthetic').is_dir()
    # a .txt list of paths (plain infer accepts it as well); save_dir defaults under ./workspace/output
    lst = [str(root / 'val' / nm) for nm in ['c.png', 'z.png', 'a.png']]
    (tmp_path / 'list.txt').write_text('\n'.join(lst))
    monkeypatch.chdir(tmp_path)
    want, res = restated_export(net, [imread(p) for p in lst], kw, obj_id_start=9, img_id_start=99, names=['c.png', 'z.png', 'a.png'])
    net.infer(str(tmp_path / 'list.txt'), save_annotation=str(out), obj_id_start=9, img_id_start=99, **kw)
    _check_file(out, want, res)
    assert (tmp_path / 'workspace' / 'output' / 'synthetic').is_dir()
    plain = net.infer(str(tmp_path / 'list.txt'), output_type='numpy', **kw)
    assert isinstance(plain, list) and [len(p) for p in plain] == [len(r) for r in res]
    # a COCO json: image ids from the file, val_dir default dirname(dirname(json))/val, or explicit
    jp = root / 'annotations' / 'inst.json'
    jp.write_text(json.dumps({'images': [{'id': 31, 'file_name': 'a.png'}, {'id': 5, 'file_name': 'z.png'},
                                         {'id': 12, 'file_name': 'b.png'}], 'annotations': [], 'categories': []}))
    seq = ['a.png', 'z.png', 'b.png']
    want, res = restated_export(net, [imread(str(root / 'val' / s)) for s in seq], kw, names=seq, ids=[31, 5, 12])
    net.infer(str(jp), save_annotation=str(out), **kw)
    d = _check_file(out, want, res)
    assert [im['id'] for im in d['images']] == [31, 5, 12]
    other = tmp_path / 'elsewhere'
    other.mkdir()
    for s in seq:
        (other / s).write_bytes((root / 'val' / s).read_bytes())
    net.infer(str(jp), save_annotation=str(out), val_dir=str(other), **kw)
    assert open(out, encoding='utf-8').read() == want
    with pytest.raises(NotImplementedError):
        net.infer(str(jp))
    with pytest.raises(NotImplementedError):
        net.infer(full[0], save_annotation=str(out), save_visualization=True)
    with pytest.raises(NotImplementedError):
        net.infer(full[0], save_annotation=str(out), infer_tags=True)


def test_batched_export_equals_one_by_one_exports(tmp_path, monkeypatch):
    from PIL import Image
    from utils.constants import CATEGORIES
    monkeypatch.setenv('CSM_DET_BATCH', '2')
    net = _net('refinenet_isnet')
    assert net.det_batch == 2
    kw, full, empty = _thr_kw(net)
    frames = full[:4] + empty[:1]
    paths = []
    for k, im in enumerate(frames):
        p = tmp_path / ('f%d.png' % k)
        Image.fromarray(im[..., ::-1]).save(str(p))
        paths.append(str(p))
    out = tmp_path / 'all.json'
    net.infer(paths, save_annotation=str(out), obj_id_start=4, img_id_start=6, **kw)
    images, anns = [], []
    o, i = 4, 6
    for p in paths:
        one = tmp_path / 'one.json'
        net.infer(p, save_annotation=str(one), obj_id_start=o, img_id_start=i, **kw)
        d = json.loads(open(one, encoding='utf-8').read())
        images += d['images']
        anns += d['annotations']
        o += len(d['annotations'])
        i += 1
    from utils.io_utils import NumpyEncoder
    want = json.dumps({"info": {}, "licenses": [], "images": images, "annotations": anns, "categories": CATEGORIES},
                      ensure_ascii=False, cls=NumpyEncoder)
    assert open(out, encoding='utf-8').read() == want and len(anns) >= 4
