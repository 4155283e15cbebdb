"""CPU: COCO annotation export of AnimeInsSeg.infer(save_annotation=...) -- the host pieces.

rle_encode_ref / rle_decode_ref restate pycocotools' maskApi.c (rleEncode + rleToString, rleFrString + rleDecode) as
utils/io_utils.py:327-333 mask2rle reaches it; the GPU tests (test_gpu_coco_export.py) hold the device encoder to them."""
import json
import os

import numpy as np
import pytest


def rle_counts_ref(m):
    """rleEncode of (m > 0) in column-major order, starting from the value 0"""
    a = (np.asarray(m) > 0).astype(np.int8).T.reshape(-1)
    change = np.flatnonzero(np.diff(np.concatenate([[0], a])))
    return np.diff(np.concatenate([[0], change, [a.size]])).astype(np.int64)


def rle_string_ref(cnts):
    """rleToString: from the fourth count on store cnts[i] - cnts[i-2]; 5-bit groups, low first, 0x20 = more, + 48"""
    out = []
    cnts = [int(c) for c in cnts]
    for i, c in enumerate(cnts):
        x = c - cnts[i - 2] if i > 2 else c
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if ch & 0x10 else (x != 0)
            if more:
                ch |= 0x20
            out.append(chr(ch + 48))
    return ''.join(out)


def rle_encode_ref(m):
    """pycocotools.mask.encode(np.asfortranarray(m[..., None] > 0).astype(np.uint8))[0]['counts'].decode()"""
    return rle_string_ref(rle_counts_ref(m))


def rle_decode_ref(s, h, w):
    """rleFrString + rleDecode: an independent inverse (runs alternate from 0, column-major)"""
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    assert sum(cnts) == h * w and min(cnts) >= 0
    flat = np.repeat(np.arange(len(cnts)) % 2, cnts).astype(np.uint8)
    return flat.reshape(w, h).T


def test_restatement_pins():
    assert rle_encode_ref(np.zeros((3, 4), np.uint8)) == "<"
    assert rle_encode_ref(np.ones((3, 4), np.uint8)) == "0<"
    m = np.array([[0, 1, 1, 0], [1, 1, 0, 0], [0, 0, 0, 1]], np.uint8)
    assert rle_counts_ref(m).tolist() == [1, 1, 1, 2, 1, 1, 4, 1]
    assert rle_encode_ref(m) == "11110O30"                        # 'O': the -1 delta of the fourth count
    m = np.zeros((40, 30), np.uint8)
    m[5:20, 3:10] = 1
    m[30:35, 20:28] = 1
    assert rle_encode_ref(m) == "m3?i000000000000Y=FQC0000000000000b1"
    assert rle_encode_ref(m * 255) == rle_encode_ref(m)            # > 0, like mask2rle


def test_decoder_round_trips_random_masks():
    rng = np.random.default_rng(1)
    for it in range(200):
        h, w = (int(v) for v in rng.integers(1, 40, 2))
        m = (rng.random((h, w)) < rng.choice([0.0, 0.01, 0.5, 0.99, 1.0])).astype(np.uint8)
        if it % 5 == 0:
            m[:, : w // 2] = 0
        s = rle_encode_ref(m)
        assert np.array_equal(rle_decode_ref(s, h, w), m), (h, w)
    big = np.zeros((1100, 1000), np.uint8)                        # counts > 2^20 and large negative deltas
    big[1, 2] = big[1099, 999] = big[500, 3] = 1
    assert np.array_equal(rle_decode_ref(rle_encode_ref(big), 1100, 1000), big)


def test_coco_json_image_order_duplicates_and_val_dir(tmp_path):
    from cartoonsegmentation_amd.segmentation import coco_image_paths
    d = tmp_path / 'ds' / 'annotations'
    d.mkdir(parents=True)
    jp = d / 'val.json'
    jp.write_text(json.dumps({'images': [{'id': 7, 'file_name': 'a.png'}, {'id': 3, 'file_name': 'b.png'},
                                         {'id': 7, 'file_name': 'c.png'}, {'id': 11, 'file_name': 'b.png'}],
                              'annotations': [], 'categories': []}))
    paths, ids = coco_image_paths(str(jp))
    val = os.path.join(str(tmp_path / 'ds'), 'val')
    # getImgIds(): first-insertion order of the ids, a later duplicate replaces the entry (id 7 -> c.png)
    assert paths == [os.path.join(val, 'c.png'), os.path.join(val, 'b.png'), os.path.join(val, 'b.png')]
    # imgp2ids: the later id of the same path wins, as the reference's dict assignment does
    assert ids == {os.path.join(val, 'c.png'): 7, os.path.join(val, 'b.png'): 11}
    paths, ids = coco_image_paths(str(jp), val_dir='/elsewhere')
    assert paths[0] == '/elsewhere/c.png' and ids['/elsewhere/c.png'] == 7


def test_read_imglst_from_txt(tmp_path):
    from animeinsseg import read_imglst_from_txt as r2
    from utils.io_utils import read_imglst_from_txt
    p = tmp_path / 'list.txt'
    p.write_text('/x/a.png\n/x/b c.jpg\r\né.png', encoding='utf8')
    assert read_imglst_from_txt(str(p)) == ['/x/a.png', '/x/b c.jpg', 'é.png'] and r2 is read_imglst_from_txt


def test_numpy_encoder_and_json_helpers(tmp_path):
    from utils.constants import CATEGORIES
    from utils.io_utils import NumpyEncoder, dict2json, json2dict
    seg = np.ones((3, 5), np.uint8)
    area = seg.sum()                                               # np.uint64 (reference :592)
    score = np.float32(0.8123456)
    bbox = np.array([1, 2, 3, 4], np.int32).astype(np.float32).tolist()
    d = {'area': area, 'score': float(score), 'raw': score, 'bbox': bbox, 'arr': np.arange(3), 'ok': np.bool_(True),
         'name': '画像', 'categories': CATEGORIES}
    txt = json.dumps(d, ensure_ascii=False, cls=NumpyEncoder)
    assert txt == ('{"area": 15, "score": 0.8123456239700317, "raw": 0.8123456239700317, "bbox": [1.0, 2.0, 3.0, 4.0], '
                   '"arr": [0, 1, 2], "ok": true, "name": "画像", "categories": [{"id": 0, "name": "object", "isthing": 1}]}')
    p = str(tmp_path / 'a.json')
    dict2json(d, p)
    assert open(p, encoding='utf-8').read() == txt and json2dict(p)['area'] == 15
    with pytest.raises(TypeError):
        json.dumps({'x': object()}, cls=NumpyEncoder)


def test_library_exports_the_rle_symbols():
    from cartoonsegmentation_amd import _lib
    syms = {'csm_mask_rle_scratch_bytes', 'csm_mask_rle_measure', 'csm_mask_rle_write'}
    assert syms <= set(_lib.declared_symbols())
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in syms)
    # O(n * W) scratch, independent of the number of runs; 0 for shapes outside the contract
    assert lib.csm_mask_rle_scratch_bytes(10, 1024, 1024) == 10 * 1024 * 8 * 28
    assert lib.csm_mask_rle_scratch_bytes(3, 100, 7) == 3 * 7 * 1 * 28
    assert lib.csm_mask_rle_scratch_bytes(1, 1 << 16, 1 << 15) == 0


def test_infer_signature_keeps_the_export_arguments():
    import inspect
    from animeinsseg import AnimeInsSeg
    sig = inspect.signature(AnimeInsSeg.infer).parameters
    assert sig['save_annotation'].default == '' and sig['obj_id_start'].default == -1 and sig['img_id_start'].default == -1
    assert sig['val_dir'].default is None and sig['save_dir'].default == ''
