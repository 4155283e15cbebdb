"""CPU: AnimeInstances.resize at the identity size.  Bool masks come back as the same storage, int32 boxes as they are; any other
dtype converts by the expressions the method has always had, written out here.  Values and dtypes are those expressions' in every case."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cartoonsegmentation_amd.anime_instances import AnimeInstances  # noqa: E402

H, W = 13, 17


def _old_resize(masks, bboxes, h, w):
    """the method's expressions for an identity resize before the copies were dropped"""
    oh, ow = int(masks.shape[1]), int(masks.shape[2])
    hs, ws = h / oh, w / ow
    b = bboxes.float()
    b[:, ::2] *= hs
    b[:, 1::2] *= ws
    return masks.to(torch.float) > 0.3, torch.round(b).int()


def _case(box_dtype, mask_dtype=torch.bool):
    g = torch.Generator().manual_seed(4)
    masks = (torch.rand((3, H, W), generator=g) > 0.5).to(mask_dtype)
    boxes = torch.tensor([[0, 0, W, H], [3, 5, 7, 2], [-4, 1, (1 << 24) - 1, 9]], dtype=box_dtype)
    return masks, boxes, torch.tensor([0.9, 0.5, 0.4])


@pytest.mark.parametrize("box_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_identity_resize_of_bool_masks(box_dtype):
    masks, boxes, scores = _case(box_dtype)
    ref_m, ref_b = _old_resize(masks.clone(), boxes.clone(), H, W)
    inst = AnimeInstances(masks, boxes, scores)
    inst.resize(H, W)
    assert inst.masks.dtype == ref_m.dtype == torch.bool and torch.equal(inst.masks, ref_m)
    assert inst.bboxes.dtype == ref_b.dtype == torch.int32 and torch.equal(inst.bboxes, ref_b)
    assert inst.masks.data_ptr() == masks.data_ptr()                  # no copy of the masks
    if box_dtype == torch.int32:
        assert inst.bboxes.data_ptr() == boxes.data_ptr()             # nor of int32 boxes
    else:
        assert torch.equal(boxes, _case(box_dtype)[1])                # the caller's int64 boxes are not written to


def test_identity_resize_of_uint8_masks_converts_as_before():
    masks, boxes, scores = _case(torch.int32, torch.uint8)
    ref_m, ref_b = _old_resize(masks.clone(), boxes.clone(), H, W)
    inst = AnimeInstances(masks, boxes, scores)
    inst.resize(H, W)
    assert inst.masks.dtype == torch.bool and torch.equal(inst.masks, ref_m)
    assert inst.bboxes.dtype == torch.int32 and torch.equal(inst.bboxes, ref_b)


def test_other_sizes_still_scale_boxes_and_masks():
    masks, boxes, scores = _case(torch.int32)
    inst = AnimeInstances(masks.clone(), boxes.clone(), scores)
    inst.resize(2 * H, 2 * W)
    b = boxes.float()
    b[:, ::2] *= 2.0
    b[:, 1::2] *= 2.0
    assert torch.equal(inst.bboxes, torch.round(b).int())
    ref = torch.nn.functional.interpolate(masks.to(torch.float).unsqueeze(1), (2 * H, 2 * W), mode='area').squeeze(1) > 0.3
    assert tuple(inst.masks.shape) == (3, 2 * H, 2 * W) and torch.equal(inst.masks, ref)
