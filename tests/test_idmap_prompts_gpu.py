"""GPU: csrc/idmap_prompts.hip.  The prompts entry gives, for every listed object, `PIL.Image.resize(NEAREST)` of its own plane byte for
byte and the box of the result exactly -- values 0 and 255, absent and repeated values, frames without objects, 255 objects in a frame,
several row segments and column tiles, tables and frame entries out of range.  The census entry gives numpy's `bincount` and the
`any` boxes per frame and value."""
import numpy as np
import pytest
import torch

from tests import idmap_cases as ic
from univs_amd import _lib, idmap_ops, ops
from univs_amd.data import idmap_rule, nearest_table

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")


def run_prompts(ids, frame, value, out_hw):
    ids_d, frame_d, value_d = idmap_ops.upload_prompts(ids, frame, value, dev)
    out = idmap_ops.idmap_prompts_u8(ids_d, frame_d, value_d, out_hw)
    assert out is not None
    masks, boxes = out
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == (len(frame),) + tuple(out_hw) and masks.is_cuda and masks.is_contiguous()
    assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (len(frame), 4) and boxes.is_cuda
    return masks.cpu().numpy(), boxes.cpu().numpy()


def check(ids, frame, value, out_hw):
    """The kernel against Pillow per object, and against the numpy statement."""
    got, boxes = run_prompts(ids, frame, value, out_hw)
    want, want_boxes = ic.pillow_prompts(ids, frame, value, out_hw)
    diff = got != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert np.array_equal(boxes, want_boxes), (boxes.tolist(), want_boxes.tolist())
    rule_masks, rule_boxes = idmap_rule.prompts_resized(ids, frame, value, out_hw)
    assert np.array_equal(got, rule_masks) and np.array_equal(boxes, rule_boxes)
    return got, boxes


@pytest.mark.parametrize("Ho", [1, 17])
@pytest.mark.parametrize("Wo", [1, 3, 4, 5, 63, 64, 65, 129])
def test_output_widths_at_the_edges_of_the_lanes_four_columns(Ho, Wo):
    ids = np.stack([ic.idmap("regions", 13, 40, (0, 1, 2, 255)), ic.idmap("noise", 13, 40, (0, 1, 2, 255), seed=1)])
    check(ids, [0, 0, 0, 0, 1, 1, 1], [0, 1, 2, 255, 255, 0, 2], (Ho, Wo))


@pytest.mark.parametrize("in_hw,out_hw", [((2, 2), (7, 7)), ((7, 7), (2, 2)), ((37, 53), (37, 53)), ((37, 53), (20, 29)),
                                          ((37, 53), (74, 106)), ((97, 131), (300, 200))])
@pytest.mark.parametrize("kind", ["noise", "regions"])
def test_scales(in_hw, out_hw, kind):
    ids = ic.idmap(kind, *in_hw, values=(0, 1, 7, 255))[None]
    check(ids, [0, 0, 0, 0], [0, 1, 7, 255], out_hw)


def test_absent_and_repeated_values():
    ids = ic.idmap("regions", 37, 53, (0, 1, 2))[None]
    got, boxes = check(ids, [0, 0, 0, 0], [1, 9, 1, 2], (50, 70))
    assert not got[1].any() and boxes[1].tolist() == [0, 0, 0, 0]      # listed, absent: a zero plane and a zero box
    assert got[0].any() and np.array_equal(got[0], got[2]) and np.array_equal(boxes[0], boxes[2])   # listed twice: both written


def test_a_one_pixel_object_vanishes_on_the_down_scale_and_one_touches_all_borders():
    ids = np.zeros((1, 37, 53), np.uint8)
    ids[0, 0, :], ids[0, -1, :], ids[0, :, 0], ids[0, :, -1] = 3, 3, 3, 3   # a frame around the map
    ids[0, 11, 20] = 5
    assert nearest_table(37, 12).tolist().count(11) == 0 or nearest_table(53, 17).tolist().count(20) == 0
    got, boxes = check(ids, [0, 0], [5, 3], (12, 17))
    assert boxes[0].tolist() == [0, 0, 0, 0] and not got[0].any()
    got, boxes = check(ids, [0, 0], [5, 3], (74, 106))
    assert boxes[1].tolist() == [0, 0, 106, 74] and boxes[0].tolist() == [40, 22, 42, 24]


def test_frames_with_no_one_and_seven_objects_in_one_call():
    ids = np.stack([ic.idmap("regions", 37, 53, (0, 1), seed=1), ic.idmap("noise", 37, 53, (0, 9), seed=2),
                    ic.idmap("regions", 37, 53, (0, 1, 2, 3, 4, 5, 6, 255), seed=3), ic.idmap("noise", 37, 53, (0, 1), seed=4)])
    check(ids, [0] + [2] * 7, [1, 1, 2, 3, 4, 5, 6, 255], (50, 70))      # frame 1 in the middle and frame 3 list nothing
    check(ids, [1, 3, 3], [9, 0, 1], (20, 29))                          # frames 0 and 2 list nothing


def test_255_objects_of_one_pixel_each_in_one_frame():
    ids = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    got, boxes = check(ids, [0] * 255, list(range(1, 256)), (32, 48))
    assert (got.reshape(255, -1).sum(1) == 6).all()


def test_three_objects_over_several_row_segments_and_column_tiles():
    ids = ic.idmap("regions", 201, 301, (0, 1, 2, 3), seed=2)[None]
    ids[0, 0, 0], ids[0, -1, -1] = 3, 3                               # its box spans every workgroup's tile
    got, boxes = check(ids, [0, 0, 0], [1, 2, 3], (620, 1400))
    assert boxes[2].tolist() == [0, 0, 1400, 620]


def test_no_objects():
    ids = torch.zeros((1, 4, 4), dtype=torch.uint8, device=dev)
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    masks, boxes = idmap_ops.idmap_prompts_u8(ids, empty, empty, (3, 5))
    assert tuple(masks.shape) == (0, 3, 5) and tuple(boxes.shape) == (0, 4)


def test_tables_frames_and_values_out_of_range_are_clamped():
    """The entry is called with tables whose ends lie outside the source, frame entries outside [0, F) and a value outside [0, 255]:
    the launch finishes, the entries act as clamped, and the bytes around the results keep their value."""
    H, W, Ho, Wo = 37, 53, 50, 70
    ids = np.stack([ic.idmap("regions", H, W, (0, 1, 255), seed=1), ic.idmap("noise", H, W, (0, 1, 255), seed=2)])
    frame, value = np.array([-5, 0, 1, 7], np.int32), np.array([1, -3, 300, 1], np.int32)
    ty, tx = nearest_table(H, Ho).copy(), nearest_table(W, Wo).copy()
    ty[:3], ty[-2:], tx[0], tx[-4:] = -7, 10 ** 6, -(2 ** 31), 2 ** 31 - 1
    n, pad = 4 * Ho * Wo, 259
    buf = torch.full((pad + n + pad,), 0xA5, dtype=torch.uint8, device=dev)
    boxes = torch.full((2 + 4 * 4 + 2,), -77, dtype=torch.int32, device=dev)
    ids_d, frame_d, value_d = idmap_ops.upload_prompts(ids, frame, value, dev)
    ty_d, tx_d = torch.from_numpy(ty).to(dev), torch.from_numpy(tx).to(dev)
    ok = ops._call("idmap_prompts_u8", _lib.load().univs_idmap_prompts_u8, ids_d, ops._ptr(ids_d), 2, H, W, ops._ptr(frame_d), ops._ptr(value_d),
                   4, ops._ptr(ty_d), ops._ptr(tx_d), Ho, Wo, buf.data_ptr() + pad, boxes.data_ptr() + 8)
    assert ok
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:pad] == 0xA5).all() and (host[pad + n:] == 0xA5).all()
    cy, cx = np.clip(ty, 0, H - 1), np.clip(tx.astype(np.int64), 0, W - 1)
    want = np.stack([ids[f][cy][:, cx] == v for f, v in zip((0, 0, 1, 1), (1, 0, 255, 1))]).astype(np.uint8)
    assert np.array_equal(host[pad:pad + n].reshape(4, Ho, Wo), want)
    b = boxes.cpu().numpy()
    assert b[:2].tolist() == [-77, -77] and b[-2:].tolist() == [-77, -77]
    assert np.array_equal(b[2:-2].reshape(4, 4), ic.pc.any_boxes(want))
    rule_masks, rule_boxes = idmap_rule.prompts(ids, frame, value, ty, tx)
    assert np.array_equal(rule_masks, want) and np.array_equal(rule_boxes, b[2:-2].reshape(4, 4))


# ---- the census --------------------------------------------------------------------------------------------------------------------------
def check_census(ids):
    out = idmap_ops.idmap_census_u8(torch.from_numpy(ids).to(dev))
    assert out is not None
    count, box = out
    assert count.dtype == torch.int32 and tuple(count.shape) == (ids.shape[0], 256) and box.dtype == torch.int32
    assert tuple(box.shape) == (ids.shape[0], 256, 4)
    want_count, want_box = ic.numpy_census(ids)
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert np.array_equal(box.cpu().numpy(), want_box)
    rule_count, rule_box = idmap_rule.census(ids)
    assert np.array_equal(rule_count, want_count) and np.array_equal(rule_box, want_box)
    return want_count


@pytest.mark.parametrize("hw", [(1, 1), (13, 40), (13, 41), (7, 3), (201, 301)])
def test_census_of_three_frames(hw):
    ids = np.stack([ic.idmap("regions", *hw, (0, 1, 2, 255), seed=1), ic.idmap("noise", *hw, (0, 3, 200), seed=2),
                    ic.idmap("regions", *hw, (9, 8), seed=3)])
    check_census(ids)


def test_census_of_a_one_value_map_and_of_all_256_values():
    count = check_census(np.full((1, 37, 53), 77, np.uint8))
    assert count[0, 77] == 37 * 53 and count.sum() == 37 * 53
    ids = np.stack([np.arange(256, dtype=np.uint8).reshape(16, 16), ic.idmap("noise", 16, 16, range(256), seed=5)])
    count = check_census(ids)
    assert (count[0] == 1).all()


def test_census_of_no_frames():
    count, box = idmap_ops.idmap_census_u8(torch.zeros((0, 4, 4), dtype=torch.uint8, device=dev))
    assert tuple(count.shape) == (0, 256) and tuple(box.shape) == (0, 256, 4)
