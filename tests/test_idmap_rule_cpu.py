"""CPU: univs_amd/data/idmap_rule.py, the numpy statement of include/univs_idmap_hip.h.  `prompts` equals Pillow's NEAREST resize of every
object's own plane (the gather argument: resize(idmap) == v is resize(idmap == v)), also in palette mode and at 2 -> 7; `census` equals
numpy's `bincount` and the `any` boxes; both reproduce the recorded bytes of tests/golden/g37_vos_folders_pil.npz."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests import idmap_cases as ic
from tests import prompt_masks_cases as pc
from univs_amd.data import idmap_rule, nearest_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [((2, 2), (7, 7)), ((7, 7), (2, 2)), ((37, 53), (37, 53)), ((37, 53), (20, 29)), ((37, 53), (74, 106)), ((13, 40), (17, 129)),
          ((97, 131), (300, 200))]


def _tool():
    spec = importlib.util.spec_from_file_location("gen_golden_vos_folders", os.path.join(ROOT, "tools", "gen_golden_vos_folders.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@pytest.mark.parametrize("in_hw,out_hw", SCALES)
@pytest.mark.parametrize("kind", ["noise", "regions"])
def test_prompts_equal_pillow_per_object(in_hw, out_hw, kind):
    ids = np.stack([ic.idmap(kind, *in_hw, values=(0, 1, 7, 255)), ic.idmap(kind, *in_hw, values=(0, 7, 8), seed=1)])
    frame, value = [0, 0, 0, 0, 0, 1, 1, 1], [0, 1, 7, 255, 7, 8, 1, 0]   # 7 twice; 1 is absent from frame 1
    masks, boxes = idmap_rule.prompts_resized(ids, frame, value, out_hw)
    want, want_boxes = ic.pillow_prompts(ids, frame, value, out_hw)
    assert masks.dtype == np.uint8 and boxes.dtype == np.int32
    assert np.array_equal(masks, want) and np.array_equal(boxes, want_boxes)
    assert not masks[6].any() and boxes[6].tolist() == [0, 0, 0, 0] and np.array_equal(masks[2], masks[4])


def test_the_resize_of_a_palette_image_is_the_same_gather():
    from PIL import Image
    m = ic.idmap("noise", 2, 2, (0, 1, 2, 255))
    im = Image.fromarray(m, mode="P")
    im.putpalette(ic.PALETTE)
    resized = np.asarray(im.resize((7, 7), Image.NEAREST))
    assert np.array_equal(resized, m[nearest_table(2, 7)][:, nearest_table(2, 7)])
    for v in (0, 1, 2, 255):
        assert np.array_equal(resized == v, pc.pillow_resize((m == v).astype(np.uint8), (7, 7)).astype(bool))


def test_prompts_clamp_frames_values_and_tables():
    ids = np.stack([ic.idmap("noise", 5, 6, (0, 1, 255)), ic.idmap("noise", 5, 6, (0, 1, 255), seed=1)])
    ty, tx = np.array([-4, 0, 4, 99]), np.array([-1, 5, 2 ** 31 - 1])
    masks, _ = idmap_rule.prompts(ids, [-3, 9], [300, -2], ty, tx)
    assert np.array_equal(masks[0], ids[0][[0, 0, 4, 4]][:, [0, 5, 5]] == 255) and np.array_equal(masks[1], ids[1][[0, 0, 4, 4]][:, [0, 5, 5]] == 0)
    with pytest.raises(ValueError):
        idmap_rule.prompts(np.zeros((2, 3), np.uint8), [0], [0], [0], [0])
    with pytest.raises(ValueError):
        idmap_rule.census(np.zeros((1, 2, 3), np.int32))


@pytest.mark.parametrize("hw", [(1, 1), (13, 40), (13, 41), (37, 53)])
def test_census_equals_bincount_and_any(hw):
    ids = np.stack([ic.idmap("regions", *hw, (0, 1, 2, 255), seed=1), ic.idmap("noise", *hw, range(256), seed=2), np.full(hw, 77, np.uint8)])
    count, box = idmap_rule.census(ids)
    want_count, want_box = ic.numpy_census(ids)
    assert count.dtype == np.int32 and box.dtype == np.int32 and count.shape == (3, 256) and box.shape == (3, 256, 4)
    assert np.array_equal(count, want_count) and np.array_equal(box, want_box)
    assert count[2, 77] == hw[0] * hw[1] and box[2, 77].tolist() == [0, 0, hw[1], hw[0]] and not box[2, 76].any()


def test_converter_box_is_the_converters_bounding_box():
    m = np.zeros((9, 11), bool)
    m[2:5, 3:9] = True
    _, box = idmap_rule.census(m.astype(np.uint8)[None])
    assert idmap_rule.converter_box(box[0, 1]) == ic.box_of(m) == [3, 2, 5, 2]


@pytest.mark.parametrize("case", ic.GOLDEN_CASES, ids=ic.case_id)
def test_recorded_pillow_bytes_are_reproduced(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "g37_vos_folders_pil.npz"))
    recipe = json.loads(bytes(g["recipe"]).decode())
    assert recipe["cases"] == [ic.case_id(c) for c in ic.GOLDEN_CASES]
    (H, W), out_hw = case
    name = ic.case_id(case)
    ids = _tool().golden_idmap(H, W)
    assert np.array_equal(ids, g[f"{name}/ids"])                    # the stored id map is the closed-form one
    values = recipe["values"]
    masks, boxes = idmap_rule.prompts_resized(ids[None], [0] * len(values), values, out_hw)
    assert np.array_equal(masks, g[f"{name}/masks"]) and np.array_equal(boxes, g[f"{name}/boxes"])
    assert np.array_equal(ids[nearest_table(H, out_hw[0])][:, nearest_table(W, out_hw[1])], g[f"{name}/resized_ids"])
