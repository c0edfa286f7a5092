"""GPU: csrc/mask_prompt_resize.hip gives `PIL.Image.resize(NEAREST)` of run-length coded masks byte for byte and the boxes of the
results exactly; absent masks, several masks and frames in one launch; a table with entries out of range; the mapper gives the same
annotations with resize="gpu" and resize="host"; a video on disk through the mapper and the VOS driver to PNGs and back."""
import os
import types

import numpy as np
import pytest
import torch

from tests import prompt_masks_cases as pc
from univs_amd import _lib, ops, prompts_ops
from univs_amd.data import VOSTestMapper, load_vos_json, nearest_table
from univs_amd.evaluation.vis_counts import runs_from_rles

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")


def run_kernel(masks, out_hw, compressed=False):
    """(uint8 [N, Ho, Wo], int32 [N, 4]) on the host; `masks`: 0 / 1 arrays of one size, None for an absent mask."""
    H, W = next(m for m in masks if m is not None).shape
    runs = runs_from_rles([None if m is None else pc.code_of(m, compressed) for m in masks], H, W, device=dev)
    out = prompts_ops.resize_rle_masks_u8(runs, (H, W), out_hw)
    assert out is not None
    got, boxes = out
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(masks),) + tuple(out_hw) and got.is_cuda and got.is_contiguous()
    assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (len(masks), 4) and boxes.is_cuda
    return got.cpu().numpy(), boxes.cpu().numpy()


def check(masks, out_hw, compressed=False):
    got, boxes = run_kernel(masks, out_hw, compressed)
    want = np.stack([np.zeros(out_hw, np.uint8) if m is None else pc.pillow_resize(m, out_hw) for m in masks])
    diff = got != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert np.array_equal(boxes, pc.any_boxes(want))
    return got, boxes


@pytest.mark.parametrize("Ho", [1, 17])
@pytest.mark.parametrize("Wo", [1, 63, 64, 65, 129])
def test_output_widths_at_the_edges_of_the_lane_tile(Ho, Wo):
    check([pc.mask("noise", 13, 40), pc.mask("blob", 13, 40)], (Ho, Wo))


@pytest.mark.parametrize("in_hw,out_hw", [((2, 2), (7, 7)), ((7, 7), (2, 2)), ((37, 53), (37, 53)), ((37, 53), (20, 29)),
                                          ((37, 53), (74, 106)), ((97, 131), (300, 200))])
@pytest.mark.parametrize("kind", ["noise", "blob"])
def test_scales(in_hw, out_hw, kind):
    check([pc.mask(kind, *in_hw)], out_hw, compressed=kind == "blob")


@pytest.mark.parametrize("out_hw", [(9, 14), (5, 9), (31, 70)])
@pytest.mark.parametrize("kind", ["empty",                          # one run
                                  "full",                           # an empty first run
                                  "last",                           # foreground ending on the last pixel
                                  "span",                           # one run spanning several source columns, columns without a boundary
                                  "checker"])                       # H W runs
def test_mask_contents(kind, out_hw, hw=(9, 14)):
    m = pc.mask(kind, *hw)
    if kind == "checker":
        assert len(pc.counts_of(m)) == hw[0] * hw[1]
    _, boxes = check([m], out_hw)
    if kind == "empty":
        assert boxes.tolist() == [[0, 0, 0, 0]]
    if kind == "full":
        assert boxes.tolist() == [[0, 0, out_hw[1], out_hw[0]]]


@pytest.mark.parametrize("out_hw", [(100, 180), (620, 1400)])
def test_a_checkerboard_of_60501_runs_over_several_row_segments_and_column_tiles(out_hw):
    test_mask_contents("checker", out_hw, hw=(201, 301))


def test_several_masks_absent_ones_and_two_frames_in_one_launch():
    """Five masks as the mapper sends them: two objects of one frame, an absent mask, two objects of another frame."""
    masks = [pc.mask("blob", 37, 53, 1), pc.mask("noise", 37, 53, 2), None, pc.mask("span", 37, 53), pc.mask("blob", 37, 53, 5)]
    got, boxes = check(masks, (50, 70))
    assert not got[2].any() and boxes[2].tolist() == [0, 0, 0, 0]
    got, boxes = check([None, pc.mask("blob", 37, 53, 1), None], (20, 29))
    assert boxes[0].tolist() == boxes[2].tolist() == [0, 0, 0, 0] and boxes[1].any()


def test_no_masks():
    runs = runs_from_rles([], 4, 4, device=dev)
    masks, boxes = prompts_ops.resize_rle_masks_u8(runs, (4, 4), (3, 5))
    assert tuple(masks.shape) == (0, 3, 5) and tuple(boxes.shape) == (0, 4)


def test_a_table_with_entries_out_of_range_is_clamped():
    """The entry is called with tables whose ends lie outside the source: the launch finishes, the entries act as clamped to
    [0, n_in), and the bytes around the results keep their value."""
    H, W, Ho, Wo = 37, 53, 50, 70
    m = [pc.mask("blob", H, W, 1), pc.mask("noise", H, W, 2)]
    runs = runs_from_rles([pc.code_of(x) for x in m], H, W, device=dev)
    ty, tx = nearest_table(H, Ho).copy(), nearest_table(W, Wo).copy()
    ty[:3], ty[-2:], tx[0], tx[-4:] = -7, 10 ** 6, -(2 ** 31), 2 ** 31 - 1
    n, pad = 2 * Ho * Wo, 259
    buf = torch.full((pad + n + pad,), 0xA5, dtype=torch.uint8, device=dev)
    boxes = torch.full((2 + 4 * 2 + 2,), -77, dtype=torch.int32, device=dev)
    ty_d, tx_d = torch.from_numpy(ty).to(dev), torch.from_numpy(tx).to(dev)
    ok = ops._call("resize_rle_masks_u8", _lib.load().univs_resize_rle_masks_u8, runs.bounds, ops._ptr(runs.bounds), ops._ptr(runs.starts),
                   runs.bounds.numel(), 2, H, W, ops._ptr(ty_d), ops._ptr(tx_d), Ho, Wo, buf.data_ptr() + pad, boxes.data_ptr() + 8)
    assert ok
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:pad] == 0xA5).all() and (host[pad + n:] == 0xA5).all()
    cy, cx = np.clip(ty, 0, H - 1), np.clip(tx.astype(np.int64), 0, W - 1)
    want = np.stack([x[cy][:, cx] for x in m])
    assert np.array_equal(host[pad:pad + n].reshape(2, Ho, Wo), want)
    b = boxes.cpu().numpy()
    assert b[:2].tolist() == [-77, -77] and b[-2:].tolist() == [-77, -77] and np.array_equal(b[2:-2].reshape(2, 4), pc.any_boxes(want))


@pytest.mark.parametrize("case", pc.GOLDEN_CASES, ids=pc.case_id)
def test_recorded_pillow_bytes_are_reproduced(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "g33_prompt_masks_pil.npz"))
    (kind, H, W), out_hw = case
    name = pc.case_id(case)
    runs = runs_from_rles([{"size": [H, W], "counts": g[f"{name}/counts"].tolist()}], H, W, device=dev)
    masks, boxes = prompts_ops.resize_rle_masks_u8(runs, (H, W), out_hw)
    assert np.array_equal(masks[0].cpu().numpy(), g[f"{name}/mask"]) and np.array_equal(boxes[0].cpu().numpy(), g[f"{name}/box"])


def test_mapper_gpu_equals_mapper_host(tmp_path):
    path, root, _ = pc.write_vos_dataset(str(tmp_path))
    for record in load_vos_json(path, root, "sot_davis17_val"):
        host = VOSTestMapper(20, 100, resize="host")(record)
        gpu = VOSTestMapper(20, 100, resize="gpu", device=dev)(record)
        assert [len(a) for a in gpu["instances"]] == [len(a) for a in host["instances"]] and sum(len(a) for a in gpu["instances"]) > 0
        for a, b in zip(gpu["instances"], host["instances"]):
            assert a.ori_ids == b.ori_ids and a.image_size == b.image_size
            if len(a):
                assert a.gt_masks.is_cuda and a.gt_boxes.tensor.is_cuda and a.gt_classes.is_cuda
            assert a.gt_masks.dtype == b.gt_masks.dtype and torch.equal(a.gt_masks.cpu(), b.gt_masks)
            assert a.gt_boxes.tensor.dtype == b.gt_boxes.tensor.dtype and torch.equal(a.gt_boxes.tensor.cpu(), b.gt_boxes.tensor)
            assert a.gt_classes.dtype == b.gt_classes.dtype and torch.equal(a.gt_classes.cpu(), b.gt_classes)
        assert all(torch.equal(x.cpu(), y) for x, y in zip(gpu["image"], host["image"]))
        skip = ("image", "image_padding_mask", "instances")
        assert {k: v for k, v in gpu.items() if k not in skip} == {k: v for k, v in host.items() if k not in skip}


def test_video_on_disk_through_the_mapper_and_the_vos_driver_to_pngs_and_back(tmp_path):
    """The scripted scene of tests/test_vos_gpu.py, written to disk at twice its size: frames as PNGs, the objects' first masks as
    run-length codes in a json.  The mapper halves both (a 2 -> 1 NEAREST resize of a rectangle with even corners is the rectangle), so
    its annotations are the scene's; the driver returns one id map per frame at the record's size with the ids of the json, and
    `write_vos_pngs` / `read_results` round-trip them."""
    import json
    from PIL import Image
    from tests import cases
    from tests.test_clip_loop_cpu import _move
    from univs_amd import run
    from univs_amd.evaluation.davis import read_results
    from univs_amd.inference.video_vos import FrameAnnotations, InferenceVideoVOS
    case = cases.SCRIPT_CASE
    (h, w), n = case["image_size"], case["n_frames"]
    head = cases.ScriptedHead(case)
    os.makedirs(tmp_path / "JPEGImages" / "clip0")
    for f, frame in enumerate(cases.loop_frames(case)):
        Image.fromarray(frame.permute(1, 2, 0).to(torch.uint8).numpy()).resize((2 * w, 2 * h), Image.NEAREST).save(tmp_path / "JPEGImages" / "clip0" / f"{f:05d}.png")
    annotations = []
    for oid, (j, f_ann) in cases.VOS_OBJECTS.items():
        x0, y0, x1, y1 = head.rect(j, f_ann)
        m = np.zeros((2 * h, 2 * w), np.uint8)
        m[2 * y0:2 * y1, 2 * x0:2 * x1] = 1
        segms = [pc.code_of(m, compressed=oid != 22) if f == f_ann else None for f in range(n)]
        annotations.append({"id": oid, "video_id": 1, "category_id": case_class(cases, j), "iscrowd": 0, "segmentations": segms,
                            "bboxes": [[0, 0, 1, 1] if s else None for s in segms]})
    data = {"videos": [{"id": 1, "file_names": [f"clip0/{f:05d}.png" for f in range(n)], "height": 2 * h, "width": 2 * w, "length": n}],
            "annotations": annotations, "categories": [{"id": i + 1, "name": str(i)} for i in range(case["K"])]}
    (tmp_path / "vos.json").write_text(json.dumps(data))
    record = load_vos_json(str(tmp_path / "vos.json"), str(tmp_path / "JPEGImages"), "sot_ytbvos18_val")[0]
    d = VOSTestMapper(h, w, resize="gpu", device=dev)(record)
    assert tuple(d["image"][0].shape) == (3, h, w) and d["image"][0].device.type == dev.type

    # the mapper's annotations are the scene's (tests/cases.py builds them by hand for the driver tests)
    for got, want in zip(d["instances"], cases.vos_targets_sot(FrameAnnotations, case)[0]["instances"]):
        assert got.ori_ids == want.ori_ids and got.image_size == want.image_size
        if len(want):
            assert torch.equal(got.gt_masks.cpu().float(), want.gt_masks) and torch.equal(got.gt_boxes.tensor.cpu(), want.gt_boxes.tensor)
            assert torch.equal(got.gt_classes.cpu(), want.gt_classes)

    inf = InferenceVideoVOS(**cases.vos_kwargs(case)).to(dev)

    def hooked(features, targets=None, **k):                         # (the scripted head is host code: tests/test_clip_loop_cpu.py)
        return _move(head(_move(features, "cpu"), targets=_move(targets, "cpu"), **k), dev)
    model = types.SimpleNamespace(backbone=cases.ScriptedBackbone(), sem_seg_head=hooked)
    targets = [{"task": "sot", "dataset_name": d["dataset_name"], "prompt_type": "visual", "num_frames": case["T"], "video_len": n,
                "inter_image_size": (case["H"], case["W"]), "image_size": (h, w), "instances": d["instances"],
                "file_names": d["file_names"], "mask_palette": d["mask_palette"]}]
    with torch.no_grad():
        outputs = inf.eval(model, [d], targets)
    idmaps = torch.cat(outputs)
    assert idmaps.dtype == torch.uint8 and tuple(idmaps.shape) == (n, 2 * h, 2 * w)                    # one per frame, the record's size
    assert set(idmaps.unique().tolist()) == {0, *cases.VOS_OBJECTS}                                    # the ids of the json
    paths = run.write_vos_outputs(str(tmp_path / "out"), [d], outputs, inf.num_frames, inf.clip_stride)
    assert [os.path.relpath(p, tmp_path / "out") for p in paths] == [f"inference/Annotations/clip0/{f:05d}.png" for f in range(n)]
    back = read_results(str(tmp_path / "out" / "inference" / "Annotations"), "clip0", [f"{f:05d}" for f in range(n)])
    assert np.array_equal(back, idmaps.numpy())


def case_class(cases, j):
    return cases.SCRIPT_OBJECTS[j][0]
