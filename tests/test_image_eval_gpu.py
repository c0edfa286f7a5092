"""GPU: the image chain on the device.  The per-image driver with `sem_seg_as="labels"` equals argmax(0) of its own "scores" result;
PanopticEvaluator and SemSegEvaluator counted on the device equal the CPU counts on the g38 scenes, with png="gpu" and reader="gpu"
as with "host"; the image mapper's device route gives the host route's tensors.  All comparisons are exact."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

from tests.frames_cases import frames
from tests.image_eval_cases import SCORED, Scene, ids_to_rgb
from tests.test_image_seg_gpu import GEOMS, case, driver
from univs_amd.data import ImageTestMapper
from univs_amd.evaluation import image as ie

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("g", [GEOMS[0], GEOMS[2]], ids=str)
@pytest.mark.parametrize("fused", [True, False])
def test_driver_labels_equal_the_argmax_of_its_scores(cuda, g, fused):
    L, cls, padded, crop, out = case(cuda, g, seed=7)
    scores = driver(fused).postprocess(cls, L, padded, crop, out)
    labels = driver(fused, sem_seg_as="labels").postprocess(cls, L, padded, crop, out)
    assert "sem_seg" not in labels and "sem_seg_labels" not in scores
    got = labels["sem_seg_labels"]
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(out) and got.is_cuda
    assert torch.equal(got, scores["sem_seg"].argmax(0).to(torch.uint8))
    assert len(torch.unique(got)) > 1
    assert torch.equal(labels["panoptic_seg"][0], scores["panoptic_seg"][0])         # the other results are untouched
    with pytest.raises(ValueError, match="sem_seg_as"):
        driver(fused, sem_seg_as="bytes").postprocess(cls, L, padded, crop, out)


def evaluate(scene_name, root, device, png="host", reader="host"):
    s = Scene(scene_name, root)
    ev = ie.PanopticEvaluator(s.gt_json, s.truth_dir, str(root / "out"), device=device, png=png, reader=reader)
    for item, output in s.driver_io(device):
        ev.process([item], [output])
    return s, ev, ev.evaluate()


@pytest.mark.parametrize("name", SCORED)
def test_panoptic_evaluator_on_the_device_equals_the_cpu(cuda, name, tmp_path):
    s, ev, out = evaluate(name, tmp_path / "dev", cuda)
    s.check(out["panoptic_seg"], ev.last)                            # the reference's numbers
    _, cpu, ref = evaluate(name, tmp_path / "cpu", "cpu")
    assert json.dumps(out) == json.dumps(ref)
    for i in s.image_ids:
        assert np.array_equal(ev._tables[i].counts, cpu._tables[i].counts)
    _, ev2, both = evaluate(name, tmp_path / "both", cuda, png="gpu", reader="gpu")
    assert json.dumps(both) == json.dumps(ref)
    for i in s.image_ids:                                            # the device's PNG holds the host's pixels
        assert np.array_equal(np.array(Image.open(tmp_path / "both" / "out" / "inference" / "panoptic" / f"{i}.png")), ids_to_rgb(s.z["pred_" + i]))
    files = ie.evaluate_panoptic_files(str(tmp_path / "both" / "out" / "inference" / "panoptic"), s.gt_json, s.truth_dir, device=cuda, reader="gpu")
    assert json.dumps(files["panoptic_seg"]) == json.dumps(ref["panoptic_seg"])


@pytest.mark.parametrize("K", [3, 150, 181])
def test_semseg_evaluator_on_the_device_equals_the_cpu(cuda, K, tmp_path):
    names = ["c%d" % k for k in range(K)]
    results = {}
    for key, device, reader in (("cpu", "cpu", "host"), ("dev", cuda, "host"), ("read", cuda, "gpu")):
        ev = ie.SemSegEvaluator(str(tmp_path), K, 255, names, str(tmp_path / key), device=device, reader=reader)
        gen = np.random.default_rng(K)
        for n, (h, w) in enumerate(((31, 45), (50, 27))):
            gt = gen.integers(0, K, (h, w)).astype(np.uint8)
            gt[gen.random((h, w)) < 0.1] = 255
            pred = np.where(gen.random((h, w)) < 0.6, np.minimum(gt, K - 1), gen.integers(0, K, (h, w))).astype(np.uint8)
            Image.fromarray(gt).save(tmp_path / f"im{n}.png")
            ev.process([{"file_names": [f"/x/im{n}.jpg"]}], [{"sem_seg_labels": torch.as_tensor(pred).to(device)}])
        results[key] = (ev.evaluate(), ev._conf.cpu())
        assert ev._conf.device.type == torch.device(device).type
    for key in ("dev", "read"):
        assert torch.equal(results[key][1], results["cpu"][1]) and json.dumps(results[key][0]) == json.dumps(results["cpu"][0])
    assert int(results["cpu"][1].sum()) == 31 * 45 + 50 * 27 and 0 < results["cpu"][0]["sem_seg"]["mIoU"] < 100


def test_semantic_png_written_on_the_device_holds_the_host_s_pixels(cuda, tmp_path):
    from univs_amd.inference.results import write_semseg_prediction
    labels = torch.as_tensor(np.random.default_rng(1).integers(0, 5, (33, 47)).astype(np.uint8))
    ids = [3, 9, 200, 17, 4]
    item = {"file_names": ["/x/im.jpg"]}
    a = write_semseg_prediction(item, {"sem_seg_labels": labels}, str(tmp_path / "host"), ids, png="host")
    b = write_semseg_prediction(item, {"sem_seg_labels": labels.to(cuda)}, str(tmp_path / "gpu"), ids, png="gpu")
    assert np.array_equal(np.array(Image.open(a)), np.array(Image.open(b)))
    assert np.array_equal(np.array(Image.open(a)), np.array(ids, np.uint8)[labels.numpy()])


def test_image_mapper_on_the_device_gives_the_host_s_tensors(cuda, tmp_path):
    Image.fromarray(frames("noise", 1, 96, 130)[0]).save(tmp_path / "a.jpg", quality=90)
    record = {"file_name": str(tmp_path / "a.jpg"), "image_id": "a"}
    host = ImageTestMapper(48, 80, "BGR", 2, resize="host")(record)
    for decode in ("host", "gpu"):
        dev = ImageTestMapper(48, 80, "BGR", 2, resize="gpu", device=cuda, decode=decode)(record)
        assert len(dev["image"]) == 2 and dev["image"][0].is_cuda and torch.equal(dev["image"][0].cpu(), host["image"][0]), decode
        assert (dev["height"], dev["width"]) == (96, 130) == (host["height"], host["width"])
        assert dev["image_padding_mask"][0].is_cuda and not dev["image_padding_mask"][0].any()
