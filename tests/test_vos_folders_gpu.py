"""GPU: a VOS data set in its own folders.  The mapper gives tensor-for-tensor equal annotations from folder records with resize="gpu"
(csrc/idmap_prompts.hip), with resize="host" (Pillow), with decode="gpu" (the PNGs through the device reader) and from the json records
with resize="gpu" (csrc/mask_prompt_resize.hip); `vos_records_from_dirs(reader="gpu")` equals reader="host"; a tiny video goes through
`python -m univs_amd.run --masks-dir` to PNGs and back."""
import os

import numpy as np
import pytest
import torch

from tests import cases, idmap_cases as ic
from univs_amd import run, synth
from univs_amd.config import load_cfg
from univs_amd.data import VOSTestMapper, load_vos_json, vos_records_from_dirs
from univs_amd.evaluation.davis import read_results
from univs_amd.modeling.build import build_model

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
RULES = {"sot_davis17_val": ic.write_davis, "sot_ytbvos18_val": ic.write_ytvos, "pvos_viposeg_val": ic.write_viposeg}


def assert_same_instances(a, b):
    assert [len(x) for x in a["instances"]] == [len(x) for x in b["instances"]]
    n = 0
    for x, y in zip(a["instances"], b["instances"]):
        assert x.ori_ids == y.ori_ids and x.image_size == y.image_size
        if len(x):
            assert x.gt_masks.dtype == y.gt_masks.dtype and torch.equal(x.gt_masks.cpu(), y.gt_masks.cpu())
            assert x.gt_boxes.tensor.dtype == y.gt_boxes.tensor.dtype and torch.equal(x.gt_boxes.tensor.cpu(), y.gt_boxes.tensor.cpu())
            assert x.gt_classes.dtype == y.gt_classes.dtype and torch.equal(x.gt_classes.cpu(), y.gt_classes.cpu())
            n += len(x)
    assert a["mask_palette"] == b["mask_palette"]
    return n


@pytest.mark.parametrize("name", sorted(RULES))
def test_mapper_gives_the_same_annotations_from_four_sources(tmp_path, name):
    path, image_root, mask_root = RULES[name](str(tmp_path))
    folder, from_json = vos_records_from_dirs(image_root, mask_root, name), load_vos_json(path, image_root, name)
    n = 0
    for a, b in zip(folder, from_json):
        host = VOSTestMapper(20, 100, resize="host")(a)
        gpu = VOSTestMapper(20, 100, resize="gpu", device=dev)(a)
        json_gpu = VOSTestMapper(20, 100, resize="gpu", device=dev)(b)
        decoded = VOSTestMapper(20, 100, resize="gpu", device=dev, decode="gpu")(a)
        n += assert_same_instances(gpu, host)
        assert_same_instances(gpu, json_gpu)
        assert_same_instances(gpu, decoded)
        for inst in gpu["instances"] + decoded["instances"]:
            if len(inst):
                assert inst.gt_masks.is_cuda and inst.gt_boxes.tensor.is_cuda and inst.gt_classes.is_cuda
        assert all(torch.equal(x.cpu(), y) for x, y in zip(gpu["image"], host["image"]))
    assert n >= 3


@pytest.mark.parametrize("name", sorted(RULES))
def test_records_with_the_device_reader_equal_those_with_the_host_reader(tmp_path, name):
    _, image_root, mask_root = RULES[name](str(tmp_path))
    if name == "sot_davis17_val":                                    # a file the device reader does not take: the host expression reads it
        from PIL import Image
        m = ic.idmap("regions", ic.FH + 1, ic.FW, (0, 4), seed=3)
        Image.fromarray(np.stack([m, m, m], -1)).save(os.path.join(mask_root, "cat", "00000.png"))
    host = vos_records_from_dirs(image_root, mask_root, name, reader="host")
    assert vos_records_from_dirs(image_root, mask_root, name, reader="gpu", device=dev) == host and sum(len(o) for r in host for o in r["annotations"]) >= 3


def test_a_video_on_disk_through_run_with_masks_dir_to_pngs_and_back(tmp_path):
    """The folder route and the json route of `run.main` on the same tree and the same synthetic model write the same PNGs: the palette
    of the annotations, ids from the annotation's values."""
    path, image_root, mask_root = ic.write_davis(str(tmp_path / "DAVIS"))
    torch.save(cases.clip_table(), tmp_path / "clip.pt")
    (tmp_path / "cfg.yaml").write_text(f"""MODEL:
  META_ARCHITECTURE: UniVS_Prompt
  MASK_FORMER:
    NUM_OBJECT_QUERIES: 20
  UniVS:
    CLIP_CLASS_EMBED_PATH: {tmp_path / "clip.pt"}
    TEST:
      VIDEO_UNIFIED_INFERENCE_ENABLE: False
INPUT:
  SAMPLING_FRAME_NUM: 2
  MIN_SIZE_TEST: 32
  MAX_SIZE_TEST: 64
""")
    model = build_model(load_cfg(str(tmp_path / "cfg.yaml"))).eval()
    synth.load_synthetic(model)
    torch.save({"model": model.state_dict()}, tmp_path / "w.pth")
    base = ["--config-file", str(tmp_path / "cfg.yaml"), "--weights", str(tmp_path / "w.pth"), "--device", "cuda", "--dataset-name", "sot_davis17_val"]
    assert run.main(base + ["--video-dir", image_root, "--masks-dir", mask_root, "--reader", "gpu", "--output-dir", str(tmp_path / "folders")]) == 0
    assert run.main(base + ["--json", path, "--image-root", image_root, "--output-dir", str(tmp_path / "json")]) == 0
    for video, n, hw, values in (("bear", 3, (ic.FH, ic.FW), {0, 1, 2, 255}), ("cat", 2, (ic.FH + 1, ic.FW), {0, 4})):
        stems = [f"{i:05d}" for i in range(n)]
        folder = tmp_path / "folders" / "inference" / "Annotations" / video
        assert sorted(os.listdir(folder)) == [s + ".png" for s in stems]
        back = read_results(str(tmp_path / "folders" / "inference" / "Annotations"), video, stems)
        assert back.shape == (n,) + hw and back.dtype == np.uint8 and set(np.unique(back).tolist()) <= values
        assert np.array_equal(back, read_results(str(tmp_path / "json" / "inference" / "Annotations"), video, stems))
        from PIL import Image
        with Image.open(folder / "00000.png") as im:
            assert im.mode == "P" and im.getpalette()[:12] == ic.PALETTE[:12]
