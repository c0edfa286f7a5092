"""CPU: `python -m univs_amd.run` on a VOS data set, end to end with a small synthetic model on the CPU path of the operators
(oracle/cpu_path.py): a DAVIS-shaped tree of jpg frames, annotation PNGs and a json with first-frame run-length codes goes in,
inference/Annotations/<video>/<frame>.png and, with --davis-root, davis-metrics.txt come out."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle.cpu_path import cpu_ops
from tests import cases, prompt_masks_cases as pc
from tests.frames_cases import frames
from univs_amd import run, synth
from univs_amd.config import load_cfg
from univs_amd.modeling.build import build_model

H, W, N = 48, 72, 4
SEQS = {"bear": {1: ("blob", 1), 2: ("blob", 2)}, "camel": {1: ("blob", 3)}}      # sequence -> object id -> its mask in every frame


@pytest.fixture(scope="module")
def davis(tmp_path_factory):
    """(davis root, json, image root, config file, weights): DAVIS 2017's layout at Full-Resolution with 4 frames per sequence."""
    root = tmp_path_factory.mktemp("davis")
    davis_root = root / "DAVIS"
    image_root = davis_root / "JPEGImages" / "Full-Resolution"
    os.makedirs(davis_root / "ImageSets" / "2017")
    (davis_root / "ImageSets" / "2017" / "val.txt").write_text("".join(s + "\n" for s in SEQS))
    videos, annotations = [], []
    for v, (seq, objects) in enumerate(SEQS.items(), start=1):
        os.makedirs(image_root / seq)
        os.makedirs(davis_root / "Annotations" / "Full-Resolution" / seq)
        idmap = np.zeros((H, W), np.uint8)
        for oid, (kind, seed) in objects.items():
            idmap[pc.mask(kind, H, W, seed) > 0] = oid
        for i, f in enumerate(frames("noise", N, H, W)):
            Image.fromarray(f).save(image_root / seq / f"{i:05d}.jpg")
            im = Image.fromarray(idmap, mode="P")
            im.putpalette([0, 0, 0, 128, 0, 0, 0, 128, 0] + [0] * 759)
            im.save(davis_root / "Annotations" / "Full-Resolution" / seq / f"{i:05d}.png")
        videos.append({"id": v, "file_names": [f"{seq}/{i:05d}.jpg" for i in range(N)], "height": H, "width": W, "length": N})
        for oid in objects:
            first = pc.code_of((idmap == oid).astype(np.uint8), compressed=True)
            annotations.append({"id": 10 * v + oid, "ori_id": oid, "video_id": v, "category_id": 1, "iscrowd": 0,
                                "segmentations": [first] + [None] * (N - 1), "bboxes": [[0, 0, 1, 1]] + [None] * (N - 1)})
    (root / "vos.json").write_text(json.dumps({"videos": videos, "annotations": annotations, "categories": [{"id": 1, "name": "object"}]}))
    torch.save(cases.clip_table(), root / "clip.pt")
    (root / "cfg.yaml").write_text(f"""MODEL:
  META_ARCHITECTURE: UniVS_Prompt
  MASK_FORMER:
    NUM_OBJECT_QUERIES: 20
  UniVS:
    CLIP_CLASS_EMBED_PATH: {root / "clip.pt"}
    TEST:
      VIDEO_UNIFIED_INFERENCE_ENABLE: False
INPUT:
  SAMPLING_FRAME_NUM: 2
  MIN_SIZE_TEST: 32
  MAX_SIZE_TEST: 64
""")
    model = build_model(load_cfg(str(root / "cfg.yaml"))).eval()
    synth.load_synthetic(model)
    torch.save({"model": model.state_dict()}, root / "w.pth")
    return str(davis_root), str(root / "vos.json"), str(image_root), str(root / "cfg.yaml"), str(root / "w.pth")


def arguments(davis, out, *more):
    davis_root, path, image_root, cfg, weights = davis
    return ["--config-file", cfg, "--weights", weights, "--json", path, "--image-root", image_root, "--dataset-name", "sot_davis17_val",
            "--output-dir", str(out), "--resize", "host", "--device", "cpu", *more]


def test_vos_run_writes_the_pngs(davis, tmp_path):
    with cpu_ops():
        assert run.main(arguments(davis, tmp_path)) == 0
    for seq, objects in SEQS.items():
        folder = tmp_path / "inference" / "Annotations" / seq
        assert sorted(os.listdir(folder)) == [f"{i:05d}.png" for i in range(N)]
        for name in os.listdir(folder):
            with Image.open(folder / name) as im:
                assert im.mode == "P" and im.getpalette()[:9] == [0, 0, 0, 128, 0, 0, 0, 128, 0]      # the palette of the annotations
                a = np.asarray(im)
            assert a.shape == (H, W) and a.dtype == np.uint8 and set(np.unique(a).tolist()) <= {0, *objects}      # the `ori_id`s
    assert not os.path.exists(tmp_path / "inference" / "davis-metrics.txt") and not list(tmp_path.glob("*.pt"))


def test_vos_run_scores_with_the_davis_evaluator(davis, tmp_path, capsys):
    with cpu_ops():
        assert run.main(arguments(davis, tmp_path, "--davis-root", davis[0])) == 0
    text = (tmp_path / "inference" / "davis-metrics.txt").read_text()
    assert "Saving metric J" in text and "Saving metric F" in text
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(res) == {"J", "F"} and len(res["J"]["M"]) == 3       # two objects of one sequence, one of the other
    assert sorted(res["J"]["M_per_object"]) == ["bear_1", "bear_2", "camel_1"]
