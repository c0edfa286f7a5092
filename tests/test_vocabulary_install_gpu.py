"""GPU: `vocabulary.install` on the synthetic model on the device: the checks of tests/test_vocabulary_install_cpu.py on the HIP operators."""
import pytest

from tests.test_vocabulary_install_cpu import check_image_driver, check_install

pytestmark = pytest.mark.gpu


def test_install_on_the_synthetic_model(cuda):
    check_install(cuda)


def test_image_driver_under_the_installed_name(cuda):
    check_image_driver(cuda)


@pytest.mark.parametrize("sub_task", ["vss", "vps"])
def test_video_run_under_a_categories_file(cuda, tmp_path, monkeypatch, sub_task):
    """`python -m univs_amd.run --video-dir D --class-names F --sub-task S`: the entity loop under the installed vocabulary; the names
    reach legend.json and inference/vocabulary.json.  (The table comes from a stand-in: the synthetic model's is 640 wide.)"""
    import json
    import os

    import torch

    from tests import cases
    from tests import overlay_cases as oc
    from univs_amd import run, vocabulary
    names = ["person", "traffic light", "dog", "giraffe", "red jacket", "cats dogs"]
    (tmp_path / "cats.json").write_text(json.dumps({"categories": [{"id": 7 * i + 3, "name": n, "isthing": int(i % 2)} for i, n in enumerate(names)]}))
    os.makedirs(tmp_path / "videos")
    oc.write_videos(str(tmp_path / "videos"), n_videos=1)
    cfg, weights = oc.write_model(str(tmp_path), "vis")                 # the config's own sub-task is another one
    monkeypatch.setattr(vocabulary, "class_embeddings", lambda n, enc, tok=None: cases.clip_table()[2924:2924 + len(n)].clone())
    monkeypatch.setattr(vocabulary, "build_lang_encoder", lambda w, device=None: None)
    out = tmp_path / "out"
    assert run.main(["--config-file", cfg, "--weights", weights, "--video-dir", str(tmp_path / "videos"), "--device", "cuda", "--output-dir", str(out),
                     "--class-names", str(tmp_path / "cats.json"), "--clip-weights", "clip.pkl", "--sub-task", sub_task, "--visualize", "gpu"]) == 0
    assert json.load(open(out / "inference" / "vocabulary.json")) == {str(i): n for i, n in enumerate(names)}
    saved = torch.load(out / "video0.pt")
    assert saved["task"] == sub_task
    if sub_task == "vss":
        assert int(torch.as_tensor(saved["pred_masks"]).max()) < len(names)
    else:
        assert all(1 <= i["category_id"] <= len(names) and i["isthing"] == ((i["category_id"] - 1) % 2 == 1) for i in saved["segments_infos"])
    legend = json.load(open(out / "inference" / "Overlays" / "video0" / "legend.json"))
    assert (legend or sub_task == "vps") and {e["name"] for e in legend.values()} <= set(names)      # (a panoptic map may hold no segment)
