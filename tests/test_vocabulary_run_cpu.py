"""CPU: `python -m univs_amd.run --class-names`: the argument rules, that the argument lists of the existing run tests parse as they
did, and an image run end to end under a vocabulary made from a names file (the table itself comes from a stand-in here: the text
tower behind `class_embeddings` has tests of its own, and the synthetic model's table is 640 wide)."""
import glob
import json
import os

import numpy as np
import pytest
from PIL import Image

from oracle.cpu_path import cpu_ops
from tests import cases
from tests.test_image_run_cpu import CATEGORIES, H, N, W, tree  # noqa: F401  (the fixture: images, config, weights, categories)
from univs_amd import run, vocabulary

BASE = ["--config-file", "c", "--weights", "w", "--output-dir", "o"]
NEW = ("class_names", "clip_weights", "sub_task")
NAMES = ["person", "traffic light", "dog", "giraffe", "red jacket"]


@pytest.fixture
def files(tmp_path):
    txt, js, bare = tmp_path / "names.txt", tmp_path / "categories.json", tmp_path / "bare.json"
    txt.write_text("\n".join(NAMES) + "\n")
    js.write_text(json.dumps({"categories": [{"id": i + 1, "name": n, "isthing": int(i < 3)} for i, n in enumerate(NAMES)]}))
    bare.write_text(json.dumps({"categories": [{"id": i + 1, "name": n} for i, n in enumerate(NAMES)]}))
    return str(txt), str(js), str(bare)


def test_class_names_go_with_a_folder_of_frames_or_of_images(files):
    txt, js, bare = files
    a = run.parse_args(BASE + ["--video-dir", "d", "--class-names", txt])
    assert (a.class_names, a.sub_task, a.clip_weights, a.dataset_name, a.image, a.vos) == (txt, None, None, "custom", False, False)
    a = run.parse_args(BASE + ["--video-dir", "d", "--class-names", js, "--sub-task", "vps", "--clip-weights", "clip.pkl", "--dataset-name", "mine"])
    assert (a.sub_task, a.clip_weights, a.dataset_name) == ("vps", "clip.pkl", "mine")
    assert run.parse_args(BASE + ["--video-dir", "d", "--class-names", txt, "--sub-task", "vss"]).sub_task == "vss"
    a = run.parse_args(BASE + ["--image-dir", "d", "--class-names", txt])                       # no --dataset-name, no --categories-json
    assert a.image is True and a.dataset_name == "custom" and a.categories_json is None


@pytest.mark.parametrize("more,text", [
    (["--video-dir", "d", "--sub-task", "vps", "--class-names", "TXT"], "--sub-task vps needs to know which names are things"),
    (["--video-dir", "d", "--sub-task", "vps", "--class-names", "BARE"], "--sub-task vps needs to know which names are things"),
    (["--json", "j", "--image-root", "r", "--dataset-name", "ytvis_2021_val", "--class-names", "TXT"], "not with --json"),
    (["--video-dir", "d", "--sub-task", "vis"], "go with --class-names"),
    (["--video-dir", "d", "--clip-weights", "w"], "go with --class-names"),
    (["--image-dir", "d", "--class-names", "TXT", "--sub-task", "vss"], "an image run has none"),
    (["--image-dir", "d", "--class-names", "TXT", "--dataset-name", "coco"], "none of the named ones"),
    (["--video-dir", "d", "--class-names", "TXT", "--gt-json", "g"], "no evaluator"),
    (["--video-dir", "d", "--class-names", "TXT", "--masks-dir", "m", "--dataset-name", "sot_davis17_val"], "not for a VOS run"),
    (["--video-dir", "d", "--class-names", "TXT", "--sub-task", "panoptic"], "invalid choice")])
def test_argument_errors(files, capsys, more, text):
    names = dict(zip(("TXT", "JS", "BARE"), files))
    with pytest.raises(SystemExit):
        run.parse_args(BASE + [names.get(m, m) for m in more])
    assert text in capsys.readouterr().err


# the argument lists of the run tests that were here before (tests/test_frames_mapper_cpu.py, test_vos_mapper_cpu.py,
# test_vos_folders_cpu.py, test_image_run_cpu.py, test_overlay_rule_cpu.py, test_png_capi_cpu.py, test_hota_eval_cpu.py) with what
# they are known to parse to
JS = ["--json", "j", "--image-root", "r"]
EXISTING = [
    (["--video-dir", "d", "INPUT.MIN_SIZE_TEST", "512"], dict(video_dir="d", resize="gpu", opts=["INPUT.MIN_SIZE_TEST", "512"], vos=False, image=False)),
    (JS + ["--dataset-name", "sot_davis17_val", "--davis-root", "D"], dict(vos=True, davis_root="D", pvos_data=None, image=False)),
    (JS + ["--dataset-name", "pvos_viposeg_val", "--pvos-data", "P"], dict(vos=True, pvos_data="P")),
    (JS + ["--dataset-name", "ytvis_2021_val"], dict(vos=False, dataset_name="ytvis_2021_val", image=False)),
    (["--video-dir", "J", "--masks-dir", "A", "--dataset-name", "sot_davis17_val", "--davis-root", "D", "--reader", "gpu"],
     dict(vos=True, masks_dir="A", vos_meta=None, reader="gpu")),
    (["--video-dir", "d", "--pan-gt-json", "p", "--truth-dir", "t"], dict(image=False, vos=False, pan_gt_json="p", dataset_name=None)),
    (["--dataset-name", "ade20k", "--image-root", "r", "--pan-gt-json", "p", "--truth-dir", "t", "--sem-gt-dir", "s"], dict(image=True, vos=False)),
    (["--image-dir", "d", "--dataset-name", "coco_panoptic", "--categories-json", "c"], dict(image=True, dataset_name="coco_panoptic", batch=1)),
    (["--video-dir", "d", "--visualize", "gpu", "--png", "gpu", "--decode", "gpu"], dict(visualize="gpu", png="gpu", decode="gpu", dataset_name=None)),
    (JS + ["--dataset-name", "ytvis_2021_val", "--gt-json", "g", "--hota"], dict(hota=True, gt_json="g", vos=False))]
PARENT_KEYS = {"config_file", "weights", "json", "image_root", "dataset_name", "video_dir", "masks_dir", "vos_meta", "image_dir", "sem_gt_dir", "batch",
               "output_dir", "resize", "decode", "png", "reader", "visualize", "categories_json", "device", "gt_json", "hota", "pan_gt_json",
               "truth_dir", "davis_root", "pvos_data", "opts", "image", "vos"}


@pytest.mark.parametrize("argv,expect", EXISTING, ids=lambda v: " ".join(v) if isinstance(v, list) else "")
def test_existing_argument_lists_parse_to_the_same_namespace(argv, expect):
    a = vars(run.parse_args(BASE + argv))
    assert set(a) == PARENT_KEYS | set(NEW) and all(a[k] is None for k in NEW)
    assert {k: a[k] for k in expect} == expect
    assert (a["config_file"], a["weights"], a["output_dir"]) == ("c", "w", "o")


def test_image_run_under_a_names_file(tree, files, tmp_path, monkeypatch):  # noqa: F811
    folder, cfg, weights, _ = tree
    txt, js, _ = files
    made = []

    def stand_in(names, lang_encoder, tokenizer=None):
        made.append((list(names), lang_encoder))
        return cases.clip_table()[2641:2641 + len(names)].clone()       # (rows of the synthetic table: what the synthetic head separates)
    monkeypatch.setattr(vocabulary, "class_embeddings", stand_in)
    monkeypatch.setattr(vocabulary, "build_lang_encoder", lambda w, device=None: ("encoder of", w))
    out = tmp_path / "out"
    argv = ["--config-file", cfg, "--weights", weights, "--image-dir", folder, "--output-dir", str(out), "--resize", "host", "--device", "cpu",
            "--class-names", js, "--clip-weights", "clip.pkl", "--visualize", "host"]
    with cpu_ops():
        assert run.main(argv) == 0
    assert made == [(NAMES, ("encoder of", "clip.pkl"))]
    inf = out / "inference"
    assert json.load(open(inf / "vocabulary.json")) == {str(i): n for i, n in enumerate(NAMES)}
    for i in range(N):
        sem = np.array(Image.open(inf / "sem_seg" / f"im{i}.png"))
        assert sem.shape == (H, W) and set(np.unique(sem).tolist()) <= set(range(len(NAMES)))
    records = json.load(open(inf / "coco_instances_results.json"))
    assert records and {r["category_id"] for r in records} <= {0, 1, 2}                  # the things of the file
    legends = glob.glob(str(out / "**" / "*.legend.json"), recursive=True)
    assert len(legends) == N
    for path in legends:
        shown = {v["name"] for v in json.load(open(path)).values()}
        assert shown and shown <= set(NAMES), shown
    with pytest.raises(SystemExit, match="--clip-weights"):                              # this config builds no language encoder
        run.main([a for a in argv if a not in ("--clip-weights", "clip.pkl")])
