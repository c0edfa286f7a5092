"""CPU: `vos_records_from_dirs` gives, for each of the three converter rules, the records `load_vos_json` gives for the json the converter's
rule writes from the same folders -- `png` / `value` standing in for `segmentation`; the mapper gives the same annotations and palette
from both; the errors; `python -m univs_amd.run --masks-dir`."""
import os

import numpy as np
import pytest
import torch

from tests import idmap_cases as ic
from univs_amd import run
from univs_amd.data import VOSTestMapper, load_vos_json, vos_records_from_dirs
from univs_amd.data.vos_folders import read_idmap
from univs_amd.inference.results import rle_decode

RULES = {"sot_davis17_val": ic.write_davis, "mots_mose_val": ic.write_davis, "sot_davis16_val": ic.write_davis,
         "sot_ytbvos18_val": ic.write_ytvos, "pvos_viposeg_val": ic.write_viposeg}


def assert_same_records(folder, from_json):
    """Key by key; an object's `png` / `value` is its `segmentation`'s plane."""
    assert [r["video_id"] for r in folder] == [r["video_id"] for r in from_json] and len(folder) > 0
    n_objects = 0
    for a, b in zip(folder, from_json):
        assert set(a) == set(b) | {"mask_files"}
        for key in b:
            if key != "annotations":
                assert a[key] == b[key], key
        assert a["mask_files"] == sorted(a["mask_files"]) and all(p.endswith(".png") and os.path.isfile(p) for p in a["mask_files"])
        assert [len(x) for x in a["annotations"]] == [len(x) for x in b["annotations"]]
        for objs_a, objs_b in zip(a["annotations"], b["annotations"]):
            for oa, ob in zip(objs_a, objs_b):
                assert set(oa) - {"png", "value"} == set(ob) - {"segmentation"} and "segmentation" not in oa
                assert {k: v for k, v in oa.items() if k not in ("png", "value")} == {k: v for k, v in ob.items() if k != "segmentation"}
                assert oa["png"] in a["mask_files"]
                assert np.array_equal(read_idmap(oa["png"], a["dataset_name"]) == oa["value"], rle_decode(ob["segmentation"]).astype(bool))
                n_objects += 1
    return n_objects


@pytest.mark.parametrize("name", sorted(RULES))
def test_records_equal_those_of_the_converters_json(tmp_path, name):
    path, image_root, mask_root = RULES[name](str(tmp_path))
    folder = vos_records_from_dirs(image_root, mask_root, name)
    n = assert_same_records(folder, load_vos_json(path, image_root, name))
    assert n == {"sot_ytbvos18_val": 4, "pvos_viposeg_val": 3}.get(name, 4)


def test_the_test_data_holds_what_it_is_meant_to(tmp_path):
    ic.write_davis(str(tmp_path / "d"))
    recs = {r["video_id"]: r for r in vos_records_from_dirs(str(tmp_path / "d" / "JPEGImages"), str(tmp_path / "d" / "Annotations"), "sot_davis17_val")}
    assert sorted(recs) == ["bear", "cat"]                            # "dog" has no annotations
    assert [o["value"] for o in recs["bear"]["annotations"][0]] == [1, 2, 255] and not any(recs["bear"]["annotations"][1:])   # value 3: never read
    assert (recs["cat"]["height"], recs["cat"]["width"]) == (ic.FH + 1, ic.FW) and len(recs["bear"]["mask_files"]) == 2
    ic.write_ytvos(str(tmp_path / "y"))
    recs = {r["video_id"]: r for r in vos_records_from_dirs(str(tmp_path / "y" / "JPEGImages"), str(tmp_path / "y" / "Annotations"), "sot_ytbvos18_val")}
    zz = recs["zz"]["annotations"]
    assert [(o["ori_id"], o["id"]) for o in zz[0]] == [("2", 1)] and zz[1] == [] and [(o["ori_id"], o["id"]) for o in zz[2]] == [("2", 1), ("1", 2)]
    assert [(o["ori_id"], o["id"]) for o in recs["aa"]["annotations"][0]] == [("5", 3)]      # object 6 of the meta never occurs; ids count on
    ic.write_viposeg(str(tmp_path / "v"))
    v0 = vos_records_from_dirs(str(tmp_path / "v" / "JPEGImages"), str(tmp_path / "v" / "Annotations"), "pvos_viposeg_val")[0]
    assert v0["length"] == 4 and [[(o["id"], o["category_id"]) for o in objs] for objs in v0["annotations"]] == [[(1, 12)], [], [(1, 12), (7, 3)], []]


def test_viposeg_dev_prefixes_follow_the_converters_truncation(tmp_path):
    _, image_root, mask_root = ic.write_viposeg(str(tmp_path), n_videos=12)
    for name, n in (("pvos_viposeg_val", 12), ("pvos_viposeg_dev", 1), ("pvos_viposeg_dev0.25", 3)):
        recs = vos_records_from_dirs(image_root, mask_root, name)
        assert sorted(r["video_id"] for r in recs) == sorted(f"v{k}" for k in range(n)) and recs[0]["dataset_name"] == "sot_" + name


def test_host_reader_on_a_grey_file_and_on_a_one_bit_palette_file(tmp_path):
    _, image_root, mask_root = ic.write_davis(str(tmp_path))
    m = ic.idmap("regions", ic.FH, ic.FW, (0, 1, 2, 255))
    ic.save_idmap(os.path.join(mask_root, "bear", "00000.png"), m, mode="L")
    ic.save_idmap(os.path.join(mask_root, "cat", "00000.png"), (ic.idmap("regions", ic.FH + 1, ic.FW, (0, 4), seed=3) > 0).astype(np.uint8), mode="P1")
    from univs_amd.inference import png_read
    info = png_read.parse_png(open(os.path.join(mask_root, "cat", "00000.png"), "rb").read())
    assert (info.colour_type, info.bit_depth) == (3, 1)
    recs = {r["video_id"]: r for r in vos_records_from_dirs(image_root, mask_root, "mots_mose_val", reader="host")}
    assert [o["value"] for o in recs["bear"]["annotations"][0]] == [1, 2, 255]
    assert [o["value"] for o in recs["cat"]["annotations"][0]] == [1]
    assert np.array_equal(read_idmap(recs["bear"]["annotations"][0][0]["png"]), m)


def test_errors(tmp_path):
    path, image_root, mask_root = ic.write_davis(str(tmp_path / "d"))
    with pytest.raises(NotImplementedError, match="BURST"):
        vos_records_from_dirs(image_root, mask_root, "mots_burst_val")
    with pytest.raises(ValueError, match="is no VOS data set"):
        vos_records_from_dirs(image_root, mask_root, "ytvis_2021_val")
    with pytest.raises(ValueError, match="no folder rule"):
        vos_records_from_dirs(image_root, mask_root, "sot_lasot_val")
    with pytest.raises(ValueError, match="reader="):
        vos_records_from_dirs(image_root, mask_root, "sot_davis17_val", reader="device")
    with pytest.raises(FileNotFoundError, match="meta.json"):        # the DAVIS tree has none
        vos_records_from_dirs(image_root, mask_root, "sot_ytbvos18_val")
    with pytest.raises(FileNotFoundError, match="meta.json"):
        vos_records_from_dirs(image_root, mask_root, "pvos_viposeg_val", meta_dir=str(tmp_path))
    # a PNG of another size
    ic.save_idmap(os.path.join(mask_root, "cat", "00000.png"), ic.idmap("regions", ic.FH, ic.FW, (0, 4)))
    with pytest.raises(ValueError, match=r"video cat: annotation .*00000\.png is \(12, 16\), the video's frames are \(13, 16\)"):
        vos_records_from_dirs(image_root, mask_root, "sot_davis17_val")
    os.remove(os.path.join(mask_root, "cat", "00000.png"))
    # a first PNG that is not frame 0's
    ic.save_idmap(os.path.join(mask_root, "cat", "00001.png"), ic.idmap("regions", ic.FH + 1, ic.FW, (0, 4)))
    with pytest.raises(ValueError, match="video cat: its first annotation"):
        vos_records_from_dirs(image_root, mask_root, "sot_davis17_val")


def test_meta_dir_argument(tmp_path):
    path, image_root, mask_root = ic.write_ytvos(str(tmp_path / "y"))
    os.makedirs(tmp_path / "elsewhere")
    os.replace(tmp_path / "y" / "meta.json", tmp_path / "elsewhere" / "meta.json")
    with pytest.raises(FileNotFoundError):
        vos_records_from_dirs(image_root, mask_root, "sot_ytbvos18_val")
    assert_same_records(vos_records_from_dirs(image_root, mask_root, "sot_ytbvos18_val", meta_dir=str(tmp_path / "elsewhere")),
                        load_vos_json(path, image_root, "sot_ytbvos18_val"))


@pytest.mark.parametrize("name", ["sot_davis17_val", "sot_ytbvos18_val", "pvos_viposeg_val"])
def test_mapper_host_gives_the_same_annotations_from_folders_and_from_the_json(tmp_path, name):
    path, image_root, mask_root = RULES[name](str(tmp_path))
    mapper = VOSTestMapper(20, 100, resize="host")
    n = 0
    for a, b in zip(vos_records_from_dirs(image_root, mask_root, name), load_vos_json(path, image_root, name)):
        da, db = mapper(a), mapper(b)
        assert da["mask_palette"] == db["mask_palette"] and da["mask_palette"] is not None
        if name != "pvos_viposeg_val":
            assert da["mask_palette"][:12] == ic.PALETTE[:12] and da["mask_palette"][-3:] == [255, 255, 255]
        assert len(da["instances"]) == len(db["instances"]) == a["length"]
        for x, y in zip(da["instances"], db["instances"]):
            assert x.ori_ids == y.ori_ids and x.image_size == y.image_size and len(x) == len(y)
            if len(x):
                assert x.gt_masks.dtype == y.gt_masks.dtype and torch.equal(x.gt_masks, y.gt_masks)
                assert x.gt_boxes.tensor.dtype == y.gt_boxes.tensor.dtype and torch.equal(x.gt_boxes.tensor, y.gt_boxes.tensor)
                assert x.gt_classes.dtype == y.gt_classes.dtype and torch.equal(x.gt_classes, y.gt_classes)
                n += len(x)
        assert all(torch.equal(p, q) for p, q in zip(da["image"], db["image"]))
    assert n >= 3


BASE = ["--config-file", "c.yaml", "--weights", "w.pth", "--output-dir", "out"]


@pytest.mark.parametrize("more,text", [
    (["--masks-dir", "A", "--video-dir", "J"], "--masks-dir goes with --video-dir and --dataset-name"),
    (["--masks-dir", "A", "--json", "j.json", "--image-root", "J", "--dataset-name", "sot_davis17_val"], "--masks-dir goes with --video-dir"),
    (["--masks-dir", "A", "--dataset-name", "sot_davis17_val"], "give either --json"),
    (["--masks-dir", "A", "--video-dir", "J", "--dataset-name", "ytvis_2021_val"], "--masks-dir reads a VOS data set"),
    (["--vos-meta", "M", "--video-dir", "J"], "--vos-meta goes with --masks-dir"),
    (["--video-dir", "J", "--davis-root", "D"], "--davis-root and --pvos-data score a VOS data set"),
])
def test_run_argument_errors(capsys, more, text):
    with pytest.raises(SystemExit):
        run.parse_args(BASE + more)
    assert text in capsys.readouterr().err


def test_run_arguments_of_the_folder_route():
    args = run.parse_args(BASE + ["--video-dir", "J", "--masks-dir", "A", "--dataset-name", "sot_davis17_val", "--davis-root", "D", "--reader", "gpu"])
    assert args.vos and args.masks_dir == "A" and args.vos_meta is None and args.reader == "gpu" and args.davis_root == "D"
    args = run.parse_args(BASE + ["--video-dir", "J", "--masks-dir", "A", "--dataset-name", "pvos_viposeg_dev", "--vos-meta", "M", "--pvos-data", "V"])
    assert args.vos and args.vos_meta == "M"
    assert not run.parse_args(BASE + ["--video-dir", "J"]).vos        # as before
    assert run.parse_args(BASE + ["--json", "j", "--image-root", "J", "--dataset-name", "sot_davis17_val"]).vos


def test_run_with_masks_dir_writes_the_pngs(tmp_path):
    """`python -m univs_amd.run --video-dir --masks-dir` end to end with a small synthetic model on the CPU path of the operators
    (oracle/cpu_path.py), as tests/test_vos_run_cpu.py runs the json route."""
    from PIL import Image
    from oracle.cpu_path import cpu_ops
    from tests import cases
    from univs_amd import synth
    from univs_amd.config import load_cfg
    from univs_amd.modeling.build import build_model
    _, image_root, mask_root = ic.write_davis(str(tmp_path / "DAVIS"))
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
    with cpu_ops():
        assert run.main(["--config-file", str(tmp_path / "cfg.yaml"), "--weights", str(tmp_path / "w.pth"), "--device", "cpu", "--resize", "host",
                         "--dataset-name", "sot_davis17_val", "--video-dir", image_root, "--masks-dir", mask_root, "--output-dir",
                         str(tmp_path / "out")]) == 0
    for video, n, hw, values in (("bear", 3, (ic.FH, ic.FW), {0, 1, 2, 255}), ("cat", 2, (ic.FH + 1, ic.FW), {0, 4})):
        folder = tmp_path / "out" / "inference" / "Annotations" / video
        assert sorted(os.listdir(folder)) == [f"{i:05d}.png" for i in range(n)]
        for name in os.listdir(folder):
            with Image.open(folder / name) as im:
                assert im.mode == "P" and im.getpalette()[:12] == ic.PALETTE[:12]      # the palette of the annotations
                a = np.asarray(im)
            assert a.shape == hw and set(np.unique(a).tolist()) <= values             # the annotation's values
