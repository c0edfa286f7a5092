"""The g38 scenes (tools/gen_golden_image_eval.py) as trees on disk and as the per-image driver's outputs: shared by
tests/test_image_eval_golden_cpu.py and tests/test_image_eval_gpu.py."""
import glob
import json
import os

import numpy as np
import torch
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = sorted(os.path.basename(p)[len("g38_image_eval_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "g38_image_eval_*.npz")))
SCORED = [s for s in SCENES if not s.startswith("err_")]
ERRORS = [s for s in SCENES if s.startswith("err_")]


def ids_to_rgb(ids):
    ids = np.asarray(ids).astype(np.int64)
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=-1).astype(np.uint8)


class Scene:
    """A fixture and its tree under `root`: gt.json, truth/<id>.png, and (files=True) inference/panoptic/<id>.png with
    inference/predictions.json."""

    def __init__(self, name, root, files=False):
        self.z = np.load(os.path.join(GOLDEN, f"g38_image_eval_{name}.npz"))
        self.root = str(root)
        self.gt, self.pred = json.loads(str(self.z["gt_json"])), json.loads(str(self.z["pred_json"]))
        self.image_ids = [str(i) for i in self.z["image_ids"]]
        self.truth_dir = os.path.join(self.root, "truth")
        self.gt_json = os.path.join(self.root, "gt.json")
        os.makedirs(self.truth_dir, exist_ok=True)
        with open(self.gt_json, "w") as f:
            json.dump(self.gt, f)
        for i in self.image_ids:
            Image.fromarray(ids_to_rgb(self.z["gt_" + i])).save(os.path.join(self.truth_dir, i + ".png"))
        self.panoptic_dir = os.path.join(self.root, "inference", "panoptic")
        if files:
            os.makedirs(self.panoptic_dir, exist_ok=True)
            for i in self.image_ids:
                Image.fromarray(ids_to_rgb(self.z["pred_" + i])).save(os.path.join(self.panoptic_dir, i + ".png"))
            with open(os.path.join(self.root, "inference", "predictions.json"), "w") as f:
                json.dump(self.pred, f)

    def driver_io(self, device="cpu"):
        """[(input, output)] as the mapper and the per-image driver hand them over: the class of a segment as its contiguous index."""
        contiguous = {c["id"]: k for k, c in enumerate(self.gt["categories"])}
        things = {c["id"]: bool(c["isthing"]) for c in self.gt["categories"]}
        out = []
        for i, ann in zip(self.image_ids, self.pred["annotations"]):
            infos = [{"id": s["id"], "isthing": things[s["category_id"]], "category_id": contiguous[s["category_id"]]} for s in ann["segments_info"]]
            pan = torch.as_tensor(self.z["pred_" + i].astype(np.int32)).to(device)
            out.append(({"file_name": f"/data/val/{i}.jpg", "file_names": [f"/data/val/{i}.jpg"], "image_id": i, "dataset_name": "coco_panoptic"},
                        {"panoptic_seg": (pan, infos)}))
        return out

    def check(self, numbers, res):
        """The evaluator's nine numbers and per-class record against the reference's, exactly (nan where the reference divides by zero)."""
        z = self.z
        cats = [int(c) for c in z["cats"]]
        assert list(res["per_class"]) == cats
        for k, c in enumerate(cats):
            r = res["per_class"][c]
            assert (r["tp"], r["fp"], r["fn"]) == (int(z["tp"][k]), int(z["fp"][k]), int(z["fn"][k])), (c, r)
            assert r["iou"] == float(z["iou"][k]), (c, r["iou"], float(z["iou"][k]))
        for row, (name, suffix) in enumerate((("All", ""), ("Things", "_th"), ("Stuff", "_st"))):
            for col, key in enumerate(("pq", "sq", "rq")):
                want, got = float(z["avg"][row, col]), numbers[key.upper() + suffix]
                assert (np.isnan(want) and np.isnan(got)) or got == 100 * want, (name, key, got, want)
            assert res[name]["n"] == int(z["avg"][row, 3])
