"""The test mapper for task "sot" (video object segmentation): the frames as in `VideoTestMapper`, and per frame the annotations of the
objects whose masks are given there -- normally the frame an object first appears in (univs/data/dataset_mapper_uni_vid.py:456-486
with `is_train=False`).

detectron2 is absent; its parts are restated from their documented behaviour.  Per frame the reference keeps the objects with
`iscrowd == 0`, decodes each run-length code to a full-resolution plane, resizes it with `ResizeTransform.apply_segmentation`
(`PIL.Image.fromarray(mask).resize((neww, newh), Image.NEAREST)`), stacks the planes as a bitmask and replaces the boxes of the file
by `BitMasks.get_bounding_boxes()`: [x0, y0, x1 + 1, y1 + 1] of the first and last true column and row as float32, zeros for an empty
mask.  `gt_classes` is `category_id`, `ori_ids` is `ori_id` where the annotation has one and `id` otherwise, `mask_palette` is the
palette of the video's first annotation PNG.  `instances` is one `FrameAnnotations` per frame, empty where the frame has no object.

resize="host" is that, with Pillow itself; it needs no GPU.  resize="gpu" reads the run boundaries of all annotated masks of the
video at once (`runs_from_rles`), uploads them in one copy and resizes them in one call of csrc/mask_prompt_resize.hip, which also
gives the boxes: no source-resolution plane exists, masks and boxes stay on the device.  Both give identical tensors
(tests/test_prompt_masks_gpu.py).  Sizes the kernel does not cover, and videos whose annotated frames differ in size, go the host way.

The records of `vos_records_from_dirs` (vos_folders.py) give an object as `{"png": path, "value": v}` instead of a `"segmentation"`:
its plane is (the annotation PNG's id map == v).  resize="host" opens the PNG by the converter's expression, compares and resizes that
plane with Pillow.  resize="gpu" loads the id maps of the annotated frames once -- one upload, or with decode="gpu" decoded on the
device by png_read_ops.read_pngs_device -- and gathers all objects' masks and boxes from them in one call of csrc/idmap_prompts.hip: NEAREST
is a gather, so neither planes nor codes exist.  Same tensors from all of them (tests/test_vos_folders_gpu.py), same fall-backs.
`mask_palette` is then the palette of the record's first annotation PNG, which is `get_palette`'s answer in that layout.
"""
import logging

import numpy as np
import torch
from PIL import Image

from ..evaluation.vis_counts import runs_from_rles
from ..inference.results import rle_decode
from ..inference.video_vos import FrameAnnotations
from .mapper import VideoTestMapper, _logged, get_palette
from .vos_folders import read_idmap


def bitmask_boxes(masks):
    """float32 [n, 4] of bool [n, h, w]: detectron2's `BitMasks.get_bounding_boxes`."""
    boxes = torch.zeros(masks.shape[0], 4, dtype=torch.float32)
    x_any, y_any = masks.any(dim=1), masks.any(dim=2)
    for i in range(masks.shape[0]):
        x, y = torch.where(x_any[i])[0], torch.where(y_any[i])[0]
        if len(x) > 0 and len(y) > 0:
            boxes[i] = torch.as_tensor([x[0], y[0], x[-1] + 1, y[-1] + 1], dtype=torch.float32)
    return boxes


class VOSTestMapper(VideoTestMapper):
    """`VideoTestMapper` for the records of `load_vos_json`: same constructor and `from_config`."""

    def _idmap(self, path, dataset_name):
        """The id map of an annotation PNG, read once per video."""
        cache = self.__dict__.setdefault("_idmaps", {})
        if path not in cache:
            cache[path] = read_idmap(path, dataset_name)
        return cache[path]

    def _source_plane(self, o, dataset_name):
        """uint8 [H, W] of 0 / 1: the decoded run-length code of a json record's object, (id map == value) of a folder record's."""
        if "png" in o:
            return (self._idmap(o["png"], dataset_name) == o["value"]).astype(np.uint8)
        return rle_decode(o["segmentation"])

    def _host_masks(self, objs, out_hw, dataset_name=""):
        newh, neww = out_hw
        planes = [np.asarray(Image.fromarray(self._source_plane(o, dataset_name)).resize((neww, newh), Image.NEAREST)) for o in objs]
        masks = torch.from_numpy(np.stack(planes)).bool()
        return masks, bitmask_boxes(masks)

    def _gpu_masks(self, frames, in_hw, out_hw, video_id):
        """[(masks, boxes)] of the annotated frames `frames` = [objects of a frame]: all their masks in one launch; None where the
        kernel does not cover the sizes."""
        from .. import prompts_ops
        from ..evaluation.vis_counts import Runs
        codes = [o["segmentation"] for objs in frames for o in objs]
        runs = runs_from_rles(codes, *in_hw, video=video_id)
        n = runs.starts.numel()
        packed = torch.cat([runs.starts, runs.bounds]).to(self.device)               # one upload
        out = prompts_ops.resize_rle_masks_u8(Runs(packed[n:], None, packed[:n]), in_hw, out_hw)
        if out is None:
            return None
        masks, boxes = out[0].view(torch.bool), out[1].to(torch.float32)
        ends = np.cumsum([len(objs) for objs in frames]).tolist()
        return [(masks[b - len(objs):b], boxes[b - len(objs):b]) for objs, b in zip(frames, ends)]

    def _gpu_idmap_masks(self, frames, in_hw, out_hw, video_id, dataset_name=""):
        """`_gpu_masks` for folder records: the id maps of the annotated frames go up once (or are decoded on the device), one call of
        csrc/idmap_prompts.hip gives every object's mask and box; None where the kernel does not cover the sizes, the id maps differ
        in size, or a frame's objects name more than one PNG out of order."""
        from .. import idmap_ops
        paths, frame, value = [], [], []
        for objs in frames:
            for o in objs:
                if o["png"] not in paths:
                    paths.append(o["png"])
                frame.append(paths.index(o["png"]))
                value.append(int(o["value"]))
        if any(a > b for a, b in zip(frame, frame[1:])):
            return None
        if self.decode == "gpu":
            from .vos_folders import _device_maps
            maps = _device_maps(paths, dataset_name, self.device)
            if len({tuple(m.shape) for m in maps}) != 1 or maps[0].dim() != 2:
                return None
            ids = torch.stack(maps)
            lists = torch.tensor([frame, value], dtype=torch.int32).to(self.device)
            frame_d, value_d = lists[0], lists[1]
        else:
            maps = [self._idmap(p, dataset_name) for p in paths]
            if len({m.shape for m in maps}) != 1 or maps[0].ndim != 2:
                return None
            ids, frame_d, value_d = idmap_ops.upload_prompts(np.stack(maps), frame, value, self.device)   # one upload
        out = idmap_ops.idmap_prompts_u8(ids, frame_d, value_d, out_hw)
        if out is None:
            return None
        masks, boxes = out[0].view(torch.bool), out[1].to(torch.float32)
        ends = np.cumsum([len(objs) for objs in frames]).tolist()
        return [(masks[b - len(objs):b], boxes[b - len(objs):b]) for objs, b in zip(frames, ends)]

    def __call__(self, record):
        self._idmaps = {}
        if record["task"] != "sot":
            raise ValueError(f"VOSTestMapper: a record of task {record['task']!r}; data.VideoTestMapper maps the other tasks")
        d = self._map(record)
        in_hw = (d["height"], d["width"])
        annotations = record["annotations"][:d["video_len"]]
        kept = {f: [o for o in objs if o.get("iscrowd", 0) == 0] for f, objs in enumerate(annotations)}
        kept = {f: objs for f, objs in kept.items() if objs}
        sizes = {f: tuple(d["image"][f].shape[1:]) for f in kept}
        from_folders = bool(kept) and all("png" in o for objs in kept.values() for o in objs)
        on_gpu = None
        if self.resize == "gpu" and kept:
            if len(set(sizes.values())) == 1:
                if from_folders:
                    on_gpu = self._gpu_idmap_masks(list(kept.values()), in_hw, next(iter(sizes.values())), d.get("video_id"), d["dataset_name"])
                else:
                    on_gpu = self._gpu_masks(list(kept.values()), in_hw, next(iter(sizes.values())), d.get("video_id"))
                on_gpu = on_gpu and dict(zip(kept, on_gpu))
            if on_gpu is None and "vos-uncovered" not in _logged:
                _logged.add("vos-uncovered")
                logging.getLogger("univs_amd").warning("the first-frame masks of video %s (%dx%d) are not covered by the HIP kernel: resizing "
                                                       "on the host with Pillow (logged once)", d.get("video_id"), *in_hw)
        for f in range(d["video_len"]):
            size = tuple(d["image"][f].shape[1:])
            objs = kept.get(f)
            if not objs:
                d["instances"].append(FrameAnnotations(size))
                continue
            if on_gpu is not None:
                masks, boxes = on_gpu[f]
            else:
                masks, boxes = self._host_masks(objs, size, d["dataset_name"])
                if self.resize == "gpu":
                    masks, boxes = masks.to(self.device), boxes.to(self.device)
            classes = torch.as_tensor([int(o["category_id"]) for o in objs], dtype=torch.int64, device=masks.device)
            ori_ids = [int(o["ori_id"]) if "ori_id" in o else int(o["id"]) for o in objs]
            d["instances"].append(FrameAnnotations(size, ori_ids, masks, boxes, classes))
        if record.get("mask_files"):                                 # (a folder record: what get_palette finds in that layout)
            with Image.open(record["mask_files"][0]) as im:
                d["mask_palette"] = im.convert("P").getpalette()
        else:
            d["mask_palette"] = get_palette(d["file_names"])
        self._idmaps = {}
        return d
