"""The test path of the reference's `UniVidDatasetMapper` (univs/data/dataset_mapper_uni_vid.py:295-454 with `is_train=False`): every
frame of the record, read, resized by `ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST)` and handed over as uint8 [3, h, w].

resize="host" is the reference's way, `PIL.Image.resize` per frame on the host (what detectron2's `ResizeTransform` calls for uint8
images); it needs no GPU.  resize="gpu" decodes on the host, uploads the frames of a video in batches and resizes them with
csrc/frame_resize.hip, which gives Pillow's bytes exactly (tests/test_frame_resize_gpu.py); `image` then stays on the device, where the
drivers want it.  Sizes the kernel does not cover go through Pillow.  decode="gpu" (with resize="gpu" only) also decodes on the device:
the files' compressed bytes go up, csrc/jpeg_decode.hip gives Pillow's pixels for the baseline JPEG files it covers and the decoded batch
goes straight to the resize, no pixel crosses the bus; any other file is read on the host as before (images.py: decoded_runs).  The
default is decode="host", and the dictionaries are equal tensor for tensor (tests/test_jpeg_mapper_gpu.py).

Task "sot" (first-frame annotations) has a mapper of its own, `VOSTestMapper` in vos_mapper.py; this one refuses it and says so.
Not built: raw video files, training -- each raises NotImplementedError and says which."""
import copy
import glob
import logging

import numpy as np
import torch
from PIL import Image

from ..modeling.language import clean_strings
from .images import decoded_runs, read_image
from .resize_rule import shortest_edge_size

_BATCH_BYTES = 256 << 20                                             # decoded frames uploaded and resized per launch
_logged = set()


def resize_params_from_config(cfg):
    """(short, max_size) of `build_augmentation`'s test branch (univs/data/augmentation.py:555-563)."""
    max_size = cfg.INPUT.MAX_SIZE_TEST
    if cfg.INPUT.LSJ_AUG.SQUARE_ENABLED:
        max_size = min(max_size, cfg.INPUT.LSJ_AUG.IMAGE_SIZE)
    return cfg.INPUT.MIN_SIZE_TEST, max_size


def transform_expressions_test(expressions_list):
    """`transform_expressions(..., is_train=False)` without a flip (dataset_mapper_uni_vid.py:638-674)."""
    out = []
    for expressions in expressions_list:
        if len(expressions) == 0:
            out.append("")
        elif isinstance(expressions[0], list):                       # ref-davis: [["exp1", "exp2", ...]]
            out.append(clean_strings(expressions[0]))
        else:                                                        # ref-coco, ref-youtube-vos: ["exp1"], or one string
            out.append(clean_strings(expressions))
    return out


def get_palette(file_names):
    """The palette of a DAVIS video's first annotation PNG (.../Annotations/... beside .../JPEGImages/...), None without one
    (dataset_mapper_uni_vid.py:619-636, the branch the test path reaches)."""
    anno_dir = file_names[0].split("/")[:-1]
    if "JPEGImages" not in anno_dir:
        return None
    anno_dir[anno_dir.index("JPEGImages")] = "Annotations"
    names = sorted(glob.glob("/".join(anno_dir + ["*.png"])))
    if not names:
        return None
    with Image.open(names[0]) as im:
        return im.convert("P").getpalette()


def _pil_resize(image, newh, neww):
    """detectron2's `ResizeTransform.apply_image` for a uint8 [H, W, 3] array."""
    return np.asarray(Image.fromarray(np.ascontiguousarray(image)).resize((neww, newh), Image.BILINEAR))


class VideoTestMapper:
    def __init__(self, short, max_size, image_format="RGB", resize="host", device=None, is_train=False, decode="host"):
        if is_train:
            raise NotImplementedError("training: only the test path of the mapper is built (no sampling, no augmentation, no annotations)")
        if resize not in ("gpu", "host"):
            raise ValueError(f"VideoTestMapper: resize={resize!r} (\"gpu\" or \"host\")")
        if image_format not in ("RGB", "BGR"):
            raise ValueError(f"VideoTestMapper: image_format={image_format!r} (\"RGB\" or \"BGR\")")
        if decode not in ("gpu", "host"):
            raise ValueError(f"VideoTestMapper: decode={decode!r} (\"gpu\" or \"host\")")
        if decode == "gpu" and resize != "gpu":
            raise ValueError("VideoTestMapper: decode=\"gpu\" hands device frames to the device resize: it needs resize=\"gpu\"")
        self.short, self.max_size, self.image_format, self.resize, self.decode = int(short), int(max_size), image_format, resize, decode
        self.device = torch.device("cuda" if device is None else device) if resize == "gpu" else None

    @classmethod
    def from_config(cls, cfg, resize="host", device=None, decode="host"):
        short, max_size = resize_params_from_config(cfg)
        return cls(short, max_size, cfg.INPUT.FORMAT, resize=resize, device=device, decode=decode)

    # ---- the two ways of resizing: both return the list of uint8 [3, h, w] tensors ------------------------------------------------------
    def _host(self, file_names):
        images = []
        for path in file_names:
            image = read_image(path, self.image_format)
            newh, neww = shortest_edge_size(image.shape[0], image.shape[1], self.short, self.max_size)
            images.append(torch.as_tensor(np.ascontiguousarray(_pil_resize(image, newh, neww).transpose(2, 0, 1))))
        return images

    def _gpu_batch(self, batch):
        """The resize of a batch of RGB frames of one size: host arrays [H, W, 3] (uploaded here), or one device tensor [n, H, W, 3]."""
        from .. import frames_ops
        on_device = torch.is_tensor(batch)
        H, W = batch[0].shape[:2]
        out_hw = shortest_edge_size(H, W, self.short, self.max_size)
        bgr = self.image_format == "BGR"
        out = frames_ops.resize_frames_u8(batch.contiguous() if on_device else torch.from_numpy(np.stack(batch)).to(self.device), out_hw, bgr=bgr)
        if out is None and on_device:
            batch = list(batch.cpu().numpy())
        if out is None:                                              # not covered (a down-scale beyond 4): Pillow, then the upload
            if "uncovered" not in _logged:
                _logged.add("uncovered")
                logging.getLogger("univs_amd").warning("frame resize %dx%d -> %dx%d is not covered by the HIP kernel: resizing on the host "
                                                       "with Pillow (logged once)", H, W, *out_hw)
            host = np.stack([_pil_resize(a[:, :, ::-1] if bgr else a, *out_hw).transpose(2, 0, 1) for a in batch])
            out = torch.from_numpy(host).to(self.device)
        return list(out)

    def _gpu(self, file_names):
        if self.decode == "gpu":
            return [im for run in decoded_runs(file_names, self.device, _BATCH_BYTES) for im in self._gpu_batch(run)]
        images, batch = [], []
        for path in file_names:
            image = read_image(path, "RGB")                          # (the kernel's flag reverses the channels for "BGR")
            if batch and (image.shape != batch[0].shape or (len(batch) + 1) * image.nbytes > _BATCH_BYTES):
                images += self._gpu_batch(batch)
                batch = []
            batch.append(image)
        if batch:
            images += self._gpu_batch(batch)
        return images

    def __call__(self, record):
        if not record.get("is_raw_video") and record["task"] == "sot":
            raise NotImplementedError("task \"sot\": this mapper reads no annotations; data.VOSTestMapper (vos_mapper.py) maps the records of "
                                      "data.load_vos_json, first-frame masks included")
        return self._map(record)

    def _map(self, record):
        """The mapper's dictionary of a record of any task, without per-frame annotations."""
        d = copy.deepcopy(record)
        if d.get("is_raw_video"):
            raise NotImplementedError(f"raw video input (video {d.get('video_id')}): torchvision.io is absent; convert the video to frames first")
        task = d["task"]
        d.pop("annotations", None)
        file_names = d.pop("file_names")
        n = d["length"]
        d["video_len"] = n
        d["frame_indices"] = list(range(n))
        d["file_names"] = list(file_names[:n])
        d["image"] = self._gpu(d["file_names"]) if self.resize == "gpu" else self._host(d["file_names"])
        d["image_padding_mask"] = [torch.zeros(im.shape[1:], dtype=torch.uint8, device=im.device) for im in d["image"]]
        d["instances"] = []
        if task == "grounding":
            expressions = d["expressions"]
            if expressions and isinstance(expressions[0], list):
                expressions = sum(expressions, [])
            d["expressions"] = transform_expressions_test(expressions)
            d["exp_obj_ids"] = d["exp_id"]
            if "davis" in d["dataset_name"]:
                d["mask_palette"] = get_palette(file_names)
        return d
