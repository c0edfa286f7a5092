"""The test path of the reference's `CocoDatasetMapper.__call__` (univs/data/dataset_mapper.py:461-528 with `is_train=False`): one image,
read in INPUT.FORMAT, resized by `ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST)` (the LSJ square caps the long edge: mapper.py's
`resize_params_from_config`) and handed over as SAMPLING_FRAME_NUM copies of one uint8 [3, h, w] tensor, the driver's clip of one image.

The reading and the resizing are `VideoTestMapper`'s, one image per call: resize="host" is Pillow, resize="gpu" goes through
frames_ops.resize_frames_u8, decode="gpu" (with it) through jpeg_ops; the tensors are equal byte for byte whichever way.
Training is not built."""
import copy

import torch
from PIL import Image

from .images import _apply_exif_orientation
from .mapper import VideoTestMapper, resize_params_from_config


class ImageTestMapper(VideoTestMapper):
    def __init__(self, short, max_size, image_format="RGB", sampling_frame_num=1, resize="host", device=None, is_train=False, decode="host"):
        if is_train:
            raise NotImplementedError("training: only the test path of the image mapper is built (no sampling, no augmentation, no annotations)")
        super().__init__(short, max_size, image_format, resize=resize, device=device, decode=decode)
        self.sampling_frame_num = int(sampling_frame_num)

    @classmethod
    def from_config(cls, cfg, resize="host", device=None, decode="host", is_train=False):
        short, max_size = resize_params_from_config(cfg)
        return cls(short, max_size, cfg.INPUT.FORMAT, cfg.INPUT.SAMPLING_FRAME_NUM, resize=resize, device=device, is_train=is_train, decode=decode)

    def __call__(self, record):
        d = copy.deepcopy(record)
        d["has_stuff"] = False
        if "dataset_name" not in d:
            panoptic = "pan_seg_file_name" in d
            d["dataset_name"] = "coco_panoptic" if panoptic else "coco"
            d["has_stuff"] = panoptic
        d["task"] = "detection"
        d.pop("annotations", None)
        file_name = d.pop("file_name")
        n = self.sampling_frame_num
        image = (self._gpu([file_name]) if self.resize == "gpu" else self._host([file_name]))[0]
        d["has_mask"] = True
        d["video_len"] = n
        d["frame_indices"] = list(range(n))
        d["image"] = [image] * n
        d["image_padding_mask"] = [torch.zeros(image.shape[1:], dtype=torch.uint8, device=image.device)] * n
        d["instances"] = []
        d["file_names"] = [file_name] * n
        if "panoptic" in d["dataset_name"]:
            d["file_name"] = file_name                               # (the panoptic evaluator names its PNG after it)
        if "height" not in d or "width" not in d:                    # `check_image_size`: the file's own size where the record has none
            d["height"], d["width"] = self._size(file_name)
        return d

    @staticmethod
    def _size(file_name):
        """(height, width) as `read_image` would return them, from the file's header: no pixel is decoded."""
        with Image.open(file_name) as im:
            w, h = _apply_exif_orientation(im).size
        return int(h), int(w)
