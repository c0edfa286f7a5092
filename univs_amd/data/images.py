"""`read_image` of detectron2's detection_utils (the reference's copy: univs/data/detection_utils.py:60-187), restated because
detectron2 is absent: open with PIL, apply the EXIF orientation, convert to RGB, reverse the channels for "BGR".

`read_images` reads a list of files either that way (decode="host", the default) or with the device JPEG decoder (decode="gpu":
jpeg_ops.py, csrc/jpeg_decode.hip), which gives Pillow's bytes for the baseline files it covers; every other file, and every file
whose data breaks a rule, goes through `read_image` unchanged and is uploaded, so a corrupt file raises what the host reader raises."""
import logging

import numpy as np
from PIL import Image

_EXIF_ORIENT = 274                                                   # the EXIF tag "Orientation"
_TRANSPOSE = {2: Image.FLIP_LEFT_RIGHT, 3: Image.ROTATE_180, 4: Image.FLIP_TOP_BOTTOM, 5: Image.TRANSPOSE, 6: Image.ROTATE_270,
              7: Image.TRANSVERSE, 8: Image.ROTATE_90}


def _apply_exif_orientation(image):
    try:
        exif = image.getexif()
    except Exception:                                                # (files whose EXIF block does not parse are read as they are)
        exif = None
    method = None if exif is None else _TRANSPOSE.get(exif.get(_EXIF_ORIENT))
    return image if method is None else image.transpose(method)


def read_image(path, format="RGB"):
    """uint8 [H, W, 3] of the file in `format`, "RGB" or "BGR" (a reversed view of the RGB array, as in the reference)."""
    if format not in ("RGB", "BGR"):
        raise ValueError(f"read_image: format {format!r} (\"RGB\" or \"BGR\")")
    with open(path, "rb") as f:
        image = _apply_exif_orientation(Image.open(f)).convert("RGB")
        a = np.asarray(image)
    return a[:, :, ::-1] if format == "BGR" else a


_logged = set()


def decoded_runs(paths, device, batch_bytes=256 << 20):
    """decode="gpu" for the mappers: the files as runs of consecutive frames of one size, uint8 [n, H, W, 3] RGB device tensors
    (jpeg_ops.decode_runs); the first file the host had to read is logged once."""
    from .. import jpeg_ops
    datas = []
    for path in paths:
        with open(path, "rb") as f:
            datas.append(f.read())

    def fell_back(k, reason):
        if "jpeg-fallback" not in _logged:
            _logged.add("jpeg-fallback")
            logging.getLogger("univs_amd").warning("%s is not decoded by the HIP JPEG decoder (%s): reading it on the host with Pillow "
                                                   "(logged once)", paths[k], reason)
    return jpeg_ops.decode_runs(datas, device, lambda k: read_image(paths[k], "RGB"), batch_bytes=batch_bytes, on_fallback=fell_back)


def read_images(paths, decode="host", device=None, format="RGB"):
    """One image per file: with decode="host" the host arrays of `read_image` (today's path, untouched), with decode="gpu" uint8
    [H, W, 3] device tensors with the same bytes, decoded by csrc/jpeg_decode.hip where it covers the file and by `read_image` +
    upload where it does not."""
    if decode not in ("host", "gpu"):
        raise ValueError(f"read_images: decode={decode!r} (\"host\" or \"gpu\")")
    if format not in ("RGB", "BGR"):
        raise ValueError(f"read_images: format {format!r} (\"RGB\" or \"BGR\")")
    if decode == "host":
        return [read_image(path, format) for path in paths]
    import torch
    device = torch.device("cuda" if device is None else device)
    frames = [frame for run in decoded_runs(list(paths), device) for frame in run]
    return [f.flip(2) for f in frames] if format == "BGR" else frames
