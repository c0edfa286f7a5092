"""`read_image` of detectron2's detection_utils (the reference's copy: univs/data/detection_utils.py:60-187), restated because
detectron2 is absent: open with PIL, apply the EXIF orientation, convert to RGB, reverse the channels for "BGR"."""
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
