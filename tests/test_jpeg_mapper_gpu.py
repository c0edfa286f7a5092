"""GPU: the test mappers with decode="gpu" (the frames decoded by csrc/jpeg_decode.hip and handed to the device resize) against
decode="host", resize="gpu": the dictionaries are equal tensor for tensor."""
import os

import pytest
import torch

from tests import jpeg_cases as cases
from univs_amd.data import VideoTestMapper, video_records_from_dir

pytestmark = pytest.mark.gpu


def _folder(root, video, files):
    os.makedirs(os.path.join(root, video))
    for i, data in enumerate(files):
        with open(os.path.join(root, video, f"{i:05d}.jpg"), "wb") as f:
            f.write(data)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k in ("image", "image_padding_mask"):
            assert len(a[k]) == len(b[k])
            for x, y in zip(a[k], b[k]):
                assert x.device == y.device and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("fmt", ["RGB", "BGR"])
def test_a_folder_of_frames_and_a_mixed_folder(cuda, tmp_path, fmt):
    _folder(str(tmp_path), "a_frames", cases.frames(5, 75, 131))
    mixed = [cases.encode(cases.content("smooth", 40, 48, 77), "420", 90), cases.uncovered_files()["progressive"],
             cases.encode(cases.content("noise", 40, 48, 78), "420", 75)]
    _folder(str(tmp_path), "b_mixed", mixed)
    records = video_records_from_dir(str(tmp_path))
    assert [r["length"] for r in records] == [5, 3]
    host = VideoTestMapper(60, 100, fmt, resize="gpu", device=cuda)
    gpu = VideoTestMapper(60, 100, fmt, resize="gpu", device=cuda, decode="gpu")
    for r in records:
        a, b = host(r), gpu(r)
        assert all(im.device == cuda and im.dtype == torch.uint8 and im.shape[0] == 3 for im in b["image"])
        _same(a, b)


def test_decode_gpu_needs_resize_gpu():
    with pytest.raises(ValueError, match="needs resize=\"gpu\""):
        VideoTestMapper(60, 100, decode="gpu", resize="host")
    with pytest.raises(ValueError, match="needs resize=\"gpu\""):
        VideoTestMapper(60, 100, decode="gpu")
