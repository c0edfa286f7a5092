"""CPU: the overlay rule (univs_amd/inference/overlay_rule.py) on hand-worked pixels, its table helpers, `idmap_from_instances`, and the
host writer of `results.write_overlay_jpegs`."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import overlay_cases as oc
from univs_amd.data import jpeg_encode_rule
from univs_amd.inference import overlay_rule as ov
from univs_amd.inference.results import write_overlay_jpegs

LUT = np.array([[9, 9, 9, 0], [200, 100, 0, 255], [0, 0, 255, 128]], np.uint8)


def test_alpha_0_255_and_128_by_hand():
    frame = np.full((1, 3, 3), (100, 50, 201), np.uint8)
    out = ov.overlay_rule(frame, np.array([[0, 1, 2]]), LUT, edge=None)
    assert out[0, 0].tolist() == [100, 50, 201]                      # alpha 0: the frame's pixel
    assert out[0, 1].tolist() == [200, 100, 0]                       # alpha 255: the table's colour
    # alpha 128: (100 127 + 0 128 + 127) // 255 = 50, (50 127 + 0 + 127) // 255 = 25, (201 127 + 255 128 + 127) // 255 = 228
    assert out[0, 2].tolist() == [50, 25, 228]
    assert out.dtype == np.uint8 and out.shape == frame.shape


def test_ids_are_clamped_on_both_sides():
    frame = np.full((1, 4, 3), 60, np.uint8)
    out = ov.overlay_rule(frame, np.array([[-5, 0, 2, 77]]), LUT, edge=None)
    assert out[0, 0].tolist() == out[0, 1].tolist() == [60, 60, 60] and out[0, 2].tolist() == out[0, 3].tolist()
    assert np.array_equal(ov.overlay_rule(frame, np.array([[-5, 0, 2, 77]], np.int32), LUT), ov.overlay_rule(frame, np.array([[0, 0, 2, 2]], np.uint8), LUT))


def test_edges_need_a_differing_neighbour_inside_the_image():
    frame = np.full((4, 5, 3), 10, np.uint8)
    edge = (255, 255, 240)
    full = ov.overlay_rule(frame, np.ones((4, 5), np.int64), LUT, edge)
    assert (full == np.array([200, 100, 0])).all()                   # an object that fills the image: leaving the image is no edge
    ids = np.zeros((4, 5), np.int64)
    ids[1, 2] = 1                                                    # a one-pixel object: the pixel itself is the contour; the background (alpha 0) is not
    out = ov.overlay_rule(frame, ids, LUT, edge)
    assert out[1, 2].tolist() == list(edge) and (np.delete(out.reshape(-1, 3), 7, axis=0) == 10).all()
    ids = np.array([[1, 1, 2, 2]] * 3)                               # two objects side by side: both columns at the border between them
    out = ov.overlay_rule(np.full((3, 4, 3), 10, np.uint8), ids, LUT, edge)
    assert (out[:, 1:3] == np.array(edge)).all() and (out[:, 0] == np.array([200, 100, 0])).all() and (out[:, 3] == np.array([5, 5, 133])).all()
    diag = np.array([[1, 0], [0, 1]])                                # diagonal neighbours do not count, but each 1 has a 0 beside it
    assert (ov.overlay_rule(np.full((2, 2, 3), 10, np.uint8), diag, LUT, edge)[diag == 1] == np.array(edge)).all()
    none = ov.overlay_rule(np.full((3, 4, 3), 10, np.uint8), ids, LUT, edge=None)
    assert (none[:, :2] == np.array([200, 100, 0])).all() and (none[:, 2:] == np.array([5, 5, 133])).all()
    # ids that clamp to the same row are one object
    assert not (ov.overlay_rule(np.full((1, 2, 3), 10, np.uint8), np.array([[2, 9]]), LUT, edge) == np.array(edge)).all(-1).any()


def test_arguments_are_checked():
    frame = np.zeros((2, 2, 3), np.uint8)
    for bad in (lambda: ov.overlay_rule(frame, np.zeros((2, 3), int), LUT), lambda: ov.overlay_rule(frame, np.zeros((2, 2)), LUT),
                lambda: ov.overlay_rule(frame.astype(np.int16), np.zeros((2, 2), int), LUT), lambda: ov.overlay_rule(frame, np.zeros((2, 2), int), LUT[:, :3]),
                lambda: ov.overlay_rule(frame, np.zeros((2, 2), int), LUT, edge=(1, 2)), lambda: ov.overlay_rule(frame, np.zeros((2, 2), int), LUT, edge=(1, 2, 256))):
        with pytest.raises(ValueError):
            bad()


def test_table_helpers():
    lut = ov.lut_from_palette([0, 0, 0, 128, 0, 0, 0, 128, 0])
    assert lut.tolist() == [[0, 0, 0, 0], [128, 0, 0, 128], [0, 128, 0, 128]] and lut.dtype == np.uint8
    assert ov.lut_from_palette(np.arange(6, dtype=np.uint8), alpha=200).tolist() == [[0, 1, 2, 0], [3, 4, 5, 200]]
    assert ov.default_palette(4).tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0]]      # the DAVIS palette
    cats = {7: {"id": 7, "color": [1, 2, 3], "isthing": 1}, 3: {"id": 3, "color": (9, 8, 7), "isthing": 0}}
    lut, order = ov.lut_from_categories(cats)
    assert lut.tolist() == [[0, 0, 0, 0], [9, 8, 7, 204], [1, 2, 3, 204]] and order == [None, 3, 7]
    assert ov.lut_from_categories(cats, ov.ALPHA_VSS)[0][1:, 3].tolist() == [153, 153]
    assert (ov.ALPHA_VOS, ov.ALPHA_VPS, ov.ALPHA_VSS, ov.OFF_WHITE) == (128, round(0.8 * 255), round(0.6 * 255), (255, 255, 240))


def test_idmap_from_instances_ties_and_threshold():
    masks = torch.zeros((4, 1, 2, 3), dtype=torch.bool)
    masks[0, 0, :, 0:2] = True
    masks[1, 0, :, 1:3] = True
    masks[2, 0, 0, :] = True
    masks[3, 0] = True
    ids = ov.idmap_from_instances(masks, torch.tensor([0.5, 0.9, 0.5, 0.01]))
    # instance 1 (0.9) wins where it covers; 0 and 2 tie at 0.5 in (0, 0): the lower index; instance 3, below the threshold, is not drawn
    assert ids.tolist() == [[[1, 2, 2], [1, 2, 2]]] and ids.dtype == torch.int32
    assert ov.idmap_from_instances(masks, torch.tensor([0.5, 0.9, 0.5, 0.01]), score_thresh=0.0)[0, 1, 2] == 2
    only3 = ov.idmap_from_instances(masks, torch.tensor([0.0, 0.0, 0.0, 0.02]))
    assert (only3 == 4).all()                                        # the threshold keeps a score equal to it
    assert not ov.idmap_from_instances(masks, torch.zeros(4)).any()
    assert ov.idmap_from_instances(masks[2:3], torch.tensor([0.3])).tolist() == [[[1, 1, 1], [0, 0, 0]]]
    with pytest.raises(ValueError):
        ov.idmap_from_instances(masks, torch.zeros(3))


def test_the_host_writer(tmp_path):
    frames, ids = oc.scene(40, 48, T=2)
    names = [f"/data/clip7/{i:05d}.png" for i in range(5)]
    paths = write_overlay_jpegs(str(tmp_path), names, 3, list(frames), torch.from_numpy(ids), oc.LUT, quality=75, sampling="422")
    assert [os.path.relpath(p, tmp_path) for p in paths] == ["inference/Overlays/clip7/00003.jpg", "inference/Overlays/clip7/00004.jpg"]
    for p, f, m in zip(paths, frames, ids):
        data = open(p, "rb").read()
        assert data == jpeg_encode_rule.encode_rule(ov.overlay_rule(f, m, oc.LUT), 75, "422")
        with Image.open(io.BytesIO(data)) as im:
            assert im.size == (48, 40)
    assert write_overlay_jpegs(str(tmp_path), names, 0, [], np.zeros((0, 4, 4), int), oc.LUT) == []
    with pytest.raises(ValueError, match="frames against"):
        write_overlay_jpegs(str(tmp_path), names, 0, list(frames), ids[:1], oc.LUT)


def test_visualize_defaults_to_off():
    from univs_amd import run
    base = ["--config-file", "c", "--weights", "w", "--video-dir", "d", "--output-dir", "o"]
    assert run.parse_args(base).visualize == "off" and run.parse_args(base + ["--visualize", "gpu"]).visualize == "gpu"
    with pytest.raises(SystemExit):
        run.parse_args(base + ["--visualize", "device"])
