"""GPU: the overlay path of the device JPEG encoder (csrc/jpeg_encode.hip with ids and lut) against `encode_rule(overlay_rule(...))`, the
two writers of `results.write_overlay_jpegs` against each other, and `python -m univs_amd.run --visualize gpu` end to end."""
import json
import os

import numpy as np
import pytest
import torch

from tests import overlay_cases as oc
from univs_amd import jpegenc_ops
from univs_amd.data import jpeg_encode_rule as rule
from univs_amd.inference import overlay_rule as ov
from univs_amd.inference.results import write_overlay_jpegs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes():
    """{size: (frames, ids)}, computed once and left unchanged."""
    return {size: oc.scene(*size) for size in oc.SIZES}


@pytest.mark.parametrize("size", oc.SIZES)
@pytest.mark.parametrize("dtype", (torch.int32, torch.uint8, torch.int64))
@pytest.mark.parametrize("edge", ((255, 255, 240), None))
def test_the_fused_entry_is_the_overlay_rule_then_the_encoder_rule(cuda, scenes, size, dtype, edge):
    frames, ids = scenes[size]
    ids_t = torch.from_numpy(ids)
    if dtype == torch.uint8:                                         # (bytes hold no negative id: those pixels become 249, beyond the table)
        ids_t = ids_t.to(torch.uint8)
    want_ids = ids_t.numpy()
    assert (want_ids >= len(oc.LUT)).any() and ((want_ids < 0).any() or dtype == torch.uint8)
    for sampling, quality in (("420", 90), ("444", 100), ("422", 30)):
        got = jpegenc_ops.encode_jpegs(torch.from_numpy(frames).to(cuda), quality, sampling, ids=ids_t.to(cuda, dtype), lut=oc.LUT, edge=edge)
        want = [rule.encode_rule(ov.overlay_rule(f, m, oc.LUT, edge), quality, sampling) for f, m in zip(frames, want_ids)]
        assert got == want, (size, dtype, edge, sampling, [a == b for a, b in zip(got, want)])
    plain = jpegenc_ops.encode_jpegs(torch.from_numpy(frames).to(cuda), 90, "420")
    assert plain != jpegenc_ops.encode_jpegs(torch.from_numpy(frames).to(cuda), 90, "420", ids=ids_t.to(cuda, dtype), lut=oc.LUT, edge=edge)


def test_a_transparent_table_leaves_the_frames_files(cuda, scenes):
    frames, ids = scenes[oc.SIZES[0]]
    lut = oc.LUT.copy()
    lut[:, 3] = 0
    rgb = torch.from_numpy(frames).to(cuda)
    assert jpegenc_ops.encode_jpegs(rgb, 90, "420", ids=torch.from_numpy(ids).to(cuda), lut=lut) == jpegenc_ops.encode_jpegs(rgb, 90, "420")
    with pytest.raises(ValueError, match="go together"):
        jpegenc_ops.encode_jpegs(rgb, 90, "420", ids=torch.from_numpy(ids).to(cuda))
    with pytest.raises(ValueError, match="integer"):
        jpegenc_ops.encode_jpegs(rgb, 90, "420", ids=torch.from_numpy(ids).to(cuda).float(), lut=lut)


def test_the_two_writers_give_the_same_files(cuda, scenes, tmp_path):
    frames, ids = scenes[oc.SIZES[1]]
    names = [f"/data/clip7/{i:05d}.png" for i in range(2 + len(frames))]
    host = write_overlay_jpegs(str(tmp_path / "host"), names, 2, list(frames), ids, oc.LUT, jpeg="host")
    gpu = write_overlay_jpegs(str(tmp_path / "gpu"), names, 2, torch.from_numpy(frames).to(cuda), torch.from_numpy(ids).to(cuda), oc.LUT, jpeg="gpu")
    assert [os.path.relpath(p, tmp_path / "host") for p in host] == [os.path.relpath(p, tmp_path / "gpu") for p in gpu] == \
        [f"inference/Overlays/clip7/{i:05d}.jpg" for i in range(2, 2 + len(frames))]
    for a, b, f, m in zip(host, gpu, frames, ids):
        data = open(a, "rb").read()
        assert data == open(b, "rb").read() == rule.encode_rule(ov.overlay_rule(f, m, oc.LUT), 90, "420")
    # host frames and ids are uploaded by the gpu writer; other settings reach both
    again = write_overlay_jpegs(str(tmp_path / "gpu2"), names, 2, list(frames), ids, oc.LUT, edge=None, quality=75, sampling="444", jpeg="gpu")
    host2 = write_overlay_jpegs(str(tmp_path / "host2"), names, 2, list(frames), ids, oc.LUT, edge=None, quality=75, sampling="444", jpeg="host")
    assert [open(p, "rb").read() for p in again] == [open(p, "rb").read() for p in host2]
    with pytest.raises(ValueError, match="jpeg="):
        write_overlay_jpegs(str(tmp_path), names, 0, list(frames), ids, oc.LUT, jpeg="device")


def test_run_with_visualize_gpu_writes_the_tree(cuda, tmp_path, capsys):
    from univs_amd import run
    os.makedirs(tmp_path / "videos")
    oc.write_videos(str(tmp_path / "videos"))
    cfg, weights = oc.write_model(str(tmp_path), "vss")
    base = ["--config-file", cfg, "--weights", weights, "--video-dir", str(tmp_path / "videos"), "--device", "cuda"]
    assert run.main(base + ["--output-dir", str(tmp_path / "gpu"), "--visualize", "gpu", "--decode", "gpu"]) == 0
    assert run.main(base + ["--output-dir", str(tmp_path / "off")]) == 0
    host_args = run.parse_args(base + ["--output-dir", str(tmp_path / "host"), "--visualize", "host"])
    for v in range(2):
        # the host writer on the output the run saved: numpy and Pillow on the files' own pixels
        names = [str(tmp_path / "videos" / f"video{v}" / f"{i:05d}.jpg") for i in range(5)]
        saved = torch.load(tmp_path / "gpu" / f"video{v}.pt")
        assert len(run.write_overlays(host_args, [{"file_names": names, "video_id": f"video{v}"}], saved)) == 5
        folder = tmp_path / "gpu" / "inference" / "Overlays" / f"video{v}"
        assert sorted(os.listdir(folder)) == [f"{i:05d}.jpg" for i in range(5)] + ["legend.json"]
        legend = json.loads((folder / "legend.json").read_text())
        assert legend and all(set(e) == {"name", "color", "alpha"} and e["alpha"] == ov.ALPHA_VSS for e in legend.values())
        for name in os.listdir(folder):                              # the same model, the same frames: the host writer's files
            assert (folder / name).read_bytes() == (tmp_path / "host" / "inference" / "Overlays" / f"video{v}" / name).read_bytes()
        assert os.path.exists(tmp_path / "gpu" / f"video{v}.pt")
    assert not os.path.exists(tmp_path / "off" / "inference")         # the default writes what it wrote before
    # an instance result comes merged into run-length codes: one line, nothing written
    cfg, weights = oc.write_model(str(tmp_path), "vis")
    capsys.readouterr()
    assert run.main(["--config-file", cfg, "--weights", weights, "--video-dir", str(tmp_path / "videos"), "--device", "cuda", "--output-dir",
                     str(tmp_path / "vis"), "--visualize", "gpu"]) == 0
    assert capsys.readouterr().out.count("nothing written") == 2 and not os.path.exists(tmp_path / "vis" / "inference")
