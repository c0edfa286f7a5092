"""GPU: the four file scorers with reader="gpu" return what they return with reader="host" -- the same dictionaries and the same
result-file texts -- on one small scene each, written by Pillow; the host readers are disabled meanwhile, so the planes can only have
come from csrc/png_inflate.hip.  One scene is scored again with its predictions re-written by the device encoder (png="gpu")."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import davis_eval_cases, pvos_eval_cases, vps_eval_cases, vss_eval_cases
from univs_amd import png_ops
from univs_amd.evaluation import _counts, davis, pvos, vps, vss

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _texts(directory):
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(directory, "*.txt")))}


@pytest.fixture
def no_host_reader(monkeypatch):
    """The Pillow loops of the four scorers raise: what is scored inside this fixture was decoded on the device."""
    def refuse(*a, **k):
        raise AssertionError("the host reader was called")
    monkeypatch.setattr(vps, "_read_rgb", refuse)
    monkeypatch.setattr(vss, "_read", refuse)
    monkeypatch.setattr(davis, "_read", refuse)
    monkeypatch.setattr(pvos, "_read_u8", refuse)
    return monkeypatch


def test_vps(tmp_path, no_host_reader):
    fx = vps_eval_cases.load("short")
    submit, truth, gt_file = vps_eval_cases.write_tree(fx, str(tmp_path))
    g = vps.evaluate_vps_files(submit, truth, gt_file, device=DEV, output_dir=str(tmp_path / "g"), reader="gpu")
    no_host_reader.undo()
    h = vps.evaluate_vps_files(submit, truth, gt_file, device=DEV, output_dir=str(tmp_path / "h"))
    assert g["files"] == h["files"] and repr(g["vpq"]) == repr(h["vpq"]) and repr(g["stq"]) == repr(h["stq"])
    assert _texts(tmp_path / "g") == _texts(tmp_path / "h") and len(_texts(tmp_path / "g")) == len(h["files"])
    vps_eval_cases.check_score(fx, g)


def test_vss(tmp_path, no_host_reader):
    fx = vss_eval_cases.load("short")
    submit, data = vss_eval_cases.write_tree(fx, str(tmp_path))
    g = vss.evaluate_vss_files(submit, data, fx["split_file"], device=DEV, output_dir=str(tmp_path / "g"), reader="gpu")
    no_host_reader.undo()
    h = vss.evaluate_vss_files(submit, data, fx["split_file"], device=DEV, output_dir=str(tmp_path / "h"))
    assert g["files"] == h["files"] and _texts(tmp_path / "g") == _texts(tmp_path / "h") and len(g["files"]) == 3
    vss_eval_cases.check_score(fx, g)


def test_davis(tmp_path, no_host_reader):
    for name in ("semi_clean", "unsup_clean"):
        fx = davis_eval_cases.load(name)
        root, res = davis_eval_cases.write_tree(fx, str(tmp_path / name))
        kw = dict(resolution=fx["resolution"], metrics=fx["metrics"], device=DEV)
        g = davis.evaluate_davis_files(root, res, fx["task"], output_dir=str(tmp_path / name / "g"), reader="gpu", **kw)
        no_host_reader.undo()
        h = davis.evaluate_davis_files(root, res, fx["task"], output_dir=str(tmp_path / name / "h"), **kw)
        assert repr(g) == repr(h) and _texts(tmp_path / name / "g") == _texts(tmp_path / name / "h")
        davis_eval_cases.check_result(fx, g)
        no_host_reader.setattr(davis, "_read", lambda *a: (_ for _ in ()).throw(AssertionError("the host reader was called")))


def test_pvos_and_again_with_predictions_written_by_the_device(tmp_path, no_host_reader):
    fx = pvos_eval_cases.load("clean")
    data, res = pvos_eval_cases.write_tree(fx, str(tmp_path))
    dg, dh = {}, {}
    g = pvos.evaluate_pvos_files(res, data, eval_decay=True, device=DEV, details=dg, reader="gpu")
    # the same results, compressed by csrc/png_deflate.hip this time: other files, the same maps
    from PIL import Image
    for video in sorted(os.listdir(res)):
        paths = sorted(glob.glob(os.path.join(res, video, "*.png")))
        maps = np.stack([np.array(Image.open(p)) for p in paths])
        files = png_ops.png_files(png_ops.deflate_maps(torch.from_numpy(maps).to(DEV)), maps.shape[1], maps.shape[2], 1, list(range(256)) * 3)
        for p, f in zip(paths, files):
            with open(p, "wb") as fh:
                fh.write(f)
    g2 = pvos.evaluate_pvos_files(res, data, eval_decay=True, device=DEV, reader="gpu")
    no_host_reader.undo()
    h = pvos.evaluate_pvos_files(res, data, eval_decay=True, device=DEV, details=dh)
    assert repr(g) == repr(h) == repr(g2) and pvos.scores_text(g) == pvos.scores_text(h) and repr(dg) == repr(dh)
    pvos_eval_cases.check_result(fx, g, dg)


def test_an_irregular_video_goes_through_the_host_loop_and_raises_what_it_raises(tmp_path):
    fx = pvos_eval_cases.load("err_size_mismatch")
    data, res = pvos_eval_cases.write_tree(fx, str(tmp_path))
    with pytest.raises(ValueError) as eg:
        pvos.evaluate_pvos_files(res, data, eval_decay=True, device=DEV, reader="gpu")
    with pytest.raises(ValueError) as eh:
        pvos.evaluate_pvos_files(res, data, eval_decay=True, device=DEV)
    assert str(eg.value) == str(eh.value)
    before = len(_counts.HOST_FALLBACKS)
    missing = os.path.join(str(tmp_path), "missing.png")
    assert _counts.device_stack([missing], "gpu", DEV) is None
    assert len(_counts.HOST_FALLBACKS) == before + 1 and _counts.HOST_FALLBACKS[-1][0] == missing      # the hand-over leaves a sign


def test_the_evaluators_read_their_ground_truth_on_the_device_during_process(tmp_path, no_host_reader):
    """`VPSEvaluator.process` and `VSSEvaluator.process` count a video at once from the tensor they are handed and the ground-truth files:
    with reader="gpu" those files are decoded on the device, and the scores are the ones of reader="host"."""
    fx = vps_eval_cases.load("short")
    scores = {}
    for reader in ("gpu", "host"):
        if reader == "host":
            no_host_reader.undo()
        root = str(tmp_path / ("vps_" + reader))
        _, truth, gt_file = vps_eval_cases.write_tree(fx, os.path.join(root, "tree"))
        ev = vps.VPSEvaluator(vps_eval_cases.metadata_categories(fx), gt_file, truth, os.path.join(root, "out"), device=DEV, reader=reader)
        ev.reset()
        np.random.seed(0)
        for video in fx["gt_json"]["videos"]:
            inputs, outputs = vps_eval_cases.vps_outputs(fx, video["video_id"], DEV)
            ev.process([inputs], outputs)
        assert len(ev._tables) == len(fx["gt_json"]["videos"])       # every video was counted in process
        scores[reader] = ev.evaluate()
    assert scores["gpu"]["files"] == scores["host"]["files"]
    no_host_reader.setattr(vss, "_read", lambda *a: (_ for _ in ()).throw(AssertionError("the host reader was called")))
    fx = vss_eval_cases.load("short")
    scores = {}
    for reader in ("gpu", "host"):
        if reader == "host":
            no_host_reader.undo()
        root = str(tmp_path / ("vss_" + reader))
        submit, data = vss_eval_cases.write_tree(fx, os.path.join(root, "tree"), predictions=False)
        ev = vss.VSSEvaluator(vss_eval_cases.CONTIGUOUS_TO_DATASET, 255, vss_eval_cases.NUM_CLASSES, data, fx["split_file"], submit, device=DEV,
                              reader=reader)
        ev.reset()
        for v in fx["videos"]:
            inputs, outputs = vss_eval_cases.vss_outputs(fx, v, DEV)
            ev.process([inputs], outputs)
        assert len(ev._counts) == len(fx["videos"])
        scores[reader] = ev.evaluate()
    assert scores["gpu"]["files"] == scores["host"]["files"]
