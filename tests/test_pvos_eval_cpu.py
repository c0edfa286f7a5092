"""CPU: the ATen formulation of the panoptic-VOS counts and the host arithmetic on them against what the reference recorded (g30
fixtures, tools/gen_golden_pvos_eval.py): the operator counts exactly, the returned dictionary bit for bit with its NaNs, the per-object
values in append order, pvos-ious.txt byte for byte, the error types.  Nothing here reads the reference."""
import os

import numpy as np
import pytest
import torch

from tests import pvos_eval_cases as C
from univs_amd.evaluation import pvos
from univs_amd.evaluation import pvos_counts as pc


def test_operator_counts_equal_the_reference_exactly():
    fx = C.load("operators")
    counts = C.operator_counts(fx, pc.pvos_counts_aten, "cpu")
    C.check_operators(fx, counts)
    full = counts[29]                                                 # 2 d + 1 = 59 rows of the 64: a window rarely stays inside
    assert int(full[..., 3:].sum()) > 0 and (counts[1][..., 4] < counts[1][..., 1]).any()
    for a, b in zip(C.DS[:-1], C.DS[1:]):                             # more erosions leave no fewer boundary pixels; areas do not move
        assert (counts[a][..., 3:] <= counts[b][..., 3:]).all() and torch.equal(counts[a][..., :3], counts[b][..., :3])


def _mask_to_boundary(mask, d):
    """`mask_to_boundary` (a one-pixel zero border, d erosions by 3 x 3 whose own border never erodes) restated with numpy and SciPy."""
    import scipy.ndimage
    h, w = mask.shape
    padded = np.pad(mask, 1, constant_values=0)
    eroded = scipy.ndimage.binary_erosion(padded, structure=np.ones((3, 3), np.uint8), iterations=d, border_value=1).astype(np.uint8)
    return mask - eroded[1:h + 1, 1:w + 1]


@pytest.mark.parametrize("T,H,W,d,K", [(1, 5, 7, 1, 3), (2, 33, 50, 2, 5), (2, 20, 24, 15, 4), (1, 61, 47, 7, 9)])
def test_aten_counts_equal_iterated_erosion_on_random_maps(T, H, W, d, K):
    gt, pred = C.maps(T, H, W, K, 7 * H + W + d)
    got = pc.pvos_counts_aten(torch.from_numpy(gt), torch.from_numpy(pred), d, K).numpy()
    ref = np.zeros((T, K, 6), np.int64)
    for t in range(T):
        for k in range(1, K + 1):
            g, p = (gt[t] == k).astype(np.uint8), (pred[t] == k).astype(np.uint8)
            gb, pb = _mask_to_boundary(g, d), _mask_to_boundary(p, d)
            ref[t, k - 1] = ((g & p).sum(), g.sum(), p.sum(), ((gb * pb) > 0).sum(), (gb > 0).sum(), (pb > 0).sum())
    print({n: int(ref[..., i].sum()) for i, n in enumerate(C.CELLS)})
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    assert all(ref[..., i].sum() > 0 for i in (0, 3, 4, 5))


@pytest.mark.parametrize("name", C.SCORED)
def test_scenes_reproduce_dictionary_values_and_text(name, tmp_path, caplog):
    fx, data, res = C.check_scene(name, str(tmp_path), "cpu")
    out = os.path.dirname(res)
    ev = pvos.PVOSEvaluator("viposeg_valid", os.path.join(data, "JPEGImages"), output_dir=out, device="cpu")
    assert ev.data_path == data and ev.eval_decay
    ev.reset()
    ev.process([{}], {})
    with caplog.at_level("INFO", logger=pvos.__name__):
        got = ev.evaluate()
    assert C.same(list(got.values()), fx["values"])
    with open(os.path.join(out, "pvos-ious.txt"), newline="") as f:
        text = f.read()
    assert text == str(fx["text"]) and "\n" not in text
    assert "{}: {:.2f}".format("decay", got["decay"]) in caplog.messages
    assert "{}: {:.2f}".format("overall_iou", got["overall_iou"] * 100) in caplog.messages


@pytest.mark.parametrize("name", C.ERRORS)
def test_error_scenes_raise_the_recorded_type(name, tmp_path):
    C.check_error_scene(name, str(tmp_path), "cpu")


def test_what_the_scenes_pin():
    """The scenes hold what they are named for (so a regenerated fixture cannot quietly stop testing it)."""
    fx = C.load("duplicate_ids")
    ids = [int(x) for m in fx["ann_44_twice"] for x in np.unique(m) if x]
    assert sorted(ids).count(3) == 2 and sorted(ids).count(1) == 2
    assert C.load("fewer_results")["res_seqs"] == ["10_a", "30_c"] and len(C.load("fewer_results")["seqs"]) == 3
    many = C.load("many_objects")
    assert many["decay_k"].tolist() == [8, 16, 24, 32, 40, 48, 56, 64]           # 64 has data and is left out of the fit
    edges = C.load("edges")
    assert edges["gt_52_edges"].max() == 255 and (edges["gt_52_edges"][3] == 1).all() and (edges["pred_52_edges"][3] == 1).all()
    assert "124" in str(C.load("unlisted_class")["obj_class"])
    for name in C.SCORED:
        assert len(C.load(name)["decay_k"]) >= 2, name


def test_an_empty_group_is_nan_and_only_it():
    v = C.load("empty_group")
    nan_keys = [k for k, x in zip(v["keys"].tolist(), v["values"]) if np.isnan(x)]
    assert nan_keys == ["thing_unseen_miou", "thing_unseen_biou", "thing_unseen_iou", "overall_iou"]


def test_class_tuples_equal_the_reference_lists():
    fx = C.load("classes")
    assert fx["thing_seen"].tolist() == list(pvos.THING_SEEN_CLASS) and fx["thing_unseen"].tolist() == list(pvos.THING_UNSEEN_CLASS)
    assert fx["stuff_seen"].tolist() == list(pvos.STUFF_SEEN_CLASS) and fx["stuff_unseen"].tolist() == list(pvos.STUFF_UNSEEN_CLASS)
    assert [str(v) for v in fx["other_machine_videos"]] == list(pvos.OTHER_MACHINE_VIDEOS) and len(pvos.OTHER_MACHINE_VIDEOS) == 23
    assert int(fx["other_machine_class"]) == pvos.OTHER_MACHINE_CLASS == 98
    # the routing order of the reference: 98 by the video's name, then unseen things, unseen stuff, seen things, seen stuff
    assert pvos.group_of(98, "187_WUZUSD4477I") == "stuff_unseen" and pvos.group_of(98, "20_abc") == "stuff_seen"
    assert [pvos.group_of(c, "v") for c in (102, 9, 60, 28, 124)] == ["thing_unseen", "stuff_unseen", "thing_seen", "stuff_seen", None]


def test_special_cases_of_one_object():
    assert pvos.ious_from_counts((0, 5, 0, 0, 5, 0)) == (0., 0.) and pvos.ious_from_counts((0, 0, 5, 0, 0, 5)) == (0., 0.)
    assert pvos.ious_from_counts((0, 0, 0, 0, 0, 0)) == (1., 1.)
    assert pvos.ious_from_counts((2, 4, 6, 1, 3, 2)) == (2 / 8, 1 / 4)
    assert pvos.ious_from_counts((2, 4, 6, 0, 0, 0)) == (2 / 8, 0)    # a boundary union of 0


def test_dilation():
    assert [pc.dilation(*s) for s in ((720, 1280), (1080, 1920), (2160, 3840), (40, 56), (120, 214), (5, 7))] == [29, 44, 88, 1, 5, 1]
    assert pc.dilation(480, 854, ratio=0.008) == 8 and pc.D_MAX >= 44


def test_wrapper_contract():
    z = torch.zeros((2, 8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        pc.pvos_video_counts(z, z, 1, 1)
    with pytest.raises(RuntimeError, match="uint8"):
        pc.pvos_counts_aten(z.int(), z, 1, 1)
    with pytest.raises(RuntimeError, match="same non-empty"):
        pc.pvos_counts_aten(z, z[:, :4], 1, 1)
    with pytest.raises(RuntimeError, match="d 0"):
        pc.pvos_counts_aten(z, z, 0, 1)
    with pytest.raises(RuntimeError, match="K=0"):
        pc.pvos_counts_aten(z, z, 1, 0)
    assert pc.pvos_counts(z, z, 1, 3).shape == (2, 3, 6)              # CPU tensors: the ATen formulation
    assert pc.pvos_counts_aten(z, z, 1, 300).shape == (2, 300, 6)     # ids above 255 cannot occur: their cells stay zero


def test_wrapper_contract_with_the_library_stubbed(monkeypatch):
    """Through `ops._call`, stream last, the zeroed output handed over just before it, None on ERR_NOT_IMPLEMENTED, no launch beyond a
    coverage bound (read from the module's constants) and one exactly at them."""
    from tests.test_eval_counts_contract_cpu import _Stub
    from univs_amd import _lib, ops
    u8 = torch.zeros((2, 4, 6), dtype=torch.uint8)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.setattr(ops, "_stream_ptr", lambda t: "stream")
    lib = _Stub(_lib.OK)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    out = pc.pvos_video_counts(u8, u8, 3, 7)
    assert tuple(out.shape) == (2, 7, 6) and out.dtype == torch.int32 and not out.any()
    ((called, args),) = lib.calls
    assert called == "univs_pvos_counts" and args[-1] == "stream" and args[-2] == out.data_ptr()
    assert [a for a in args if isinstance(a, int) and a < 1 << 32] == [2, 4, 6, 3, 7]                 # T, H, W, d, K
    lib.code = _lib.ERR_NOT_IMPLEMENTED
    assert pc.pvos_video_counts(u8, u8, 3, 7) is None
    lib.code = _lib.ERR_LAUNCH
    with pytest.raises(_lib.UnivsHipError) as e:
        pc.pvos_video_counts(u8, u8, 3, 7)
    assert str(e.value) == "pvos_video_counts failed (code -3): stub"
    lib.code, lib.calls = _lib.OK, []
    assert pc.pvos_video_counts(u8, u8, pc.D_MAX + 1, 7) is None and pc.pvos_video_counts(u8, u8, 3, pc.K_MAX + 1) is None
    assert lib.calls == []
    assert pc.pvos_video_counts(u8, u8, pc.D_MAX, pc.K_MAX) is not None and len(lib.calls) == 1


def test_exports_and_command_line(tmp_path, capsys):
    from univs_amd import evaluation
    assert evaluation.evaluate_pvos_files is pvos.evaluate_pvos_files and evaluation.PVOSEvaluator is pvos.PVOSEvaluator
    assert evaluation.pvos_video_counts is pc.pvos_video_counts and evaluation.pvos_counts_aten is pc.pvos_counts_aten
    assert evaluation.dilation is pc.dilation
    for n in ("PVOSEvaluator", "evaluate_pvos_files", "pvos_video_counts", "pvos_counts_aten", "dilation"):
        assert n in evaluation.__all__
    fx = C.load("clean")
    data, res = C.write_tree(fx, str(tmp_path))
    got = pvos.main(["--res_path", res, "--data_path", data, "--eval_decay", "--device", "cpu"])
    assert C.same(list(got.values()), fx["values"]) and "overall_iou:" in capsys.readouterr().out
    assert "decay" not in pvos.main(["--res_path", res, "--data_path", data, "--device", "cpu"])
