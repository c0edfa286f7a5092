"""GPU: csrc/png_deflate.hip gives the zlib streams of univs_amd/inference/png_rule.py byte for byte, on the frames of tests/png_cases.py
with one and three frames per call, uint8 and int32 ids, with and without a look-up table; and the four writers of
inference/results.py with png="gpu" write the files of png="host" as far as Pillow's decoder can tell: the same paths, arrays, modes
and palettes, the same VPS record, the same evaluator results."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import png_cases
from univs_amd import png_ops
from univs_amd.inference import png_rule, results

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _stack(px, N):
    """N frames of one shape from one case: the frame, its rows reversed, its columns rolled by one pixel."""
    return np.stack([px, px[::-1], np.roll(px, 1, axis=1)][:N])


@functools.lru_cache(maxsize=None)
def _rule_streams(name):
    px = dict(png_cases.cases())[name]
    return tuple(png_rule.zlib_stream(f) for f in _stack(px, 3))


def _ids_lut(stack):
    N, H, W, C = stack.shape
    ids, lut = png_cases.ids_and_lut(stack.reshape(N * H, W, C))
    return ids.reshape(N, H, W), lut


GROUPS = sorted({n.split("-")[0] + "-c" + n[-1] for n, _ in png_cases.cases()})


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("N", [1, 3])
def test_streams_equal_the_rule_byte_for_byte(group, N):
    pattern, c = group.split("-c")
    for name, px in png_cases.cases():
        if not (name.startswith(pattern + "-") and name.endswith("x" + c)):
            continue
        stack = _stack(px, N)
        want = list(_rule_streams(name)[:N])
        ids, lut = _ids_lut(stack)
        got = png_ops.deflate_maps(torch.from_numpy(ids).to(DEV), torch.from_numpy(lut).to(DEV), channels=px.shape[2])
        assert got == want, name
        # the other id type (when the colours fit a byte both exist), and the identity without a table
        if ids.dtype == np.uint8:
            got = png_ops.deflate_maps(torch.from_numpy(ids.astype(np.int32)).to(DEV), torch.from_numpy(lut).to(DEV), channels=px.shape[2])
            assert got == want, name + " int32"
        if px.shape[2] == 1:
            got = png_ops.deflate_maps(torch.from_numpy(np.ascontiguousarray(stack[..., 0])).to(DEV))
            assert got == want, name + " identity"


def test_offsets_are_the_cumulative_lengths_and_streams_inflate():
    import zlib
    px = dict(png_cases.cases())["blocks7-33x517x3"]
    stack = _stack(px, 3)
    ids, lut = _ids_lut(stack)
    got = png_ops.deflate_maps(torch.from_numpy(ids).to(DEV), torch.from_numpy(lut).to(DEV), channels=3)
    assert [len(g) for g in got] == [len(s) for s in _rule_streams("blocks7-33x517x3")]
    for g, f in zip(got, stack):
        assert zlib.decompress(g) == png_rule.filtered_rows(f).tobytes()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_ids_outside_the_table_are_clamped(C, dtype):
    K = 5
    lut = (np.arange(K * C).reshape(K, C) * 17 + 3).astype(np.uint8)
    rng = np.random.default_rng(7)
    ids = np.repeat(rng.integers(0, 9, (2, 19, 8)), 6, axis=2).astype(dtype)          # ids 5 .. 8 are >= K
    if dtype == np.int32:
        ids[:, ::3] -= 4                                                                # ... and some below 0
        ids[0, 0, 0], ids[1, 1, 1] = -2 ** 31, 2 ** 31 - 1
    want = png_rule.deflate_maps(ids, lut, C)
    assert png_rule.lut_bytes(ids, lut, C).max() == lut[K - 1].max()
    got = png_ops.deflate_maps(torch.from_numpy(ids).to(DEV), torch.from_numpy(lut).to(DEV), channels=C)
    assert got == want


def test_more_frames_than_threads_and_more_stripes_than_threads():
    """png_frames_kernel sums the frame lengths in pieces of ceil(N / 256) frames per thread, png_place_kernel the sizes before a stripe
    256 at a time: 300 small frames, and one frame of 300 one-row stripes (rows of 12289 bytes: R = 1)."""
    rng = np.random.default_rng(11)
    ids = np.repeat(rng.integers(0, 4, (300, 2, 3)), 2, axis=2).astype(np.uint8)[:, :, :5]
    got = png_ops.deflate_maps(torch.from_numpy(ids).to(DEV))
    assert got == png_rule.deflate_maps(ids) and len(got) == 300
    tall = np.zeros((1, 300, 12288), np.uint8)
    tall[0, np.arange(300), np.arange(300) * 40] = 200
    tall[0, 257:, 9000:9100] = 7
    assert png_rule.stripe_rows(12289) == 1
    assert png_ops.deflate_maps(torch.from_numpy(tall).to(DEV)) == png_rule.deflate_maps(tall)


def test_a_row_beyond_the_stripe_cap_is_not_covered():
    ids = torch.from_numpy(np.ascontiguousarray(png_cases.NOT_COVERED[1][None, ..., 0])).to(DEV)
    assert png_ops.deflate_maps(ids) is None
    assert png_rule.deflate_maps(ids.cpu().numpy()) is None


def test_two_calls_on_one_stream_give_equal_bytes():
    px = dict(png_cases.cases())["long_runs-33x517x1"]
    ids = torch.from_numpy(np.ascontiguousarray(_stack(px, 3)[..., 0])).to(DEV)
    first = png_ops.deflate_maps(ids)
    second = png_ops.deflate_maps(ids)
    assert first == second == list(_rule_streams("long_runs-33x517x1"))


# ---- through the writers: a 3-frame 37 x 53 video ---------------------------------------------------------------------------------------
T, H, W = 3, 37, 53
NAMES = [f"vid0/{i:05d}.jpg" for i in range(T)]


def _idmap(n_ids, seed):
    rng = np.random.default_rng(seed)
    return np.repeat(np.repeat(rng.integers(0, n_ids, (T, 8, 6)), 5, axis=1), 9, axis=2)[:, :H, :W]


def _decoded(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im).copy(), im.mode, im.getpalette()


def _same_files(a, b):
    assert [os.path.relpath(p, a[0]) for p in a[1]] == [os.path.relpath(p, b[0]) for p in b[1]]
    for pa, pb in zip(a[1], b[1]):
        (xa, ma, la), (xb, mb, lb) = _decoded(pa), _decoded(pb)
        assert ma == mb and la == lb and xa.shape == xb.shape and np.array_equal(xa, xb), pa


@pytest.mark.parametrize("palette", [None, "davis"])
def test_write_vos_pngs(tmp_path, palette):
    pal = None if palette is None else [(i * 37 + j * 11) % 256 for i in range(256) for j in range(3)]
    maps = torch.from_numpy(_idmap(6, 0).astype(np.uint8))
    host = results.write_vos_pngs(str(tmp_path / "h"), NAMES, 0, maps, pal)
    gpu = results.write_vos_pngs(str(tmp_path / "g"), NAMES, 0, maps.to(DEV), pal, png="gpu")
    _same_files((str(tmp_path / "h"), host), (str(tmp_path / "g"), gpu))
    assert _decoded(gpu[0])[1] == ("L" if pal is None else "P")


def test_write_rvos_pngs(tmp_path):
    masks = torch.from_numpy(((_idmap(2, 1)[None] + np.arange(2)[:, None, None, None]) % 2 * 255).astype(np.uint8))
    res = {"ids": [3, 11], "masks": masks}
    host = results.write_rvos_pngs(str(tmp_path / "h"), NAMES, 0, res)
    gpu = results.write_rvos_pngs(str(tmp_path / "g"), NAMES, 0, {"ids": [3, 11], "masks": masks.to(DEV)}, png="gpu")
    _same_files((str(tmp_path / "h"), host), (str(tmp_path / "g"), gpu))


CATEGORIES = {c: {"id": c, "isthing": int(c % 2), "color": [(c * 40) % 256, (c * 70 + 20) % 256, (c * 110 + 5) % 256]} for c in range(1, 6)}


def _vps_video():
    pan = _idmap(7, 2).astype(np.int64)                                                # id 0: no segment
    infos = [{"id": i, "isthing": bool(CATEGORIES[1 + i % 5]["isthing"]), "category_id": 1 + i % 5} for i in (3, 1, 6, 2, 9)]
    inputs = {"file_names": NAMES, "frame_indices": list(range(T)), "video_id": "vid0"}
    return inputs, {"image_size": (H, W), "pred_masks": torch.from_numpy(pan), "segments_infos": infos}


def _files_under(root):
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.endswith(".png"))


def test_write_vps_predictions(tmp_path):
    inputs, outputs = _vps_video()
    np.random.seed(5)
    host = results.write_vps_predictions(inputs, outputs, str(tmp_path / "h"), CATEGORIES)
    np.random.seed(5)
    outputs_dev = dict(outputs, pred_masks=outputs["pred_masks"].to(DEV))
    gpu = results.write_vps_predictions(inputs, outputs_dev, str(tmp_path / "g"), CATEGORIES, png="gpu")
    assert gpu == host
    _same_files((str(tmp_path / "h"), _files_under(tmp_path / "h")), (str(tmp_path / "g"), _files_under(tmp_path / "g")))
    assert len(_files_under(tmp_path / "g")) == T and _decoded(_files_under(tmp_path / "g")[0])[1] == "RGB"


def _vss_video():
    sem = _idmap(5, 3).astype(np.int64)
    sem[:, :4, :7] = 255
    inputs = {"file_names": NAMES, "frame_indices": list(range(T)), "video_id": "vid0"}
    return inputs, {"image_size": (H, W), "pred_masks": torch.from_numpy(sem)}, {i: 3 + 2 * i for i in range(5)}


def test_write_vss_predictions(tmp_path):
    inputs, outputs, mapping = _vss_video()
    host = results.write_vss_predictions(inputs, outputs, str(tmp_path / "h"), mapping)
    gpu = results.write_vss_predictions(inputs, dict(outputs, pred_masks=outputs["pred_masks"].to(DEV)), str(tmp_path / "g"), mapping, png="gpu")
    _same_files((str(tmp_path / "h"), host), (str(tmp_path / "g"), gpu))
    assert _decoded(gpu[0])[0].max() == 255 and _decoded(gpu[0])[1] == "L"


def _equal(a, b):
    """Equality of the evaluators' results: dictionaries and lists of numbers, strings and arrays."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, (np.ndarray, torch.Tensor)) or isinstance(b, (np.ndarray, torch.Tensor)):
        return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def _vps_evaluator(root, png):
    from tests import vps_eval_cases as VC
    from univs_amd.evaluation import vps
    fx = VC.load("clean")
    _, truth, gt_file = VC.write_tree(fx, os.path.join(root, "tree"))
    out_dir = os.path.join(root, "out")
    ev = vps.VPSEvaluator(VC.metadata_categories(fx), gt_file, truth, out_dir, device=DEV, png=png)
    ev.reset()
    np.random.seed(0)
    for video in fx["gt_json"]["videos"]:
        inputs, outputs = VC.vps_outputs(fx, video["video_id"], DEV)
        ev.process([inputs], outputs)
    score = ev.evaluate()
    # ... and once more from the files that were written, which the evaluator itself did not read
    files = vps.evaluate_vps_files(out_dir, truth, gt_file, device=DEV, output_dir=os.path.join(root, "again"))
    return score, files, ev._predictions


def test_the_vps_evaluator_returns_the_same_results_either_way(tmp_path):
    host, gpu = _vps_evaluator(str(tmp_path / "h"), "host"), _vps_evaluator(str(tmp_path / "g"), "gpu")
    assert gpu[2] == host[2] and len(host[2]) > 0
    assert _equal(gpu[0], host[0]) and _equal(gpu[1], host[1]) and gpu[1]["files"] == host[1]["files"] == host[0]["files"]
    _same_files((str(tmp_path / "h"), _files_under(tmp_path / "h" / "out")), (str(tmp_path / "g"), _files_under(tmp_path / "g" / "out")))


def _vss_evaluator(root, png, name):
    from tests import vss_eval_cases as SC
    from univs_amd.evaluation import vss
    fx = SC.load(name)
    submit, data = SC.write_tree(fx, os.path.join(root, "tree"), predictions=False)
    ev = vss.VSSEvaluator(SC.CONTIGUOUS_TO_DATASET, 255, SC.NUM_CLASSES, data, fx["split_file"], submit, device=DEV, png=png)
    ev.reset()
    for v in fx["videos"]:
        inputs, outputs = SC.vss_outputs(fx, v, DEV)
        ev.process([inputs], outputs)
    score = ev.evaluate()
    files = vss.evaluate_vss_files(submit, data, fx["split_file"], device=DEV, output_dir=os.path.join(root, "again"))
    return score, files, submit


def test_the_vss_evaluator_returns_the_same_results_either_way(tmp_path):
    from tests import vss_eval_cases as SC
    name = SC.EVALUATOR_SCORED[0]
    host, gpu = _vss_evaluator(str(tmp_path / "h"), "host", name), _vss_evaluator(str(tmp_path / "g"), "gpu", name)
    assert _equal(gpu[0], host[0]) and _equal(gpu[1], host[1]) and gpu[1]["files"] == host[1]["files"] == host[0]["files"]
    _same_files((str(tmp_path / "h"), _files_under(host[2])), (str(tmp_path / "g"), _files_under(gpu[2])))
