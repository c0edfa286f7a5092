"""CPU: the tenth header of the C ABI (include/univs_png_hip.h): its symbol is exported and bound, the binding read from it is the
recorded one (tests/png_capi_signatures.txt), its entry answers invalid and uncovered arguments before any launch, the wrapper refuses
CPU tensors with the standard sentence; the four writers keep writing the parent's files byte for byte by default, and the host-side
half of their png="gpu" branch (tables, paths, records, chunks) gives files that decode to the same pixels when the rule stands in for
the kernel."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, ops, png_ops
from univs_amd.inference import png_rule, results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "univs_png_deflate_maps"
COVERED = "not covered (C in {1, 3}, rows_per_stripe (W C + 1) <= 24576, N H (W C + 1) < 2^31)"
POINTERS = ("src", "scratch", "out", "offsets")


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_png_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbol_is_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == [NAME] == sorted(_lib.PNG_SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_png_hip.h but not exported"
        res, args = _lib.PNG_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signature_is_the_recorded_one_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "png_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.PNG_SIGNATURES) == recorded == [NAME + " I PIIIIPIIIPPPP"]
    others = (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FUSED_SIGNATURES) | set(_lib.PVOS_SIGNATURES) |
              set(_lib.SEMANTIC_SIGNATURES) | set(_lib.ENCODER_SIGNATURES) | set(_lib.SWIN_SIGNATURES) | set(_lib.FRAMES_SIGNATURES) |
              set(_lib.PROMPTS_SIGNATURES))
    assert not set(_lib.PNG_SIGNATURES) & others
    assert (len(_lib.SIGNATURES), len(_lib.FRAMES_SIGNATURES), len(_lib.PROMPTS_SIGNATURES)) == (76, 1, 1)
    assert "png_deflate.hip" in build.SOURCES and any(h.endswith("univs_png_hip.h") for h in build.HEADERS)


def _call(lib, p, i32, N, H, W, lut, K, C, R, null=()):
    a = {k: (None if k in null else p) for k in POINTERS}
    return getattr(lib, NAME)(a["src"], i32, N, H, W, p if lut else None, K, C, R, a["scratch"], a["out"], a["offsets"], None)


@pytest.fixture
def host():
    """A host buffer's address: never read, the entry answers before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


# (src_is_i32, N, H, W, lut given, K, C, rows_per_stripe)
@pytest.mark.parametrize("args", [(0, -1, 4, 4, 1, 2, 1, 16), (0, 1, 0, 4, 1, 2, 1, 16), (0, 1, 4, -2, 1, 2, 1, 16), (0, 1, 4, 4, 1, 0, 1, 16),
                                  (0, 1, 4, 4, 1, 2, 0, 16), (0, 1, 4, 4, 1, 2, 1, 0), (1, 1, 4, 4, 0, 1, 1, 16), (0, 1, 4, 4, 0, 1, 3, 16),
                                  (0, 0, 4, 4, 1, 2, -1, 16)])
def test_bad_sizes_are_invalid_arguments(host, args):
    lib = _lib.load()
    assert _call(lib, host, *args) == _lib.ERR_INVALID_ARGUMENT
    i32, N, H, W, lut, K, C, R = args
    assert lib.univs_last_error().decode() == (f"{NAME}: bad arguments src_is_i32={i32} N={N} H={H} W={W} lut={'given' if lut else 'NULL'} "
                                               f"K={K} C={C} rows_per_stripe={R}")


@pytest.mark.parametrize("null", POINTERS)
def test_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _call(lib, host, 0, 1, 4, 4, 1, 2, 1, 16, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": NULL data pointer"


@pytest.mark.parametrize("args", [
    (0, 1, 4, 4, 1, 2, 2, 16),                      # two channels
    (0, 1, 4, 4, 1, 2, 4, 16),
    (0, 1, 1, 24576, 0, 1, 1, 1),                   # a row one byte over the stripe cap
    (0, 1, 4, 8192, 1, 2, 3, 1),
    (0, 1, 4, 1280, 0, 1, 1, 20),                   # a stripe of 20 rows of 1281 bytes is beyond the LDS plan
    (0, 70000, 3000, 10, 0, 1, 1, 16),              # 2.3e9 filtered bytes
    (1, 2, 50000, 24000, 1, 2, 1, 1),
])
def test_beyond_its_bounds_the_entry_answers_not_implemented_before_any_launch(host, args):
    lib = _lib.load()
    assert _call(lib, host, *args) == _lib.ERR_NOT_IMPLEMENTED, args
    assert lib.univs_last_error().decode() == f"{NAME}: {COVERED}"


def test_no_frames_is_success_without_a_launch():
    lib = _lib.load()
    assert _call(lib, None, 0, 0, 4, 4, 0, 1, 1, 16) == _lib.OK      # (NULL pointers: nothing is read)


def test_wrapper_refuses_cpu_tensors_with_the_standard_sentence():
    ids = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError) as e:
        png_ops.deflate_maps(ids)
    assert str(e.value) == str(ops._cpu_refusal("deflate_maps", "tensor on cpu"))
    assert "Not implemented on the CPU" in str(e.value)
    assert not hasattr(ops, "deflate_maps")                          # (ops.py's public set is pinned: the wrapper lives beside it)
    with pytest.raises(ValueError):
        results.write_vos_pngs("unused", ["v/0.jpg"], 0, ids, png="device")


# ---- the writers ------------------------------------------------------------------------------------------------------------------------
T, H, W = 3, 37, 53
NAMES = [f"vid0/{i:05d}.jpg" for i in range(T)]
PALETTE = [(i * 37 + j * 11) % 256 for i in range(256) for j in range(3)]
CATEGORIES = {c: {"id": c, "isthing": int(c % 2), "color": [(c * 40) % 256, (c * 70 + 20) % 256, (c * 110 + 5) % 256]} for c in range(1, 6)}


def _idmap(n_ids, seed):
    rng = np.random.default_rng(seed)
    return np.repeat(np.repeat(rng.integers(0, n_ids, (T, 8, 6)), 5, axis=1), 9, axis=2)[:, :H, :W]


def _pillow(plane, palette=None):
    """The parent's way to a file: `Image.fromarray`, `putpalette`, `save`."""
    from PIL import Image
    img = Image.fromarray(plane)
    if palette is not None:
        img.putpalette(palette)
    buf = io.BytesIO()
    img.save(buf, format="PNG")
    return buf.getvalue()


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _vps_video():
    pan = _idmap(7, 2).astype(np.int64)                              # id 0: no segment; 3 is listed twice, 9 has no pixel
    infos = [{"id": i, "isthing": bool(CATEGORIES[1 + i % 5]["isthing"]), "category_id": 1 + i % 5} for i in (3, 1, 6, 2, 9, 3)]
    inputs = {"file_names": NAMES, "frame_indices": list(range(T)), "video_id": "vid0"}
    return inputs, {"image_size": (H, W), "pred_masks": torch.from_numpy(pan), "segments_infos": infos}


def _vss_video():
    sem = _idmap(5, 3).astype(np.int64)
    sem[:, :4, :7] = 255
    inputs = {"file_names": NAMES, "frame_indices": list(range(T)), "video_id": "vid0"}
    return inputs, {"image_size": (H, W), "pred_masks": torch.from_numpy(sem)}, {i: 3 + 2 * i for i in range(5)}


def test_the_default_writers_write_the_parents_files_byte_for_byte(tmp_path):
    maps = _idmap(6, 0).astype(np.uint8)
    for pal in (None, PALETTE):
        paths = results.write_vos_pngs(str(tmp_path / f"vos{pal is None}"), NAMES, 0, torch.from_numpy(maps), pal)
        assert [_read(p) for p in paths] == [_pillow(m, pal) for m in maps]
        assert paths == results.write_vos_pngs(str(tmp_path / f"vos{pal is None}"), NAMES, 0, torch.from_numpy(maps), pal, png="host")
    masks = ((_idmap(2, 1)[None] + np.arange(2)[:, None, None, None]) % 2 * 255).astype(np.uint8)
    paths = results.write_rvos_pngs(str(tmp_path / "rvos"), NAMES, 0, {"ids": [3, 11], "masks": torch.from_numpy(masks)})
    assert [_read(p) for p in paths] == [_pillow(m) for m in masks.reshape(-1, H, W)]
    inputs, outputs = _vps_video()
    np.random.seed(5)
    record = results.write_vps_predictions(inputs, outputs, str(tmp_path / "vps"), CATEGORIES)
    np.random.seed(5)
    gen = results.IdGenerator(CATEGORIES)
    pan, rgb = outputs["pred_masks"].numpy(), np.zeros((T, H, W, 3), np.uint8)
    for info in outputs["segments_infos"]:
        rgb[pan == info["id"]] = gen.get_color(info["category_id"])
    assert [_read(os.path.join(str(tmp_path / "vps"), "pan_pred", "vid0", a["file_name"].replace(".jpg", ".png"))) for a in
            record["annotations"]] == [_pillow(f) for f in rgb]
    inputs, outputs, mapping = _vss_video()
    paths = results.write_vss_predictions(inputs, outputs, str(tmp_path / "vss"), mapping)
    sem = outputs["pred_masks"].numpy()
    want = np.where(sem == 255, 255, 2 * sem).astype(np.uint8)      # (3 + 2 c) - 3
    assert [_read(p) for p in paths] == [_pillow(f) for f in want]


@pytest.fixture
def rule_for_kernel(monkeypatch):
    """png="gpu" without a GPU: the maps stay where they are and the rule computes the streams the kernel would."""
    monkeypatch.setattr(results, "_on_device", lambda maps, dtype: (maps if isinstance(maps, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(maps))).to(dtype).contiguous())
    monkeypatch.setattr(png_ops, "deflate_maps", lambda src, lut=None, channels=1: png_rule.deflate_maps(
        src.numpy(), None if lut is None else lut.numpy(), channels))


def _decoded(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im).copy(), im.mode, im.getpalette()


def _same_files(root_a, a, root_b, b):
    assert [os.path.relpath(p, root_a) for p in a] == [os.path.relpath(p, root_b) for p in b] and len(a) > 0
    for pa, pb in zip(a, b):
        (xa, ma, la), (xb, mb, lb) = _decoded(pa), _decoded(pb)
        assert ma == mb and la == lb and xa.shape == xb.shape and np.array_equal(xa, xb), pa


def _files_under(root):
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.endswith(".png"))


def test_the_gpu_branch_of_the_writers_around_the_rule(tmp_path, rule_for_kernel):
    h, g = str(tmp_path / "h"), str(tmp_path / "g")
    maps = torch.from_numpy(_idmap(6, 0).astype(np.uint8))
    for pal in (None, PALETTE):
        _same_files(h, results.write_vos_pngs(h, NAMES, 0, maps, pal), g, results.write_vos_pngs(g, NAMES, 0, maps.numpy(), pal, png="gpu"))
    masks = torch.from_numpy(((_idmap(2, 1)[None] + np.arange(2)[:, None, None, None]) % 2 * 255).astype(np.uint8))
    res = {"ids": [3, 11], "masks": masks}
    _same_files(h, results.write_rvos_pngs(h, NAMES, 0, res), g, results.write_rvos_pngs(g, NAMES, 0, res, png="gpu"))
    inputs, outputs = _vps_video()
    np.random.seed(5)
    host = results.write_vps_predictions(inputs, outputs, h, CATEGORIES)
    np.random.seed(5)
    assert results.write_vps_predictions(inputs, outputs, g, CATEGORIES, png="gpu") == host
    _same_files(h, _files_under(os.path.join(h, "pan_pred")), g, _files_under(os.path.join(g, "pan_pred")))
    inputs, outputs, mapping = _vss_video()
    _same_files(h, results.write_vss_predictions(inputs, outputs, h, mapping), g,
                results.write_vss_predictions(inputs, outputs, g, mapping, png="gpu"))
    with pytest.raises(KeyError):                                    # a predicted class without a dataset id: the host's error
        results.write_vss_predictions(inputs, outputs, g, {0: 3}, png="gpu")


def test_where_the_kernel_does_not_cover_the_size_the_frames_go_through_pillow(tmp_path, rule_for_kernel):
    wide = np.zeros((1, 2, png_rule.STRIPE_BYTES), np.uint8)
    wide[0, 1, 5:900] = 3
    names = ["v/0.jpg"]
    host = results.write_vos_pngs(str(tmp_path / "h"), names, 0, torch.from_numpy(wide), PALETTE)
    gpu = results.write_vos_pngs(str(tmp_path / "g"), names, 0, torch.from_numpy(wide), PALETTE, png="gpu")
    assert _read(gpu[0]) == _read(host[0])


def test_the_command_line_takes_png_and_the_evaluators_pass_it_on(tmp_path):
    from univs_amd import run
    from univs_amd.evaluation.vps import VPSEvaluator
    from univs_amd.evaluation.vss import VSSEvaluator
    base = ["--config-file", "c", "--weights", "w", "--video-dir", "d", "--output-dir", "o"]
    assert run.parse_args(base).png == "host" and run.parse_args(base + ["--png", "gpu"]).png == "gpu"
    with pytest.raises(SystemExit):
        run.parse_args(base + ["--png", "zlib"])
    assert VPSEvaluator({}, "gt.json", "truth", str(tmp_path / "vps")).png == "host"
    assert VPSEvaluator({}, "gt.json", "truth", str(tmp_path / "vps"), png="gpu").png == "gpu"
    assert VSSEvaluator({0: 1}, 255, 124, "data", "val.txt", str(tmp_path / "vss")).png == "host"
    assert VSSEvaluator({0: 1}, 255, 124, "data", "val.txt", str(tmp_path / "vss"), png="gpu").png == "gpu"
