"""CPU: the semantic-extraction driver (univs_amd/inference/video_semantic_extraction.py) -- its ATen path against the reference's own
results (golden g25_semantic_*, tools/gen_golden_semantic.py: tokens, features, head calls, file names), the saved files, the config
keys and a reference-style yaml, the `UniVS_Prompt` dispatch with the switch on and off, a small model end to end on the oracle's CPU
operators, and the argument checks of the op and of its C entry (no device touched)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle.cpu_path import cpu_ops
from tests import cases
from tests.test_minvis_cpu import video_input
from univs_amd import _lib, ops, synth
from univs_amd.config import get_cfg, load_cfg
from univs_amd.inference.video_semantic_extraction import AtenSteps, InferenceVideoSemanticExtraction
from univs_amd.modeling.build import build_model
from univs_amd.workloads import SemanticClipHead

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ["g25_semantic_r8", "g25_semantic_r32_720p", "g25_semantic_t3", "g25_semantic_default_size"]


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    d = {k: g[k] for k in g.files}
    for k in ("recipe", "names", "calls"):
        d[k] = json.loads(bytes(d[k]).decode())
    return d, d["recipe"]


def driver(r, out_dir, device="cpu", fused=True):
    return InferenceVideoSemanticExtraction(
        hidden_dim=r["C"], num_queries=r["N"], overlap_threshold=0.0, overlap_threshold_entity=0.5, stability_score_thresh=0.0,
        size_divisibility=32, LSJ_aug_image_size=1024, LSJ_aug_enable_test=False, sem_seg_postprocess_before_inference=False,
        pixel_mean=[0.0] * 3, pixel_std=[1.0] * 3, num_frames=r["T"], num_classes=1, semantic_extraction_compression_ratio=r["ratio"],
        semantic_extraction_compression_ratio_temporal=r["t_itv"], semantic_extraction_output_dir="" if r["default_dir"] else out_dir,
        fused=fused).to(device)


def stand_ins(r, root, device="cpu"):
    head = SemanticClipHead(r["seed"], r["C"], r["N"], r["h"], r["w"])
    model = type("M", (), {})()
    model.backbone = lambda x: {"res2": x}
    model.head = head
    model.sem_seg_head = lambda f, targets=None: {k: v.to(device) for k, v in head(f, targets).items()}
    images = type("I", (), {})()
    images.tensor = torch.zeros(r["V"], 1, *r["padded"], device=device)
    images.image_sizes = [tuple(r["crop"])] * r["V"]
    inputs = [{"video_id": r["video_id"], "video_len": r["V"]}]
    if r["out"] is not None:
        inputs[0].update(height=r["out"][0], width=r["out"][1])
    targets = [{"file_names": [f"{root}/raw/set1/{r['video_id']}/{i:05d}.jpg" for i in range(r["V"])]}]
    return model, inputs, images, targets


def run_driver(r, root, device="cpu", fused=True):
    """The driver's `inference_video` into `root` -> (head calls, directory written, file names, the two loaded tensors)."""
    out_dir = os.path.join(str(root), "out")
    d = driver(r, out_dir, device, fused)
    model, inputs, images, targets = stand_ins(r, str(root), device)
    with torch.no_grad():
        assert d.inference_video(model, inputs, images, targets) is None           # as the reference
    where = out_dir if not r["default_dir"] else f"{root}/raw/set1".replace("raw", "semantic_extraction")
    names = sorted(os.listdir(where))
    loaded = [torch.load(os.path.join(where, n), map_location=None) for n in names]
    return model.head.calls, names, loaded


def check_against_golden(g, calls, names, loaded, feature_bound=None):
    assert names == g["names"] and len(names) == 2
    assert [[c[0], c[1], c[2]] for c in calls] == g["calls"]
    feats, toks = loaded                                                           # '._compression...' sorts before '._obj_tokens...'
    for t in loaded:
        assert t.device.type == "cpu" and t.dtype == torch.float32 and t.is_contiguous()
    ref_t, ref_f = torch.from_numpy(g["obj_tokens"]), torch.from_numpy(g["features"])
    assert toks.shape == ref_t.shape and torch.equal(toks, ref_t)
    assert feats.shape == ref_f.shape
    if feature_bound is None:
        assert torch.equal(feats, ref_f)
    else:
        err = float((feats - ref_f).abs().max())
        bound = feature_bound * max(1.0, float(ref_f.abs().max()))
        print(f"features max |diff| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (err, bound)


@pytest.mark.parametrize("name", NAMES)
def test_driver_cpu_matches_reference(name, tmp_path):
    """The same ATen CPU kernels and the same expressions as the reference: tokens and features bit for bit."""
    g, r = load_golden(name)
    check_against_golden(g, *run_driver(r, tmp_path))


def test_goldens_cover_what_they_claim():
    recipes = {n: load_golden(n)[1] for n in NAMES}
    gs = {n: load_golden(n)[0] for n in NAMES}
    assert any(r["V"] % r["T"] for r in recipes.values())                                          # a shorter last clip
    assert any(r["V"] > 2 * r["T"] for r in recipes.values())                                      # more than one backbone window
    assert any(c[1][0] % recipes[n]["t_itv"] for n in NAMES for c in gs[n]["calls"]
               if any(f % recipes[n]["t_itv"] == 0 for f in c[1]))                                 # a kept frame that is not its clip's first
    assert any(r["crop"][0] < r["padded"][0] and r["crop"][1] < r["padded"][1] for r in recipes.values())
    outs = [r for r in recipes.values() if r["out"] is not None]
    assert any(r["out"][0] > r["crop"][0] for r in outs) and any(r["out"][0] < r["crop"][0] for r in outs)
    assert any(r["out"][0] % r["ratio"] for r in outs)                                             # int(out / ratio) truncates
    assert any(r["ratio"] == 32 and tuple(r["out"]) == (720, 1280) for r in outs)
    assert any(g["features"].shape[-1] % 4 for g in gs.values())
    assert gs["g25_semantic_r32_720p"]["features"].shape == (2, 8, 22, 40)
    assert all(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < 100_000 for n in NAMES)


def test_extract_allocates_the_video_tensor_once_and_returns_device_tensors():
    g, r = load_golden("g25_semantic_t3")
    d = driver(r, "unused")
    model, inputs, images, targets = stand_ins(r, "root")
    toks, feats = d.extract(model, inputs, images, targets)
    assert torch.equal(toks, torch.from_numpy(g["obj_tokens"])) and torch.equal(feats, torch.from_numpy(g["features"]))
    assert feats.is_contiguous() and feats.shape[0] == -(-r["V"] // r["t_itv"])
    inputs[0]["video_len"] = r["V"] + 1
    with pytest.raises(AssertionError):
        d.extract(model, inputs, images, targets)


def test_output_directory_and_file_name_rules(tmp_path):
    r = load_golden("g25_semantic_r8")[1]
    d = driver(dict(r, default_dir=True), "")
    names = ["datasets/internvid/raw/InternVId-FLT_1/clip.mp4/00000.jpg"]
    assert d.output_dir(names) == "datasets/internvid/semantic_extraction/InternVId-FLT_1"
    d.semantic_extraction_output_dir = None
    assert d.output_dir(names) == "datasets/internvid/semantic_extraction/InternVId-FLT_1"
    d.semantic_extraction_output_dir = str(tmp_path / "a" / "b")
    assert d.output_dir(names) == str(tmp_path / "a" / "b")
    assert d.file_names("v") == ("v._obj_tokens_8_1.pt", "v._compression_mask_features_8_1.pt")
    for _ in range(2):                                                              # makedirs(exist_ok=True): a second video, same place
        paths = d.save("v", names, torch.zeros(4, 3, 2)[::2], torch.ones(2, 3, 2, 2))
    assert [os.path.basename(p) for p in paths] == list(d.file_names("v")) and all(os.path.exists(p) for p in paths)
    assert torch.load(paths[0]).shape == (2, 3, 2)
    with pytest.raises(NotImplementedError, match="frame sharding"):
        d.set_frame_shard(object())


# ---- config and dispatch ------------------------------------------------------------------------------------------------------------
def test_config_keys_defaults_and_reference_style_yaml(tmp_path):
    se = get_cfg().MODEL.UniVS.TEST.SEMANTIC_EXTRACTION
    assert se.ENABLE is False and se.COMPRESSION_RATIO == 32 and se.COMPRESSION_RATIO_TEMPORAL == 1 and se.OUTPUT_DIR == ""
    y = tmp_path / "semantic.yaml"
    y.write_text("MODEL:\n  UniVS:\n    TEST:\n      SEMANTIC_EXTRACTION:\n        ENABLE: True\n        COMPRESSION_RATIO: 8\n"
                 "        COMPRESSION_RATIO_TEMPORAL: 2\n        OUTPUT_DIR: 'output/semantic'\n")
    cfg = load_cfg(str(y))
    se = cfg.MODEL.UniVS.TEST.SEMANTIC_EXTRACTION
    assert se.ENABLE is True and se.COMPRESSION_RATIO == 8 and se.COMPRESSION_RATIO_TEMPORAL == 2 and se.OUTPUT_DIR == "output/semantic"
    d = InferenceVideoSemanticExtraction(cfg)
    assert d.semantic_extraction_compression_ratio == 8 and d.semantic_extraction_compression_ratio_temporal == 2
    assert d.semantic_extraction_output_dir == "output/semantic" and d.semantic_extraction_enable is True
    assert d.num_frames == cfg.INPUT.SAMPLING_FRAME_NUM and d.num_frames_window_test == 2 * d.num_frames and d.fused


def small_model(enable, out_dir="", ratio=8, t_itv=1):
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE = "UniVS_Prompt"
    cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES = 20
    cfg.MODEL.UniVS.CLIP_CLASS_EMBED_PATH = cases.clip_table()
    cfg.MODEL.UniVS.TEST.VIDEO_UNIFIED_INFERENCE_ENABLE = False
    cfg.INPUT.SAMPLING_FRAME_NUM = 2
    cfg.INPUT.LSJ_AUG.IMAGE_SIZE = 128
    se = cfg.MODEL.UniVS.TEST.SEMANTIC_EXTRACTION
    se.ENABLE, se.COMPRESSION_RATIO, se.COMPRESSION_RATIO_TEMPORAL, se.OUTPUT_DIR = enable, ratio, t_itv, out_dir
    return build_model(cfg).eval()


def test_dispatch_checks_the_switch_first_and_is_unchanged_when_off():
    on = small_model(True)
    assert on.semantic_extraction_enable is True and isinstance(on.inference_video_semantic_extraction, InferenceVideoSemanticExtraction)
    seen = []
    on.inference_video_semantic_extraction.eval = lambda m, b: seen.append(b[0]["dataset_name"])
    for name in ("ovis", "coco_panoptic", "vipseg"):                                # whatever the dataset or task: the switch comes first
        assert on(video_input(name)) is None
    assert on(video_input("ovis", task="grounding")) is None
    assert seen == ["ovis", "coco_panoptic", "vipseg", "ovis"]
    off = small_model(False)
    assert off.semantic_extraction_enable is False
    off.inference_video_semantic_extraction.eval = lambda m, b: seen.append("wrong")
    off.inference_video_vis_fast.eval = lambda m, b: {"vis": 1}
    assert off(video_input("ovis")) == {"vis": 1} and "wrong" not in seen
    from univs_amd.modeling.meta_arch.univs_prompt import UniVS_Prompt
    bare = UniVS_Prompt(backbone=on.backbone, sem_seg_head=on.sem_seg_head, prepare_targets=on.prepare_targets, text_prompt_encoder=None,
                        inference_video_entity=on.inference_video_entity, inference_video_vos=on.inference_video_vos,
                        pixel_mean=[0, 0, 0], pixel_std=[1, 1, 1], video_unified_inference_enable=False, custom_videos_enable=False,
                        custom_videos_text=[], semantic_extraction_enable=True).eval()
    with pytest.raises(NotImplementedError, match="inference_video_semantic_extraction"):
        bare(video_input("ovis"))


def test_small_model_end_to_end_writes_the_two_files(tmp_path):
    model = small_model(True, str(tmp_path / "sem"), ratio=8, t_itv=2)
    synth.load_synthetic(model)
    with cpu_ops():
        assert model(video_input("ovis", n=3, video_id="v0")) is None
    assert sorted(os.listdir(tmp_path / "sem")) == ["v0._compression_mask_features_8_2.pt", "v0._obj_tokens_8_2.pt"]
    toks = torch.load(tmp_path / "sem" / "v0._obj_tokens_8_2.pt")
    feats = torch.load(tmp_path / "sem" / "v0._compression_mask_features_8_2.pt")
    assert tuple(toks.shape) == (2, 256, 20) and tuple(feats.shape) == (2, 256, 8, 12)              # frames 0 and 2 of 3; 64 x 96 / 8
    assert toks.dtype == feats.dtype == torch.float32 and torch.isfinite(toks).all() and torch.isfinite(feats).all()


# ---- the op and its C entry without a device --------------------------------------------------------------------------------------------
def test_op_refuses_cpu_tensors_and_autograd():
    x = torch.zeros(2, 3, 4, 6)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.bilinear_crop_nearest(x, (16, 24), (15, 22), (3, 5))
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.bilinear_crop_nearest(x.requires_grad_(), (16, 24), (15, 22), (3, 5))


def test_aten_steps_are_the_three_reference_expressions():
    import torch.nn.functional as F
    x = torch.randn(5, 3, 6, 9, generator=torch.Generator().manual_seed(0))
    out = torch.full((2, 3, 4, 7), 9.0)
    AtenSteps((24, 36), (22, 33), (4, 7)).compress(x, 1, 2, out)
    U = F.interpolate(x, size=(24, 36), mode="bilinear", align_corners=False)[..., :22, :33]
    assert torch.equal(out, F.interpolate(U, size=(4, 7), mode="nearest")[1::2][:2])


def test_c_entry_validates_its_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.univs_bilinear_crop_nearest_f32
    good = dict(T=5, C=4, h=8, w=12, Hp=32, Wp=48, Hi=30, Wi=45, hc=3, wc=5, t_first=0, t_step=1, K=5)

    def call(**over):
        a = dict(good, **over)
        return fn(None, a["T"], a["C"], a["h"], a["w"], a["Hp"], a["Wp"], a["Hi"], a["Wi"], a["hc"], a["wc"], a["t_first"], a["t_step"], a["K"],
                  None, None)

    assert call(K=0) == _lib.OK and call(K=-3) == _lib.OK                                            # nothing to do, nothing launched
    bad = [dict(Hi=33), dict(Wi=49), dict(h=0), dict(w=-1), dict(C=0), dict(T=0), dict(Hp=0), dict(hc=0), dict(wc=0), dict(t_step=0),
           dict(t_first=-1), dict(t_first=1), dict(t_step=2, K=4), dict(t_first=4, K=2)]
    for over in bad:
        assert call(**over) == _lib.ERR_INVALID_ARGUMENT, over
        assert b"univs_bilinear_crop_nearest_f32" in lib.univs_last_error(), over
    assert call(t_step=2, K=3) == _lib.ERR_INVALID_ARGUMENT and b"NULL" in lib.univs_last_error()   # valid frames 0, 2, 4: next check
    assert call(Hi=33, K=0) == _lib.ERR_INVALID_ARGUMENT                                            # the geometry is checked first
