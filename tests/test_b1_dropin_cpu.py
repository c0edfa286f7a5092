"""Boundary B1: what the REFERENCE's callers above the module boundary do with this repository's modules
(`backbone`, `sem_seg_head`) -- the "drops in unchanged" claim of the north star, against the reference's own outputs:

  * the long-video split call (univs/univs_prompt_longvideo.py:397-406: `pixel_decoder.forward_features(features)` ->
    `predictor(multi_scale_features, mask_features, mask_features_bfe_conv, targets=...)`) and the attributes it reads
    (:562-571: `predictor.pe_layer`, `.input_proj[i]`, `.level_embed.weight`, `.forward_prompt_encoder`), against the
    reference's modules on the same inputs (goldens g3, g6 and g22, oracle/gen_golden.py);
  * `MaskFormer_Video`'s call (mask2former_video/video_maskformer_model.py:208-209: `sem_seg_head(features)`).

The reference's clip loop (`InferenceVideoEntity.inference_video`) over these modules is pinned by golden g11a
(tests/test_clip_loop_cpu.py).  The four HIP operators are replaced by the oracle's CPU stand-ins (oracle/cpu_path.py), as in
every CPU module test."""
import os

import numpy as np
import pytest
import torch

from oracle.cpu_path import cpu_ops
from tests import cases, helpers


def test_long_video_split_call_and_attributes(golden_dir):
    """univs_prompt_longvideo.py:397-406, :562-571 against the reference's modules on the same inputs: its forward_features
    (golden g3), its split call's outputs (g6: the reference's head runs forward_features -> predictor) and its attributes (g22)."""
    g3 = np.load(os.path.join(golden_dir, "g3_pixel_decoder.npz"))
    g6 = np.load(os.path.join(golden_dir, "g6_head_first_clip.npz"))
    g = np.load(os.path.join(golden_dir, "g22_long_video_split.npz"))
    case = cases.HEAD_CASE
    feats = cases.backbone_features(case)
    ours = helpers.build_head(case, "cpu", return_aux=False)
    with cpu_ops(), torch.no_grad():
        t_o = ours.pixel_decoder.forward_features(feats)
        assert len(t_o) == 4 and len(t_o[3]) == int(g["n_ms"])
        for a, k in zip(t_o[:3], ("mask_features", "mask_features_bfe_conv", "enc0")):
            assert (a - torch.from_numpy(g3[k])).abs().max().item() < 1e-4, k
        for i, a in enumerate(t_o[3]):
            assert (a - torch.from_numpy(g3[f"ms{i}"])).abs().max().item() < 1e-4, i
        mask_features, mask_features_bfe_conv, multi_scale = t_o[0], t_o[1], t_o[-1]
        out_o = ours.predictor(multi_scale, mask_features, mask_features_bfe_conv, targets=cases.targets_first_clip(case))
        whole = ours(feats, targets=cases.targets_first_clip(case))
    for k in ("pred_logits", "pred_masks", "pred_embds"):
        assert (out_o[k] - torch.from_numpy(g6[k])).abs().max().item() < 1e-3, k
        assert torch.equal(out_o[k], whole[k]), k           # the split call IS the head's forward
    # the attributes the long-video model reads directly, on the reference's own maps
    p_o = ours.predictor
    ms_r = [torch.from_numpy(g3[f"ms{i}"]) for i in range(int(g["n_ms"]))]
    x = ms_r[0]
    with torch.no_grad():
        pos_o = p_o.pe_layer(x.view(1, case["T"], -1, *x.shape[-2:]), None)
        assert (pos_o - torch.from_numpy(g["pe_ms0"])).abs().max().item() < 1e-5
        for i in range(3):
            want = torch.from_numpy(g[f"input_proj{i}"]) if f"input_proj{i}" in g.files else ms_r[i]
            assert torch.equal(p_o.input_proj[i](ms_r[i]), want), i
    assert torch.equal(p_o.level_embed.weight.detach(), torch.from_numpy(g["level_embed"]))
    assert callable(p_o.forward_prompt_encoder) and ours.num_classes == int(g["num_classes"])


def test_maskformer_video_is_registered_and_calls_the_head_without_targets():
    """video_maskformer_model.py:208-209: `features = self.backbone(images.tensor); outputs = self.sem_seg_head(features)`."""
    import univs_amd.modeling.meta_arch.univs_prompt  # noqa: F401  (registers the META_ARCH classes, as build_model does)
    from univs_amd.registry import META_ARCH_REGISTRY
    assert "MaskFormer_Video" in META_ARCH_REGISTRY
    from univs_amd.modeling.meta_arch.univs_prompt import MaskFormer_Video
    case = cases.HEAD_CASE
    head = helpers.build_head(case, "cpu", return_aux=False)
    with cpu_ops(), torch.no_grad(), pytest.raises(ValueError):
        head(cases.backbone_features(case))          # no targets and no opt-in: raises, as the reference's decoder does
    calls = []

    class Backbone(torch.nn.Module):
        size_divisibility = 32

        def forward(self, x):
            calls.append(tuple(x.shape))
            return cases.backbone_features(case)
    m = MaskFormer_Video(backbone=Backbone(), sem_seg_head=head, num_frames=case["T"], size_divisibility=32,
                         pixel_mean=(123.675, 116.28, 103.53), pixel_std=(58.395, 57.12, 57.375)).eval()
    frames = [torch.zeros(3, case["H"], case["W"]) for _ in range(case["T"])]
    with cpu_ops(), torch.no_grad():
        out = m([{"image": frames, "height": case["H"], "width": case["W"]}])
    assert calls == [(case["T"], 3, case["H"], case["W"])]
    assert set(out) >= {"pred_logits", "pred_masks"} and out["pred_masks"].shape[2] == case["T"]
