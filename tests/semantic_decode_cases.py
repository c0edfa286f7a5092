"""What tests/test_semantic_decode_cpu.py, tests/test_semantic_decode_gpu.py and tools/gen_golden_semantic_decode.py share: the recipes
of the g31 fixtures turned back into tensors (seeded with numpy's RandomState, so every machine makes the same values), the converter of
a recipe, and the comparison of `convert` with what the reference's `ConvertSemanticFeatureToMask.convert` returned.

A fixture (tests/golden/g31_semantic_decode_<case>.npz) stores the recipe -- seed, sizes, thresholds, scales -- and from the reference:
`indices`, per row `confidence`, `quality` and `counts` (of all N rows), the returned `cls_logits` and `mask_logits`, and the names its
checkpoint rule matched and skipped.  The generator asserts that no counted logit, no quality and no confidence lies within 1e-3 of its
threshold, so indices and counts are compared for equality."""
import json
import os

import numpy as np
import torch

from univs_amd.inference.semantic_to_mask import PREDICTOR_PREFIX, ConvertSemanticFeatureToMask

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a", "b", "c", "d", "e"]
TOL = 1e-3                                                           # the project's parity contract: max |difference| of a logit
JSON_KEYS = ("recipe", "matched", "skipped")
LEVELS = np.array([-2.0, -0.8, -0.3, 0.3, 0.8, 2.0])


def load(case):
    with np.load(os.path.join(GOLDEN, f"g31_semantic_decode_{case}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    for k in JSON_KEYS:
        fx[k] = json.loads(bytes(fx[k]).decode())
    return fx


def checkpoint(r):
    """The seeded state dict of the predictor's heads under the full checkpoint's key prefix, plus one unrelated key and one key of the
    wrong size (`decoder_norm.bias` with C + 1 entries: the rule skips it and the bias keeps its initial zeros)."""
    rs = np.random.RandomState(r["seed"])
    C, E, P = r["C"], r["text_emb_dim"], PREDICTOR_PREFIX

    def t(a):
        return torch.from_numpy(np.asarray(a, dtype=np.float32))
    sd = {"backbone.stem.weight": t(rs.normal(0, 1, (3, 3))),
          P + "decoder_norm.weight": t(1 + 0.1 * rs.normal(0, 1, C)),
          P + "decoder_norm.bias": t(0.1 * rs.normal(0, 1, C + 1))}
    for i in range(3):
        sd[P + f"mask_embed.layers.{i}.weight"] = t(rs.normal(0, 1, (C, C)) * np.sqrt((2.0 if i < 2 else 1.0) / C))
        sd[P + f"mask_embed.layers.{i}.bias"] = t(0.1 * rs.normal(0, 1, C))
    sd[P + "vis2text_projection.weight"] = t(rs.normal(0, 1, (E, C)) / np.sqrt(C))
    sd[P + "vis2text_projection.bias"] = t(0.1 * rs.normal(0, 1, E))
    sd[P + "cls_temp.weight"] = t([[np.log(r["cls_scale"])]])
    return sd


def clip_table(r):
    rs = np.random.RandomState(r["seed"] + 1)
    return torch.from_numpy(rs.normal(0, 1, (r["K"], r["text_emb_dim"])).astype(np.float32))


def inputs(r):
    """(mask_feats [T, C, h, w], obj_tokens [T, C, N]) as the extraction driver saves them: CPU float32.  A row's tokens share a
    component over the frames, so that rows differ in confidence.  The features are one direction in channel space, at one of six
    LEVELS per pixel, plus a little noise: the logits of a (row, frame) pair then gather around six values (as the logits of real masks
    gather around an inside and an outside value), rows differ in quality, and a seed exists for which no logit lies near +-1 -- among
    the 57 200 counted logits of case c a Gaussian cloud always has some that do."""
    rs = np.random.RandomState(r["seed"] + 2)
    T, C, N, h, w = r["T"], r["C"], r["N"], r["h"], r["w"]
    tokens = rs.normal(0, 1, (1, C, N)) + 0.5 * rs.normal(0, 1, (T, C, N))
    level = LEVELS[rs.randint(0, len(LEVELS), (T, 1, h, w))]
    feats = (level * rs.normal(0, 1, (1, C, 1, 1)) + 2e-4 * rs.normal(0, 1, (T, C, h, w))) * r["feat_scale"]
    return torch.from_numpy(feats.astype(np.float32)), torch.from_numpy(tokens.astype(np.float32))


def keywords(r):
    return dict(hidden_dim=r["C"], mask_dim=r["C"], text_emb_dim=r["text_emb_dim"], apply_cls_thres=r["cls_thres"],
                apply_mask_quality_thres=r["quality_thres"], temporal_stride=r["stride"])


def converter(r, device, wrapped=True):
    sd = checkpoint(r)
    return ConvertSemanticFeatureToMask(clip_class_embed_path=clip_table(r), pretrained_ckpt={"model": sd} if wrapped else sd, device=device,
                                        **keywords(r))


def check_against_fixture(conv, fx):
    """`convert` and the scores behind it against the fixture: indices and counts equal, quality bit-equal, logits within TOL; returns
    what convert returned."""
    r = fx["recipe"]
    feats, tokens = inputs(r)
    cls_logits, mask_logits, indices = conv.convert(feats, tokens, only_high_conf_masks=r["only_high"])
    for x in (cls_logits, mask_logits, indices):
        assert x.device.type == conv.device.type
    assert indices.dtype == torch.int64 and cls_logits.dtype == torch.float32 and mask_logits.dtype == torch.float32
    assert indices.cpu().tolist() == fx["indices"].tolist()
    assert tuple(cls_logits.shape) == fx["cls_logits"].shape == (len(fx["indices"]), r["T"], r["K"])
    assert tuple(mask_logits.shape) == fx["mask_logits"].shape == (len(fx["indices"]), r["T"], r["h"], r["w"])
    for name, got in (("cls_logits", cls_logits), ("mask_logits", mask_logits)):
        err = float((got.cpu() - torch.from_numpy(fx[name])).abs().max()) if got.numel() else 0.0
        print(f"{name}: max |diff| {err:.3e} (bound {TOL:.0e})")
        assert err <= TOL, (name, err)
    cls_all, mask_embed = conv.heads(tokens.to(conv.device))
    confidence, quality, counts = conv.scores(cls_all, mask_embed, feats.to(conv.device))
    assert counts.dtype == torch.int32 and counts.cpu().tolist() == fx["counts"].tolist()
    assert quality.dtype == torch.float32 and torch.equal(quality.cpu(), torch.from_numpy(fx["quality"]))
    err = float((confidence.cpu() - torch.from_numpy(fx["confidence"])).abs().max())
    print(f"confidence: max |diff| {err:.3e} (bound {TOL:.0e})")
    assert err <= TOL, err
    return cls_logits, mask_logits, indices
