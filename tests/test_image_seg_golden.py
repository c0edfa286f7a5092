"""The per-image driver (univs_amd/inference/image_generic_seg.py) against the reference's own post-processing (tests/golden/g23_*.npz,
made by tools/gen_golden_image.py: `InferenceImageGenericSegmentation.inference_image` of the reference on closed-form decoder outputs).
The CPU test runs the driver's ATen formulation, the GPU test the fused kernels of csrc/image_post.hip.  Differences are allowed only
where the fixture records that the reference's own result sits within rounding of a decision:
  panoptic     pixels whose top-two score * sigmoid gap is < 1e-6 (or whose winner has |U| < 1e-5): `pan_tie`
  instances    the same (class, score) set (scores within 1e-6 relative); mask pixels flip only where |logit| < 1e-5: `inst_near0`
  sem_seg      the same argmax outside near-ties (`sem_tie`); sampled values within 1e-5 * max(1, |value|)
segments_info must be identical."""
import json
import os

import numpy as np
import pytest
import torch

from univs_amd.config import get_cfg
from univs_amd.inference.image_generic_seg import InferenceImageGenericSegmentation
from univs_amd.workloads import image_blob_logits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["g23_coco_panoptic", "g23_ade20k"]


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    r = json.loads(d.pop("recipe").tobytes())
    return r, d


def run_driver(r, device, fused):
    Qp = r["Q"] + r["C"]
    lowres_crop = (r["crop"][0] * r["h"] // r["padded"], r["crop"][1] * r["w"] // r["padded"])
    L, cls = image_blob_logits(r["seed"], Qp, r["h"], r["w"], r["C"], lowres_crop)
    cfg = get_cfg()
    t = cfg.MODEL.MASK_FORMER.TEST
    t.SEMANTIC_ON, t.INSTANCE_ON, t.PANOPTIC_ON = r["semantic_on"], r["instance_on"], r["panoptic_on"]
    t.OVERLAP_THRESHOLD, t.OBJECT_MASK_THRESHOLD, t.STABILITY_SCORE_THRESH = r["overlap"], r["object_mask"], r["stability"]
    cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES = r["Q"]
    d = InferenceImageGenericSegmentation(cfg, thing_contiguous_ids={r["dataset"]: r["things"]})
    d.fused = fused
    with torch.no_grad():
        return d.postprocess(cls.to(device), L.to(device), (r["padded"], r["padded"]), tuple(r["crop"]), tuple(r["out"]),
                             dataset_name=r["dataset"])


def unpack(bits, shape):
    return torch.from_numpy(np.unpackbits(bits)[: int(np.prod(shape))].reshape(shape).astype(bool))


def compare(r, g, res):
    H0, W0 = r["out"]
    if r["panoptic_on"]:
        pan, info = res["panoptic_seg"]
        assert info == json.loads(g["pan_info"].tobytes())
        ref = torch.from_numpy(g["pan"])
        tie = unpack(g["pan_tie"], (H0, W0))
        diff = pan.cpu() != ref
        assert not bool((diff & ~tie).any()), int((diff & ~tie).sum())
        assert int(tie.sum()) <= 1e-3 * tie.numel()                  # the named bound: near-ties are rare on these recipes
    if r["instance_on"]:
        inst = res["instances"]
        rs, rc = torch.from_numpy(g["inst_scores"]), torch.from_numpy(g["inst_classes"])
        assert len(inst.scores) == len(rs)
        masks = unpack(g["inst_masks"], (len(rs), H0, W0))
        near0 = unpack(g["inst_near0"], (len(rs), H0, W0))
        boxes = torch.from_numpy(g["inst_boxes"])
        got_s, got_c = inst.scores.cpu(), inst.pred_classes.cpu()
        got_m, got_b = inst.pred_masks.cpu() > 0, inst.pred_boxes.tensor.cpu()
        used = set()
        for i in range(len(rs)):                                     # the reference's top-k order is unspecified: match as sets
            cand = [j for j in range(len(got_s)) if j not in used and int(got_c[j]) == int(rc[i])
                    and abs(float(got_s[j]) - float(rs[i])) <= 1e-6 * abs(float(rs[i]))]
            assert cand, (i, int(rc[i]), float(rs[i]))
            j = min(cand, key=lambda j: abs(float(got_s[j]) - float(rs[i])))
            used.add(j)
            flips = got_m[j] != masks[i]
            assert not bool((flips & ~near0[i]).any()), (i, int((flips & ~near0[i]).sum()))
            if not bool(flips.any()):
                assert torch.equal(got_b[j], boxes[i])
    if r["semantic_on"]:
        sem = res["sem_seg"].cpu()
        assert sem.shape == (r["C"], H0, W0)
        tie = unpack(g["sem_tie"], (H0, W0))
        differ = sem.argmax(0) != torch.from_numpy(g["sem_argmax"]).long()
        assert not bool((differ & ~tie).any())
        idx = torch.from_numpy(g["sem_idx"]).long()
        val = torch.from_numpy(g["sem_val"])
        got = sem[idx[:, 0], idx[:, 1], idx[:, 2]]
        assert float(((got - val).abs() / val.abs().clamp(min=1.0)).max()) < 1e-5


@pytest.mark.parametrize("name", CASES)
def test_driver_matches_the_reference_cpu(name):
    r, g = load(name)
    compare(r, g, run_driver(r, "cpu", fused=False))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_driver_matches_the_reference_gpu(cuda, name):
    r, g = load(name)
    compare(r, g, run_driver(r, cuda, fused=True))
