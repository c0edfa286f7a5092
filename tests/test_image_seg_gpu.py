"""GPU: the per-image post-processing kernels (csrc/image_post.hip, ops.image_*) against the ATen formulation of the same step
(inference/image_generic_seg.py: AtenSteps), the driver's three results fused against the same driver on ATen, and the peak memory of
the fused post-processing at the shipped geometry (1024 x 1024 LSJ square, Q' = 200 + 133)."""
import pytest
import torch

from univs_amd import ops
from univs_amd.inference.image_generic_seg import AtenSteps, InferenceImageGenericSegmentation
from univs_amd.config import get_cfg
from univs_amd.workloads import image_blob_logits

pytestmark = pytest.mark.gpu

GEOMS = [  # (Q', low-res h, w, padded, crop, original size)
    (333, 64, 64, (256, 256), (192, 256), (150, 200)),
    (333, 64, 64, (256, 256), (256, 171), (256, 171)),      # identity second resize
    (50, 40, 56, (160, 224), (157, 221), (314, 442)),       # odd sizes, an up-sampling second resize
]


class SameTaps(AtenSteps):
    """ATen on U made by ops.bilinear_resample: the taps and the expression of the kernels, so integer results compare exactly."""

    @property
    def U(self):
        if self._U is None:
            self._U = ops.bilinear_resample(self.L, self.padded)
        return self._U


def case(cuda, g, seed=0):
    Q, h, w, padded, crop, out = g
    L, cls = image_blob_logits(seed, Q, h, w, 133, (crop[0] * h // padded[0], crop[1] * w // padded[1]))
    return L.to(cuda), cls.to(cuda), padded, crop, out


@pytest.mark.parametrize("g", GEOMS, ids=str)
def test_image_mask_stats_exact(cuda, g):
    L, _, padded, crop, _ = case(cuda, g)
    got = ops.image_mask_stats(L, padded, crop)
    ref = SameTaps(L, padded, crop).mask_stats()
    assert torch.equal(got, ref), (got != ref).nonzero()[:5].tolist()
    assert int(got[:, 6].sum()) > 0 and int(got[:, 0].sum()) > 0


@pytest.mark.parametrize("g", GEOMS, ids=str)
def test_image_panoptic_ids_counts_and_paint_exact(cuda, g):
    L, cls, padded, crop, out = case(cuda, g)
    K = min(120, L.shape[0])
    gen = torch.Generator().manual_seed(3)
    planes = torch.randperm(L.shape[0], generator=gen)[:K].to(cuda)
    scores = torch.rand(K, generator=gen).to(cuda)
    scores[1] = scores[0]                                           # a tie of scores: the first k wins where the masks tie too
    ref_steps = SameTaps(L, padded, crop)
    ids, counts = ops.image_panoptic_ids(L, padded, crop, planes, scores)
    rids, rcounts = ref_steps.panoptic_ids(planes, scores)
    assert torch.equal(ids, rids), int((ids != rids).sum())
    assert torch.equal(counts, rcounts)
    lut = torch.randint(0, 9, (K,), generator=gen).tolist()
    pan, seen = ops.image_panoptic_paint(ids, torch.tensor(lut, dtype=torch.int32, device=cuda), out)
    rpan, rseen = AtenSteps.panoptic_paint(rids, lut, out)
    assert torch.equal(pan, rpan)
    present = {lut[k] for k in range(K) if int(seen[k])}
    assert present == set(torch.unique(rpan).tolist()) - {0}


@pytest.mark.parametrize("g", GEOMS, ids=str)
def test_image_semseg_within_fp32_rounding(cuda, g):
    L, cls, padded, crop, _ = case(cuda, g)
    Qs = min(200, L.shape[0])
    planes = torch.arange(L.shape[0] - Qs, L.shape[0], device=cuda).flip(0)
    for C in (133, 150, 7, 171):
        probs = (cls[:Qs, :C].sigmoid() / 0.06).softmax(-1) if C <= 133 else torch.rand(Qs, C, device=cuda).softmax(-1)
        got = ops.image_semseg(L, padded, crop, planes, probs)
        ref = SameTaps(L, padded, crop).semseg(planes, probs)
        assert got.shape == ref.shape == (C,) + tuple(crop)
        err = (got - ref).abs() / ref.abs().clamp(min=1.0)
        assert float(err.max()) < 1e-5, (C, float(err.max()))


@pytest.mark.parametrize("g", GEOMS, ids=str)
def test_image_instance_masks_exact(cuda, g):
    L, _, padded, crop, out = case(cuda, g)
    planes = torch.tensor([5, 0, 17, 5, L.shape[0] - 1] + list(range(20, 40)), dtype=torch.int64, device=cuda)
    masks, rec = ops.image_instance_masks(L, padded, crop, planes, out)
    rmasks, rrec = SameTaps(L, padded, crop).instance_masks(planes, out)
    assert masks.dtype == torch.uint8 and masks.shape == (len(planes),) + tuple(out)
    assert torch.equal(masks, rmasks), int((masks != rmasks).sum())
    assert torch.equal(rec[:, 2:7], rrec[:, 2:7])
    # against ATen's own resizes: sign flips only where the double-resized logit is within rounding of 0
    Uref = torch.nn.functional.interpolate(L[None], size=padded, mode="bilinear", align_corners=False)[0][planes, : crop[0], : crop[1]]
    v = torch.nn.functional.interpolate(Uref[None], size=out, mode="bilinear", align_corners=False)[0]
    flips = masks.bool() != (v > 0)
    assert bool((v[flips].abs() < 1e-5).all())


def test_image_ops_refuse_the_cpu_and_report_what_they_do_not_cover(cuda):
    L = torch.zeros(3, 8, 8)
    with pytest.raises(RuntimeError):
        ops.image_mask_stats(L, (16, 16), (16, 16))
    Ld = L.to(cuda)
    with pytest.raises(RuntimeError):
        ops.image_mask_stats(Ld, (16, 16), (17, 16))                 # crop larger than the padded size
    many = torch.zeros(ops.IMAGE_MAX_KEPT + 1, dtype=torch.int64, device=cuda)
    assert ops.image_panoptic_ids(Ld, (16, 16), (16, 16), many, torch.zeros(len(many), device=cuda)) is None


def driver(fused, **kw):
    cfg = get_cfg()
    for k in ("SEMANTIC_ON", "INSTANCE_ON", "PANOPTIC_ON"):
        cfg.MODEL.MASK_FORMER.TEST[k] = True
    cfg.MODEL.MASK_FORMER.TEST.OVERLAP_THRESHOLD = 0.8
    cfg.MODEL.MASK_FORMER.TEST.OBJECT_MASK_THRESHOLD = 0.05
    d = InferenceImageGenericSegmentation(cfg, thing_contiguous_ids=range(80))
    d.fused = fused
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("g", GEOMS[:2], ids=str)
@pytest.mark.parametrize("stability", [0.0, 0.02])
def test_driver_fused_matches_the_aten_driver(cuda, g, stability):
    L, cls, padded, crop, out = case(cuda, g, seed=7)
    a = driver(True, stability_score_thresh=stability).postprocess(cls, L, padded, crop, out)
    b = driver(False, stability_score_thresh=stability).postprocess(cls, L, padded, crop, out)
    # panoptic: identical but for pixels whose resized logits sit within rounding of a decision
    pa, ia = a["panoptic_seg"]
    pb, ib = b["panoptic_seg"]
    assert ia == ib and len(ia) >= 2
    assert int((pa != pb).sum()) <= 1e-3 * pa.numel()
    # instances: the same (class, score) set, masks equal but for near-zero logits
    A, B = a["instances"], b["instances"]
    assert len(A.scores) == len(B.scores) == 100
    assert torch.allclose(A.scores.sort()[0], B.scores.sort()[0], rtol=1e-3, atol=0)
    same = A.pred_classes == B.pred_classes
    assert int(same.sum()) >= 98                                    # (quality counts may differ by a pixel at |U - 1| ~ 1e-7)
    assert int((A.pred_masks[same] != B.pred_masks[same]).sum()) <= 1e-3 * A.pred_masks[same].numel()
    assert len(a["instances_rle"]) == 100 and a["instances_rle"][0]["size"] == list(out)
    # semantic: values within fp32 rounding, the same argmax but for near ties
    ra, rb = a["sem_seg"], b["sem_seg"]
    assert ra.shape == (133,) + tuple(out)
    assert float(((ra - rb).abs() / rb.abs().clamp(min=1.0)).max()) < 1e-4
    top2 = rb.topk(2, dim=0)[0]
    differ = ra.argmax(0) != rb.argmax(0)
    assert bool(((top2[0] - top2[1])[differ] < 1e-4).all())


def test_post_processing_never_builds_the_upsampled_stack(cuda):
    """Shipped geometry: Q' = 333 logits of 256 x 256 under a 1024 x 1024 LSJ square (a 768 x 1024 image of a 480 x 640 original):
    the [Q', 1024, 1024] fp32 stack the reference builds is 1.40 GB; the fused post-processing's peak stays below it."""
    L, cls = image_blob_logits(11, 333, 256, 256, 133, (192, 256))
    L, cls = L.to(cuda), cls.to(cuda)
    stack = 333 * 1024 * 1024 * 4
    d = driver(True)
    d.postprocess(cls, L, (1024, 1024), (768, 1024), (480, 640))            # warm-up (kernels loaded)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = d.postprocess(cls, L, (1024, 1024), (768, 1024), (480, 640))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert len(r["panoptic_seg"][1]) > 0 and len(r["instances"].scores) == 100
    assert peak < stack, (peak, stack)
