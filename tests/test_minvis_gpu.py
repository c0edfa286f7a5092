"""GPU: the kernels of csrc/video_post.hip against their ATen formulation (video_minvis.AtenSteps, the reference's expressions on the
resized stack), both MinVIS-style drivers on the device against the reference's results (golden g24_*), the None -> ATen fall-back, and
the peak memory of the post-processing (the reference's [K, V, Hp, Wp] stack is never built)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_minvis_cpu import check_vis, check_vps, load_golden, run_driver
from univs_amd import ops
from univs_amd.inference import video_minvis
from univs_amd.inference.video_minvis import AtenSteps, FusedSteps, clip_frame_counts, scale_to_mean_

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")


def blobs(seed, Q, V, h, w):
    """Mean-like mask logits [Q, V, h, w]: -5 plus a moving Gaussian blob per row, plus noise (objects overlap and win pixels)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    c = torch.rand(Q, 2, generator=g) * torch.tensor([h, w])
    vel = (torch.rand(Q, 2, generator=g) - 0.5)
    s = 1.5 + 3 * torch.rand(Q, generator=g)
    amp = 4 + 8 * torch.rand(Q, generator=g)
    M = torch.empty(Q, V, h, w)
    for v in range(V):
        cy, cx = (c[:, 0] + vel[:, 0] * v).view(-1, 1, 1), (c[:, 1] + vel[:, 1] * v).view(-1, 1, 1)
        M[:, v] = -5 + amp.view(-1, 1, 1) * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s.view(-1, 1, 1) ** 2))
    return (M + 0.1 * torch.randn(M.shape, generator=g)).to(dev)


GEOMS = [  # (Q, V, h, w, padded, crop, out)
    (12, 7, 16, 24, (64, 96), (60, 90), (45, 68)),
    (9, 5, 20, 28, (80, 112), (80, 101), (120, 151)),
]


@pytest.mark.parametrize("T,n_clips", [(2, 9), (3, 6)])
def test_accumulate_matches_stack_and_mean(T, n_clips):
    """Bit-identical to the reference's stack-and-mean on the same device inputs at T = 2; at T >= 3 only the summation order differs."""
    g = torch.Generator().manual_seed(T)
    Qm, Q, h, w = 14, 10, 15, 22                                  # h w = 330: not a multiple of 4 (the scalar instantiation) ...
    for hw in ((h, w), (16, 24)):                                 # ... and a multiple of 4 (the float4 one)
        clips = [(torch.randn(Qm, T, *hw, generator=g) * 3).to(dev) for _ in range(n_clips)]
        perms = [torch.randperm(Qm, generator=g)[:Q].to(dev) for _ in range(n_clips)]
        V = n_clips + T - 1
        S = torch.zeros(Q, V, *hw, device=dev)
        for i, (c, p) in enumerate(zip(clips, perms)):
            ops.minvis_accumulate(S, c, p, i)
        got = scale_to_mean_(S, clip_frame_counts(n_clips, T))
        ref = torch.stack([torch.stack([clips[v - t][perms[v - t]][:, t] for t in range(min(v + 1, T)) if v - t < n_clips]).mean(dim=0)
                           for v in range(V)], dim=1)
        if T == 2:
            assert torch.equal(got, ref)
        else:
            torch.testing.assert_close(got, ref, rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("geom", GEOMS)
def test_mask_stats_and_instance_masks_match_aten(geom):
    Q, V, h, w, padded, crop, out = geom
    M = blobs(1, Q, V, h, w)
    rows = torch.tensor([3, 0, 7, 3, Q - 1], dtype=torch.int32, device=dev)
    fused, aten = FusedSteps(M, padded, crop), AtenSteps(M, padded, crop)
    U = aten.U(rows)
    for step in (1, 2, 5):
        got, ref = fused.mask_stats(rows, step), aten.mask_stats(rows, step)
        near = torch.stack([((U[:, ::step] - 1).abs() < 1e-5).flatten(1).sum(-1), ((U[:, ::step] + 1).abs() < 1e-5).flatten(1).sum(-1)], -1)
        assert ((got - ref).abs() <= near).all(), (got, ref)
    got, ref = fused.instance_masks(rows, out), aten.instance_masks(rows, out)
    assert got.shape == ref.shape == (5, V) + out and got.dtype == torch.uint8
    Vd = torch.stack([F.interpolate(u[None], size=out, mode="bilinear", align_corners=False)[0] for u in U])
    diff = got != ref
    assert not (diff & (Vd.abs() >= 1e-5)).any() and int(diff.sum()) <= 4


@pytest.mark.parametrize("geom", GEOMS)
def test_panoptic_kernels_match_aten(geom):
    Q, V, h, w, padded, crop, out = geom
    M = blobs(2, Q, V, h, w)
    rows = torch.tensor([1, 4, 2, 6, 0], dtype=torch.int32, device=dev)
    scores = torch.tensor([0.9, 0.7, 0.85, 0.6, 0.75], device=dev)
    fused, aten = FusedSteps(M, padded, crop), AtenSteps(M, padded, crop)
    ids, ref_ids = fused.panoptic_ids(rows, scores), aten.panoptic_ids(rows, scores)
    P = aten.probs(rows)
    prob = scores.view(-1, 1, 1, 1) * P
    t2 = prob.topk(2, dim=0)[0]
    tie = ((t2[0] - t2[1]) < 1e-6) | ((P - 0.5).abs() < 1e-6).any(0)
    assert ids.dtype == torch.int32 and ids.shape == (V,) + crop
    assert not ((ids != ref_ids) & ~tie).any()
    assert (ref_ids == -1).any() and (ref_ids >= 0).any()          # background and segments both present
    # counts and paint from the SAME ids (the kernel's), so that the comparison isolates the output-size step
    counts, ref_counts = fused.panoptic_counts(rows, ids, out), aten.panoptic_counts(rows, ids, out)
    Pout = torch.stack([F.interpolate(P[k][None], size=out, mode="bilinear", align_corners=False)[0] for k in range(len(P))])
    near = ((Pout - 0.5).abs() < 1e-6).flatten(1).sum(-1)
    d = (counts.cpu() - ref_counts).abs()
    assert (d[:, 0] == 0).all() and (d[:, 1] <= near.cpu()).all() and (d[:, 2] <= near.cpu()).all(), (counts, ref_counts)
    lut = [3, 0, 5, 3, 7]
    pan, ref_pan = fused.panoptic_paint(rows, ids, lut, out), aten.panoptic_paint(rows, ids, lut, out)
    assert pan.dtype == torch.int32 and pan.shape == (V,) + out
    assert int((pan != ref_pan).sum()) <= int(near.sum()) and (pan != 0).any()


@pytest.mark.parametrize("name", ["g24_vis_t2", "g24_vis_t3", "g24_vis_zero_shot"])
def test_vis_driver_gpu_matches_reference(name):
    g, r = load_golden(name)
    check_vis(run_driver(r, device=dev), g, r, exact=False)


@pytest.mark.parametrize("name", ["g24_vps_t2", "g24_vps_t3"])
def test_vps_driver_gpu_matches_reference(name):
    g, r = load_golden(name)
    check_vps(run_driver(r, device=dev), g, r, exact=False)


def test_none_falls_back_to_the_aten_formulation(monkeypatch):
    """Every op returning None (a shape no kernel covers) sends the step to AtenSteps: same results as the fused path."""
    g, r = load_golden("g24_vps_t2")
    for op in ("video_mask_stats", "video_instance_masks", "video_panoptic_ids", "video_panoptic_counts", "video_panoptic_paint"):
        monkeypatch.setattr(ops, op, lambda *a, **k: None)
    calls = []
    real = AtenSteps.panoptic_ids
    monkeypatch.setattr(AtenSteps, "panoptic_ids", lambda self, *a: calls.append(1) or real(self, *a))
    check_vps(run_driver(r, device=dev), g, r, exact=False)
    g, r = load_golden("g24_vis_t2")
    check_vis(run_driver(r, device=dev), g, r, exact=False)
    assert calls
    rows = torch.tensor([0], device=dev)
    M = torch.zeros(1, 70000, 2, 2, device=dev)
    monkeypatch.undo()
    assert ops.video_instance_masks(M, (4, 4), (4, 4), rows, (4, 4)) is None        # N V > 65535: not covered, not an error


def test_post_processing_peak_memory_stays_near_the_running_sum():
    """A 60-frame video at 256 x 448 padded: the post-processing allocates its outputs and little else, far under the reference's
    K V Hp Wp fp32 stack."""
    Q, V, h, w, padded, crop = 20, 60, 64, 112, (256, 448), (240, 427)
    M = blobs(3, Q, V, h, w)
    stack = Q * V * padded[0] * padded[1] * 4
    small = 16 << 20
    cls = torch.full((Q, 25), 0.02, device=dev)
    cls[torch.arange(Q), torch.arange(Q) % 25] = torch.linspace(0.3, 0.9, Q, device=dev)
    vis = video_minvis.InferenceVideoVISFast(num_queries=Q, stability_score_thresh=0.0, size_divisibility=32, LSJ_aug_image_size=1024,
                                             LSJ_aug_enable_test=False, pixel_mean=[0.0] * 3, pixel_std=[1.0] * 3, num_frames=2,
                                             num_frames_window_test=5, test_topk_per_image=100).to(dev)
    out = (240, 427)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = vis.postprocess(cls, M, padded, crop, out)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert len(res["pred_masks"]) >= 5
    assert peak < 3 * V * out[0] * out[1] + small and peak < stack / 10, (peak, stack)
    vps = video_minvis.InferenceVideoVPS(num_queries=Q, stability_score_thresh=0.0, size_divisibility=32, LSJ_aug_image_size=1024,
                                         LSJ_aug_enable_test=False, pixel_mean=[0.0] * 3, pixel_std=[1.0] * 3, num_frames=2,
                                         num_frames_window_test=2, test_topk_per_image=10, object_mask_threshold=0.05,
                                         overlap_threshold=0.5, thing_dataset_ids=[1, 2, 3]).to(dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = vps.postprocess(cls, M, padded, crop, out)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = V * crop[0] * crop[1] * 4 + V * out[0] * out[1] * 4           # the interim ids and the painted map
    assert res["pred_masks"].shape == (V,) + out and res["segments_infos"]
    assert peak < outputs + small and peak < stack / 10, (peak, outputs, stack)
