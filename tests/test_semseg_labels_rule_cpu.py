"""CPU: the two rules of include/univs_imagelabels_hip.h as numpy states them (inference/semseg_labels_rule.py) against ATen: the
labels equal `F.interpolate(...).argmax(0)` wherever the two largest resized values differ by more than rounding, the tie rule exactly
on constructed planes, the confusion rule against `bincount`, and the ATen forms the driver and the evaluators use on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from univs_amd import imagelabels_ops as il
from univs_amd.inference.image_generic_seg import AtenSteps
from univs_amd.inference.semseg_labels_rule import label_confusion_rule, resized_plane, semseg_labels_rule

GEOMS = [((13, 9), (40, 31)), ((37, 53), (19, 23)), ((24, 32), (24, 32)), ((3, 4), (1, 1)), ((3, 4), (1, 3)), ((3, 4), (1, 5)),
         ((16, 65), (9, 34))]


def aten(r, size):
    return F.interpolate(torch.as_tensor(r)[None], size=tuple(size), mode="bilinear", align_corners=False)[0]


@pytest.mark.parametrize("geom", GEOMS, ids=str)
@pytest.mark.parametrize("C", [1, 2, 7, 150])
def test_rule_equals_aten_but_for_near_ties(geom, C):
    (hi, wi), size = geom
    r = np.random.default_rng(100 * C + hi).standard_normal((C, hi, wi)).astype(np.float32)
    got = semseg_labels_rule(r, size)
    dense = aten(r, size)
    assert got.dtype == np.uint8 and got.shape == tuple(size)
    # the resized values themselves against ATen's: a source coordinate below n carries up to eps n of absolute rounding error (its
    # product and its subtraction, each half an ulp of a number below n), and so does the weight taken from it; a weight's error moves
    # the value by at most that times the spread of the plane, 2 max|r|, along each axis; the blend adds four roundings of values
    # below max|r|
    tol = np.finfo(np.float32).eps * np.abs(r).max() * (2 * (hi + wi) + 4)
    mine = np.stack([resized_plane(p, size) for p in r])
    assert np.abs(mine - dense.numpy()).max() <= tol
    ref = dense.argmax(0).numpy()
    differ = got != ref
    if C > 1:
        top2 = dense.topk(2, dim=0)[0].numpy()
        assert ((top2[0] - top2[1])[differ] <= 2 * tol).all()
        assert differ.mean() < 0.01
    else:
        assert not differ.any()
    assert np.array_equal(AtenSteps.semseg_labels(torch.as_tensor(r), size).numpy(), ref)


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_tie_rules_are_exact(geom):
    (hi, wi), size = geom
    rng = np.random.default_rng(7)
    C = 9
    r = rng.standard_normal((C, hi, wi)).astype(np.float32)
    r[3] = r.max() + 1 + rng.random((hi, wi), dtype=np.float32)      # planes 3 and 5 identical and maximal -> 3
    r[5] = r[3]
    assert (semseg_labels_rule(r, size) == 3).all()
    same = np.repeat(r[:1], C, axis=0)                               # all planes equal -> 0
    assert (semseg_labels_rule(same, size) == 0).all()
    last = same.copy()                                               # the maximum only in the last plane -> C - 1
    last[C - 1] += 1
    assert (semseg_labels_rule(last, size) == C - 1).all()
    # (the ATen form on the CPU only where the maximum is clear: its resize there does not give equal planes equal bits, so on exact
    # ties its argmax is not the first plane; on the GPU the dense form is ops.bilinear_resample, tests/test_semseg_labels_gpu.py)
    assert (AtenSteps.semseg_labels(torch.as_tensor(last), size) == C - 1).all()


def test_rule_refuses_what_the_kernel_does_not_cover():
    with pytest.raises(ValueError):
        semseg_labels_rule(np.zeros((257, 2, 2), np.float32), (2, 2))
    with pytest.raises(ValueError):
        semseg_labels_rule(np.zeros((2, 2), np.float32), (2, 2))


def maps(K, shape, seed, ignore=255):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, K, shape).astype(np.uint8)
    gt[rng.random(shape) < 0.1] = ignore
    pred = rng.integers(0, K, shape).astype(np.uint8)
    return gt, pred


@pytest.mark.parametrize("K", [1, 2, 19, 150, 181])
def test_confusion_rule_equals_bincount_and_the_aten_form(K):
    H, W = 23, 31
    gt, pred = maps(K, (H, W), K)
    conf = label_confusion_rule(gt, pred, K)
    g = np.where(gt == 255, K, gt).astype(np.int64)
    ref = np.bincount((K + 1) * g.ravel() + pred.ravel(), minlength=(K + 1) ** 2).reshape(K + 1, K + 1)
    assert conf.dtype == np.int64 and np.array_equal(conf, ref)
    assert conf.sum() == H * W                                       # every pixel is in one cell
    assert conf[K].sum() == (gt == 255).sum() > 0                    # the ignore label goes to row K
    assert conf[:, K].sum() == 0
    got = il.label_confusion(torch.as_tensor(gt), torch.as_tensor(pred), K)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), conf)
    # detectron2's matrix is this one transposed: bincount((K + 1) pred + gt)
    d2 = np.bincount((K + 1) * pred.ravel().astype(np.int64) + g.ravel(), minlength=(K + 1) ** 2).reshape(K + 1, K + 1)
    assert np.array_equal(conf.T, d2)


def test_confusion_accumulates_and_keeps_the_check_for_the_caller():
    K = 5
    conf, stray = il.new_confusion(K, "cpu")
    g1, p1 = maps(K, (8, 9), 1)
    g2, p2 = maps(K, (3, 4), 2)
    g2[0, 0] = 100
    il.label_confusion(torch.as_tensor(g1), torch.as_tensor(p1), K, conf=conf, stray=stray)
    il.label_confusion(torch.as_tensor(g2), torch.as_tensor(p2), K, conf=conf, stray=stray)       # (no error here: no read-back)
    assert stray.tolist() == [1, 0] and int(conf.sum()) == 72 + 12 - 1
    with pytest.raises(ValueError):
        il.raise_on_stray(stray, K)


def test_a_stray_ground_truth_byte_is_a_value_error():
    K = 10
    gt, pred = maps(K, (6, 7), 3)
    gt[2, 3] = 200
    for fn in (lambda: label_confusion_rule(gt, pred, K), lambda: il.label_confusion(torch.as_tensor(gt), torch.as_tensor(pred), K)):
        with pytest.raises(ValueError, match="1 ground-truth pixels are neither a class below 10 nor the ignore label 255"):
            fn()
    gt[2, 3] = K                                                     # K itself is no class either
    with pytest.raises(ValueError):
        label_confusion_rule(gt, pred, K)
    gt[2, 3] = 0
    pred[0, 0] = K + 1
    for fn in (lambda: label_confusion_rule(gt, pred, K), lambda: il.label_confusion(torch.as_tensor(gt), torch.as_tensor(pred), K)):
        with pytest.raises(ValueError, match="1 predicted pixels are above 10"):
            fn()
    with pytest.raises(RuntimeError):
        il.label_confusion(torch.as_tensor(gt), torch.as_tensor(pred[:3]), K)
