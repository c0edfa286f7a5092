"""GPU: the labels of a semantic result without its [C, H, W] tensor (csrc/semseg_labels.hip, imagelabels_ops.semseg_labels) against
`ops.bilinear_resample(r, size).argmax(0)` byte for byte, and the confusion count of two label maps against the ATen `bincount`.
All comparisons are exact."""
import pytest
import torch

from univs_amd import imagelabels_ops as il
from univs_amd import ops

pytestmark = pytest.mark.gpu

GEOMS = [((13, 9), (40, 31)),            # up
         ((37, 53), (19, 23)),           # down
         ((24, 32), (24, 32)),           # identity
         ((3, 4), (1, 1)), ((3, 4), (1, 3)), ((3, 4), (1, 5)),     # W in {1, 3, 5}, H = 1
         ((64, 257), (33, 130))]         # the last partial group of four; several workgroups
CLASSES = [1, 2, 7, 133, 150, 256]


def dense(r, size):
    return ops.bilinear_resample(r, size).argmax(0).to(torch.uint8)


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_labels_equal_the_dense_argmax(cuda, C, geom):
    (hi, wi), size = geom
    gen = torch.Generator().manual_seed(1000 * C + hi)
    r = torch.randn((C, hi, wi), generator=gen).to(cuda)
    got = il.semseg_labels(r, size)
    ref = dense(r, size)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(size)
    assert torch.equal(got, ref), (got != ref).nonzero()[:5].tolist()
    if C >= 7:
        assert len(torch.unique(got)) > 1 or got.numel() == 1


@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[1], GEOMS[6]], ids=str)
def test_the_first_maximum_wins(cuda, geom):
    (hi, wi), size = geom
    gen = torch.Generator().manual_seed(5)
    C = 9
    r = torch.randn((C, hi, wi), generator=gen).to(cuda)
    r[3] = r.max() + 1 + torch.rand((hi, wi), generator=gen).to(cuda)   # planes 3 and 5 identical and maximal -> 3
    r[5] = r[3]
    got = il.semseg_labels(r, size)
    assert torch.equal(got, torch.full_like(got, 3)) and torch.equal(got, dense(r, size))
    same = r[:1].expand(C, hi, wi).contiguous()                          # all planes equal -> 0
    got = il.semseg_labels(same, size)
    assert torch.equal(got, torch.zeros_like(got)) and torch.equal(got, dense(same, size))
    last = same.clone()                                                  # the maximum only in the last plane -> C - 1
    last[C - 1] += 1
    got = il.semseg_labels(last, size)
    assert torch.equal(got, torch.full_like(got, C - 1)) and torch.equal(got, dense(last, size))
    ties = torch.randint(0, 3, (150, hi, wi), generator=gen).float().to(cuda)   # many exact ties across the four class quarters
    got = il.semseg_labels(ties, size)
    assert torch.equal(got, dense(ties, size))


def test_a_row_of_labels_that_starts_off_a_dword_and_a_view_of_r(cuda):
    r = torch.randn((8, 11, 7), generator=torch.Generator().manual_seed(2)).to(cuda)
    assert torch.equal(il.semseg_labels(r, (9, 6)), dense(r, (9, 6)))    # W = 6: every other row starts at byte 2 of a dword
    part = r[2:7]                                                        # contiguous, 16-byte aligned or not: scalar loads only
    assert torch.equal(il.semseg_labels(part, (22, 14)), dense(part, (22, 14)))


def test_more_than_256_classes_are_not_covered(cuda):
    assert il.semseg_labels(torch.zeros((257, 4, 4), device=cuda), (4, 4)) is None
    with pytest.raises(RuntimeError):
        il.semseg_labels(torch.zeros((3, 4, 4), device=cuda, dtype=torch.float16), (4, 4))


def maps(K, n, seed, ignore=255, frac=0.1):
    gen = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, K, (n,), generator=gen, dtype=torch.int64)
    gt[torch.rand(n, generator=gen) < frac] = ignore
    runs = torch.rand(n, generator=gen) < 0.5                            # long runs of one cell beside scattered ones
    pred = torch.where(runs, gt.clamp(max=K - 1), torch.randint(0, K, (n,), generator=gen))
    return gt.to(torch.uint8), pred.to(torch.uint8)


def both(gt, pred, K, ignore=255):
    a = il.new_confusion(K, gt.device)
    b = il.new_confusion(K, gt.device)
    ran = il.label_confusion_u8(gt, pred, K, ignore, *a)
    il.label_confusion_aten(gt, pred, K, ignore, *b)
    return ran, a, b


@pytest.mark.parametrize("K", [1, 2, 133, 150, 180])
def test_confusion_equals_the_bincount(cuda, K):
    gt, pred = maps(K, 48 * 72 + 3, K)
    ran, (conf, stray), (rconf, rstray) = both(gt.to(cuda), pred.to(cuda), K)
    assert ran is True and torch.equal(conf, rconf) and torch.equal(stray, rstray)
    assert int(conf.sum()) == gt.numel() and int(stray.sum()) == 0
    assert int(conf[K].sum()) == int((gt == 255).sum()) > 0 and int(conf[:, K].sum()) == 0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_confusion_at_the_tile_edges(cuda, n):
    gt, pred = maps(19, n, n)
    ran, (conf, stray), (rconf, _) = both(gt.to(cuda), pred.to(cuda), 19)
    assert ran is True and torch.equal(conf, rconf) and int(conf.sum()) == n and int(stray.sum()) == 0


def test_one_cell_over_a_whole_wave(cuda):
    gt = torch.full((4096,), 3, dtype=torch.uint8, device=cuda)
    conf = il.label_confusion(gt, gt, 5)
    assert int(conf[3, 3]) == 4096 and int(conf.sum()) == 4096


def test_confusion_accumulates_over_two_calls_and_two_dimensional_maps(cuda):
    K = 21
    g1, p1 = maps(K, 40 * 30, 1)
    g2, p2 = maps(K, 17 * 5, 2)
    conf, stray = il.new_confusion(K, cuda)
    il.label_confusion(g1.view(40, 30).to(cuda), p1.view(40, 30).to(cuda), K, conf=conf, stray=stray)
    il.label_confusion(g2.view(17, 5).to(cuda), p2.view(17, 5).to(cuda), K, conf=conf, stray=stray)
    ref = il.label_confusion(g1, p1, K) + il.label_confusion(g2, p2, K)                  # (the CPU: the bincount)
    assert torch.equal(conf.cpu(), ref) and int(conf.sum()) == 40 * 30 + 17 * 5


def test_the_ignore_label_is_a_parameter(cuda):
    K = 6
    gt, pred = maps(K, 999, 3, ignore=77)
    ran, (conf, stray), (rconf, _) = both(gt.to(cuda), pred.to(cuda), K, ignore=77)
    assert ran is True and torch.equal(conf, rconf) and int(conf[K].sum()) == int((gt == 77).sum()) > 0
    none = gt.clamp(max=K - 1)                                       # ignore_label = -1: nothing is ignored
    ran, (conf, stray), (rconf, _) = both(none.to(cuda), pred.to(cuda), K, ignore=-1)
    assert ran is True and torch.equal(conf, rconf) and int(conf[K].sum()) == 0


def test_a_stray_byte_is_counted_apart_and_raises(cuda):
    K = 10
    gt, pred = maps(K, 5000, 4)
    gt[1234], gt[4999] = 200, K                                      # neither a class nor 255
    pred[77] = K + 1
    pred[1234] = 250                                                 # (a pixel whose ground truth is stray counts once, there)
    ran, (conf, stray), (rconf, rstray) = both(gt.to(cuda), pred.to(cuda), K)
    assert ran is True and stray.tolist() == rstray.tolist() == [2, 1] and torch.equal(conf, rconf)
    assert int(conf.sum()) == 5000 - 3
    with pytest.raises(ValueError, match="2 ground-truth pixels are neither a class below 10 nor the ignore label 255"):
        il.label_confusion(gt.to(cuda), pred.to(cuda), K)
    gt[1234], gt[4999] = 0, 0                                        # (pixel 1234's prediction is counted now: its ground truth fits)
    with pytest.raises(ValueError, match="2 predicted pixels are above 10"):
        il.label_confusion(gt.to(cuda), pred.to(cuda), K)


def test_beyond_the_lds_table_the_kernel_answers_none_and_the_bincount_counts(cuda):
    K = 181                                                          # 182^2 = 33124 cells
    gt, pred = maps(K, 3000, 6)
    conf, stray = il.new_confusion(K, cuda)
    assert il.label_confusion_u8(gt.to(cuda), pred.to(cuda), K, 255, conf, stray) is None and int(conf.sum()) == 0
    got = il.label_confusion(gt.to(cuda), pred.to(cuda), K)
    assert torch.equal(got.cpu(), il.label_confusion(gt, pred, K)) and int(got.sum()) == 3000
    off = torch.zeros(4004, dtype=torch.uint8, device=cuda)[1:4001]  # maps that do not start on a dword
    small = il.new_confusion(3, cuda)
    assert il.label_confusion_u8(off, off, 3, 255, *small) is None
    assert int(il.label_confusion(off, off, 3)[0, 0]) == 4000
