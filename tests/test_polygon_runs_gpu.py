"""GPU: polygons to run-length boundaries by the kernel (csrc/polygon_runs.hip, polygon_ops.polygons_to_runs) against the host
formulation on the whole corpus of tests/polygon_cases.py in ONE launch, tensor for tensor; the kernel's statuses (every object done
but the one above the crossing cap, which comes out equal through the host); mixed sizes; a second stream; and COCOSegmEval on the
device against itself on the CPU, bit for bit."""
import numpy as np
import pytest
import torch

from tests import coco_scene
from tests import polygon_cases as cases
from univs_amd import polygon_ops
from univs_amd.data import polygon_rule as rule

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def on_device():
    objects, sizes = cases.objects_and_sizes()
    return polygon_ops.polygons_to_runs_status(objects, sizes, "cuda")


def _same(got, want):
    for name, g, w in zip(("bounds", "ones", "starts"), got, want):
        assert g.dtype == torch.int32 and g.is_cuda and g.shape == w.shape, name
        assert torch.equal(g.cpu(), w), (name, int((g.cpu() != w).nonzero()[0]))


def test_the_whole_corpus_in_one_launch_equals_the_host_formulation(on_device):
    _same(on_device[0], cases.expected())


def test_every_object_is_done_by_the_kernel_but_the_one_above_the_cap(on_device):
    runs, status = on_device
    names = cases.names()
    assert status.shape == (len(names),) and [names[i] for i in np.flatnonzero(status)] == ["above_cap"]
    i = names.index("above_cap")
    assert status[i] == 1
    want = cases.expected()
    a, b = int(want.starts[i]), int(want.starts[i + 1])
    assert b - a > 1 and torch.equal(runs.bounds[a:b].cpu(), want.bounds[a:b])          # equal through the fallback
    assert status[names.index("at_cap")] == 0


def test_mixed_sizes_and_absent_objects_in_one_call():
    objects = [[[1, 1, 5, 1, 5, 5, 1, 5]], None, [[0.5, 0.5, 60.2, 3.1, 31.7, 62.9]], [], [[0, 0, 1, 0, 1, 1, 0, 1]], [[2, 2, 200, 2, 200, 9, 2, 9]]]
    sizes = [(7, 7), (5, 5), (64, 63), (1, 1), (1, 1), (11, 300)]
    runs, status = polygon_ops.polygons_to_runs_status(objects, sizes, "cuda")
    _same(runs, rule.runs_from_polygons_host(objects, sizes))
    assert status.tolist() == [0] * 6 and runs.starts.diff().tolist()[1] == 0 and runs.bounds[-1].item() == 3300
    empty = polygon_ops.polygons_to_runs([], [], "cuda")
    assert empty.starts.tolist() == [0] and empty.bounds.numel() == 0


def test_on_a_second_stream():
    objects, sizes = cases.objects_and_sizes()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        runs = polygon_ops.polygons_to_runs(objects[2400:2900], sizes[2400:2900], "cuda")
    s.synchronize()
    _same(runs, rule.runs_from_polygons_host(objects[2400:2900], sizes[2400:2900]))


def test_coco_segm_eval_on_the_device_equals_itself_on_the_cpu():
    from univs_amd.evaluation.coco import evaluate_predictions_on_coco
    dataset, results = coco_scene.scene(crowd=True)
    dev, cpu = evaluate_predictions_on_coco(dataset, results, "cuda"), evaluate_predictions_on_coco(dataset, results, "cpu")
    assert dev.gt_runs.is_cuda and polygon_ops.LAST_STATUS is not None and not polygon_ops.LAST_STATUS.any()
    _same(dev.gt_runs, cpu.gt_runs)
    assert np.array_equal(dev.stats, cpu.stats) and dev.summary == cpu.summary and (dev.stats[:3] > 0).all()
    for k in ("precision", "recall", "scores"):
        assert np.array_equal(dev.eval[k], cpu.eval[k])
    assert all(np.array_equal(dev.ious[k], cpu.ious[k]) for k in cpu.ious)
