"""What tests/test_vis_eval_cpu.py and tests/test_vis_overlap_gpu.py share: the g29 fixtures (tools/gen_golden_vis_eval.py), the
comparison of a score with what the reference recorded, and the masks of the kernel tests.  The counts are integers and the scores
the same float64 operations on them: no tolerance anywhere."""
import json
import os

import numpy as np
import torch

from univs_amd.evaluation import vis_counts as vc
from univs_amd.evaluation import ytvis
from univs_amd.inference import results as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORED = ["clean", "score_ties", "crowd", "none_frames", "over_maxdets", "area_ranges", "absent_category", "mixed_gt_rle", "zero_union"]
ERRORS = ["err_unknown_video", "err_not_a_list"]
ERROR_TYPES = {"AssertionError": AssertionError}


def load(name):
    with np.load(os.path.join(GOLDEN, f"g29_vis_eval_{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    fx["gt"], fx["results"] = json.loads(str(fx["gt_json"])), json.loads(str(fx["results_json"]))
    fx["class_names"] = [str(n) for n in fx["class_names"]]
    return fx


def same(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True)


def check_scene(fx, device):
    """The fixture scored on `device` against every table the reference recorded -> the YTVISEval."""
    ev = ytvis.YTVISEvaluator(fx["gt"], thing_classes=fx["class_names"], device=device)
    ev.reset()
    ev.process(None, fx["results"])
    res = ev.evaluate()
    e = ev.last_eval
    print("stats", e.stats.tolist())
    assert same(e.stats, fx["stats"])
    for k in ("precision", "recall", "scores"):
        assert same(e.eval[k], fx[k]), k
    keys = [tuple(int(v) for v in k) for k in fx["ious_keys"]]
    assert [k for k, v in e.ious.items() if len(v) > 0] == keys
    for i, k in enumerate(keys):
        assert same(e.ious[k], fx[f"ious_{i}"]), k
    assert list(res) == ["segm"] and list(res["segm"]) == [str(k) for k in fx["derived_keys"]]
    assert same(list(res["segm"].values()), fx["derived_values"])
    assert e.summary == [str(s) for s in fx["lines"]]
    return e


# ---- masks of the kernel tests ---------------------------------------------------------------------------------------------------------
def runs_of(masks, absent=(), device=None):
    """bool [N, T, H, W] -> Runs of its N T masks (None at the flat indices `absent`), through the string coder."""
    N, T, H, W = masks.shape
    rles = R.rle_encode_masks(torch.as_tensor(masks).reshape(N * T, H, W))
    return vc.runs_from_rles([None if i in absent else r for i, r in enumerate(rles)], H, W, device=device)


def brute(d, g, d_absent=(), g_absent=()):
    """int64 [D, G, T]: the dense AND-count of bool [D, T, H, W] and [G, T, H, W]."""
    d, g = torch.as_tensor(d).clone(), torch.as_tensor(g).clone()
    for x, absent in ((d, d_absent), (g, g_absent)):
        for i in absent:
            x[i // x.shape[1], i % x.shape[1]] = False
    return torch.einsum("dtn,gtn->dgt", d.flatten(2).to(torch.int64), g.flatten(2).to(torch.int64))


def blobs(N, T, H, W, seed, fill=0.35):
    """bool [N, T, H, W]: smooth random regions (a few runs per column), different in every mask."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((N, T, H, W), bool)
    for n in range(N):
        for t in range(T):
            for _ in range(3):
                cy, cx = rng.uniform(0, H), rng.uniform(0, W)
                ry, rx = rng.uniform(1, max(2, H * fill)), rng.uniform(1, max(2, W * fill))
                out[n, t] |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return out


def comb(H, W, teeth):
    """bool [H, W] with exactly `teeth` foreground runs of one pixel (column-major, every other pixel), from pixel 1 on."""
    flat = np.zeros(H * W, bool)
    flat[1:2 * teeth:2] = True
    assert 2 * teeth <= H * W
    return flat.reshape(W, H).T.copy()
