"""What tests/test_pvos_eval_cpu.py and tests/test_pvos_eval_gpu.py share: the g30 fixtures (tools/gen_golden_pvos_eval.py), the
VIPOSeg trees painted from them, the label maps of the kernel tests, and the comparison of a score with what the reference recorded.
The counts are integers and the scores the same float64 operations on them: no tolerance anywhere."""
import os

import numpy as np
import torch

from univs_amd.evaluation import pvos

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORED = ["clean", "enter_leave", "duplicate_ids", "edges", "fewer_results", "unlisted_class", "empty_group", "many_objects", "wide"]
ERRORS = ["err_frame_count", "err_missing_class", "err_80_objects", "err_size_mismatch"]
ERROR_TYPES = {"AssertionError": AssertionError, "KeyError": KeyError, "ValueError": ValueError}
DS = (1, 2, 5, 8, 18, 29)
CELLS = ("I", "A_g", "A_p", "BI", "B_g", "B_p")


def load(name):
    with np.load(os.path.join(GOLDEN, f"g30_pvos_eval_{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    if "seqs" in fx:
        fx["seqs"], fx["res_seqs"] = [str(s) for s in fx["seqs"]], [str(s) for s in fx["res_seqs"]]
    return fx


def write_tree(fx, root):
    """The fixture as a VIPOSeg split and a result directory: (data_path, res_path); the results lie in `<root>/out/Annotations`."""
    from PIL import Image
    data, res = os.path.join(root, "VIPOSeg", "valid"), os.path.join(root, "out", "Annotations")
    os.makedirs(res, exist_ok=True)
    for s in fx["seqs"]:
        todo = [(os.path.join(data, "Annotations_gt", s), "gt"), (os.path.join(data, "Annotations", s), "ann")]
        if s in fx["res_seqs"]:
            todo.append((os.path.join(res, s), "pred"))
        for sub, k in todo:
            os.makedirs(sub, exist_ok=True)
            for m, n in zip(fx[f"{k}_{s}"], fx[f"{k}_names_{s}"].tolist()):
                Image.fromarray(m).save(os.path.join(sub, n), format="PNG")
    with open(os.path.join(data, "obj_class.json"), "w") as f:
        f.write(str(fx["obj_class"]))
    return data, res


def same(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True)


def check_result(fx, res, details, text=None):
    """The dictionary against the reference's bit for bit (NaNs in the same places), the per-object values behind it in append order,
    and the text of pvos-ious.txt byte for byte."""
    assert list(res) == fx["keys"].tolist()
    assert same(list(res.values()), fx["values"]), (res, fx["values"])
    n = 0
    for g in pvos.GROUPS:
        for k in (f"{g}_miou", f"{g}_biou"):
            assert same(details[k], fx[k]), k
        n += len(details[f"{g}_miou"])
    table = {k: v for k, v in details["decay"].items() if v != []}
    assert list(table) == fx["decay_k"].tolist() and [len(v) for v in table.values()] == fx["decay_n"].tolist()
    assert same([x for v in table.values() for x in v], fx["decay_v"])
    print("objects scored", len(details["objects"]), "in a group", n, "decay keys", list(table))
    assert len(details["objects"]) == int(fx["decay_n"].sum()) > 0
    assert pvos.scores_text(res) == str(fx["text"])
    if text is not None:
        assert text == str(fx["text"])


def check_scene(name, root, device):
    """One scored scene end to end through `evaluate_pvos_files` on `device`, then through the evaluator for the text file."""
    fx = load(name)
    data, res = write_tree(fx, root)
    details = {}
    got = pvos.evaluate_pvos_files(res, data, eval_decay=True, device=device, details=details)
    check_result(fx, got, details)
    return fx, data, res


def check_error_scene(name, root, device):
    import pytest
    fx = load(name)
    data, res = write_tree(fx, root)
    with pytest.raises(ERROR_TYPES[str(fx["error"])]):
        pvos.evaluate_pvos_files(res, data, eval_decay=True, device=device)


def operator_counts(fx, counts_fn, device):
    """{d: counts [T, K, 6]} of the operator fixture's stacks from `counts_fn` on `device`."""
    g, p = torch.from_numpy(fx["gt"]).to(device), torch.from_numpy(fx["pred"]).to(device)
    return {d: counts_fn(g, p, d, int(fx["K"])) for d in DS}


def check_operators(fx, counts):
    assert tuple(fx["ds"].tolist()) == DS and fx["gt"].shape == (3, 64, 96)
    for d, c in counts.items():
        assert c.dtype == torch.int32 and np.array_equal(c.cpu().numpy(), fx[f"counts_d{d}"]), d


# ---- synthetic inputs of the kernel tests -------------------------------------------------------------------------------------------
def maps(T, H, W, K, seed, top=None):
    """gt / pred uint8 [T, H, W]: label maps without holes.  Rectangles of the ids 0 .. K + 1 (0 and K + 1 are not counted but break
    uniformity) over a background of id 1, the result a perturbed copy; objects on all four borders and in the corners, single pixels,
    a large uniform region (so that not every pixel is boundary at a small d), id `top` (255 in the K = 255 case) on both sides."""
    rng = np.random.default_rng(seed)
    hi = min(K + 1, 255)
    out = []
    for side in range(2):
        m = np.ones((T, H, W), np.uint8)
        r = np.random.default_rng(seed)                               # the same rectangles on both sides ...
        for t in range(T):
            for _ in range(12):
                k = int(r.integers(0, hi + 1))
                h, w = int(r.integers(1, max(2, H // 2))), int(r.integers(1, max(2, W // 2)))
                y, x = int(r.integers(0, H)), int(r.integers(0, W))
                dy, dx = (int(v) for v in rng.integers(-1, 2, 2)) if side else (0, 0)     # ... shifted by a pixel in the result
                m[t, max(0, y + dy):y + dy + h, max(0, x + dx):x + dx + w] = k
            m[t, 0, : W // 2] = 2 if K > 1 else 1                     # first row
            m[t, H - 1, W // 3:] = 1                                  # last row, with the bottom-right pixel
            m[t, H // 2:, 0] = min(3, K)                              # first column
            m[t, H // 2, W // 2] = min(2, K) + side                   # a single pixel
            if top is not None:
                m[t, H // 4: H // 4 + 3, W // 4: W // 4 + 4 + side] = top
        out.append(m)
    return out[0], out[1]
