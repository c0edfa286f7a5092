"""What the HOTA tests share: the golden fixtures (tests/golden/g34_hota_*.npz, tools/gen_golden_hota.py) and the bit-for-bit comparison of
a result dictionary with a recorded one."""
import glob
import json
import os

import numpy as np

from univs_amd.evaluation import hota

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORED = ("clean", "more_tracks_than_gt", "more_gt_than_tracks", "one_by_one", "t1", "empty_frames", "enter_leave", "exact_fractions",
          "all_zero_frame", "full_64x64", "multi_class")
EARLY = ("no_tracks", "no_gt")
ERRORS = ("err_size_mismatch", "err_unknown_video")
_cache = {}


def names():
    return sorted(os.path.basename(p)[len("g34_hota_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "g34_hota_*.npz")))


def load(name):
    """-> (annotation dictionary, result list, options of the evaluator, the recorded arrays); read once, handed out as fresh copies of
    the JSON and the one read-only record."""
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f"g34_hota_{name}.npz")) as z:
            _cache[name] = {k: z[k] for k in z.files}
        for v in _cache[name].values():
            v.setflags(write=False)
    rec = _cache[name]
    opts = {"score_thresh": float(rec["score_thresh"]), "class_agnostic": bool(rec["class_agnostic"])}
    return json.loads(str(rec["gt_json"])), json.loads(str(rec["results_json"])), opts, rec


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_result(res, rec, prefix):
    for f in hota.FIELDS:
        assert same_bits(res[f], rec[f"{prefix}__{f}"]), (prefix, f, np.asarray(res[f]), rec[f"{prefix}__{f}"])


def assert_recorded(ev, out, rec):
    """The evaluator `ev` after `evaluate()` returned `out`, against the recorded dictionaries: every sequence, every class, both
    combinations, bit for bit."""
    assert [f"{vid}__{key}" for vid, key in sorted(ev.sequences, key=lambda k: list(rec["seq_keys"]).index(f"{k[0]}__{k[1]}"))] == list(rec["seq_keys"])
    for (vid, key), res in ev.sequences.items():
        assert_result(res, rec, f"seq__{vid}__{key}")
    assert [str(k) for k in out["per_class"]] == list(rec["cls_keys"])
    for key, res in out["per_class"].items():
        assert_result(res, rec, f"cls__{key}")
    assert_result(out["cls_comb_cls_av"], rec, "cls_av")
    assert_result(out["cls_comb_det_av"], rec, "det_av")
    for row, res in (("cls_comb_cls_av", out["cls_comb_cls_av"]), ("cls_comb_det_av", out["cls_comb_det_av"])):
        for f in hota.SUMMARY_FIELDS:
            assert out["summary"][row][f] == float(np.mean(res[f]))


def evaluate(name, device):
    ann, res, opts, rec = load(name)
    ev = hota.HOTAEvaluator(ann, device=device, **opts)
    ev.process(None, res)
    return ev, ev.evaluate(), rec
