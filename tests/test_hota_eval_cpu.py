"""CPU: HOTA scoring (univs_amd/evaluation/hota.py over hota_counts.py).  The rule in numpy (`hota_counts_aten`) and the evaluator give
the reference's recorded dictionaries bit for bit on every scored fixture (tests/golden/g34_hota_*.npz, tools/gen_golden_hota.py) and
the recorded error texts on the error fixtures; the command line writes hota-final.txt; the kernel wrapper keeps the contract of
_counts.py with the library stubbed; `run.parse_args` takes --hota only with --gt-json; the eleventh header's binding is the recorded
one (tests/hota_capi_signatures.txt) and its entries answer bad and uncovered arguments before any launch."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import hota_cases
from tests.test_capi_contract_cpu import signature_lines
from tests.test_eval_counts_contract_cpu import _Stub
from univs_amd import _lib, build, ops
from univs_amd.evaluation import hota
from univs_amd.evaluation import hota_counts as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["univs_hota_counts", "univs_lsa_max_f64"]
COVERED = "not covered (at most 64 ids per side of a class, A <= 32, T <= 65535, D G T < 2^31)"


def test_every_fixture_of_the_issue_is_there():
    assert hota_cases.names() == sorted(hota_cases.SCORED + hota_cases.EARLY + hota_cases.ERRORS)


def test_the_labels_and_thresholds_are_the_references():
    assert len(hota.ARRAY_LABELS) == 19 and hota.ARRAY_LABELS.tobytes() == np.arange(0.05, 0.99, 0.05).tobytes()
    assert hota.THRESHOLDS.tobytes() == np.array([a - np.finfo('float').eps for a in np.arange(0.05, 0.99, 0.05)]).tobytes()
    assert hota.FIELDS == ['HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA', 'OWTA', 'HOTA_TP', 'HOTA_FN', 'HOTA_FP', 'HOTA(0)',
                           'LocA(0)', 'HOTALocA(0)']


@pytest.mark.parametrize("name", hota_cases.SCORED + hota_cases.EARLY)
def test_the_evaluator_gives_the_recorded_dictionaries_bit_for_bit(name):
    ev, out, rec = hota_cases.evaluate(name, "cpu")
    hota_cases.assert_recorded(ev, out, rec)


@pytest.mark.parametrize("name", hota_cases.SCORED)
def test_the_rule_gives_the_recorded_sequences_from_its_tables(name, monkeypatch):
    """`hota_counts_aten` on the tensors the evaluator hands over: one call per video, the tables of every class cut out by `of_class`
    give the recorded sequence results; the tables have the documented shapes and packing."""
    calls = []
    monkeypatch.setattr(hota, "hota_counts", lambda *a: calls.append(a) or hc.hota_counts_aten(*a))
    ev, out, rec = hota_cases.evaluate(name, "cpu")
    hota_cases.assert_recorded(ev, out, rec)
    assert len(calls) >= 1
    for gt_area, tr_area, inter, gt_ids, gt_starts, tr_ids, tr_starts, thr in calls:
        tables = hc.hota_counts_aten(gt_area, tr_area, inter, gt_ids, gt_starts, tr_ids, tr_starts, thr)
        C, T, A = len(gt_starts) - 1, int(gt_area.shape[1]), len(thr)
        cells = int((np.diff(gt_starts) * np.diff(tr_starts)).sum())
        assert tuple(tables.tp_fn_fp.shape) == (C, A, 3) and tuple(tables.matches.shape) == (A * cells,)
        assert tuple(tables.loca_sum.shape) == (C, A) and tables.loca_sum.dtype == torch.float64
        assert tuple(tables.match_col.shape) == (T * int(gt_starts[-1]),)
        for c in range(C):
            tp_fn_fp, matches, loca, gc, pc, col = tables.of_class(c, gt_starts, tr_starts, T)
            g, p = len(gc), len(pc)
            assert matches.shape == (A, g, p) and col.shape == (T, g) and col.min() >= -1 and col.max() < p
            ga, ta = gt_area[gt_ids[gt_starts[c]:gt_starts[c + 1]]].numpy(), tr_area[tr_ids[tr_starts[c]:tr_starts[c + 1]]].numpy()
            assert np.array_equal(gc, (ga > 0).sum(1)) and np.array_equal(pc, (ta > 0).sum(1))
            assert np.array_equal(tp_fn_fp[:, 0] + tp_fn_fp[:, 1], np.full(A, (ga > 0).sum()))      # TP + FN = ground-truth detections
            assert np.array_equal(tp_fn_fp[:, 0] + tp_fn_fp[:, 2], np.full(A, (ta > 0).sum()))
            assert np.array_equal(matches.sum(axis=(1, 2)), tp_fn_fp[:, 0])
            assert (col[ga.T == 0] == -1).all()                      # an absent ground truth is matched to nothing


def test_exact_fractions_sit_on_the_comparison():
    """IoUs of exactly 1/2, 1/4, 3/4, 1/5, 19/20 count at their own alpha: 25 matched pairs, five of each fraction."""
    ev, out, rec = hota_cases.evaluate("exact_fractions", "cpu")
    tp = out["cls_comb_det_av"]["HOTA_TP"]
    for frac, n_at_or_above in ((0.2, 25), (0.25, 20), (0.5, 15), (0.75, 10), (0.95, 5)):
        a = int(round(frac / 0.05)) - 1
        assert tp[a] == n_at_or_above and tp[a + 1 if a < 18 else a] <= n_at_or_above, (frac, tp)
    assert tp[int(round(0.2 / 0.05))] == 20 and tp[int(round(0.5 / 0.05))] == 10


@pytest.mark.parametrize("name", hota_cases.ERRORS)
def test_error_scenes_raise_the_recorded_texts(name):
    ann, res, opts, rec = hota_cases.load(name)
    kind = {"ValueError": ValueError, "AssertionError": AssertionError}[str(rec["error"])]
    with pytest.raises(kind) as e:
        hota.evaluate_hota_files(ann, res, device="cpu", **opts)
    assert str(e.value) == str(rec["error_text"])


def test_polygons_stay_not_implemented_and_a_file_without_annotations_is_refused():
    ann, res, opts, _ = hota_cases.load("one_by_one")
    res[0]["segmentations"][0] = [[1.0, 1.0, 5.0, 1.0, 5.0, 5.0]]
    with pytest.raises(NotImplementedError):
        hota.evaluate_hota_files(ann, res, device="cpu")
    with pytest.raises(ValueError):
        hota.HOTAEvaluator({"videos": ann["videos"], "categories": ann["categories"]})


def test_process_video_by_video_and_in_any_order_gives_the_same(tmp_path):
    ann, res, opts, rec = hota_cases.load("clean")
    ev = hota.HOTAEvaluator(ann, output_dir=str(tmp_path), device="cpu", **opts)
    for vid in (2, 1):
        ev.process(None, [r for r in res if r["video_id"] == vid])
    out = ev.evaluate()
    hota_cases.assert_recorded(ev, out, rec)
    assert sorted(os.listdir(tmp_path)) == ["hota-final.txt", "results.json"]
    with pytest.raises(ValueError):
        ev.process(None, [r for r in res if r["video_id"] == 1])     # a video is counted once
    ev.reset()
    assert ev.evaluate()["cls_comb_det_av"]["HOTA_TP"].sum() == 0    # nothing processed: every ground truth is missed


def test_the_command_line_writes_hota_final(tmp_path, capsys):
    ann, res, opts, rec = hota_cases.load("enter_leave")
    gt_path, res_path = tmp_path / "gt.json", tmp_path / "out" / "results.json"
    os.makedirs(res_path.parent)
    gt_path.write_text(json.dumps(ann))
    res_path.write_text(json.dumps(res))
    before = res_path.read_bytes()
    assert hota.main(["--gt_json", str(gt_path), "--results", str(res_path), "--class_agnostic", "--device", "cpu"]) == 0
    printed = capsys.readouterr().out.splitlines()
    lines = (tmp_path / "out" / "hota-final.txt").read_text().splitlines()
    assert lines == printed and len(lines) == 1 + 2 + 1 and res_path.read_bytes() == before
    assert lines[0].split() == ["HOTA"] + hota.SUMMARY_FIELDS and lines[3].split()[0] == "all"
    want = ["{0:1.5g}".format(100 * float(np.mean(rec["det_av__" + f]))) for f in hota.SUMMARY_FIELDS]
    assert lines[2].split() == ["cls_comb_det_av"] + want
    assert hota.main(["--gt_json", str(gt_path), "--results", str(res_path), "--score_thresh", "2", "--output_dir", str(tmp_path / "o2"),
                      "--device", "cpu"]) == 0                       # every track dropped: all missed
    assert float((tmp_path / "o2" / "hota-final.txt").read_text().splitlines()[1].split()[1]) == 0.0


def test_idmaps_give_what_the_run_length_path_gives():
    """One scene rendered both ways: disjoint boxes as RLE tracks and as id maps (ids in the order of the tracks)."""
    T, H, W = 4, 20, 28
    gt_map, pr_map = np.zeros((T, H, W), np.int32), np.zeros((T, H, W), np.int32)
    for t in range(T):
        for k in range(3):
            gt_map[t, 1 + 6 * k:5 + 6 * k, 2 + t:10 + t] = k + 1
        for k in range(4):
            if not (k == 2 and t == 1):
                pr_map[t, 2 + 4 * k:5 + 4 * k, 4 + 2 * t:13 + t] = 10 * (k + 1)
    gt_map[3][gt_map[3] == 2] = 0                                     # ground truth 2 leaves in the last frame
    from univs_amd.inference.results import rle_encode_masks
    video = {"id": 1, "height": H, "width": W, "length": T}
    anns = [{"id": k, "video_id": 1, "category_id": 1, "iscrowd": 0, "segmentations": rle_encode_masks(torch.from_numpy(gt_map == k))}
            for k in (1, 2, 3)]
    res = [{"video_id": 1, "score": 0.9, "category_id": 1, "segmentations": rle_encode_masks(torch.from_numpy(pr_map == k))}
           for k in (10, 20, 30, 40)]
    out = hota.evaluate_hota_files({"videos": [video], "categories": [{"id": 1, "name": "x"}], "annotations": anns}, res, device="cpu")
    maps = hota.hota_from_idmaps(gt_map, pr_map, device="cpu")
    assert maps["HOTA_TP"].sum() > 0
    for f in hota.FIELDS:
        assert hota_cases.same_bits(maps[f], out["per_class"][1][f]), f
    empty = hota.hota_from_idmaps(gt_map, np.zeros_like(pr_map), device="cpu")
    assert np.array_equal(empty["HOTA_FN"], np.full(19, 11.0)) and empty["LocA(0)"] == 1.0


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------------------
def _call(G=3, D=5, T=2, g=(2, 1), p=(4, 1), A=19):
    gt_starts, tr_starts = np.concatenate([[0], np.cumsum(g)]), np.concatenate([[0], np.cumsum(p)])
    return (torch.ones(G, T, dtype=torch.int32), torch.ones(D, T, dtype=torch.int32), torch.ones(D, G, T, dtype=torch.int32),
            np.arange(gt_starts[-1]) % G, gt_starts, np.arange(tr_starts[-1]) % D, tr_starts, np.linspace(0.05, 0.95, A))


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    with pytest.raises(RuntimeError) as e:
        hc.hota_video_counts(*_call())
    assert str(e.value) == str(ops._cpu_refusal("hota_video_counts", "gt on cpu"))
    with pytest.raises(RuntimeError) as e:
        hc.lsa_max(torch.zeros(1, 64, 64, dtype=torch.float64), torch.ones(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32))
    assert "Not implemented on the CPU" in str(e.value)
    for bad in (dict(g=(2, 2)), dict(p=(4, 2))):                      # more ids listed than ... is fine; starts that do not fit are not
        a = list(_call(**bad))
        a[4 if "g" in bad else 6] = np.array([0, 1, 9])
        with pytest.raises(RuntimeError):
            hc.hota_counts_aten(*a)
    a = list(_call())
    a[3] = np.array([0, 1, 7])                                       # an id outside the table
    with pytest.raises(RuntimeError):
        hc.hota_counts_aten(*a)
    a = list(_call())
    a[2] = a[2].to(torch.int64)
    with pytest.raises(RuntimeError):
        hc.hota_counts_aten(*a)


def test_wrapper_contract_with_the_library_stubbed(monkeypatch):
    """Through `ops._call`, stream last, the six outputs handed over just before it (match_col filled with -1, the others with 0), None
    on ERR_NOT_IMPLEMENTED, the wrapper's name on a launch error, no launch and no allocation beyond a coverage bound, one launch
    exactly at it, two devices refused."""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.setattr(ops, "_stream_ptr", lambda t: "stream")
    lib = _Stub(_lib.OK)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    out = hc.hota_video_counts(*_call())
    assert [tuple(o.shape) for o in out] == [(2, 19, 3), (19 * 9,), (2, 19), (3,), (5,), (2 * 3,)]
    assert [o.dtype for o in out] == [torch.int32, torch.int32, torch.float64, torch.int32, torch.int32, torch.int32]
    assert all(bool((o == 0).all()) for o in out[:5]) and bool((out.match_col == -1).all())
    ((called, args),) = lib.calls
    assert called == "univs_hota_counts" and args[-1] == "stream"
    assert [a for a in args if isinstance(a, int) and a < 1 << 32] == [5, 3, 2, 2, 2, 4, 19]      # D, G, T, C, max_g, max_p, A
    assert list(args[-7:-1]) == [o.data_ptr() for o in out]
    lib.code = _lib.ERR_NOT_IMPLEMENTED
    assert hc.hota_video_counts(*_call()) is None
    lib.code = _lib.ERR_LAUNCH
    with pytest.raises(_lib.UnivsHipError) as e:
        hc.hota_video_counts(*_call())
    assert str(e.value) == "hota_video_counts failed (code -3): stub"
    lib.code, lib.calls = _lib.OK, []
    made = []
    real_full, real_zeros = torch.full, torch.zeros
    monkeypatch.setattr(torch, "full", lambda *a, **k: made.append("full") or real_full(*a, **k))
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: made.append("zeros") or real_zeros(*a, **k))
    for beyond in (dict(G=65, g=(65,), p=(5,)), dict(D=65, g=(3,), p=(65,)), dict(A=33)):
        call = _call(**beyond)
        del made[:]
        assert hc.hota_video_counts(*call) is None and made == [], beyond
    assert lib.calls == []
    monkeypatch.undo()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.setattr(ops, "_stream_ptr", lambda t: "stream")
    monkeypatch.setattr(_lib, "load", lambda: lib)
    assert hc.hota_video_counts(*_call(G=64, D=64, g=(64,), p=(64,), A=32)) is not None and len(lib.calls) == 1
    # 65 ids fall back to the rule through `hota_counts`, and give its tables
    call = _call(G=65, g=(65,), p=(5,))
    got, want = hc.hota_counts(*call), hc.hota_counts_aten(*call)
    assert len(lib.calls) == 1 and all(torch.equal(a, b) for a, b in zip(got, want))
    a = list(_call())
    a[1] = a[1].to("meta")
    with pytest.raises(RuntimeError) as e:
        hc.hota_video_counts(*a)
    assert str(e.value) == "hota_video_counts: gt on cpu, pred on meta"


def test_run_takes_hota_only_with_gt_json():
    from univs_amd import run
    base = ["--config-file", "c", "--weights", "w", "--video-dir", "d", "--output-dir", "o"]
    assert run.parse_args(base).hota is False
    assert run.parse_args(base + ["--gt-json", "g.json", "--hota"]).hota is True
    assert run.parse_args(base + ["--gt-json", "g.json"]).hota is False
    with pytest.raises(SystemExit):
        run.parse_args(base + ["--hota"])
    with pytest.raises(SystemExit):
        run.parse_args(base + ["--hota", "--pan-gt-json", "p.json", "--truth-dir", "t"])
    ann, _, _, _ = hota_cases.load("one_by_one")
    args = run.parse_args(base + ["--gt-json", "g.json", "--hota", "--device", "cpu"])
    args.gt_json = ann
    assert isinstance(run.build_evaluator(args), hota.HOTAEvaluator)
    args.hota = False
    from univs_amd.evaluation.ytvis import YTVISEvaluator
    assert isinstance(run.build_evaluator(args), YTVISEvaluator)


# ---- the eleventh header ------------------------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "univs_hota_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == NAMES == sorted(_lib.HOTA_SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_hota_hip.h but not exported"
        res, args = _lib.HOTA_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signatures_are_the_recorded_ones_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "hota_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.HOTA_SIGNATURES) == recorded == ["univs_hota_counts I PPPIIIPPPPIIIPIPPPPPPP", "univs_lsa_max_f64 I PPPIPP"]
    others = (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FUSED_SIGNATURES) | set(_lib.PVOS_SIGNATURES) |
              set(_lib.SEMANTIC_SIGNATURES) | set(_lib.ENCODER_SIGNATURES) | set(_lib.SWIN_SIGNATURES) | set(_lib.FRAMES_SIGNATURES) |
              set(_lib.PROMPTS_SIGNATURES) | set(_lib.PNG_SIGNATURES))
    assert not set(_lib.HOTA_SIGNATURES) & others
    assert (len(_lib.SIGNATURES), len(_lib.PNG_SIGNATURES)) == (76, 1)
    assert "hota_count.hip" in build.SOURCES and any(h.endswith("univs_hota_hip.h") for h in build.HEADERS)
    assert build.SOURCE_FLAGS == {"hota_count.hip": ["-ffp-contract=off"]}      # IEEE operations in the order written, for this file alone
    assert "-ffast-math" not in build._flags() and not any("contract" in f for f in build._flags())


@pytest.fixture
def host():
    """A host buffer's address: never read, the entries answer before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


def _counts_entry(lib, p, D=5, G=3, T=2, C=2, max_g=2, max_p=4, A=19, null=None):
    ptr = [p] * 14
    if null is not None:
        ptr[null] = None
    return lib.univs_hota_counts(ptr[0], ptr[1], ptr[2], D, G, T, ptr[3], ptr[4], ptr[5], ptr[6], C, max_g, max_p, ptr[7], A, *ptr[8:], None)


@pytest.mark.parametrize("bad", [dict(D=0), dict(G=0), dict(T=0), dict(C=0), dict(A=0), dict(max_g=-1), dict(max_p=-1)])
def test_bad_sizes_are_invalid_arguments(host, bad):
    lib = _lib.load()
    assert _counts_entry(lib, host, **bad) == _lib.ERR_INVALID_ARGUMENT
    v = dict(dict(D=5, G=3, T=2, C=2, max_g=2, max_p=4, A=19), **bad)
    assert lib.univs_last_error().decode() == ("univs_hota_counts: bad arguments D={D} G={G} T={T} C={C} max_g={max_g} max_p={max_p} "
                                               "A={A}").format(**v)
    assert lib.univs_lsa_max_f64(host, host, host, -1, host, None) == _lib.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("null", range(14))
def test_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _counts_entry(lib, host, null=null) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == "univs_hota_counts: NULL data pointer"
    if null < 4:
        ptr = [host] * 4
        ptr[null] = None
        assert lib.univs_lsa_max_f64(ptr[0], ptr[1], ptr[2], 3, ptr[3], None) == _lib.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("beyond", [dict(max_g=65), dict(max_p=65), dict(A=33), dict(T=65536), dict(D=2048, G=2048, T=512)])
def test_beyond_its_bounds_the_entry_answers_not_implemented_before_any_launch(host, beyond):
    lib = _lib.load()
    assert _counts_entry(lib, host, **beyond) == _lib.ERR_NOT_IMPLEMENTED
    assert lib.univs_last_error().decode() == f"univs_hota_counts: {COVERED}"


def test_no_problems_is_success_without_a_launch():
    assert _lib.load().univs_lsa_max_f64(None, None, None, 0, None, None) == _lib.OK
