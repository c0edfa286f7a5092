"""CPU: the NEAREST rule of univs_amd/data/resize_rule.py (`nearest_table`, `resize_nearest`) equals `PIL.Image.resize(NEAREST)` element
for element, is not the closed form, and reproduces the recorded bytes of tests/golden/g33_prompt_masks_pil.npz."""
import json
import os

import numpy as np
import pytest

from tests import prompt_masks_cases as pc
from univs_amd.data import nearest_table, resize_nearest
from univs_amd.evaluation.vis_counts import runs_from_rles

PAIRS = [(2, 7), (2, 15), (7, 2), (1, 5), (5, 1), (1, 1), (9, 9), (64, 64)]
_rng = np.random.default_rng(20261020)
RANDOM_PAIRS = [tuple(int(v) for v in _rng.integers(1, 400, 2)) for _ in range(40)]


def closed_form(n_in, n_out):
    return np.floor((np.arange(n_out) + 0.5) * (n_in / n_out)).astype(np.int32)


def check(in_hw, out_hw, seed=0):
    m = pc.mask("noise", *in_hw, seed=seed)
    got = resize_nearest(m, *out_hw)
    assert got.dtype == np.uint8 and got.shape == tuple(out_hw) and got.flags.c_contiguous
    assert np.array_equal(got, pc.pillow_resize(m, out_hw)), (in_hw, out_hw)


@pytest.mark.parametrize("n_in,n_out", PAIRS + RANDOM_PAIRS)
def test_rule_equals_pillow_on_either_axis(n_in, n_out):
    t = nearest_table(n_in, n_out)
    assert t.dtype == np.int32 and t.shape == (n_out,) and t.min() >= 0 and t.max() < n_in and (np.diff(t) >= 0).all()
    check((n_in, 5), (n_out, 9))
    check((6, n_in), (4, n_out), seed=1)
    check((n_in, n_in), (n_out, n_out), seed=2)


@pytest.mark.parametrize("in_hw,out_hw", [((480, 854), (720, 1280)), ((1080, 1920), (720, 1280))])
def test_rule_equals_pillow_at_the_sizes_of_the_data_sets(in_hw, out_hw):
    check(in_hw, out_hw)


def test_the_closed_form_is_not_pillows_table():
    """Pillow accumulates the source coordinate by repeated addition; floor((i + 0.5) n_in / n_out) differs from that at 2 -> 7, and
    Pillow agrees with the accumulated table."""
    assert nearest_table(2, 7).tolist() == [0, 0, 0, 0, 1, 1, 1]
    assert closed_form(2, 7).tolist() == [0, 0, 0, 1, 1, 1, 1]
    column = np.array([[0], [1]], np.uint8)
    assert pc.pillow_resize(column, (7, 1))[:, 0].tolist() == nearest_table(2, 7).tolist()
    differing = sum(not np.array_equal(nearest_table(a, b), closed_form(a, b)) for a in range(1, 40) for b in range(1, 40))
    assert differing > 0


def test_bad_sizes_raise():
    with pytest.raises(ValueError):
        nearest_table(0, 4)
    with pytest.raises(ValueError):
        nearest_table(4, 0)
    with pytest.raises(ValueError):
        resize_nearest(np.zeros(4, np.uint8), 2, 2)


@pytest.mark.parametrize("case", pc.GOLDEN_CASES, ids=pc.case_id)
def test_recorded_pillow_bytes_are_reproduced(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "g33_prompt_masks_pil.npz"))
    assert json.loads(bytes(g["recipe"]).decode())["cases"] == [pc.case_id(c) for c in pc.GOLDEN_CASES]
    (kind, H, W), out_hw = case
    name = pc.case_id(case)
    m = pc.mask(kind, H, W)
    assert pc.counts_of(m) == g[f"{name}/counts"].tolist()          # the stored code is the closed-form mask's
    runs_from_rles([pc.code_of(m)], H, W)                           # ... and a valid one
    got = resize_nearest(m, *out_hw)
    assert np.array_equal(got, g[f"{name}/mask"])
    assert np.array_equal(pc.any_boxes(got[None])[0], g[f"{name}/box"])
