"""CPU: the integer rule of the test-time resize (univs_amd/data/resize_rule.py) equals `PIL.Image.resize(BILINEAR)` bit for bit, on
the machine's Pillow and on the bytes recorded from Pillow 12.2.0 (tests/golden/g32_frames_pil.npz, tools/gen_golden_frames.py); the
tables have the stated form; the size rule gives the worked examples."""
import json
import os

import numpy as np
import pytest

from tests.frames_cases import CASES, GOLDEN_CASES, KINDS, UNCOVERED, case_id, frames
from univs_amd.data.resize_rule import KSIZE_MAX, axis_ksize, resize_tables, resize_u8_reference, shortest_edge_size

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g32_frames_pil.npz")


@pytest.mark.parametrize("case", CASES + UNCOVERED + GOLDEN_CASES[3:8], ids=case_id)
def test_rule_equals_pillow_bit_for_bit(case):
    Image = pytest.importorskip("PIL.Image")
    (T, Hi, Wi), (Ho, Wo) = case
    for kind in KINDS:
        src = frames(kind, T, Hi, Wi)
        for t in range(T):
            want = np.asarray(Image.fromarray(src[t]).resize((Wo, Ho), Image.BILINEAR))
            got = resize_u8_reference(src[t], Ho, Wo)
            assert got.dtype == np.uint8 and got.shape == (Ho, Wo, 3)
            assert np.array_equal(got, want), (kind, t, int(np.abs(got.astype(int) - want).max()))
    gray = frames("noise", 1, Hi, Wi)[0, :, :, 0]                    # a two-dimensional array goes the same way
    assert np.array_equal(resize_u8_reference(gray, Ho, Wo), np.asarray(Image.fromarray(gray).resize((Wo, Ho), Image.BILINEAR)))


def test_rule_equals_the_recorded_pillow_bytes():
    g = np.load(GOLDEN)
    recipe = json.loads(bytes(g["recipe"]).decode())
    assert recipe["cases"] == [case_id(c) for c in GOLDEN_CASES] and recipe["kinds"] == list(KINDS)
    for case in GOLDEN_CASES:
        (T, Hi, Wi), (Ho, Wo) = case
        for kind in KINDS:
            want = g[f"{case_id(case)}/{kind}"]
            src = frames(kind, T, Hi, Wi)
            assert want.shape == (T, Ho, Wo, 3) and want.dtype == np.uint8
            for t in range(T):
                assert np.array_equal(resize_u8_reference(src[t], Ho, Wo), want[t]), (case, kind)


def test_the_intermediate_rounding_is_part_of_the_answer():
    """Horizontal first, uint8 in between: the other order gives other bytes on noise."""
    a = frames("noise", 1, 37, 53)[0]
    assert not np.array_equal(resize_u8_reference(a, 20, 29), resize_u8_reference(resize_u8_reference(a, 20, 53), 20, 29))
    assert np.array_equal(resize_u8_reference(a, 20, 29), resize_u8_reference(resize_u8_reference(a, 37, 29), 20, 29))
    assert np.array_equal(resize_u8_reference(a, 37, 53), a)         # both axes keep their size: no pass


@pytest.mark.parametrize("n_in,n_out", [(53, 29), (53, 106), (7, 96), (1, 3), (160, 80), (128, 32), (96, 7), (64, 1), (1920, 1280), (854, 1139)])
def test_tables_have_the_stated_form(n_in, n_out):
    first, count, coef = resize_tables(n_in, n_out)
    ksize = axis_ksize(n_in, n_out)
    assert first.dtype == count.dtype == coef.dtype == np.int32 and first.shape == count.shape == (n_out,) and coef.shape == (n_out, ksize)
    assert ksize == int(np.ceil(max(n_in / n_out, 1.0))) * 2 + 1
    assert (first >= 0).all() and (count >= 1).all() and (count <= ksize).all() and (first + count <= n_in).all()
    assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()
    assert (coef >= 0).all() and all((coef[i, count[i]:] == 0).all() for i in range(n_out))
    # the weights are normalised before they are rounded: each row sums to 2^22 up to half a unit per tap, so a sum of 255 s stays in 32 bits
    assert (np.abs(coef.sum(1).astype(np.int64) - (1 << 22)) <= count).all()
    assert 255 * int(coef.sum(1).max()) + (1 << 21) < 2 ** 31
    # what the kernel's launcher assumes of one tile of 16 output rows
    span = (first + count)[np.minimum(np.arange(n_out) + 15, n_out - 1)] - first
    assert int(span.max()) <= (15 * n_in + n_out - 1) // n_out + ksize + 1


def test_coverage_constant_is_a_down_scale_of_four():
    assert KSIZE_MAX == 9 == axis_ksize(128, 32) and axis_ksize(129, 32) == 11 and axis_ksize(2160, 720) == 7 and axis_ksize(5, 500) == 3


@pytest.mark.parametrize("args,want", [((720, 1280, 720, 1280), (720, 1280)), ((1080, 1920, 720, 1280), (720, 1280)),
                                       ((480, 854, 640, 1333), (640, 1139)), ((1280, 720, 640, 1024), (1024, 576))])
def test_shortest_edge_size_on_worked_examples(args, want):
    """Restated from detectron2's `ResizeShortestEdge.get_output_shape` and NOT pinned to it: detectron2 is absent, these are worked
    examples of the stated rule."""
    assert shortest_edge_size(*args) == want
