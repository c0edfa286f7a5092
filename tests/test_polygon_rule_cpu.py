"""CPU: the polygon rule (univs_amd/data/polygon_rule.py).  The anchors and the integer rectangles pin the literal rule; the parity form
and the numpy formulation are the literal rule on the whole corpus of tests/polygon_cases.py; the conditions the corpus has to meet are
asserted; the four refusals."""
import numpy as np
import pytest

from tests import polygon_cases as cases
from univs_amd.data import polygon_rule as rule


def test_anchors():
    assert rule.polygon_counts([0.5, 0.5, 5.5, 1.0, 3.0, 6.2], 7, 6) == [8, 2, 5, 4, 3, 4, 3, 2, 11]
    assert rule.polygon_counts([-3, -2, 9, -2, 9, 12, -3, 12], 7, 6) == [0, 42]
    assert rule.polygon_counts([1, 2, 4, 2, 4, 5, 1, 5], 7, 6) == [9, 3, 4, 3, 4, 3, 16]      # columns 1..3, rows 2..4: by hand


def test_integer_rectangles_exhaustively():
    h, w = 8, 9
    objects, masks = [], []
    for x0 in range(w + 1):
        for x1 in range(x0 + 1, w + 1):
            for y0 in range(h + 1):
                for y1 in range(y0 + 1, h + 1):
                    objects.append([[x0, y0, x1, y0, x1, y1, x0, y1]])
                    m = np.zeros((h, w), bool)
                    m[y0:y1, x0:x1] = True
                    masks.append(m)
    assert len(objects) == 45 * 36
    runs = rule.runs_from_polygons_host(objects, [(h, w)] * len(objects))
    b, ones, s = (x.numpy() for x in runs)
    for i, (obj, m) in enumerate(zip(objects, masks)):
        assert (rule.dense_from_counts(rule.polygon_counts(obj[0], h, w), h, w) == m).all(), obj
        assert list(b[s[i]:s[i + 1]]) == rule.boundaries_from_dense(m), obj
        assert ones[s[i + 1] - 1] == m.sum()


def test_the_corpus_meets_its_conditions():
    objects, sizes = cases.objects_and_sizes()
    names = cases.names()
    assert len(set(names)) == len(names) and sum(n.startswith("edge_") for n in names) == 49 * 49
    assert all(h in cases.SIZES and w in cases.SIZES for n, _, (h, w) in cases.corpus() if not n.startswith(("comb", "at_cap", "above_cap")))
    assert len(set(sizes)) > 30                                          # mixed within the one call
    crossings, points, verts = rule.crossing_counts(*rule.pack(objects, sizes))
    at = dict(zip(names, crossings.tolist()))
    assert [at[f"comb_crossings_{c}"] for c in (62, 64, 66, 254, 256, 258)] == [62, 64, 66, 254, 256, 258]
    assert at["at_cap"] == rule.MAX_CROSSINGS and at["above_cap"] == rule.MAX_CROSSINGS + 2
    assert sorted(n for n, c in at.items() if c > rule.MAX_CROSSINGS) == ["above_cap"]
    assert points.max() <= rule.MAX_POINTS and verts.max() <= rule.MAX_VERTS and verts.max() >= 300
    stored = cases.expected().starts.diff().tolist()
    at = dict(zip(names, stored))
    assert [at[f"comb_stored_{c}"] for c in (63, 64, 65, 255, 256, 257)] == [63, 64, 65, 255, 256, 257]
    assert at["absent"] == 0 and at["empty_mask"] == 1 and at["all_one_point"] == 1
    assert any(len(o) == k for o in objects for k in (2, 3, 4))


def test_the_crossing_count_from_the_vertices_is_the_count_of_recorded_positions():
    objects, sizes = cases.objects_and_sizes()
    crossings = rule.crossing_counts(*rule.pack(objects, sizes))[0]
    for i in range(0, len(objects), 7):
        assert crossings[i] == sum(len(rule._positions(np.asarray(xy, float), *sizes[i])) for xy in objects[i]), cases.names()[i]


def test_literal_rule_parity_form_and_host_formulation_agree_on_the_corpus():
    runs = cases.expected()
    b, ones, s = (x.numpy() for x in runs)
    assert runs.starts.numel() == len(cases.corpus()) + 1 and s[-1] == b.shape[0] == ones.shape[0]
    for i, (name, polygons, (h, w)) in enumerate(cases.corpus()):
        got = list(b[s[i]:s[i + 1]])
        if len(polygons) == 1:
            literal = list(np.cumsum(rule.polygon_counts(polygons[0], h, w)))
            assert literal == rule.polygon_boundaries_parity(polygons[0], h, w) == got, name
        else:
            assert rule.object_runs(polygons, h, w) == got, name                      # the union cases: against the dense OR
        if got:
            dense = np.repeat(np.arange(len(got)) % 2 == 1, np.diff([0] + got))
            assert list(ones[s[i]:s[i + 1]]) == [int(dense[:k].sum()) for k in got], name
            assert got[-1] == h * w and all(x < y for x, y in zip(got, got[1:])), name


def test_batches_do_not_change_the_result():
    objects, sizes = cases.objects_and_sizes()
    a, b = cases.expected(), rule.runs_from_polygons_host(objects[2300:], sizes[2300:], batch_points=3000)
    lo = int(a.starts[2300])
    assert (a.bounds[lo:] == b.bounds).all() and (a.ones[lo:] == b.ones).all() and (a.starts[2300:] - lo == b.starts).all()


@pytest.mark.parametrize("xy,why", [([1, 2, 3, 4, 5, 6, 7], "an odd count"), ([1, 2, 3, 4], "fewer than 3 points"),
                                    ([1, 2, 3, float("nan"), 5, 6], "non-finite"), ([1, 2, float("inf"), 4, 5, 6], "non-finite"),
                                    ([1, 2, 3, 4, 5, 2.0 ** 24 + 2], "beyond 2\\^24"), ([1, -2.0 ** 25, 3, 4, 5, 6], "beyond 2\\^24")])
def test_the_four_refusals_name_the_annotation(xy, why):
    with pytest.raises(ValueError, match=why):
        rule.polygon_counts(xy, 7, 7)
    with pytest.raises(ValueError, match="annotation 17, polygon 1: .*" + why):
        rule.runs_from_polygons_host([[[1, 1, 5, 1, 5, 5]], [[1, 1, 5, 1, 5, 5], xy]], [(7, 7), (7, 7)], names=["annotation 16", "annotation 17"])
    assert rule.check_polygon([1, 2, 3, 4, 5, 2.0 ** 24]).shape == (6,)               # the bound itself is accepted
