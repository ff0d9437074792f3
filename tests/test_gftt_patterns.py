"""CPU: the designed inputs of tests/gftt_patterns.py take the branches they were designed for, asserted on tests/gftt_restatement.py: counts, which rule fired, that
the tie case has ties, that the seam cases sit on seams, the stop at 200 and the capacity seam."""
import numpy as np
import pytest

from tests import gftt_patterns as gp
from tests import gftt_restatement as gr


def _corners(c):
    return [tuple(int(v) for v in p) for p in c["want"]["corners"]]


def test_sizes():
    assert _corners(gp.size_case(3, 3)) == [(1, 1)]                                          # the one interior pixel
    assert gp.size_case(2, 40)["want"]["n_candidates"] == 0                                   # no pixel has a 3 x 3 neighbourhood
    for w, h in gp.SIZES[2:]:
        c = gp.size_case(w, h)
        xs, ys = c["want"]["corners"][:, 0], c["want"]["corners"][:, 1]
        assert len(xs) >= 4 and c["want"]["n_candidates"] > len(xs)                           # the distance rule drops some
        assert xs.min() <= 3 and ys.min() <= 3 and xs.max() >= w - 4 and ys.max() >= h - 4    # corners beside every border: in the first and in the last, partial tiles
    assert 70 % 10 == 0 and 64 % 10 and 127 % 10                                              # a whole and a partial last column of cells


def test_border_rules():
    c = gp.border_corner_case()
    h, w = c["img"].shape
    dx, dy = gr.derivatives(c["img"])
    assert dx[1, 1] * dy[1, 1] * dx[h - 2, w - 2] * dy[h - 2, w - 2] < 0                      # the two corners' Dx Dy have different signs
    assert {(1, 1), (w - 2, h - 2)} <= set(_corners(c))
    a, b = gr.min_eigen(c["img"]), gr.min_eigen(c["img"], "image")
    assert (a[1:-1, 1:-1] == b[1:-1, 1:-1]).all() and (a[0] != b[0]).any() and (a[:, 0] != b[:, 0]).any()  # the variants differ on the border only
    assert not gp.same_features(c["want"], c["image_variant"])                                # ... which decides the corners
    m = gp.border_maximum_case()
    eig = gr.min_eigen(m["img"])
    assert np.argmax(eig) < eig.shape[1] and m["want"]["max_val"] == eig.max() and m["mask"].all()          # the maximum is on row 0, inside the mask
    assert all(y >= 1 for _, y in _corners(m)) and len(_corners(m)) >= 1
    assert m["want"]["n_candidates"] < gr.good_features(m["img"][1:], None, 200, 0.1, 10.0)["n_candidates"] + 50


def test_mask_rules():
    c = gp.masked_maximum_case()
    assert c["want"]["max_val"] < c["open"]["want"]["max_val"] and c["want"]["threshold"] < c["open"]["want"]["threshold"]
    assert all(c["mask"][y, x] for x, y in _corners(c)) and _corners(c) != _corners(c["open"])
    e = gp.empty_mask_case()
    assert e["want"]["max_val"] == 0 and e["want"]["n_candidates"] == 0 and gr.good_features(e["img"], None, 200, 0.1, 10.0)["n_candidates"] > 0
    f = gp.flat_case()
    assert f["want"]["max_val"] == 0 and f["want"]["n_candidates"] == 0


def test_tie_rule():
    c = gp.tie_case()
    s = c["want"]["sorted"]
    ties = [(a, b) for a, b in zip(s, s[1:]) if a[0] == b[0]]
    assert len(ties) >= 20 and all(a[1] > b[1] for a, b in ties)                              # equal values: the higher raster index first
    first = _corners(c)[0]
    assert first[1] * c["img"].shape[1] + first[0] == s[0][1]


def test_distance_and_seams():
    c = gp.distance_case()
    ax, ay = c["at"]
    assert c["want"]["n_candidates"] == 4 and [i for _, i in c["want"]["sorted"]] == [ay * 64 + ax, (ay - 7) * 64 + ax + 7, (ay + 8) * 64 + ax + 6, ay * 64 + ax - 10]
    assert _corners(c) == [(ax, ay), (ax + 6, ay + 8), (ax - 10, ay)]                        # 100 and 100 kept, 98 dropped
    s = gp.seam_case()
    assert s["want"]["n_candidates"] == 8 and _corners(s) == [(8, 12), (57, 30), (27, 18), (45, 45)]
    dropped = [(13, 14), (62, 33), (32, 22), (45, 52)]
    for (x, y), (u, v) in zip(_corners(s), dropped):
        assert (x // 10, y // 10) != (u // 10, v // 10) and (x - u) ** 2 + (y - v) ** 2 < 100  # each pair straddles a seam of the grid
    assert 62 // 10 == 6 and 64 - 60 < 10                                                     # ... one of them the last, partial column
    assert (27 // 10, 18 // 10) == (2, 1) and (32 // 10, 22 // 10) == (3, 2)                # ... one diagonal


def test_stop_and_counts():
    c = gp.stop_case()
    assert c["want"]["n_candidates"] == 224 and len(_corners(c)) == 200 and 200 % 64 != 0
    assert gr.select_all_pairs(c["want"]["sorted"], c["img"].shape[1], 0, 5.0).__len__() == 224  # every one is acceptable: the stop is the only limit
    assert _corners(c) == [(i % 100, i // 100) for _, i in c["want"]["sorted"][:200]]
    assert gp.count_case(64)["want"]["n_candidates"] == 64 and gp.count_case(65)["want"]["n_candidates"] == 65
    assert len(_corners(gp.count_case(65))) == 65
    b = gp.batch_case()
    assert [len(_corners(x)) for x in b["cases"]] == [0, 1, 199, 200, 200] and b["cases"][4]["want"]["n_candidates"] == 224


def test_capacity_seam():
    c = gp.capacity_case(0)
    assert c["want"]["n_candidates"] == gr.MAX_CANDIDATES == 8192 and len(_corners(c)) == 200
    assert len({v for v, _ in c["want"]["sorted"]}) == 1                                      # one value: the order is the raster index, descending
    over = gp.capacity_case(1)
    with pytest.raises(gr.Capacity) as e:
        gr.good_features(over["img"], None, 200, 0.1, 10.0)
    assert e.value.args[0] == gr.MAX_CANDIDATES + 1 == over["n_candidates"]


def test_mask_building_branches():
    o0, o1, o2 = (gp.mask_order_case(k) for k in range(3))
    assert o0["trace"] == [(0, "drawn"), (1, "zero")] and o1["trace"] == [(1, "drawn"), (0, "zero")] and o2["trace"] == [(0, "drawn"), (1, "zero")]
    assert (o0["want"]["good"] != o1["want"]["good"]).any() and (o0["want"]["good"] == o2["want"]["good"]).all()
    assert o0["want"]["pts"].tobytes() != o1["want"]["pts"].tobytes()                         # ... and so do the corners
    e = gp.mask_edge_case()
    assert [t for _, t in e["trace"]] == ["zero", "drawn", "outside", "outside"] + ["drawn"] * 6 and e["want"]["n_mask_outside"] == 2
    good, obj = e["want"]["good"], e["objmask"]
    assert gr.cv_round(gp.MW - 0.4) == gp.MW and obj[34, 0] == 1                              # x rounds to cols: the pixel read is (0, 34)
    assert good[33, gp.MW - 1] == 0 and good[33, gp.MW - 11] == 255 and obj[33, gp.MW - 11] == 2   # ... and the disc is centred on column `cols`: 10 columns of it are in the image
    assert good[40, 0] == 0 and good[0, 25] == 0 and good[45, gp.MW - 1] == 0 and good[gp.MH - 1, 70] == 0 and good[gp.MH - 1, gp.MW - 1] == 0  # clipped at every border and a corner
    assert good[45, 30] == 255 and good[46, 30] == 0 and good[66, 30] == 0 and good[67, 30] == 255 and obj[45, 30] == 1   # (30.5, 55.5) rounds to (30, 56): rows 46 .. 66
    assert good[56, 19] == 255 and good[56, 20] == 0 and good[56, 39] == 0 and obj[56, 39] == 1                           # ... columns from 20 on (31 would start at 21)
    for c in (o0, e):
        assert all(c["want"]["good"][int(y), int(x)] == 255 for x, y in c["want"]["pts"])     # no new corner in a drawn disc or on the background


def test_new_point_branches():
    two, behind, missing = gp.depth_case("two"), gp.depth_case("behind"), gp.depth_case("missing")
    w = two["want"]
    assert set(w["object_id"]) == {0, 1} and w["x3D_valid"].all()
    assert {round(float(z), 3) for z in (w["x3D"][:, 2] - gp.TWC[2, 3])} == {2.5, 4.0}        # the pose's third row is (0, 0, 1 | 2): z is the cuboid's depth
    assert not behind["want"]["x3D_valid"].any() and not behind["want"]["x3D"].any() and behind["want"]["pts"].tobytes() == w["pts"].tobytes()
    assert missing["want"] is None                                                            # object 1 has no cuboid
