"""The inputs of tests/test_cuboid_edges_gpu.py are what that file says they are: every drawer of tests/cuboid_patterns.py, for every case of the GPU file, against
the CPU oracle alone.  No device is needed, so the GPU cases' preconditions can be checked anywhere; the GPU file asserts them again from the ROIs a batch reports."""
import numpy as np
import pytest

from tests import cuboid_patterns as cp


def test_host_rules_restated():
    """The ROI of a box, the ladder and the residency rule as tests/cuboid_patterns.py restates them: fixed points worked out by hand from cuboid.hip."""
    assert cp.roi_of_box([33, 29, 561, 407, 0.9], 640, 480) == cp.SERP_ROI
    assert cp.roi_of_box([440, 150, 199, 329, 0.5], 640, 480) == (420, 130, 219, 349)  # clipped at the right and the bottom
    assert cp.roi_of_box([300, 100, 8, 150, 0.5], 640, 480) == (290, 90, 28, 170)      # a thin box: 10 pixels around it
    for r in [(60, 40, 63, 65), (8, 12, 1281, 240)]:
        assert cp.roi_of_box(cp.box_for_roi(*r, 1400, 264), 1400, 264) == r
    assert [cp.dt_kernel(w) for w in (1, 256, 257, 320, 321, 1280, 1281)] == ["dt_wave<4>", "dt_wave<4>", "dt_wave<5>", "dt_wave<5>", "dt_wave<6>", "dt_wave<20>", "dt"]
    assert [cp.dt_kernel(w, "block") for w in (189, 1024, 1025, 1236)] == ["dt_block", "dt_block", "dt", "dt"]
    assert cp.residency_heights(280) == (287, 288) and cp.score_unit_fits(281, 286) and not cp.score_unit_fits(600, 440)
    for i, j in [(255, 0), (0, 178), (3, 172), (100, 99)]:  # (all below 2^24: a float holds them exactly)
        assert cp.chamfer_ij(np.float32((i * cp.DT_HV + j * cp.DT_DIAG) / 65536.0)) == (i, j)


def test_components_and_bands():
    e = np.zeros((40, 300), np.uint8)
    e[3, 5:200] = 255; e[4, 200] = 255; e[20, 0] = 255; e[19, 299] = 255  # a line with a diagonal step; two pixels that are neighbours in memory only
    assert cp.components(e) == 3 and cp.bands(e) == (2, 3)


@pytest.mark.parametrize("seeded", ["far", "near", None])
def test_serpentine(oracle, seeded):
    assert cp.roi_of_box(cp.box_for_roi(*cp.SERP_ROI, cp.SERP_W, cp.SERP_H), cp.SERP_W, cp.SERP_H) == cp.SERP_ROI
    cp.pre_serpentine(oracle, cp.serpentine(seeded=seeded), cp.SERP_ROI, seeded)


@pytest.mark.parametrize("roi,y,kind,seam", cp.WRAP_CASES)
def test_row_wrap(oracle, roi, y, kind, seam):
    cp.pre_row_wrap(oracle, roi, y, kind, seam)


@pytest.mark.parametrize("kind", ["texture", "noise", "scene"])
def test_dense(oracle, kind):
    boxes, rois = cp.dense_boxes()
    assert [cp.roi_of_box(b, 640, 480) for b in boxes] == rois
    assert [r[2] for r in rois[:4]] == [63, 64, 65, 256] and rois[6][0] == 0 and rois[7][1] == 0 and rois[8][0] + rois[8][2] == 639 and rois[9][1] + rois[9][3] == 479
    cp.pre_dense(oracle, kind, cp.dense_frame(kind), rois)


def test_dense_wide(oracle):
    W, H, roi = cp.DENSE_WIDE
    assert roi[2] > cp.CC_BAND // 2 and cp.dt_kernel(roi[2]) == "dt"
    cp.pre_dense(oracle, "noise", cp.orb_patterns.noise(W, H, 4), [roi])


@pytest.mark.parametrize("low,high,what", cp.THRESHOLD_CASES)
def test_thresholds(oracle, low, high, what):
    cp.pre_thresholds(oracle, cp.serpentine(seeded="far"), cp.SERP_ROI, low, high, what)


@pytest.mark.parametrize("w,mode", cp.LADDER_CASES)
def test_ladder(oracle, w, mode):
    boxes, rois = cp.ladder_boxes(w)
    assert [cp.roi_of_box(b, cp.LADDER_W, cp.LADDER_H) for b in boxes] == rois
    assert max(r[2] for r in rois) == w and rois[1][2] < 64 and rois[2][2] == 65
    cp.pre_ladder_sparse(oracle, cp.ladder_sparse(w), rois[0])
    cp.pre_ladder_textured(oracle, cp.ladder_textured(w), rois[0])


def test_codes_near_the_limit(oracle):
    s = cp.limit_scene()
    for case in ("straight", "diagonal"):
        img, box, roi, d = cp.limit_straight_case(oracle, s, 0, "near") if case == "straight" else cp.limit_diagonal_case(oracle)
        i, j = cp.chamfer_ij(d.max())
        assert (i >= 250) if case == "straight" else (j >= 170)
        _, dbg = oracle.detect_cuboid(img, s["K"], s["Twc"], box[None], s["lines"], debug=True)
        assert dbg["row_count"][0] > 0
        cp.pre_corners_in_band(dbg["rows"], roi, d)


def test_escape_among_edges(oracle):
    s = cp.limit_scene()
    maxima = [cp.limit_straight_case(oracle, s, bi, kind)[3].max() for bi, kind in enumerate(("near", "below", "escape"))]
    assert maxima[0] < maxima[1] < cp.SC_ESC_D <= maxima[2] and maxima[1] >= cp.SC_ESC_D - 1


def test_residency_and_clamp(oracle):
    s = cp.limit_scene()
    img, boxes, rois = cp.residency_case()
    assert [cp.roi_of_box(b, 640, 480) for b in boxes] == rois and cp.score_unit_fits(*rois[0][2:]) and not cp.score_unit_fits(*rois[1][2:])
    _, dbg = oracle.detect_cuboid(img, s["K"], s["Twc"], boxes, s["lines"], debug=True)
    assert min(dbg["row_count"][:2]) > 0
    for kind in ("texture", "escape"):
        img, box, roi = cp.clamp_case(kind)
        _, dbg = oracle.detect_cuboid(img, s["K"], s["Twc"], box[None], s["lines"], debug=True)
        cp.pre_clamp(oracle, kind, img, roi, dbg["rows"])
