"""GPU parity of the cuboid detector's image stages with the CPU oracle, bit for bit, where tests/test_cuboid_gpu.py does not go: hysteresis components that
cross dozens of band seams and are seeded from either end, candidates that are neighbours in memory and not in the image, dense edge maps in ROIs around one wave /
one band / half a band wide, Canny thresholds other than the default, every distance-transform kernel at both ends of its width range with distances carried across
the whole ROI, chamfer codes at the top of their range, a unit that leaves the codes because of one far pixel among edges, the residency boundary of
score_unit_fits and the clamp of samples on x == w / y == h.

Every case: build a CuboidBatch, run it, read every unit; assert the case's precondition from the ROI the batch reports and the ORACLE's maps (the drawers and the
preconditions are tests/cuboid_patterns.py's, proven without a device by tests/test_cuboid_patterns.py); assert edges == oracle.canny_roi and dist ==
oracle.canny_dt_roi with array_equal for every unit; where proposals matter, the comparisons of tests/test_cuboid_gpu.py::test_batch_stages_match_oracle, imported.
No pixel may differ and nothing is skipped.

Not yet run on a device: no MI355X was available when this file was written.  The preconditions hold on the oracle (tests/test_cuboid_patterns.py); the kernels'
side of every comparison, and the mutations each group is meant to catch, are unverified."""
import numpy as np
import pytest

from cube_slam_amd.cuboid import CuboidBatch, detect_3d_cuboid
from tests import cuboid_patterns as cp
from tests.test_cuboid_gpu import REL, _cmp_cuboids, _oracle_opts

pytestmark = pytest.mark.gpu

NO_LINES = np.zeros((0, 4))


@pytest.fixture(scope="module")
def scene():
    return cp.limit_scene()


def _run(ctx, scene, grays, boxes_list, lines=None, det=None, low=None, high=None, timed=None):
    """One batch over grays[f] with boxes_list[f] (no height sampling: one unit per box) -> (units, cuboids, score_stats, launches of the kernel `timed`)."""
    det = det or detect_3d_cuboid(ctx)
    det.set_calibration(scene["K"])
    o = det.opts()
    if low is not None:
        o.canny_low, o.canny_high = low, high
    F = len(grays)
    b = CuboidBatch(ctx, np.stack(grays), scene["K"], np.stack([scene["Twc"]] * F), boxes_list, [NO_LINES if lines is None else lines] * F, o)
    n_timed = None
    if timed:
        ctx.timing(True); ctx.timing_reset()
    try:
        b.run()
        if timed:
            n_timed = ctx.timing_get(timed)[1]
    finally:
        if timed:
            ctx.timing(False)
    n_units = sum(len(bx) for bx in boxes_list)
    assert b.stats()["n_units"] == n_units
    units = [b.unit(u) for u in range(n_units)]
    got, ss = b.read(), b.score_stats()
    b.close()
    return units, got, ss, n_timed


def _check_maps(oracle, units, grays, rois=None, low=80, high=200):
    """Every unit's edge map and distance map equal the oracle's over the ROI the batch reports (and that ROI is the one the case was drawn for)."""
    if rois is not None:
        assert [u["roi"] for u in units] == [tuple(r) for r in rois]
    for k, info in enumerate(units):
        x, y, w, h = info["roi"]
        g = grays[info["frame"]]
        assert np.array_equal(info["edges"], oracle.canny_roi(g, x, y, w, h, low, high)), "canny, unit %d, ROI %r" % (k, info["roi"])
        assert np.array_equal(info["dist"], oracle.canny_dt_roi(g, x, y, w, h, low, high)), "distance transform, unit %d, ROI %r" % (k, info["roi"])


def _check_proposals(oracle, ctx, scene, units, got, grays, boxes_list, lines):
    """n_valid, the integer columns of the rows, the rows and the cuboids against the oracle: test_batch_stages_match_oracle's comparisons.  -> the oracle's rows per unit."""
    oo = _oracle_opts(oracle, detect_3d_cuboid(ctx))
    ref, per_unit, u = [], [], 0
    for g, boxes in zip(grays, boxes_list):
        r, dbg = oracle.detect_cuboid(g, scene["K"], scene["Twc"], boxes, lines, opts=oo, debug=True)
        ref += r
        row0 = 0
        for seg in range(len(boxes)):
            info = units[u]
            assert info["n_hs"] == 1
            n = int(dbg["row_count"][seg])
            rows_ref = dbg["rows"][row0:row0 + n]
            assert info["n_valid"] == n, (info["n_valid"], n)
            assert np.array_equal(info["rows"][:, [0, 1, 3, 6]], rows_ref[:, [0, 1, 3, 6]])
            assert np.allclose(info["rows"], rows_ref, rtol=REL, atol=1e-9)
            per_unit.append(rows_ref)
            row0 += n
            u += 1
    _cmp_cuboids(got, ref)
    return per_unit


# ------------------------------------------------------------------------------------------------ 1. hysteresis
@pytest.mark.parametrize("form", ["far", "near", "twins"])
def test_serpentine(ctx, oracle, scene, form):
    """One weak component of 29 012 pixels through 61 of the ROI's 66 bands, made an edge by a 22-pixel strong patch at its far end (the highest ids: the root has to
    travel back through every band seam) or at its near end; and a batch in which the full ROI's arena neighbours are the unseeded twin's empty ones.  The border
    kernel is shown to have run."""
    seeds = {"far": ["far"], "near": ["near"], "twins": ["far", None, "near", None]}[form]
    grays = [cp.serpentine(seeded=s) for s in seeds]
    box = cp.box_for_roi(*cp.SERP_ROI, cp.SERP_W, cp.SERP_H)
    units, _, _, n_border = _run(ctx, scene, grays, [[box]] * len(grays), timed="cuboid_canny_cc_border")
    for info, s in zip(units, seeds):
        assert info["roi"] == cp.SERP_ROI
        e = cp.pre_serpentine(oracle, grays[info["frame"]], info["roi"], s)
        assert (np.count_nonzero(e) == 0) == (s is None)
    _check_maps(oracle, units, grays)
    assert n_border == 1, "cuboid_canny_cc_border ran"


@pytest.mark.parametrize("roi,y,kind,seam", cp.WRAP_CASES)
def test_row_wrap(ctx, oracle, scene, roi, y, kind, seam):
    """A strong edge that ends in the last column of one row and a weak edge that starts in the first column of a following row (or the same row, for the NE pair):
    neighbours in memory only.  The weak edge must vanish; in the twin, where the two blocks touch, it must stay.  seam: the pair straddles a band seam."""
    apart, joined = cp.pre_row_wrap(oracle, roi, y, kind, seam)
    box = cp.box_for_roi(*roi, cp.WRAP_W, cp.WRAP_H)
    units, _, _, n_border = _run(ctx, scene, [apart, joined], [[box], [box]], timed="cuboid_canny_cc_border")
    _check_maps(oracle, units, [apart, joined], [roi, roi])
    assert n_border == 1, "cuboid_canny_cc_border ran"


@pytest.mark.parametrize("kind", ["texture", "noise", "scene"])
def test_dense_frames(ctx, oracle, scene, kind):
    """Edge densities of 30 % and more (asserted for the texture and the noise) in ROIs 63, 64 and 65 wide, one whose rows divide a band and fill the last one
    exactly, two whose last band holds 1 and 16 pixels, and one clipped at each image border."""
    gray = cp.dense_frame(kind)
    boxes, rois = cp.dense_boxes()
    units, _, _, _ = _run(ctx, scene, [gray], [boxes])
    assert [u["roi"] for u in units] == rois
    cp.pre_dense(oracle, kind, gray, [u["roi"] for u in units])
    _check_maps(oracle, units, [gray], rois)


def test_dense_wide_roi(ctx, oracle, scene):
    """A ROI 2 100 wide in a 2 200-wide noise frame: a band holds less than two rows, so a pixel's upper neighbours lie one and two bands back; the serial distance
    transform runs with more than 64 KB of row buffers."""
    W, H, roi = cp.DENSE_WIDE
    gray = cp.orb_patterns.noise(W, H, 4)
    units, _, _, _ = _run(ctx, scene, [gray], [[cp.box_for_roi(*roi, W, H)]])
    assert units[0]["roi"] == roi and roi[2] > cp.CC_BAND // 2 and cp.dt_kernel(roi[2]) == "dt"
    cp.pre_dense(oracle, "noise", gray, [roi])
    _check_maps(oracle, units, [gray])


@pytest.mark.parametrize("low,high,what", cp.THRESHOLD_CASES)
def test_canny_thresholds(ctx, oracle, scene, low, high, what):
    """canny_low / canny_high of the options reach the kernels: a pair under which every pixel of the serpentine is strong, one that leaves nothing, one that leaves the patch."""
    gray = cp.serpentine(seeded="far")
    units, _, _, _ = _run(ctx, scene, [gray], [[cp.box_for_roi(*cp.SERP_ROI, cp.SERP_W, cp.SERP_H)]], low=low, high=high)
    cp.pre_thresholds(oracle, gray, units[0]["roi"], low, high, what)
    _check_maps(oracle, units, [gray], [cp.SERP_ROI], low, high)


# ------------------------------------------------------------------------------------------------ 2. distance-transform ladder
@pytest.mark.parametrize("w,mode", cp.LADDER_CASES)
def test_distance_transform_ladder(ctx, oracle, scene, monkeypatch, w, mode):
    """The widest ROI of a batch picks the kernel (cp.dt_kernel restates plan_derived and cs_cuboid_batch_run): cuboid_dt_wave<4 .. 20> at one past the rung below, at
    64 C - 1 and at 64 C; the serial cuboid_dt from 1 281; under CUBESLAM_DT=block cuboid_dt_block with 11 and 16 waves and the serial kernel from 1 025.  Three narrow
    ROIs (63, 65 and 130 wide) ride along under the wide one's C.  Two frames per width, one batch each: a sparse one whose few edges sit in the wide ROI's corners and
    on its border rows and columns (every other pixel's distance is carried across the lanes: maximum above 200 px), and a texture with a flat third."""
    if mode == "block":
        monkeypatch.setenv("CUBESLAM_DT", "block")
    boxes, rois = cp.ladder_boxes(w)
    for gray, pre in ((cp.ladder_sparse(w), cp.pre_ladder_sparse), (cp.ladder_textured(w), cp.pre_ladder_textured)):
        units, _, _, n_dt = _run(ctx, scene, [gray], [boxes], timed="cuboid_dt")
        assert n_dt == 1
        widths = [u["roi"][2] for u in units]
        assert widths == [w, 63, 65, 130]
        pre(oracle, gray, units[0]["roi"])
        _check_maps(oracle, units, [gray], rois)


# ------------------------------------------------------------------------------------------------ 3. codes at their limit, the escape among edges
def _assert_ij(d, straight):
    i, j = cp.chamfer_ij(d.max())
    assert (i >= 250) if straight else (j >= 170), (i, j)


@pytest.mark.parametrize("case", ["straight", "diagonal"])
def test_codes_near_the_limit(ctx, oracle, scene, case):
    """The ROI's largest distance lies in [236, 244) -- 250 or more straight steps, or 170 or more diagonal ones: the top of sc_encode2's table -- every unit is scored
    from codes, and at least 32 corners of the oracle's proposals fall on pixels between 217 and 244 px."""
    img, box, roi, d = cp.limit_straight_case(oracle, scene, 0, "near") if case == "straight" else cp.limit_diagonal_case(oracle)
    _assert_ij(d, case == "straight")
    units, got, ss, _ = _run(ctx, scene, [img], [box[None]], lines=scene["lines"])
    assert units[0]["roi"] == roi
    assert ss["float_units"] == 0 and ss["code_units"] == 1
    _check_maps(oracle, units, [img])
    rows = _check_proposals(oracle, ctx, scene, units, got, [img], [box[None]], scene["lines"])
    cp.pre_corners_in_band(rows[0], roi, d)
    assert len(got[0]) >= 1


def test_escape_among_edges(ctx, oracle, scene):
    """One batch, three units with an edge across each ROI: the largest distance 250 straight steps, within 1 px below 244, and at or past 244.  Only the last leaves the
    codes -- because of its far pixels, not because its map is empty."""
    cases = [cp.limit_straight_case(oracle, scene, bi, kind) for bi, kind in enumerate(("near", "below", "escape"))]
    grays, boxes_list = [c[0] for c in cases], [c[1][None] for c in cases]
    units, got, ss, _ = _run(ctx, scene, grays, boxes_list, lines=scene["lines"])
    for info, (img, box, roi, d) in zip(units, cases):
        assert info["roi"] == roi and np.count_nonzero(oracle.canny_roi(img, *roi)) >= roi[2]
    assert cases[0][3].max() < cases[1][3].max() < cp.SC_ESC_D <= cases[2][3].max() and cases[1][3].max() >= cp.SC_ESC_D - 1
    _check_maps(oracle, units, grays)
    rows = _check_proposals(oracle, ctx, scene, units, got, grays, boxes_list, scene["lines"])
    for r, (img, box, roi, d) in zip(rows, cases):
        cp.pre_corners_in_band(r, roi, d)
    assert ss["float_units"] == 1 and ss["code_units"] == 2


# ------------------------------------------------------------------------------------------------ 4. residency boundary, clamp
def test_residency_boundary(ctx, oracle, scene):
    """score_unit_fits: w h + max(w + 2, 8) <= 80 864.  Two textured ROIs 280 wide in one batch, 287 rows (resident) and 288 rows (the map would fit, the entries that
    repeat its last pixel would not: partly resident)."""
    img, boxes, rois = cp.residency_case()
    units, got, ss, _ = _run(ctx, scene, [img], [boxes], lines=scene["lines"])
    (w0, h0), (w1, h1) = units[0]["roi"][2:], units[1]["roi"][2:]
    assert w0 == w1 and h1 == h0 + 1 and cp.score_unit_fits(w0, h0) and not cp.score_unit_fits(w1, h1)
    assert ss["float_units"] == 0 and ss["code_units"] == 2
    _check_maps(oracle, units, [img], rois)
    rows = _check_proposals(oracle, ctx, scene, units, got, [img], [boxes], scene["lines"])
    assert min(len(r) for r in rows) > 0


@pytest.mark.parametrize("kind", ["texture", "escape"])
def test_clamp_of_a_clipped_roi(ctx, oracle, scene, kind):
    """A box whose right edge is the last column and whose bottom is the last row, its ROI too large to be resident: corners on x == w / y == h index past the map and
    take min(idx, a_last) -- with a textured map (the head in LDS, the tail and the clamp from the float map) and with a map that holds pixels without a code."""
    img, box, _ = cp.clamp_case(kind)
    units, got, ss, _ = _run(ctx, scene, [img], [box[None]], lines=scene["lines"])
    roi = units[0]["roi"]
    assert ss["float_units"] == (1 if kind == "escape" else 0)
    _check_maps(oracle, units, [img])
    rows = _check_proposals(oracle, ctx, scene, units, got, [img], [box[None]], scene["lines"])
    cp.pre_clamp(oracle, kind, img, roi, rows[0])
