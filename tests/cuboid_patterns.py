"""Frames and boxes that put the image stages of the cuboid detector (Canny with union-find hysteresis, the distance-transform kernels, the 16-bit chamfer
codes of cuboid_sweep_score) where a test wants them.  A helper, not a test module: it reads nothing but its arguments, draws with constants, and the only
generators with a seed are the project's own (synth.texture_image, synth.cuboid_scene, orb_patterns.noise).  tests/test_cuboid_patterns.py proves every
precondition against the CPU oracle; tests/test_cuboid_edges_gpu.py asserts them again and compares the kernels' maps.

Grey levels.  A straight step of s grey levels has the Sobel L1 magnitude 4 s: WEAK = 30 gives 120, between the default thresholds 80 / 200 (a candidate that
is an edge only if its component holds a strong pixel); STRONG = 150 gives 600.  The strongest response of a STRONG patch is its convex corner pixel, 900.

The host rules restated here (cube_slam_amd/csrc/cuboid.hip): plan_build (box -> ROI, box_proposal_detail.cpp:107-161), plan_derived and cs_cuboid_batch_run
(which distance-transform kernel a batch runs), score_unit_fits (which ROIs are resident as codes)."""
import numpy as np

from cube_slam_amd import synth
from tests import orb_patterns

CC_BAND = 4096                # pixels per workgroup of cuboid_canny_cc_local
BG, WEAK, STRONG = 100, 30, 150
DT_HV, DT_DIAG = 62587, 89738  # chamfer steps * 65536
SC_MAP_ENTRIES = 80864         # 16-bit codes one CU keeps
SC_ESC_D = 244.0               # a pixel at or past it has no code
DT_RUNGS = (4, 5, 6, 8, 10, 12, 16, 20)
DT_KERNELS = tuple("dt_wave<%d>" % c for c in DT_RUNGS) + ("dt_block", "dt")


# ------------------------------------------------------------------------------------------------ host rules
def roi_of_box(box, W, H):
    """(x, y, w, h) of the ROI plan_build gives a box [x y w h ...] without height sampling."""
    left, top, bw, bh = int(box[0]), int(box[1]), int(box[2]), int(box[3])
    right = int(left + box[2])
    ew = min(max(min(20, bw - 100), 10), max(min(20, bh - 100), 10))
    x, r = max(0, left - ew), min(W - 1, right + ew)
    y, b = max(0, top - ew), min(H - 1, top + bh + ew)
    return x, y, r - x, b - y


def box_for_roi(x, y, w, h, W, H):
    """A box whose ROI is exactly (x, y, w, h), nothing clipped."""
    for ew in range(10, 21):
        box = [x + ew, y + ew, w - 2 * ew, h - 2 * ew, 0.9]
        if box[2] > 0 and box[3] > 0 and roi_of_box(box, W, H) == (x, y, w, h):
            return box
    raise ValueError("no box gives the ROI %r" % ((x, y, w, h),))


def dt_kernel(max_roi_w, mode="wave"):
    """The distance-transform kernel of a batch, a function of its widest ROI and CUBESLAM_DT: plan_derived picks the first rung with 64 C >= width (none past
    1 280, none at all in block mode); cs_cuboid_batch_run then launches cuboid_dt_wave<C>, else cuboid_dt_block up to 1 024 columns, else the serial cuboid_dt."""
    need = (max_roi_w + 63) // 64
    c = next((c for c in DT_RUNGS if c >= need), 0)
    if mode == "block":
        c = 0
    if c:
        return "dt_wave<%d>" % c
    return "dt_block" if max_roi_w <= 1024 else "dt"


def score_unit_fits(w, h):
    """cuboid.hip score_unit_fits: the code map and the w + 2 (at least 8) entries that repeat its last pixel fit one CU."""
    return w * h + max(w + 2, 8) <= SC_MAP_ENTRIES


def chamfer_ij(d):
    """(i, j) with d * 65536 = i * DT_HV + j * DT_DIAG, integers only; unique for d < 256 (tests/test_cabi.py::test_chamfer_code_number_theory)."""
    t = int(round(float(d) * 65536))
    assert t == float(d) * 65536
    for j in range(0, t // DT_DIAG + 1):
        if (t - j * DT_DIAG) % DT_HV == 0:
            return (t - j * DT_DIAG) // DT_HV, j
    raise ValueError("%r is no chamfer distance" % d)


# ------------------------------------------------------------------------------------------------ what a test asks of a map
def components(edges):
    """Number of 8-connected components of the non-zero pixels (a plain flood fill)."""
    h, w = edges.shape
    pw = w + 2
    free = bytearray((np.pad(edges != 0, 1)).astype(np.uint8).tobytes())
    nb = (-pw - 1, -pw, -pw + 1, -1, 1, pw - 1, pw, pw + 1)
    n = 0
    for p in np.flatnonzero(np.pad(edges != 0, 1)).tolist():
        if not free[p]:
            continue
        n += 1
        free[p] = 0
        stack = [p]
        while stack:
            q = stack.pop()
            for d in nb:
                if free[q + d]:
                    free[q + d] = 0
                    stack.append(q + d)
    return n


def bands(edges):
    """(bands of CC_BAND consecutive ROI pixels that hold a non-zero pixel, bands of the ROI)."""
    p = np.flatnonzero(edges)
    return len(np.unique(p // CC_BAND)), (edges.size + CC_BAND - 1) // CC_BAND


def candidates(oracle, gray, roi, low=80):
    """The non-maximum-suppressed pixels above `low`, strong or weak: Canny with both thresholds at `low` keeps every one of them."""
    return oracle.canny_roi(gray, *roi, low=low, high=low)


# ------------------------------------------------------------------------------------------------ hysteresis
SERP_W, SERP_H, SERP_ROI = 640, 480, (13, 9, 601, 447)


def serpentine(W=SERP_W, H=SERP_H, rect=(40, 30, 590, 440), seeded="far", thick=6, pitch=16):
    """A boustrophedon stripe WEAK above a flat ground over rect = (x0, y0, x1, y1): runs `thick` high every `pitch` rows, joined alternately at the right and the
    left end.  seeded = "far": one patch STRONG above ground at the stripe's last end (the bottom: the component's only strong pixels have its highest ids);
    "near": at its first end (the lowest ids); None: no patch -- the twin, all of whose candidates are weak."""
    img = np.full((H, W), BG, np.uint8)
    x0, y0, x1, y1 = rect
    ys = list(range(y0, y1 - thick + 1, pitch))
    for k, y in enumerate(ys):
        img[y:y + thick, x0:x1] = BG + WEAK
        if k + 1 < len(ys):
            xs = x1 - thick if k % 2 == 0 else x0
            img[y:y + pitch + thick, xs:xs + thick] = BG + WEAK
    if seeded == "far":
        xs = x0 if (len(ys) - 1) % 2 == 1 else x1 - thick
        img[ys[-1]:ys[-1] + thick, xs:xs + thick] = BG + STRONG
    elif seeded == "near":
        img[ys[0]:ys[0] + thick, x0:x0 + thick] = BG + STRONG
    else:
        assert seeded is None
    return img


WRAP_KINDS = ("W", "NE", "NW")


def row_wrap(W, H, roi, y, kind, joined=False, span=100):
    """-> (image, (column, row) of the strong pixel, (column, row) of the weak pixel), ROI coordinates.  A STRONG block with a horizontal edge that runs out of the
    ROI on one side and a WEAK block with a horizontal edge that runs out on the other side, `span` columns of each inside, placed so that the two end pixels are
    neighbours in memory (row-major ROI) and not in the image; the union-find's column guards are all that keeps them apart:
      kind "W":  strong through (w - 1, y), weak through (0, y + 1): the weak pixel's p - 1      (guard x > 0)
      kind "NE": strong through (0, y),     weak through (w - 1, y): the weak pixel's p - w + 1  (guard x + 1 < w)
      kind "NW": strong through (w - 1, y), weak through (0, y + 2): the weak pixel's p - w - 1  (guard x > 0)
    The blocks are w - 2 span columns apart, so the weak edge is no edge.  joined = True is the twin: the weak block lies in the strong one's rows and up against it,
    the two edges are one line, and the weak edge is kept."""
    rx, ry, w, h = roi
    assert kind in WRAP_KINDS and 2 * span + 8 < w and ry + y >= 26 and 1 <= y < h - 30 and rx >= 8 and rx + w + 8 <= W
    img = np.full((H, W), BG, np.uint8)
    left, right = (rx - 8, rx + span), (rx + w - span, rx + w + 8)
    if kind == "NE":  # both blocks hang below their upper edge; the edge row is the row above the first bright row
        rows = slice(ry + y + 1, ry + y + 27)
        img[rows, (left[1] - 20 if joined else right[0]):right[1]] = BG + WEAK
        img[rows, left[0]:left[1]] = BG + STRONG
        return img, (0, y), (w - 1, y)
    y_w = y + (1 if kind == "W" else 2)
    img[ry + y - 25:ry + y + 1, right[0]:right[1]] = BG + STRONG                                 # lower edge: the last bright row is the edge row
    if joined:  # the weak block in the strong one's rows and up against it: one lower edge along row y
        img[ry + y - 25:ry + y + 1, left[0]:right[0]] = BG + WEAK
        return img, (w - 1, y), (0, y)
    img[ry + y_w + 1:ry + y_w + 27, left[0]:left[1]] = BG + WEAK                                 # upper edge: the row above the first bright row
    return img, (w - 1, y), (0, y_w)


# ------------------------------------------------------------------------------------------------ dense frames
# ROI shapes (w, h): widths around one wave; 4096 % w == 0 with the last band exactly full (64 x 64, 256 x 128); the last band holding 1 and 16 pixels
DENSE_SHAPES = [(63, 65), (64, 64), (65, 63), (256, 128), (113, 145), (240, 239)]
DENSE_WIDE = (2200, 100, (20, 10, 2100, 70))  # frame and a ROI wider than half a band: a band holds less than two rows


def dense_frame(kind, W=640, H=480):
    if kind == "texture":
        return synth.texture_image(11, W, H)
    if kind == "noise":
        return orb_patterns.noise(W, H, 3)
    assert kind == "scene"
    return synth.cuboid_scene(21, W=W, H=H, n_boxes=3, bg_texture=0.5)["gray"]


def dense_boxes(W=640, H=480):
    """-> (boxes, the ROIs they must give): DENSE_SHAPES side by side inside the frame, then one ROI clipped at each image border (left, top, right, bottom)."""
    assert all(1 <= (w * h) % CC_BAND <= 16 for w, h in DENSE_SHAPES[4:]) and all((w * h) % CC_BAND == 0 for w, h in DENSE_SHAPES[1:4:2])
    rois, x = [], 30
    for k, (w, h) in enumerate(DENSE_SHAPES):
        rois.append((x % (W - w - 60) + 30, 40 + 30 * k, w, h))
        x += w + 37
    boxes = [box_for_roi(*r, W, H) for r in rois]
    for b in ([5, 200, 150, 150, 0.9], [200, 5, 150, 150, 0.9], [W - 160, 150, 159, 150, 0.9], [300, H - 180, 150, 179, 0.9]):
        boxes.append(b)
        rois.append(roi_of_box(b, W, H))
    return np.array(boxes, np.float64), rois


# ------------------------------------------------------------------------------------------------ distance-transform ladder
LADDER_W, LADDER_H = 1400, 264
LADDER_X, LADDER_Y, LADDER_ROI_H = 8, 12, 240


def ladder_widths():
    """Per rung C: one past the rung below, 64 C - 1 and 64 C; 1 280 is the last rung's 64 C, 1 281 goes to the serial kernel."""
    out, prev = [255, 256], 4
    for c in DT_RUNGS[1:]:
        out += [64 * prev + 1, 64 * c - 1, 64 * c]
        prev = c
    return out + [1281]


LADDER_BLOCK_WIDTHS = [704, 1023, 1024, 1025]


def ladder_boxes(w):
    """-> (boxes, ROIs): the wide ROI of width w and three narrow ones that ride along under its C -- 63 wide over its top-left corner, 65 wide over its bottom-right
    corner, 130 wide in its middle."""
    W, H, x, y, h = LADDER_W, LADDER_H, LADDER_X, LADDER_Y, LADDER_ROI_H
    rois = [(x, y, w, h), (x, y, 63, 100), (x + w - 65, y + h - 100, 65, 100), (x + w // 2 - 65, y + 60, 130, 120)]
    return np.array([box_for_roi(*r, W, H) for r in rois], np.float64), rois


def ladder_sparse(w):
    """Flat ground with isolated bright squares and one vertical bar, all within 16 pixels of the wide ROI's top-left and bottom-right corners; the two corner squares
    straddle the ROI's corners, so their edges cross column 0, row 0, column w - 1 and row h - 1.  Everything between is farther from an edge than any code reaches,
    and a pixel's distance is carried across every lane of the wave."""
    img = np.full((LADDER_H, LADDER_W), BG, np.uint8)
    x0, y0, x1, y1 = LADDER_X, LADDER_Y, LADDER_X + w, LADDER_Y + LADDER_ROI_H
    img[y0 - 4:y0 + 5, x0 - 4:x0 + 5] = 250
    img[y0 + 1:y0 + 15, x0 + 12:x0 + 14] = 250   # the bar
    img[y0 + 10:y0 + 13, x0 + 4:x0 + 7] = 250
    img[y1 - 5:y1 + 4, x1 - 5:x1 + 4] = 250
    img[y1 - 12:y1 - 9, x1 - 14:x1 - 11] = 250
    return img


def ladder_textured(w):
    """A 1/f texture, flat over the left third of the wide ROI (and everything left of it): distances grow across a third of the ROI, then edges everywhere."""
    img = synth.texture_image(5, LADDER_W, LADDER_H).copy()
    img[:, :LADDER_X + w // 3] = 128
    return img


# ------------------------------------------------------------------------------------------------ codes at their limit
# The geometry (K, pose, lines, box columns) is synth.cuboid_scene(70)'s; the pixels are a flat ground with one step edge across the frame, so that every distance in a
# ROI is the chamfer distance to one line: pure straight steps to a horizontal edge, pure diagonal steps to an anti-diagonal one.  (A small square cannot do it: the
# box lies 20 pixels inside its ROI on every side the image does not clip, 20 diagonal steps are 27.4 px, and the band [217, 244) is 27 px wide -- with the ROI's far
# corner below 244 no corner of a proposal would reach 217.  A line puts a whole box edge into the band, and a ROI clipped by the image puts the box's edge on the ROI's:
# the proposals' corners then sample the ROI's largest distances themselves, so the codes at the top of the table are decoded, not only encoded.)
LIMIT_SEED = 70


def limit_scene():
    return synth.cuboid_scene(LIMIT_SEED, n_boxes=3)


def limit_straight(scene, bi, dy, W=640, H=480):
    """-> (image, box): the columns of box bi of the scene from the image's first row down, so that the ROI is clipped at the top and the box's upper edge -- where two
    corners of every proposal lie -- is the ROI's first row, and a horizontal step dy rows below it (bright from there down)."""
    bx = scene["boxes"][bi]
    assert dy + 5 <= H - 1
    box = np.array([bx[0], 0, bx[2], max(int(bx[1]) + int(bx[3]), dy + 5 - 20), 0.9])
    img = np.full((H, W), 128, np.uint8)
    img[dy:] = 250
    return img, box


LIMIT_DIAG_BOX = np.array([0, 0, 200, 240, 0.9])  # in the image's top-left corner: the ROI is clipped at the left and the top, the box's corner is the ROI's


def limit_diagonal(c, W=640, H=480):
    """-> (image, box): an anti-diagonal step x + y >= c (bright below it) and LIMIT_DIAG_BOX; the ROI's far corner is the image's origin."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.full((H, W), 128, np.uint8)
    img[xx + yy >= c] = 250
    return img, LIMIT_DIAG_BOX.copy()


def corner_distances(rows, roi, dist):
    """Distance-map values under the 8 corners of every debug row (columns 9..24: x0..x7, y0..y7), corners on x == w / y == h left out."""
    cor = np.asarray(rows)[:, 9:25].reshape(-1, 2, 8)
    cx, cy = (cor[:, 0, :] - roi[0]).astype(np.int64), (cor[:, 1, :] - roi[1]).astype(np.int64)
    ok = (cx >= 0) & (cy >= 0) & (cx < roi[2]) & (cy < roi[3])
    return dist[cy[ok], cx[ok]]


def corners_on_the_far_border(rows, roi):
    """Corners with x - roi_x == roi_w or y - roi_y == roi_h: the samples past the map that take the clamp."""
    cor = np.asarray(rows)[:, 9:25].reshape(-1, 2, 8)
    cx, cy = (cor[:, 0, :] - roi[0]).astype(np.int64), (cor[:, 1, :] - roi[1]).astype(np.int64)
    return int(((cx == roi[2]) | (cy == roi[3])).sum())


# ------------------------------------------------------------------------------------------------ residency boundary, clamp
def residency_heights(w):
    """(h, h + 1): the tallest ROI of width w that score_unit_fits keeps resident, and the first that it does not."""
    h = (SC_MAP_ENTRIES - max(w + 2, 8)) // w
    assert score_unit_fits(w, h) and not score_unit_fits(w, h + 1)
    return h, h + 1


def clamp_box(W=640, H=480, bw=401, bh=301):
    """A box whose right edge is the last column and whose bottom is the last row (tests/test_cuboid_gpu.py::test_edge_cases does it for a small one): its ROI ends on
    W - 1 / H - 1, is too large to be resident, and its pixel count is odd, so the float after the map is padding."""
    return np.array([W - 1 - bw, H - 1 - bh, bw, bh, 0.9])


def clamp_escape_image(W=640, H=480):
    """Flat but for one square far from the clamp box's bottom-right corner: the ROI has edges and pixels without a code."""
    img = np.full((H, W), 128, np.uint8)
    img[170:182, 230:242] = 250
    return img


# ------------------------------------------------------------------------------------------------ cases and their preconditions (oracle only)
# Shared by tests/test_cuboid_patterns.py (no device) and tests/test_cuboid_edges_gpu.py, which asserts them again from the ROIs the batch reports.
WRAP_W, WRAP_H = 640, 480
# (roi, y, kind, seam): seam = the pair straddles a band seam, so cuboid_canny_cc_border's guards decide instead of cuboid_canny_cc_local's
WRAP_CASES = [((37, 21, 333, 250), 100, "W", False), ((37, 21, 333, 250), 100, "NE", False), ((37, 21, 333, 250), 100, "NW", False),
              ((37, 21, 320, 250), 63, "W", True), ((37, 21, 333, 250), 12, "NE", True), ((37, 21, 333, 250), 11, "NW", True)]
THRESHOLD_CASES = [(50, 100, "all"), (1000, 1200, "none"), (130, 300, "patch")]


def pre_serpentine(oracle, gray, roi, seeded):
    """Seeded: one 8-connected component, in at least 90 % of the ROI's bands, whose strong pixels all lie past (far) / before (near) nine tenths of its pixels in
    id order.  Unseeded: candidates and no edge."""
    e = oracle.canny_roi(gray, *roi)
    cand = np.flatnonzero(candidates(oracle, gray, roi))
    assert len(cand) > 20000
    if seeded is None:
        assert not e.any()
        return e
    assert components(e) == 1 and np.array_equal(np.flatnonzero(e), cand)
    nb, total = bands(e)
    assert total >= 60 and nb >= 0.9 * total, (nb, total)
    strong = np.flatnonzero(oracle.canny_roi(gray, *roi, low=200, high=200))
    assert 0 < len(strong) < 100
    if seeded == "far":
        assert strong.min() > cand[int(0.9 * len(cand))]
    else:
        assert strong.max() < cand[int(0.1 * len(cand))]
    return e


def wrap_seam(roi, kind, p_weak):
    """Is the weak pixel's memory neighbour of this kind in the band in front of the pixel's own, with the pixel among the band's first w + 1?"""
    w = roi[2]
    x, y = p_weak
    p = y * w + x
    n = p + {"W": -1, "NE": -w + 1, "NW": -w - 1}[kind]
    p0b = p // CC_BAND * CC_BAND
    return p0b > 0 and n < p0b and p - p0b <= w


def pre_row_wrap(oracle, roi, y, kind, seam):
    """-> (apart, joined) images.  Apart: both end pixels are candidates, the strong one is an edge, the weak block's half of the ROI has no edge.  Joined: it has."""
    w = roi[2]
    assert CC_BAND % w != 0
    apart, ps, pw = row_wrap(WRAP_W, WRAP_H, roi, y, kind)
    assert abs(ps[0] - pw[0]) == w - 1 and wrap_seam(roi, kind, pw) == seam
    if kind == "W" and seam:
        assert (pw[1] * w) % CC_BAND == 0  # the weak pixel opens a band
    half = (slice(None), slice(0, w // 2)) if pw[0] == 0 else (slice(None), slice(w - w // 2, w))
    c, e = candidates(oracle, apart, roi), oracle.canny_roi(apart, *roi)
    assert c[ps[1], ps[0]] and c[pw[1], pw[0]] and e[ps[1], ps[0]] == 255
    assert c[half].any() and not e[half].any()
    joined, _, pj = row_wrap(WRAP_W, WRAP_H, roi, y, kind, joined=True)
    ej = oracle.canny_roi(joined, *roi)
    assert ej[pj[1], pj[0]] == 255 and np.count_nonzero(ej[half]) > 100 and np.count_nonzero(ej) > 2 * np.count_nonzero(e)
    return apart, joined


def pre_dense(oracle, kind, gray, rois):
    dens = [float(np.count_nonzero(oracle.canny_roi(gray, *r))) / (r[2] * r[3]) for r in rois]
    if kind != "scene":
        assert min(dens) > 0.2, dens
    return dens


def pre_thresholds(oracle, gray, roi, low, high, what):
    e = oracle.canny_roi(gray, *roi, low=low, high=high)
    n, n_default = np.count_nonzero(e), np.count_nonzero(oracle.canny_roi(gray, *roi))
    if what == "all":  # every candidate of the stripe is strong by itself
        assert n >= n_default > 20000 and np.array_equal(e, oracle.canny_roi(gray, *roi, low=high, high=high))
    elif what == "none":
        assert n == 0
    else:  # only the patch is left
        assert 0 < n < 100
    return e


def pre_ladder_sparse(oracle, gray, roi):
    e, d = oracle.canny_roi(gray, *roi), oracle.canny_dt_roi(gray, *roi)
    assert e[:, 0].any() and e[:, -1].any() and e[0].any() and e[-1].any()
    assert d.max() > 200 and np.count_nonzero(e) < 400
    return d


def pre_ladder_textured(oracle, gray, roi):
    e, d = oracle.canny_roi(gray, *roi), oracle.canny_dt_roi(gray, *roi)
    w = roi[2]
    assert not e[:, :w // 3 - 2].any() and np.count_nonzero(e[:, w // 3 + 2:]) > 0.2 * e[:, w // 3 + 2:].size
    assert d.max() > 0.9 * (w // 3)  # the flat third's distances are carried all the way from the texture
    return d


LADDER_CASES = [(w, "wave") for w in ladder_widths()] + [(w, "block") for w in LADDER_BLOCK_WIDTHS]
assert {dt_kernel(w, m) for w, m in LADDER_CASES} == set(DT_KERNELS), "the ladder cases name every distance-transform kernel"


def limit_find(oracle, make, positions, want):
    """The first position whose (image, box) gives a ROI map that `want` accepts -> (image, box, roi, map)."""
    for pos in positions:
        img, box = make(pos)
        roi = roi_of_box(box, img.shape[1], img.shape[0])
        d = oracle.canny_dt_roi(img, *roi)
        if want(d):
            return img, box, roi, d
    raise AssertionError("no position gives the wanted range")


def near_limit(d):
    return 236.0 <= d.max() < SC_ESC_D


def limit_straight_case(oracle, scene, bi, kind):
    """kind "near": ROI maximum in [236, 244) with i >= 250; "below": within 1 px below 244; "escape": a pixel at or past 244 in a ROI that has edges."""
    want = {"near": lambda d: near_limit(d) and chamfer_ij(d.max())[0] >= 250, "below": lambda d: SC_ESC_D - 1 <= d.max() < SC_ESC_D,
            "escape": lambda d: SC_ESC_D <= d.max() < 1000}[kind]
    img, box, roi, d = limit_find(oracle, lambda dy: limit_straight(scene, bi, dy), range(240, 262), want)
    assert np.count_nonzero(oracle.canny_roi(img, *roi)) >= roi[2]  # an edge across the whole ROI
    return img, box, roi, d


def limit_diagonal_case(oracle):
    img, box, roi, d = limit_find(oracle, limit_diagonal, range(300, 420), lambda d: near_limit(d) and chamfer_ij(d.max())[1] >= 170)
    assert roi[:2] == (0, 0)
    return img, box, roi, d


def pre_corners_in_band(rows, roi, d, n_min=32):
    cd = corner_distances(rows, roi, d)
    n = int(np.count_nonzero((cd >= 217.0) & (cd < SC_ESC_D)))
    assert n >= n_min, n
    return n


RESIDENCY_W = 280
CLAMP_TEXTURE_SEED = 13


def residency_case():
    """-> (image, boxes, ROIs): two textured ROIs of one width, the tallest that is resident and one row more."""
    W, H = 640, 480
    h0, h1 = residency_heights(RESIDENCY_W)
    rois = [(150, 60, RESIDENCY_W, h0), (190, 70, RESIDENCY_W, h1)]
    return synth.texture_image(11, W, H), np.array([box_for_roi(*r, W, H) for r in rois]), rois


def clamp_case(kind):
    """-> (image, box, roi): the clamp box on a texture, or on the flat frame whose one square leaves its ROI pixels without a code."""
    img = synth.texture_image(CLAMP_TEXTURE_SEED, 640, 480) if kind == "texture" else clamp_escape_image()
    box = clamp_box()
    return img, box, roi_of_box(box, 640, 480)


def pre_clamp(oracle, kind, img, roi, rows):
    W, H = img.shape[1], img.shape[0]
    assert roi[0] + roi[2] == W - 1 and roi[1] + roi[3] == H - 1 and not score_unit_fits(roi[2], roi[3]) and (roi[2] * roi[3]) % 64 != 0
    assert corners_on_the_far_border(rows, roi) >= 1
    d = oracle.canny_dt_roi(img, *roi)
    assert d[-1, -1] > 0  # the clamp's value differs from the zero padding behind the map
    if kind == "escape":
        assert d.max() >= SC_ESC_D and oracle.canny_roi(img, *roi).any()
    else:
        assert d.max() < SC_ESC_D
    return d
