"""TEST INFRASTRUCTURE: an independent numpy restatement of cv::calcOpticalFlowPyrLK as ORBmatcher::SearchByTrackingHarris / SearchByTracking call it (reference
orb_object_slam/src/ORBmatcher.cc:1548 / :1620: 8-bit single-channel images, Size(21, 21), maxLevel 3, the default criteria, flags and minEigThreshold), and of
SearchByTrackingHarris' selection pass (:1556-1579).  Nothing here is shared with the product: the float sums whose order matters are plain loops, the integer
sampling (exact in any order) is numpy slices.

OpenCV is neither in the reference tree nor installed, so the function is a STATED DEFINITION: the plain C++ (non-SIMD) branches of OpenCV 3.x
modules/video/src/lkpyramid.cpp, recalled and not checked against a build.  A SIMD build of OpenCV adds the same terms of A11, A12, A22, b1 and b2 in another order
(four or eight partial sums), so its floats can differ from these in the last bits.  To re-check against a real build: run
cv2.calcOpticalFlowPyrLK(prev, next, pts, None, winSize=(21, 21), maxLevel=3) with cv2.setUseOptimized(False) on the frames and points of tests/klt_patterns.py (lk_case, edge_case, batch_case) and compare status
exactly and nextPts / err to the last few ulps (exactly on a build without SIMD).

Inputs and defaults: maxLevel = 3, window 21 x 21, 30 iterations, epsilon = 0.01 used squared (in double), flags = 0, minEigThreshold = 1e-4.

Pyramid: level 0 is the image, level l + 1 is pyrDown of level l to ((w + 1) / 2, (h + 1) / 2): 5 x 5 [1 4 6 4 1]^2, (sum + 128) >> 8, REFLECT_101 on source
coordinates.  Building stops, and maxLevel drops, at the first level with w <= 21 || h <= 21.  Every level is padded by 21 on all sides with REFLECT_101.

Derivatives (calcSharrDeriv): int16, interleaved (Ix, Iy).  Vertical pass t0 = (r0 + r2) * 3 + r1 * 10, t1 = r2 - r0; horizontal pass Ix = t0[x + 1] - t0[x - 1],
Iy = (t1[x + 1] + t1[x - 1]) * 3 + t1[x] * 10; rows and columns at the image edge by REFLECT_101; the result is padded by 21 with constant 0.

Per point, for each level from maxLevel down to 0:
  prevPt = pt * (float)(1. / (1 << level)); nextPt = prevPt at the top level, otherwise nextPts * 2.f; nextPts = nextPt.
  prevPt -= (10, 10); iprev = cvFloor(prevPt).  If iprev.x < -21 || iprev.x >= cols || iprev.y < -21 || iprev.y >= rows: at level 0 only status = 0 and err = 0;
  continue.
  Weights with a, b the fractional parts: iw00 = cvRound((1 - a)(1 - b) 2^14), iw01 = cvRound(a (1 - b) 2^14), iw10 = cvRound((1 - a) b 2^14),
  iw11 = 2^14 - iw00 - iw01 - iw10; cvRound is round-half-even.
  Window samples over 21 x 21, row-major: ival = DESCALE(sum of 4 taps, 9); ixval, iyval = DESCALE(sum of 4 taps, 14); DESCALE(v, n) = (v + (1 << (n - 1))) >> n;
  all three stored as short.
  A11 += (float)(ixval * ixval), A12 and A22 likewise: float accumulators, summed in that order, then each multiplied by 1.f / (1 << 20).
  D = A11 * A22 - A12 * A12; minEig = (A22 + A11 - sqrt((A11 - A22)^2 + 4 A12^2)) / (2 * 21 * 21).
  If minEig < 1e-4 || D < FLT_EPSILON: status = 0 at level 0, continue.  Otherwise D = 1.f / D.
  nextPt -= (10, 10).
  Iterations, up to 30: the same range test on cvFloor(nextPt), on failure status = 0 at level 0 and break; the weights again;
  diff = DESCALE(J taps, 9) - I; b1 += (float)(diff * Ix), b2 += (float)(diff * Iy) in window order, then both times 1.f / (1 << 20);
  delta = ((A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D); nextPt += delta; nextPts = nextPt + (10, 10); break when delta . delta (in double) <= 0.01 * 0.01;
  for j > 0 with |delta.x + prevDelta.x| < 0.01 and |delta.y + prevDelta.y| < 0.01: nextPts -= delta * 0.5f, break.
  err, at level 0 while status is set, at nextPts - (10, 10): out of range -> status = 0; otherwise err = (sum of (float)|diff|, in window order) * 1.f / (32 * 21 * 21),
  which C reads as (sum * 1.f) / 14112.
"""
import numpy as np

f32 = np.float32
WIN, HALF, MAX_LEVEL, MAX_ITERS = 21, f32(10.0), 3, 30
EPS2 = 0.01 * 0.01  # criteria.epsilon *= criteria.epsilon, a double
MIN_EIG = 1e-4
FLT_EPSILON = float(np.finfo(np.float32).eps)
FLT_SCALE = f32(1.0 / (1 << 20))
W14 = 1 << 14


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101)."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def pyr_down(img):
    """cv::pyrDown of an 8-bit image to ((w + 1) / 2, (h + 1) / 2)."""
    h, w = img.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    src = img.astype(np.int32)
    k = (1, 4, 6, 4, 1)
    acc = np.zeros((dh, dw), np.int32)
    for i in range(5):
        rows = [reflect101(2 * y + i - 2, h) for y in range(dh)]
        for j in range(5):
            cols = [reflect101(2 * x + j - 2, w) for x in range(dw)]
            acc += k[i] * k[j] * src[np.ix_(rows, cols)]
    return ((acc + 128) >> 8).astype(np.uint8)


def pad_reflect101(img, n=WIN):
    h, w = img.shape
    rows = [reflect101(y - n, h) for y in range(h + 2 * n)]
    cols = [reflect101(x - n, w) for x in range(w + 2 * n)]
    return img[np.ix_(rows, cols)]


def scharr_deriv(img):
    """calcSharrDeriv: int16 [h, w, 2] = (Ix, Iy), unpadded."""
    h, w = img.shape
    s = img.astype(np.int32)
    up = s[[reflect101(y - 1, h) for y in range(h)]]
    down = s[[reflect101(y + 1, h) for y in range(h)]]
    t0 = (up + down) * 3 + s * 10
    t1 = down - up
    left = [reflect101(x - 1, w) for x in range(w)]
    right = [reflect101(x + 1, w) for x in range(w)]
    out = np.zeros((h, w, 2), np.int16)
    out[:, :, 0] = t0[:, right] - t0[:, left]
    out[:, :, 1] = (t1[:, right] + t1[:, left]) * 3 + t1 * 10
    return out


def pad_zero(d, n=WIN):
    h, w, c = d.shape
    out = np.zeros((h + 2 * n, w + 2 * n, c), d.dtype)
    out[n:n + h, n:n + w] = d
    return out


def build_pyramid(img, max_level=MAX_LEVEL):
    """buildOpticalFlowPyramid: the unpadded levels; len() - 1 is the maxLevel that remains."""
    img = np.ascontiguousarray(img, np.uint8)
    levels = [img]
    for _ in range(max_level):
        h, w = levels[-1].shape
        if (w + 1) // 2 <= WIN or (h + 1) // 2 <= WIN:
            break
        levels.append(pyr_down(levels[-1]))
    return levels


def n_levels(w, h, max_level=MAX_LEVEL):
    n = 1
    while n <= max_level and (w + 1) // 2 > WIN and (h + 1) // 2 > WIN:
        w, h, n = (w + 1) // 2, (h + 1) // 2, n + 1
    return n


def _floor(v):
    return int(np.floor(v))


def weights(a, b):
    one = f32(1.0)
    iw00 = int(np.rint((one - a) * (one - b) * f32(W14)))
    iw01 = int(np.rint(a * (one - b) * f32(W14)))
    iw10 = int(np.rint((one - a) * b * f32(W14)))
    return iw00, iw01, iw10, W14 - iw00 - iw01 - iw10


def _taps(p, iw, shift):
    """p: int32 [22, 22(, c)] -> DESCALE of the four weighted taps over 21 x 21."""
    v = p[:-1, :-1] * iw[0] + p[:-1, 1:] * iw[1] + p[1:, :-1] * iw[2] + p[1:, 1:] * iw[3]
    return (v + (1 << (shift - 1))) >> shift


def _in_range(ix, iy, cols, rows):
    return not (ix < -WIN or ix >= cols or iy < -WIN or iy >= rows)


def _seq_sum(values):
    s = f32(0.0)
    for v in values:
        s = f32(s + f32(v))
    return s


class Pyramid:
    """The padded levels and padded derivatives of one frame."""

    def __init__(self, img, max_level=MAX_LEVEL):
        self.levels = build_pyramid(img, max_level)
        self.padded = [pad_reflect101(l).astype(np.int32) for l in self.levels]
        self.deriv = [pad_zero(scharr_deriv(l)).astype(np.int32) for l in self.levels]


def track(prev, nxt, pts, trace=None):
    """calcOpticalFlowPyrLK(prev, nxt, pts, Size(21, 21), 3) -> (nextPts [n, 2] float32, status [n] uint8, err [n] float32).  prev / nxt: uint8 images or Pyramid objects.
    trace: a list that receives one set of branch names per point (tests.klt_patterns asserts its preconditions on them)."""
    P = prev if isinstance(prev, Pyramid) else Pyramid(prev)
    N = nxt if isinstance(nxt, Pyramid) else Pyramid(nxt)
    pts = np.asarray(pts, f32).reshape(-1, 2)
    n = len(pts)
    next_pts = np.zeros((n, 2), f32)
    status = np.ones(n, np.uint8)
    err = np.zeros(n, f32)
    top = len(P.levels) - 1
    for i in range(n):
        seen = set()
        for level in range(top, -1, -1):
            rows, cols = P.levels[level].shape
            scale = f32(1.0 / (1 << level))
            px, py = f32(pts[i, 0] * scale), f32(pts[i, 1] * scale)
            if level == top:
                nx, ny = px, py
            else:
                nx, ny = f32(next_pts[i, 0] * f32(2.0)), f32(next_pts[i, 1] * f32(2.0))
            next_pts[i] = (nx, ny)
            px, py = f32(px - HALF), f32(py - HALF)
            ipx, ipy = _floor(px), _floor(py)
            if not _in_range(ipx, ipy, cols, rows):
                seen.add("prev_outside_level0" if level == 0 else "prev_outside_upper")
                if level == 0:
                    status[i] = 0
                    err[i] = 0
                continue
            a, b = f32(px - f32(ipx)), f32(py - f32(ipy))
            iw = weights(a, b)
            if float(a) == 0.0 or float(b) == 0.0:
                seen.add("weight_zero_fraction")
            for t in ((f32(1) - a) * (f32(1) - b), a * (f32(1) - b), (f32(1) - a) * b):
                if float(f32(t) * f32(W14)) % 1.0 == 0.5:
                    seen.add("weight_round_tie")
            if ipx < 0:
                seen.add("pad_left")
            if ipy < 0:
                seen.add("pad_top")
            if ipx + WIN >= cols:
                seen.add("pad_right")
            if ipy + WIN >= rows:
                seen.add("pad_bottom")
            y0, x0 = ipy + WIN, ipx + WIN  # in the padded level; the window is rows y0 .. y0 + 21, columns x0 .. x0 + 21: ipx in [-21, cols - 1] keeps it inside the pad
            I = _taps(P.padded[level][y0:y0 + 22, x0:x0 + 22], iw, 9).astype(np.int16).astype(np.int32)
            d = _taps(P.deriv[level][y0:y0 + 22, x0:x0 + 22], iw, 14).astype(np.int16).astype(np.int32)
            Ix, Iy = d[:, :, 0].ravel(), d[:, :, 1].ravel()
            I = I.ravel()
            A11 = f32(_seq_sum(Ix * Ix) * FLT_SCALE)
            A12 = f32(_seq_sum(Ix * Iy) * FLT_SCALE)
            A22 = f32(_seq_sum(Iy * Iy) * FLT_SCALE)
            D = f32(f32(A11 * A22) - f32(A12 * A12))
            dA = f32(A11 - A22)
            min_eig = f32(f32(f32(A22 + A11) - np.sqrt(f32(f32(dA * dA) + f32(f32(f32(4.0) * A12) * A12)))) / f32(2 * WIN * WIN))
            if float(min_eig) < MIN_EIG or float(D) < FLT_EPSILON:
                seen.add("min_eig")
                if level == 0:
                    status[i] = 0
                continue
            D = f32(f32(1.0) / D)
            nx, ny = f32(nx - HALF), f32(ny - HALF)
            pdx = pdy = f32(0.0)
            stopped = False
            for j in range(MAX_ITERS):
                inx, iny = _floor(nx), _floor(ny)
                if not _in_range(inx, iny, cols, rows):
                    seen.add("drift_outside")
                    if level == 0:
                        status[i] = 0
                        seen.add("drift_outside_level0")
                    stopped = True
                    break
                a, b = f32(nx - f32(inx)), f32(ny - f32(iny))
                iw = weights(a, b)
                y0, x0 = iny + WIN, inx + WIN
                diff = _taps(N.padded[level][y0:y0 + 22, x0:x0 + 22], iw, 9).ravel() - I
                b1 = f32(_seq_sum(diff * Ix) * FLT_SCALE)
                b2 = f32(_seq_sum(diff * Iy) * FLT_SCALE)
                dx = f32(f32(f32(A12 * b2) - f32(A22 * b1)) * D)
                dy = f32(f32(f32(A12 * b1) - f32(A11 * b2)) * D)
                nx, ny = f32(nx + dx), f32(ny + dy)
                next_pts[i] = (f32(nx + HALF), f32(ny + HALF))
                if float(dx) * float(dx) + float(dy) * float(dy) <= EPS2:
                    seen.add("eps_stop")
                    stopped = True
                    break
                if j > 0 and abs(float(f32(dx + pdx))) < 0.01 and abs(float(f32(dy + pdy))) < 0.01:
                    next_pts[i] = (f32(next_pts[i, 0] - f32(dx * f32(0.5))), f32(next_pts[i, 1] - f32(dy * f32(0.5))))
                    seen.add("oscillation_stop")
                    stopped = True
                    break
                pdx, pdy = dx, dy
            if not stopped:
                seen.add("all_iterations")
            if status[i] and level == 0:
                ex, ey = f32(next_pts[i, 0] - HALF), f32(next_pts[i, 1] - HALF)
                iex, iey = _floor(ex), _floor(ey)
                if not _in_range(iex, iey, cols, rows):
                    seen.add("err_outside")
                    status[i] = 0
                    continue
                a, b = f32(ex - f32(iex)), f32(ey - f32(iey))
                iw = weights(a, b)
                y0, x0 = iey + WIN, iex + WIN
                diff = _taps(N.padded[level][y0:y0 + 22, x0:x0 + 22], iw, 9).ravel() - I
                err[i] = f32(f32(_seq_sum(np.abs(diff)) * f32(1.0)) / f32(32 * WIN * WIN))
        if trace is not None:
            trace.append(seen)
    return next_pts, status, err


def cv_round(v):
    return int(np.rint(f32(v)))


def search_by_tracking_harris(prev, nxt, last_pts, mask, trace=None):
    """ORBmatcher::SearchByTrackingHarris (ORBmatcher.cc:1524-1580) for one pair: last_pts = pt of LastFrame.mvKeysHarris, mask = CurrentFrame.objmask_img (uint8
    [rows, cols]).  Returns a dict: kept (indices into last_pts, for mvpMapPointsHarris), pts (mvKeysHarris of the current frame), object_id (maskval - 1),
    goodmatches, n_mask_outside, featuresklt_lastframe / featuresklt_thisframe, status, err.  The mask lookup is Mat::at<uchar>(Point2f):
    data[cvRound(y) * cols + cvRound(x)], which is the next row's first pixel when x rounds to cols; an index >= rows * cols lies beyond the image in the
    reference: such a point is dropped and counted."""
    last_pts = np.asarray(last_pts, f32).reshape(-1, 2)
    mask = np.ascontiguousarray(mask, np.uint8)
    rows, cols = mask.shape
    flat = mask.ravel()
    if len(last_pts) == 0:
        cur, status, err = np.zeros((0, 2), f32), np.zeros(0, np.uint8), np.zeros(0, f32)
    else:
        cur, status, err = track(prev, nxt, last_pts)
    kept, ids, outside = [], [], 0
    seen = set()
    for i in range(len(last_pts)):
        if not status[i]:
            continue
        x, y = cur[i]
        if x >= 0 and y >= 0 and x < f32(cols) and y < f32(rows):
            cx, cy = cv_round(x), cv_round(y)
            if cx == cols:
                seen.add("x_rounds_to_cols")
            idx = cy * cols + cx
            if idx >= rows * cols:
                outside += 1
                continue
            if flat[idx] == 0:
                seen.add("mask_zero")
                continue
            kept.append(i)
            ids.append(int(flat[idx]) - 1)
        else:
            seen.add("bounds")
    if trace is not None:
        trace.append(seen)
    kept = np.array(kept, np.int32)
    return {"kept": kept, "pts": cur[kept].astype(f32).reshape(-1, 2), "object_id": np.array(ids, np.int32), "goodmatches": len(kept), "n_mask_outside": outside,
            "featuresklt_lastframe": last_pts.copy(), "featuresklt_thisframe": cur, "status": status, "err": err}


# ---- ORBmatcher::SearchByTracking (ORBmatcher.cc:1582-1725) over Frame::GetCloestFeaturesInArea (Frame.cc:461-523) ----
GRID_COLS, GRID_ROWS = 64, 48


def _c_round(v):
    """C round(): halves away from zero"""
    v = float(v)
    return int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))


class FrameGrid:
    """mGrid of Frame::AssignFeaturesToGrid (Frame.cc:303-318) over mvKeysUn: bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY)."""

    def __init__(self, keysUn_pt, octave, bounds):
        self.pt, self.octave, self.N = np.asarray(keysUn_pt, f32).reshape(-1, 2), np.asarray(octave), len(octave)
        self.minX, self.minY = f32(bounds[0]), f32(bounds[2])
        self.wInv = f32(f32(GRID_COLS) / f32(f32(bounds[1]) - f32(bounds[0])))
        self.hInv = f32(f32(GRID_ROWS) / f32(f32(bounds[3]) - f32(bounds[2])))
        self.cells = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
        for i in range(self.N):
            px, py = _c_round(f32(f32(self.pt[i, 0] - self.minX) * self.wInv)), _c_round(f32(f32(self.pt[i, 1] - self.minY) * self.hInv))
            if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
                self.cells[px][py].append(i)

    def closest(self, x, y, r, min_level, max_level, keys_static, seen=None):
        """Frame::GetCloestFeaturesInArea: N + 1 = none."""
        x, y, r = f32(x), f32(y), f32(r)
        none = self.N + 1
        x0 = max(0, int(np.floor(f32(f32(f32(x - self.minX) - r) * self.wInv))))
        x1 = min(GRID_COLS - 1, int(np.ceil(f32(f32(f32(x - self.minX) + r) * self.wInv))))
        y0 = max(0, int(np.floor(f32(f32(f32(y - self.minY) - r) * self.hInv))))
        y1 = min(GRID_ROWS - 1, int(np.ceil(f32(f32(f32(y - self.minY) + r) * self.hInv))))
        if x0 >= GRID_COLS or x1 < 0 or y0 >= GRID_ROWS or y1 < 0:
            return none
        check = min_level > 0 or max_level >= 0
        best, min_dist = none, f32(-1)
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for j in self.cells[ix][iy]:
                    if keys_static is not None and keys_static[j]:
                        continue
                    if check and (self.octave[j] < min_level or (max_level >= 0 and self.octave[j] > max_level)):
                        continue
                    dx, dy = f32(self.pt[j, 0] - x), f32(self.pt[j, 1] - y)
                    if abs(dx) < r and abs(dy) < r:
                        d = f32(f32(dx * dx) + f32(dy * dy))
                        if seen is not None and min_dist != -1 and d == min_dist:
                            seen.add("closest_tie")
                        if min_dist == -1 or d < min_dist:
                            min_dist, best = d, j
        return best


def search_by_tracking(prev, nxt, last_pt, last_octave, eligible, object_id, numobject, th, scale_factors, grid, keys_static=None, had_map_point=None, trace=None):
    """ORBmatcher::SearchByTracking for one pair.  last_pt / last_octave = pt and octave of LastFrame.mvKeys, eligible[i] = the caller's
    `mvpMapPoints[i] && !KeysStatic[i] && mvpMapPoints[i]->is_dynamic`, object_id = LastFrame.keypoint_associate_objectID, grid = the current frame's FrameGrid,
    keys_static / had_map_point = CurrentFrame.KeysStatic / `mvpMapPoints[j] != NULL` before the call (None: empty / all NULL).  Returns train_match [N] (the last
    frame's key index whose map point the current key point takes, -1 none), lastptsinds, featuresklt_lastframe / thisframe and the four counters."""
    seen = set()
    last_pt = np.asarray(last_pt, f32).reshape(-1, 2)
    inds = [i for i in range(len(last_pt)) if eligible[i] and last_octave[i] < 3]
    train = np.full(grid.N, -1, np.int32)
    out = {"train_match": train, "lastptsinds": np.array(inds, np.int32), "featuresklt_lastframe": last_pt[inds].reshape(-1, 2), "featuresklt_thisframe": np.zeros((len(inds), 2), f32),
           "kltmatches": 0, "goodmatches": 0, "findfeaturematches": 0, "uniquematches": 0}
    if not inds:
        return out
    lastobj = last_pt[inds]
    cur, status, _ = track(prev, nxt, lastobj)
    mx, my, cnt = np.zeros(numobject, f32), np.zeros(numobject, f32), np.zeros(numobject, np.int64)
    norm = np.zeros(numobject, f32)
    for i in range(len(inds)):
        if status[i]:
            o = int(object_id[inds[i]])
            if not 0 <= o < numobject:
                raise ValueError("object id %d of a tracked point is outside [0, %d)" % (o, numobject))
            cnt[o] += 1
            mx[o] = f32(mx[o] + f32(cur[i, 0] - lastobj[i, 0]))
            my[o] = f32(my[o] + f32(cur[i, 1] - lastobj[i, 1]))
    with np.errstate(invalid="ignore", divide="ignore"):
        for o in range(numobject):
            if cnt[o] > 0:
                mx[o], my[o] = f32(mx[o] / f32(cnt[o])), f32(my[o] / f32(cnt[o]))
                norm[o] = np.sqrt(f32(f32(mx[o] * mx[o]) + f32(my[o] * my[o])))
                if norm[o] == 0:
                    seen.add("mean_flow_zero")
                mx[o], my[o] = f32(mx[o] / norm[o]), f32(my[o] / norm[o])
        assigned = np.zeros(grid.N, bool) if had_map_point is None else np.asarray(had_map_point, bool).copy()
        for i in range(len(inds)):
            if not status[i]:
                cur[i] = 0
                continue
            out["kltmatches"] += 1
            o = int(object_id[inds[i]])
            dx, dy = f32(cur[i, 0] - lastobj[i, 0]), f32(cur[i, 1] - lastobj[i, 1])
            move = np.sqrt(f32(f32(dx * dx) + f32(dy * dy)))
            dx, dy = f32(dx / move), f32(dy / move)
            if norm[o] > 20 and move > 20:
                if f32(f32(dx * mx[o]) + f32(dy * my[o])) < 0.85:
                    seen.add("direction_reject")
                    cur[i] = 0
                    continue
            out["goodmatches"] += 1
            octv = int(last_octave[inds[i]])
            radius = f32(f32(th) * f32(scale_factors[octv]))
            best = grid.closest(cur[i, 0], cur[i, 1], radius, octv, 2, keys_static, seen)
            if best < grid.N:
                if keys_static is not None and keys_static[best]:
                    cur[i] = 0
                    continue
                out["findfeaturematches"] += 1
                if not assigned[best]:
                    out["uniquematches"] += 1
                if train[best] >= 0:
                    seen.add("two_claims")
                assigned[best] = True
                train[best] = inds[i]
            else:
                seen.add("no_feature")
                cur[i] = 0
    out["featuresklt_thisframe"] = cur
    if trace is not None:
        trace.append(seen)
    return out
