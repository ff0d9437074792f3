"""TEST INFRASTRUCTURE: cv::goodFeaturesToTrack, cv::circle and the new-feature loop of Tracking::CreateNewKeyFrame (reference orb_object_slam/src/Tracking.cc:2263-2331)
restated in numpy exactly as INTEGRATION.md 4e defines them: float32 where the definition says float, float64 where it says double, the greedy walk and the disc walk
written sequentially.  It shares no code with csrc/gftt_math.h; the kernels, the host path and the mirrors are compared with it byte for byte."""
import numpy as np

f32, f64 = np.float32, np.float64
S = f32(1.0 / (4 * 3 * 255))
S2 = f32(S * f32(2))
MAX_CANDIDATES = 8192
MIN_DIST, MAX_NEW, QUALITY = 10, 200, 0.1
DISC_TABLE = (10, 9, 9, 9, 9, 8, 8, 7, 6, 4, 0)  # a checked constant: disc_half_widths() derives it from the walk


class Capacity(Exception):
    """More candidates than MAX_CANDIDATES (CS_ERR_CAPACITY); args[0] = the count."""


def cv_round(v):
    return int(np.rint(f32(v)))  # to nearest, ties to even


def derivatives(img):
    """(Dx, Dy) float32 [h, w]: Sobel 3 x 3 scaled by s, as the row filter followed by the column filter evaluates it on the REFLECT_101 image."""
    p = np.pad(np.asarray(img, np.uint8).astype(np.int32), 1, mode="reflect")  # numpy's "reflect" is REFLECT_101
    r = (p[:, 2:] - p[:, :-2]).astype(f32)                                       # rows -1 .. h: the exact integer
    dx = (r[:-2] + r[2:]) * S + r[1:-1] * S2
    q = p[:, 1:-1].astype(f32) * S2 + (p[:, :-2] + p[:, 2:]).astype(f32) * S
    dy = q[2:] - q[:-2]
    return dx, dy


def _box_eig(cov_padded):
    c = cov_padded.astype(f64)                                    # [3, h + 2, w + 2]
    rows = (c[:, :, :-2] + c[:, :, 1:-1]) + c[:, :, 2:]           # a row of three, left to right
    s = ((rows[:, :-2] + rows[:, 1:-1]) + rows[:, 2:]).astype(f32)  # three rows top to bottom, one rounding
    a, b, cc = s[0] * f32(0.5), s[1], s[2] * f32(0.5)
    return (a + cc) - np.sqrt((a - cc) * (a - cc) + b * b)


def min_eigen(img, border="cov"):
    """eig float32 [h, w].  border="cov": the definition, the box takes cov at the REFLECT_101 coordinate.  border="image": the variant that is NOT the definition,
    Sobel evaluated on the reflected image at the positions outside it (it flips the sign of Dx Dy at the mirror)."""
    img = np.asarray(img, np.uint8)
    if border == "cov":
        dx, dy = derivatives(img)
        cov = np.stack([dx * dx, dx * dy, dy * dy])
        return _box_eig(np.pad(cov, ((0, 0), (1, 1), (1, 1)), mode="reflect"))
    dx, dy = derivatives(np.pad(img, 1, mode="reflect"))
    return _box_eig(np.stack([dx * dx, dx * dy, dy * dy]))


def candidates(eig, mask, quality_level):
    """(max_val, threshold, [(e', raster index)] in raster order)."""
    h, w = eig.shape
    inside = np.ones((h, w), bool) if mask is None else np.asarray(mask) != 0
    max_val = eig[inside].max() if inside.any() else f32(0)
    t = f32(f64(max_val) * f64(quality_level))
    e = np.where(eig > t, eig, f32(0)).astype(f32)
    nb = e[1:-1, 1:-1].copy()  # the maximum of e' over the 3 x 3 neighbourhood of the interior pixels
    for j in range(3):
        for k in range(3):
            nb = np.maximum(nb, e[j:h - 2 + j, k:w - 2 + k])
    c = (e[1:-1, 1:-1] != 0) & (e[1:-1, 1:-1] == nb) & inside[1:-1, 1:-1]
    ys, xs = np.nonzero(c)  # raster order
    return max_val, t, [(e[y + 1, x + 1], (y + 1) * w + x + 1) for y, x in zip(ys, xs)]


def sort_candidates(c):
    """e' descending; equal values: the higher raster index first."""
    return sorted(c, key=lambda vi: (-f64(vi[0]), -vi[1]))


def _near(x, y, ax, ay, md2):
    dx, dy = f32(x) - f32(ax), f32(y) - f32(ay)
    return f64(dx * dx + dy * dy) < md2


def select_grid(cands, w, h, max_corners, min_distance):
    """The greedy walk with OpenCV's grid of cvRound(minDistance) cells: [(x, y, e')] in acceptance order."""
    cell = int(np.rint(f64(min_distance)))
    gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
    grid = [[] for _ in range(gw * gh)]
    md2 = f64(min_distance) * f64(min_distance)
    out = []
    for v, i in cands:
        x, y = i % w, i // w
        xc, yc = x // cell, y // cell
        good = True
        for yy in range(max(0, yc - 1), min(gh - 1, yc + 1) + 1):
            for xx in range(max(0, xc - 1), min(gw - 1, xc + 1) + 1):
                for ax, ay in grid[yy * gw + xx]:
                    if _near(x, y, ax, ay, md2):
                        good = False
        if good:
            grid[yc * gw + xc].append((x, y))
            out.append((x, y, v))
            if max_corners > 0 and len(out) == max_corners:
                break
    return out


def select_all_pairs(cands, w, max_corners, min_distance):
    """The same walk with no grid: every accepted corner is tested."""
    md2 = f64(min_distance) * f64(min_distance)
    out = []
    for v, i in cands:
        x, y = i % w, i // w
        if all(not _near(x, y, ax, ay, md2) for ax, ay, _ in out):
            out.append((x, y, v))
            if max_corners > 0 and len(out) == max_corners:
                break
    return out


def good_features(img, mask, max_corners, quality_level, min_distance, border="cov"):
    """cv::goodFeaturesToTrack: dict of corners float32 [k, 2], quality float32 [k], n_candidates, max_val, threshold."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    if w < 3 or h < 3:
        return {"corners": np.zeros((0, 2), f32), "quality": np.zeros(0, f32), "n_candidates": 0, "max_val": f32(0), "threshold": f32(0), "sorted": []}
    max_val, t, c = candidates(min_eigen(img, border), mask, quality_level)
    if len(c) > MAX_CANDIDATES:
        raise Capacity(len(c))
    c = sort_candidates(c)
    sel = select_grid(c, w, h, max_corners, min_distance)
    return {"corners": np.array([[x, y] for x, y, _ in sel], f32).reshape(-1, 2), "quality": np.array([v for _, _, v in sel], f32), "n_candidates": len(c), "max_val": max_val,
            "threshold": t, "sorted": c}


def disc_spans(radius=MIN_DIST):
    """The midpoint walk of OpenCV's Circle(), filled: [(row offset, half-width)] in the order the spans are drawn."""
    spans = []
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        spans += [(-dy, dx), (dy, dx), (-dx, dy), (dx, dy)]
        dy += 1
        err += plus
        plus += 2
        mask = -1 if err > 0 else 0  # (err <= 0) - 1
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    return spans


def disc_half_widths(radius=MIN_DIST):
    hw = [-1] * (radius + 1)
    for off, half in disc_spans(radius):
        hw[abs(off)] = max(hw[abs(off)], half)
    return tuple(hw)


def point_order(obs):
    """Observations descending, equal counts by ascending index."""
    return sorted(range(len(obs)), key=lambda i: (-int(obs[i]), i))


def build_mask(objmask, pts, obs, trace=None):
    """Tracking.cc:2265-2287: (good uint8 [h, w], n_mask_outside).  trace: a list that receives per walked point (index, 'outside' | 'zero' | 'drawn')."""
    objmask = np.asarray(objmask, np.uint8)
    rows, cols = objmask.shape
    good = np.where(objmask > 0, 255, 0).astype(np.uint8)
    flat = good.reshape(-1)
    outside = 0
    spans = disc_spans()
    for i in point_order(obs):
        rx, ry = cv_round(pts[i][0]), cv_round(pts[i][1])
        idx = ry * cols + rx
        if idx < 0 or idx >= rows * cols:
            outside += 1
            what = "outside"
        elif flat[idx] != 255:
            what = "zero"
        else:
            what = "drawn"
            for off, half in spans:
                y = ry + off
                if 0 <= y < rows:
                    good[y, max(rx - half, 0):max(min(rx + half, cols - 1) + 1, 0)] = 0
        if trace is not None:
            trace.append((i, what))
    return good, outside


class BadObject(Exception):
    """A corner's object id is at or beyond the cuboid count (CS_ERR_BAD_ARG)."""


def unproject(u, v, z, K4, Twc):
    """KeyFrame::UnprojectPixelDepth: (x3D float32 [3], valid)."""
    z = f32(z)
    if not z > 0:
        return np.zeros(3, f32), 0
    fx, fy, cx, cy = (f32(k) for k in K4)
    invfx, invfy = f32(1.0) / fx, f32(1.0) / fy
    xc = np.array([(f32(u) - cx) * z * invfx, (f32(v) - cy) * z * invfy, z], f32)
    T = np.asarray(Twc, f32).reshape(3, 4)
    out = np.zeros(3, f32)
    for r in range(3):  # one gemm row: the double sum over k ascending plus the translation, one rounding
        acc = f64(0)
        for k in range(3):
            acc += f64(T[r, k]) * f64(xc[k])
        out[r] = f32(acc * 1.0 + f64(T[r, 3]) * 1.0)
    return out, 1


def new_harris_features(img, objmask, exist_pts, exist_obs, K4, Twc, cuboid_depth, trace=None):
    """Tracking.cc:2263-2331 for one frame: dict of good, n_mask_outside, pts, object_id, x3D, x3D_valid, n_candidates."""
    objmask = np.asarray(objmask, np.uint8)
    good, outside = build_mask(objmask, np.asarray(exist_pts, f32).reshape(-1, 2), np.asarray(exist_obs).reshape(-1), trace)
    g = good_features(img, good, MAX_NEW, QUALITY, MIN_DIST)
    ids, X, valid = [], [], []
    for x, y in g["corners"]:
        oid = int(objmask[int(y), int(x)]) - 1
        if oid >= len(cuboid_depth):
            raise BadObject(oid)
        p, ok = unproject(x, y, cuboid_depth[oid], K4, Twc)
        ids.append(oid), X.append(p), valid.append(ok)
    return {"good": good, "n_mask_outside": outside, "pts": g["corners"], "object_id": np.array(ids, np.int32), "x3D": np.array(X, f32).reshape(-1, 3),
            "x3D_valid": np.array(valid, np.uint8), "n_candidates": g["n_candidates"]}
