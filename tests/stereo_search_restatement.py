"""Judge of the stereo searches (include/cubeslam_hip/stereo_search.h): a numpy restatement of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (reference
orb_object_slam/src/ORBmatcher.cc:1373-1522) and ORBmatcher::SearchByProjection(F, vpMapPoints, th) (:50-142) with their stereo branches.  A helper, not a test module.

Every float operation is an explicit np.float32 step in the reference's association.  The direction is the stated definition of stereo_search.h: a cv::Mat product is one gemm
per row, accumulated in double with k ascending and rounded once,
    twc[r] = (float)(-sum_k (double)Rcw[k][r] * (double)tcw[k])        tlc_z = (float)(sum_k (double)Rlw[2][k] * (double)twc[k] + (double)tlw[2])
and tests/test_stereo_search_restatement_pins.py holds it, with everything else here, to the reference's own text.

Windows, the sequential loops and the rotation cut are the models of tests/match_patterns.py (area, resolve, rot_bin, three_maxima), imported, not copied: this file adds what the
stereo branch adds -- the direction, the level window per direction, the predicted right coordinate and the mvuRight test ahead of the loop.  `area` is written for the bounds of
match_patterns; a frame with other bounds passes its own window function (the oracle's GetFeaturesInArea)."""
import numpy as np

from tests import match_patterns as P
from tests.match_patterns import area, resolve, rot_bin, three_maxima  # noqa: F401  (rot_bin and three_maxima run inside resolve)

f32, f64 = np.float32, np.float64
NEITHER, FORWARD, BACKWARD = 0, 1, 2


def tlc_z(Tcw, Tlw):
    """tlc.at<float>(2) of :1383-1391."""
    Tcw = np.asarray(Tcw, f32).reshape(-1)[:12].reshape(3, 4); Tlw = np.asarray(Tlw, f32).reshape(-1)[:12].reshape(3, 4)
    twc = np.zeros(3, f32)
    for r in range(3):
        acc = f64(0)
        for k in range(3):
            acc = acc + f64(Tcw[k, r]) * f64(Tcw[k, 3])
        twc[r] = f32(-acc)
    acc = f64(0)
    for k in range(3):
        acc = acc + f64(Tlw[2, k]) * f64(twc[k])
    return f32(acc + f64(Tlw[2, 3]))


def direction(Tcw, Tlw, mb, mono):
    """:1393-1394: 1 forward, 2 backward, 0 neither; strict float comparisons."""
    if mono:
        return NEITHER
    z = tlc_z(Tcw, Tlw)
    if z > f32(mb):
        return FORWARD
    if f32(-z) > f32(mb):
        return BACKWARD
    return NEITHER


def levels(d, o):
    """The level arguments of GetFeaturesInArea at :1433-1438."""
    return (o, -1) if d == FORWARD else (0, o) if d == BACKWARD else (o - 1, o + 1)


def project(wp, Tcw, intr, bounds):
    """:1407-1424 -> (u, v, invzc) or None."""
    fx, fy, cx, cy = [f32(a) for a in intr[:4]]
    T = np.asarray(Tcw, f32).reshape(-1)[:12].reshape(3, 4)
    x3Dc = np.zeros(3, f32)
    for r in range(3):
        acc = f64(0)
        for k in range(3):
            acc = acc + f64(T[r, k]) * f64(f32(wp[k]))
        x3Dc[r] = f32(acc * f64(1.0) + f64(T[r, 3]) * f64(1.0))
    with np.errstate(all="ignore"):
        invzc = f32(f64(1.0) / f64(x3Dc[2]))
        if invzc < 0:
            return None
        u = f32(f32(f32(fx * x3Dc[0]) * invzc) + cx)
        v = f32(f32(f32(fy * x3Dc[1]) * invzc) + cy)
    if u < f32(bounds[0]) or u > f32(bounds[1]):
        return None
    if v < f32(bounds[2]) or v > f32(bounds[3]):
        return None
    return u, v, invzc


def drops(ur_query, u_right, radius):
    """:1459-1465 / :104-109: the candidate is no candidate."""
    if not f32(u_right) > 0:
        return False
    er = abs(f32(f32(ur_query) - f32(u_right)))
    return bool(er > f32(radius))


class _Lists:
    """What match_patterns.resolve reads of a search, over candidate lists that are already filtered."""

    def __init__(self, keys, desc, lists, qdesc, qangle, blocks, tblocked, nnratio, check_ori):
        self.keys, self.desc, self._lists, self.qdesc, self.qangle, self.blocks = keys, desc, lists, qdesc, np.asarray(qangle, f32), np.asarray(blocks, np.uint8)
        self.tblocked = np.zeros(len(keys), np.uint8) if tblocked is None else np.asarray(tblocked, np.uint8)
        self.nnratio, self.check_ori = nnratio, check_ori
        self.t, self.q = range(len(keys)), range(len(lists))

    def lists(self, variant):
        return self._lists


def _area_fn(keys, bounds):
    assert tuple(float(b) for b in bounds) == P.BOUNDS, "match_patterns.area is written for its own bounds: pass area_fn"
    grid = P.grid_lists(keys)
    return lambda x, y, r, lo, hi: area(keys, grid, x, y, r, lo, hi)


def search_by_projection_frame(keys, desc, bounds, u_right, world_pos, valid, blocks, mp_desc, last_octave, last_angle, Tcw, Tlw, intr, bf, mb, mono, sf, th, check_ori,
                               train_blocked=None, area_fn=None, stereo_test=True):
    """:1373-1522 -> (train_match per key point of the current frame, nmatches, direction, candidates after the mvuRight test).  u_right = CurrentFrame.mvuRight; intr = (fx, fy,
    cx, cy); bf = mbf; mb = the baseline.  stereo_test = False: the monocular search the library had (levels by direction still apply)."""
    area_fn = area_fn or _area_fn(keys, bounds)
    d = direction(Tcw, Tlw, mb, mono)
    lists = []
    for i in range(len(valid)):
        if not valid[i]:
            lists.append(None); continue
        pr = project(world_pos[i], Tcw, intr, bounds)
        if pr is None:
            lists.append(None); continue
        u, v, invzc = pr
        o = int(last_octave[i])
        radius = f32(f32(th) * f32(sf[o]))
        lo, hi = levels(d, o)
        ur = f32(u - f32(f32(bf) * invzc))
        lists.append([t for t in area_fn(u, v, radius, lo, hi) if not (stereo_test and drops(ur, u_right[t], radius))])
    S = _Lists(keys, desc, lists, mp_desc, last_angle, blocks, train_blocked, 0.0, bool(check_ori))
    tm, n, _ = resolve(P.PROJ, S)
    return tm, n, d, sum(len(l) for l in lists if l is not None)


def search_local_map(keys, desc, bounds, u_right, proj_xy, proj_xr, view_cos, pred_level, in_view, blocks, mp_desc, sf, th, nnratio, train_blocked=None, area_fn=None,
                     stereo_test=True):
    """:50-142 -> (train_match, nmatches, candidates after the mvuRight test).  proj_xr = mTrackProjXR."""
    area_fn = area_fn or _area_fn(keys, bounds)
    bFactor = f64(f32(th)) != 1.0
    lists = []
    for i in range(len(in_view)):
        if not in_view[i]:
            lists.append(None); continue
        L = int(pred_level[i])
        r = f32(2.5) if f64(f32(view_cos[i])) > f64(0.998) else f32(4.0)
        if bFactor:
            r = f32(r * f32(th))
        radius = f32(r * f32(sf[L]))
        lists.append([t for t in area_fn(proj_xy[i][0], proj_xy[i][1], radius, L - 1, L) if not (stereo_test and drops(proj_xr[i], u_right[t], radius))])
    S = _Lists(keys, desc, lists, mp_desc, np.zeros(len(lists), f32), blocks, train_blocked, nnratio, False)
    tm, n, st = resolve(P.LOCAL, S)
    return tm, n, sum(len(l) for l in lists if l is not None), st
