"""Designed inputs for cs_triangulate_dynamic_points and cs_object_depth_points (include/cubeslam_hip/object_points.h): each case is built so that the property in its name
holds, and tests/test_object_points_patterns.py asserts on the CPU that it does.  Every case is a dict of plain arrays; expected() gives the restatement's answer in the layout
of the Python mirror, computed once per case and shared by the tests.

Status 3 (w == 0): the candidate of equal poses and equal rays (rows 2, 3 of A equal to rows 0, 1) does not give an exact zero under the stated Jacobi -- the null space has two
dimensions and the rotations leave a w of the order of 1e-16, which is not 0 as a float (w_zero_candidate() below returns it; the patterns test asserts it).  An input that
does exists all the same, tri_w_zero: cameras without rotation, an object that does not move and both key points exactly at the principal point make column 2 of A exactly
zero, no rotation ever touches a zero column (its gamma is 0), and v = (0, 0, 1, 0) comes out exactly: the point at infinity on the optical axis.  A has rank 3 there and the
null vector is exact in any arithmetic that skips a pair with a zero inner product, as OpenCV's Jacobi does.

No total for which total * 0.30 in double lies off the integer 3 total / 10 exists below 2^31 (the relative error of 0.30 is 2^-54.6, less than half a unit in the last place
of any multiple of 3); off_integer_totals() searches the range a frame can have and the patterns test asserts it is empty.  od_ratio_turn holds the totals next to it."""
import functools
import math

import numpy as np

from cube_slam_amd.object_points import KEYPOINT_DTYPE
from tests import object_points_restatement as R

F = np.float32
K4 = (520.0, 510.0, 325.5, 245.25)
BOUNDS = (0.0, 640.0, 0.0, 480.0)  # cells of 10 x 10 pixels


# ---- the triangulation ---------------------------------------------------------------------------------------------------------------------------------------------------------
def quat(axis, angle):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    s = math.sin(angle / 2)
    return (a[0] * s, a[1] * s, a[2] * s, math.cos(angle / 2))


def pose7(t, q=(0.0, 0.0, 0.0, 1.0)):
    return [float(t[0]), float(t[1]), float(t[2])] + [float(v) for v in q]


def tcw12(p7):
    T = R.se3_load(p7)
    Rm = R.qtoR(T[0])
    return np.array([[Rm[r][0], Rm[r][1], Rm[r][2], T[1][r]] for r in range(3)], np.float32).reshape(-1)


def project(T12, X):
    T = np.asarray(T12, np.float64).reshape(3, 4)
    xc = T[:, :3] @ np.asarray(X, float) + T[:, 3]
    return [K4[0] * xc[0] / xc[2] + K4[2], K4[1] * xc[1] / xc[2] + K4[3]]


def tri_pair(cam_last, cam_now, poses_last, poses_now, points, tracklets=None, integer_pixels=False):
    """One key-frame pair.  cam_*: pose7 of Tcw; poses_*: pose7 rows of the two cuboid tables; points: dicts with obj = (row last, row now), p = the point in the object's
    frame, and optionally kp = (kp1, kp2) as passed, idx_last, offset (world_pos = the point's world position in the last key frame + offset), rows = (obj_last, obj_now) as passed (default: obj)."""
    Tl, Tn = tcw12(cam_last), tcw12(cam_now)
    kp1, kp2, ol, on, il, wp = [], [], [], [], [], []
    for p in points:
        rl, rn = p["obj"]
        Xl = R.se3_map(R.se3_load(poses_last[rl]), list(p["p"]))
        Xn = R.se3_map(R.se3_load(poses_now[rn]), list(p["p"]))
        a, b = project(Tl, Xl), project(Tn, Xn)
        if integer_pixels:
            a, b = [round(v) for v in a], [round(v) for v in b]
        a, b = p.get("kp", (a, b))
        kp1.append(a); kp2.append(b)
        prl, prn = p.get("rows", (rl, rn))
        ol.append(prl); on.append(prn); il.append(p.get("idx_last", len(il)))
        wp.append(np.asarray(Xl) + np.asarray(p.get("offset", (0.05, -0.03, 0.08))))
    return dict(Tl=Tl, Tn=Tn, poses_last=poses_last, poses_now=poses_now, kp1=kp1, kp2=kp2, obj_last=ol, obj_now=on, idx_last=il, world_pos=wp, tracklets=tracklets)


def tri_case(pairs, use_truth=False):
    first = np.concatenate([[0], np.cumsum([len(p["kp1"]) for p in pairs])]).astype(np.int32)
    cfl = np.concatenate([[0], np.cumsum([len(p["poses_last"]) for p in pairs])]).astype(np.int32)
    cfn = np.concatenate([[0], np.cumsum([len(p["poses_now"]) for p in pairs])]).astype(np.int32)
    cat = lambda k, dt, w: np.array([v for p in pairs for v in p[k]], dt).reshape(-1, w) if w else np.array([v for p in pairs for v in p[k]], dt)
    c = dict(kind="tri", first=first, Tcw_last=np.array([p["Tl"] for p in pairs], np.float32).reshape(-1, 12), Tcw_now=np.array([p["Tn"] for p in pairs], np.float32).reshape(-1, 12),
             K4=np.array([K4] * len(pairs), np.float32).reshape(-1, 4), cub_first_last=cfl, cub_pose_last=cat("poses_last", np.float64, 7), cub_first_now=cfn,
             cub_pose_now=cat("poses_now", np.float64, 7), kp1=cat("kp1", np.float32, 2), kp2=cat("kp2", np.float32, 2), obj_last=cat("obj_last", np.int32, 0),
             obj_now=cat("obj_now", np.int32, 0), idx_last=cat("idx_last", np.int32, 0), world_pos=cat("world_pos", np.float32, 3), tracklet_last=None, tracklet_now=None)
    if use_truth:
        c["tracklet_last"] = np.array([t for p in pairs for t in p["tracklets"][0]], np.int32)
        c["tracklet_now"] = np.array([t for p in pairs for t in p["tracklets"][1]], np.int32)
    return c


CAM0 = pose7((0, 0, 0))
CAM_MOVED = pose7((-0.45, 0.02, 0.05), quat((0, 1, 0), 0.03))
OBJ_A = pose7((0.8, 0.3, 8.0), quat((0, 1, 0), 0.4))
OBJ_A_MOVED = pose7((1.5, 0.3, 7.7), quat((0, 1, 0), 0.55))
OBJ_B = pose7((-1.6, 0.2, 11.0), quat((0, 1, 0), -0.2))
OBJ_B_MOVED = pose7((-1.0, 0.2, 10.4), quat((0, 1, 0), -0.1))


def body_points(n, seed, rows=((0, 0), (1, 1))):
    rng = np.random.RandomState(seed)
    return [dict(obj=rows[j % len(rows)], p=rng.uniform(-1, 1, 3) * (1.8, 0.7, 0.8)) for j in range(n)]


def general_pair(n, seed):
    return tri_pair(CAM0, CAM_MOVED, [OBJ_A, OBJ_B], [OBJ_A_MOVED, OBJ_B_MOVED], body_points(n, seed))


def tri_no_pairs():
    """A batch of 0 pairs."""
    return tri_case([])


def tri_empty_pair_between():
    """Pairs of 5, 0 and 4 points."""
    return tri_case([general_pair(5, 1), general_pair(0, 2), general_pair(4, 3)])


def _sized(n):
    a = n // 2
    return tri_case([general_pair(a, 10 + n), general_pair(n - a, 20 + n)])


def tri_total_1():
    """1 point in all (pairs of 0 and 1)."""
    return _sized(1)


def tri_total_255():
    """255 points: one short of a block."""
    return _sized(255)


def tri_total_256():
    """256 points: exactly one block."""
    return _sized(256)


def tri_total_257():
    """257 points: one thread of a second block; the pair seam is at 128."""
    return _sized(257)


def tri_statuses():
    """Points 0, 1: no observation in the last key frame, with object rows outside their tables (not read).  2: tracklets differ.  3: 4.99 from its position; 4: 5.01.  5, 6: fine."""
    pts = body_points(7, 5)
    pts[0].update(idx_last=-1, rows=(-7, 99)); pts[1].update(idx_last=-1, rows=(2, -1))
    pts[2]["obj"] = (0, 1)
    pts[3].update(obj=(0, 0), offset=(4.99, 0, 0)); pts[4].update(obj=(0, 0), offset=(0, 0, -5.01))
    pts[5]["obj"], pts[6]["obj"] = (0, 0), (1, 1)
    return tri_case([tri_pair(CAM0, CAM_MOVED, [OBJ_A, OBJ_B], [OBJ_A_MOVED, OBJ_B_MOVED], pts, tracklets=([4, 9], [4, 9]))], use_truth=True)


def tri_tracklets_off():
    """The same points without tracklet tables: point 2 is triangulated between two different objects."""
    c = tri_statuses()
    c["tracklet_last"] = c["tracklet_now"] = None
    return c


def tri_identity_motion():
    """The object does not move between the key frames (objecttransform is the identity up to rounding); the camera does."""
    return tri_case([tri_pair(CAM0, CAM_MOVED, [OBJ_A], [OBJ_A], body_points(6, 7, rows=((0, 0),)))])


def tri_static_camera():
    """The camera does not move; the object translates: all parallax comes from the object."""
    moved = pose7((1.4, 0.25, 8.2), OBJ_A[3:])
    return tri_case([tri_pair(CAM0, CAM0, [OBJ_A], [moved], body_points(6, 8, rows=((0, 0),)))])


def tri_harris_source():
    """Sub-pixel key points, as mvKeysHarris holds them."""
    return tri_case([general_pair(9, 9)])


def tri_orb_source():
    """Key points on whole pixels, as octave 0 of mvKeysUn holds them without distortion."""
    return tri_case([tri_pair(CAM0, CAM_MOVED, [OBJ_A, OBJ_B], [OBJ_A_MOVED, OBJ_B_MOVED], body_points(9, 9), integer_pixels=True)])


def tri_w_zero():
    """Point 1 of 3: both key points at the principal point, no rotation anywhere, the object at rest: column 2 of A is exactly 0 and v = (0, 0, 1, 0)."""
    cam_now, obj = pose7((-0.45, 0.0, 0.0)), pose7((0.5, 0.2, 9.0))
    pts = body_points(3, 4, rows=((0, 0),))
    pts[1]["kp"] = ((K4[2], K4[3]), (K4[2], K4[3]))
    return tri_case([tri_pair(CAM0, cam_now, [obj], [obj], pts)])


def w_zero_candidate():
    """Equal poses and equal rays: the v the stated Jacobi returns for it."""
    c = tri_case([tri_pair(CAM0, CAM0, [OBJ_A], [OBJ_A], body_points(1, 3, rows=((0, 0),)))])
    A = R.rows(c["Tcw_last"][0], R.object_camera(c["Tcw_now"][0], c["cub_pose_now"][0], c["cub_pose_last"][0]), c["K4"][0], c["kp1"][0], c["kp2"][0])
    return A, R.jacobi_vmin4(A)


# ---- the object-depth initialisation -------------------------------------------------------------------------------------------------------------------------------------------
TWC = [np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), np.concatenate([np.array(R.qtoR(quat((0.2, 1, 0.1), 0.7)), np.float32), [[0.5], [-1.25], [2.0]]], 1).reshape(-1)]


def od_frame(points, cub_depth, draws=(), twc=1, bounds=BOUNDS):
    """points: (x, y, octave, has_map_point, object_id)"""
    k = np.zeros(len(points), KEYPOINT_DTYPE)
    for i, p in enumerate(points):
        k["x"][i], k["y"][i], k["octave"][i], k["class_id"][i], k["size"][i] = p[0], p[1], p[2], -1, 31.0
    return dict(keys=k, has_mp=[p[3] for p in points], obj=[p[4] for p in points], cub=list(cub_depth), draws=list(draws), twc=TWC[twc], bounds=bounds)


def od_case(frames):
    off = lambda k: np.concatenate([[0], np.cumsum([len(f[k]) for f in frames])]).astype(np.int32)
    cat = lambda k, dt: np.array([v for f in frames for v in f[k]], dt)
    return dict(kind="od", first=off("keys"), keys=np.concatenate([f["keys"] for f in frames] + [np.zeros(0, KEYPOINT_DTYPE)]), has_map_point=cat("has_mp", np.uint8),
                object_id=cat("obj", np.int32), cub_first=off("cub"), cuboid_depth=cat("cub", np.float32), K4=np.array([K4] * len(frames), np.float32).reshape(-1, 4),
                bounds=np.array([f["bounds"] for f in frames], np.float32).reshape(-1, 4), Twc=np.array([f["twc"] for f in frames], np.float32).reshape(-1, 12), draw_first=off("draws"),
                draws=cat("draws", np.int32))


def spread(n, obj=lambda j: 0, octave=lambda j: 0, mp=lambda j: 0, x0=15.0):
    """n key points, each in a cell of its own (cells are 10 pixels wide, 60 columns used)"""
    return [(x0 + 10.0 * (j % 60) + 0.25 * (j % 3), 25.0 + 10.0 * (j // 60) + 0.5 * (j % 2), octave(j), mp(j), obj(j)) for j in range(n)]


DRAWS = [1804289383, 846930886, 1681692777, 1714636915, 1957747793, 424238335, 719885386, 1649760492, 596516649, 1189641421] * 12  # what glibc's rand() starts with


def _f_two_in_cell():
    return od_frame([(100.0, 100.0, 0, 0, 0), (102.0, 101.0, 0, 0, 0), (231.5, 77.0, 1, 0, 1), (234.4, 84.9, 2, 0, 1), (400.0, 300.0, 0, 0, 0)] + spread(12, obj=lambda j: -1), [6.5, 9.0], DRAWS)


def od_two_in_cell():
    """Key points 0, 1 share cell (10, 10) and 2, 3 share cell (23, 8): the tracking mode takes 0, 2, 4, the local-mapping mode all five."""
    return od_case([_f_two_in_cell()])


def _f_earlier_nonqualifying():
    return od_frame([(100.0, 100.0, 3, 0, 0), (200.0, 100.0, 0, 0, -1), (101.0, 101.0, 2, 0, 0), (199.0, 99.0, 0, 0, 1), (300.0, 100.0, 0, 1, 0), (301.0, 101.0, 0, 0, 0)] +
                    spread(14, obj=lambda j: -1), [4.0, 5.0], DRAWS)


def od_earlier_nonqualifying():
    """Key point 0 (octave 3) and 1 (no object) do not take their cells: 2 and 3 do.  4 has a map point and does not take its cell either: 5 does."""
    return od_case([_f_earlier_nonqualifying()])


def _f_outside_grid():
    return od_frame([(-20.0, 100.0, 0, 0, 0), (634.9, 100.0, 0, 0, 0), (635.1, 120.0, 0, 0, 0), (100.0, 475.5, 0, 0, 0), (100.0, 474.0, 0, 0, 0), (-4.9, 50.0, 0, 0, 0), (-5.5, 60.0, 0, 0, 0)] +
                    spread(17, obj=lambda j: -1), [3.0], DRAWS)


def od_outside_grid():
    """x = -20 and x = 635.1 (round(63.51) = 64) and y = 475.5 (48) are outside the grid, 634.9 (63), 474.0 (47) and -4.9 (round(-0.49) = 0) inside, -5.5 (round(-0.55) = -1) outside."""
    return od_case([_f_outside_grid()])


UNDISTORTED_BOUNDS = (-3.7, 643.5, -2.6, 482.3)  # as Frame::ComputeImageBounds leaves them with distortion: not whole numbers


def od_truncated_bounds():
    """KeyFrame::PosInGrid subtracts KeyFrame's `const int mnMinX` = -3, not Frame's -3.7: key point 0 at x = 102.875 is in column round(105.875 * 0.09889) = 10 and key point 1
    at x = 108 in column 11, so both are candidates; with -3.7 both would round to 11 and share a cell.  The same in y for key points 2 and 3 (-2 against -2.6)."""
    return od_case([od_frame([(102.875, 200.0, 0, 0, 0), (108.0, 200.5, 0, 0, 0), (300.0, 103.567, 0, 0, 0), (300.5, 108.5, 0, 0, 0)] + spread(16, obj=lambda j: -1, x0=400.0), [4.5], DRAWS,
                             bounds=UNDISTORTED_BOUNDS)])


def od_ratio_turn():
    """Frames of 10 key points with 3 map points (3 / 10 is the double 0.30: not below it) and with 2; of 20 with 6 and with 5; of 9 with 2 (int(2.7) - 2 = 0 points)."""
    fr = [od_frame(spread(n, mp=lambda j, m=m: j < m), [5.0], DRAWS) for n, m in ((10, 3), (10, 2), (20, 6), (20, 5), (9, 2))]
    return od_case(fr)


def _f_more_than_80():
    return od_frame(spread(400, obj=lambda j: (j % 3 if j % 4 == 0 else -1)), [5.0, 6.0, 7.0], DRAWS)


def od_more_than_80():
    """400 key points, 100 candidates: int(400 * 0.30) = 120, so the tracking mode draws 80 and the local-mapping mode 100."""
    return od_case([_f_more_than_80()])


def od_max_zero():
    """3 key points: int(3 * 0.30) = 0 points although the ratio test says yes."""
    return od_case([od_frame(spread(3), [5.0], DRAWS)])


def _f_walk_past():
    pts = spread(30, obj=lambda j: (0 if j < 4 else 1) if j < 12 else -1)
    return od_frame(pts, [-1.0, 7.5], [0, 0, 0, 0] + DRAWS)


def od_walk_past():
    """30 key points, 12 candidates, int(30 * 0.30) = 9 to initialise; the first four draws are 0, so the list starts with the four key points of cuboid 0, whose depth is -1: the walk
    goes on past entry 9 into the three entries no draw touched and ends with the list, at 8 points."""
    return od_case([_f_walk_past()])


def od_depth_zero():
    """A cuboid of depth exactly 0 makes no point (z > 0 fails), one of depth 1e-3 does."""
    return od_case([od_frame(spread(20, obj=lambda j: j % 2 if j < 8 else -1), [0.0, 1e-3], DRAWS)])


def od_same_slot_twice():
    """Draws 5, 4, 3 with 8 candidates pick slot 5 three times running; then 0, 0 swap an entry with itself."""
    return od_case([od_frame(spread(27, obj=lambda j: 0 if j < 8 else -1), [4.0], [5, 4, 3, 0, 0, 7, 7, 7])])


def od_batch():
    """Every frame above in one call, with a frame of no candidates and a frame of no key points between them."""
    none = od_frame(spread(25, obj=lambda j: -1), [], [])
    empty = od_frame([], [2.0], [])
    return od_case([_f_two_in_cell(), none, _f_earlier_nonqualifying(), empty, _f_outside_grid(), _f_more_than_80(), _f_walk_past()])


def od_compaction_seams():
    """od_frame's two ordered compactions (block_rank of csrc/common.h, passes of 256 threads) over tests/compaction_seams.py, every key point in a cell of its own,
    two frames per case.  In the first the pattern is the object id (-1 where it is not set) and the cuboid lies in front of the camera: the candidates follow the
    pattern and the first-frame mode's second compaction keeps them all.  In the second every key point is a candidate and the pattern chooses between cuboid 0
    (depth 5) and cuboid 1 (depth -1): the first-frame mode's second compaction follows the pattern."""
    from tests import compaction_seams as cs
    fr = []
    for n, _, fl in cs.cases():
        fr.append(od_frame(spread(n, obj=lambda j: 0 if fl[j] else -1), [5.0, -1.0], DRAWS * 2))
        fr.append(od_frame(spread(n, obj=lambda j: 0 if fl[j] else 1), [5.0, -1.0], DRAWS * 2))
    return od_case(fr)


def off_integer_totals(limit=8192):
    return [t for t in range(0, limit + 1, 10) if float(t) * 0.30 != float(3 * t // 10)]


TRI_NAMES = ["tri_no_pairs", "tri_empty_pair_between", "tri_total_1", "tri_total_255", "tri_total_256", "tri_total_257", "tri_statuses", "tri_tracklets_off", "tri_identity_motion",
             "tri_static_camera", "tri_harris_source", "tri_orb_source", "tri_w_zero"]
OD_NAMES = ["od_two_in_cell", "od_earlier_nonqualifying", "od_outside_grid", "od_ratio_turn", "od_more_than_80", "od_max_zero", "od_walk_past", "od_depth_zero", "od_same_slot_twice",
            "od_truncated_bounds", "od_batch"]
NAMES = TRI_NAMES + OD_NAMES
MODES = (R.FIRST_FRAME, R.TRACKING, R.LOCAL_MAPPING)
TRI_KEYS = ("status", "x3D", "pos_to_obj", "dpoints")
OD_KEYS = ("n_candidates", "raw_depth_pts", "max_initialize_pts", "cand_first", "candidates", "shuffled", "new_first", "new_idx", "new_x3D")


@functools.lru_cache(maxsize=None)
def case(name):
    return globals()[name]()


@functools.lru_cache(maxsize=None)
def _expected(name, mode):
    c = case(name)
    if c["kind"] == "tri":
        infos = []
        return R.triangulate_dynamic_points(c, infos), infos
    return R.object_depth_points(c, mode), None


def expected(name, mode=None):
    """The restatement's answer (shared: do not write into it)."""
    return _expected(name, mode)[0]


def infos(name):
    """Per point of a triangulation case: A, x3D before the distance test, dist (empty for statuses 1 and 2)."""
    return _expected(name, None)[1]


def run_tri(ctx, c):
    from cube_slam_amd import object_points as O
    return O.triangulate_dynamic_points(ctx, c["first"], c["Tcw_last"], c["Tcw_now"], c["K4"], c["cub_first_last"], c["cub_pose_last"], c["cub_first_now"], c["cub_pose_now"], c["kp1"],
                                        c["kp2"], c["obj_last"], c["obj_now"], c["idx_last"], c["world_pos"], c["tracklet_last"], c["tracklet_now"])


def run_od(ctx, c, mode):
    from cube_slam_amd import object_points as O
    return O.object_depth_points(ctx, mode, c["first"], c["keys"], c["has_map_point"], c["object_id"], c["cub_first"], c["cuboid_depth"], c["K4"], c["Twc"], bounds=c["bounds"],
                                 draw_first=c["draw_first"], draws=c["draws"])


def assert_equal(got, want, keys, what):
    """Bit for bit: same dtype, same shape, same bytes (a NaN equals itself, -0 does not equal 0)."""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s, expected %s %s" % (what, k, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), "%s: %s differs\n got  %s\n want %s" % (what, k, g, w)


# ---- the driver's file format (tests/cpp/object_points_driver.cpp): int32 counts, then the arrays as the C-ABI takes them
def dump(c, mode=None):
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    b = lambda a, dt: np.ascontiguousarray(a, dt).tobytes()
    if c["kind"] == "tri":
        n_pairs, use_truth = len(c["first"]) - 1, c["tracklet_last"] is not None
        out = i32(0, n_pairs, use_truth) + b(c["first"], np.int32) + b(c["Tcw_last"], np.float32) + b(c["Tcw_now"], np.float32) + b(c["K4"], np.float32)
        out += b(c["cub_first_last"], np.int32) + b(c["cub_pose_last"], np.float64) + b(c["cub_first_now"], np.int32) + b(c["cub_pose_now"], np.float64)
        if use_truth:
            out += b(c["tracklet_last"], np.int32) + b(c["tracklet_now"], np.int32)
        return out + b(c["kp1"], np.float32) + b(c["kp2"], np.float32) + b(c["obj_last"], np.int32) + b(c["obj_now"], np.int32) + b(c["idx_last"], np.int32) + b(c["world_pos"], np.float32)
    out = i32(1, len(c["first"]) - 1, mode) + b(c["first"], np.int32) + c["keys"].tobytes() + b(c["has_map_point"], np.uint8) + b(c["object_id"], np.int32)
    out += b(c["cub_first"], np.int32) + b(c["cuboid_depth"], np.float32) + b(c["K4"], np.float32) + b(c["bounds"], np.float32) + b(c["Twc"], np.float32)
    return out + b(c["draw_first"], np.int32) + b(c["draws"], np.int32)


def expected_bytes(c, want):
    keys = TRI_KEYS if c["kind"] == "tri" else OD_KEYS
    return b"".join(np.ascontiguousarray(want[k]).tobytes() for k in keys)
