"""TEST INFRASTRUCTURE: seeded inputs for the KLT tests and their expected results from tests/klt_restatement.py, computed once per process and shared.  Every branch
of the tracker and of SearchByTrackingHarris' selection that the tests rely on is asserted on the restatement's own trace (test_klt_patterns.py), so no pattern is
vacuous."""
import numpy as np

from tests import klt_restatement as kr

f32 = np.float32
SIZES = [(42, 64), (64, 48), (168, 60), (169, 60), (169, 169)]  # width x height: level 0 only; two levels; the 168 / 169 seam; all four levels
LK_BRANCHES = {"min_eig", "prev_outside_upper", "prev_outside_level0", "drift_outside", "drift_outside_level0", "eps_stop", "oscillation_stop", "all_iterations",
               "err_outside", "pad_left", "pad_right", "pad_top", "pad_bottom", "weight_zero_fraction", "weight_round_tie"}
HARRIS_BRANCHES = {"mask_zero", "x_rounds_to_cols", "bounds"}


def texture(seed, w, h, dx=0.0, dy=0.0, flat=None, mirror=None):
    """A smooth seeded texture sampled at (x - dx, y - dy): its shift by a sub-pixel vector is exact up to the 8-bit rounding.  flat = (x0, y0, x1, y1): a constant patch.
    mirror = c: sampled at (c - x, y) instead."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = (x - dx, y - dy) if mirror is None else (mirror - x, y)
    v = np.full((h, w), 128.0)
    for _ in range(6):
        fx, fy, ph = rng.uniform(-0.35, 0.35), rng.uniform(-0.35, 0.35), rng.uniform(0, 6.28)
        v += rng.uniform(10, 22) * np.sin(fx * x + fy * y + ph)
    if flat is not None:
        v[flat[1]:flat[3], flat[0]:flat[2]] = 128.0
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def points(seed, w, h, n):
    """Random points over the image and a margin of 40 around it, and the special ones: integer coordinates (fractions exactly 0), a cvRound tie in the weights, points
    whose windows read each pad, points far outside."""
    rng = np.random.default_rng(seed)
    p = [rng.uniform([-40, -40], [w + 40, h + 40], (n, 2))]
    p.append(rng.integers(12, [w - 12, h - 12], (4, 2)).astype(np.float64))                     # a = b = 0 at level 0
    k = rng.integers(100, 16000, 3)
    p.append(np.stack([rng.integers(12, w - 12, 3).astype(np.float64), rng.integers(12, h - 12, 3) + 1.0 - (2 * k + 1) / 32768.0], 1))  # (1 - b) 2^14 = k + 0.5
    p.append(np.array([[1.5, h / 2], [w - 2.5, h / 2], [w / 2, 1.25], [w / 2, h - 2.75], [-100.0, 5.0], [w + 95.0, h + 95.0], [w + 10.0 - 0.004, h / 2 + 0.5]]))
    return np.concatenate(p).astype(f32)


_LK = {}


def lk_case(w, h):
    """{frames [3, h, w], pairs, pts (per pair), want [(nextPts, status, err)] per pair, trace}: frame 1 is `next` of pair 0 and `prev` of pair 1.  A flat patch fills
    the middle of every frame."""
    if (w, h) not in _LK:
        flat = (w // 2 - 13, h // 2 - 13, w // 2 + 14, h // 2 + 14)
        frames = np.stack([texture(w * 1000 + h, w, h, 0, 0, flat), texture(w * 1000 + h, w, h, 2.3, -1.4, flat), texture(w * 1000 + h, w, h, 1.1, 0.8, flat)])
        pts = [np.concatenate([points(w + h, w, h, 14), [[w / 2, h / 2]]]).astype(f32), points(w + h + 1, w, h, 10)]
        pairs = [(0, 1), (1, 2)]
        pyr = [kr.Pyramid(f) for f in frames]
        trace, want = [], []
        for (a, b), q in zip(pairs, pts):
            want.append(kr.track(pyr[a], pyr[b], q, trace))
        _LK[(w, h)] = {"frames": frames, "pairs": pairs, "pts": pts, "want": want, "trace": trace}
    return _LK[(w, h)]


_EDGE = {}


def edge_case():
    """The err-stage rejection.  The next frame is the texture mirrored about a column chosen so that its REFLECT_101 pad on the right shows the previous frame's content
    moved by 22 pixels: a point 22 pixels short of the range limit (x - 10 = cols) is tracked to within a few thousandths of the limit.  Where the last step, shorter
    than 0.01, carries it over, the iterations have stopped and only the err stage sees it."""
    if not _EDGE:
        w, h, flow = 100, 100, 22.0
        frames = np.stack([texture(5, w, h), texture(5, w, h, mirror=2 * (w - 1) - flow)])
        pts = np.array([[w + 10 - flow - d, y] for y in range(14, h - 13, 6) for d in (-0.012, -0.008, -0.004, -0.002, 0.002)], f32)
        trace = []
        want = kr.track(frames[0], frames[1], pts, trace)
        _EDGE.update({"frames": frames, "pairs": [(0, 1)], "pts": [pts], "want": [want], "trace": trace})
    return _EDGE


_BATCH = {}
BATCH_COUNTS = [[65, 0, 1, 130, 63], [64, 130, 0, 65, 1]]  # per-pair point counts of the two mixed calls


def batch_case():
    """Two frames of 64 x 48 tracked forwards and backwards: 130 points each way; a call's pair p takes the first BATCH_COUNTS[.][p] of its direction's points."""
    if not _BATCH:
        w, h = 64, 48
        frames = np.stack([texture(21, w, h), texture(21, w, h, -1.7, 2.2)])
        rng = np.random.default_rng(3)
        pts = [rng.uniform([-15, -15], [w + 15, h + 15], (130, 2)).astype(f32) for _ in range(2)]
        pyr = [kr.Pyramid(f) for f in frames]
        want = [kr.track(pyr[0], pyr[1], pts[0]), kr.track(pyr[1], pyr[0], pts[1])]
        _BATCH.update({"frames": frames, "pts": pts, "want": want})
    return _BATCH


def batch_call(counts):
    """(pairs, pts per pair, want per pair) of one mixed call: pair p runs in direction p % 2."""
    b = batch_case()
    pairs = [(p % 2, 1 - p % 2) for p in range(len(counts))]
    return pairs, [b["pts"][p % 2][:c] for p, c in enumerate(counts)], [tuple(a[:c] for a in b["want"][p % 2]) for p, c in enumerate(counts)]


_HARRIS = {}


def harris_case():
    """Three frames of 96 x 64 with two pairs.  Pair 0 tracks a frame onto itself, so every textured point stays where it is: points with x in [cols - 0.5, cols) round
    to cols in the mask lookup (the next row's first pixel; on the last row the index is rows * cols, beyond the mask).  The mask is 0 on the left third, object ids
    1 .. 3 elsewhere, and the first column carries id 7 so that the wrapped lookups are told apart."""
    if not _HARRIS:
        w, h = 96, 64
        frames = np.stack([texture(31, w, h), texture(31, w, h), texture(31, w, h, 1.6, -2.1)])
        mask = np.zeros((2, h, w), np.uint8)
        mask[:, :, w // 3:] = 1 + (np.arange(h)[:, None] * 3 // h)
        mask[:, :, 0] = 7
        rng = np.random.default_rng(17)
        wrap = np.array([[w - 0.25, 20.0], [w - 0.5, 33.0], [w - 0.125, h - 1.0], [w - 0.375, h - 0.75], [w + 3.0, 10.0], [-2.0, 30.0]])
        pts = [np.concatenate([rng.uniform([2, 2], [w - 2, h - 2], (30, 2)), wrap]).astype(f32), rng.uniform([-5, -5], [w + 5, h + 5], (40, 2)).astype(f32)]
        pairs = [(0, 1), (1, 2)]
        pyr = [kr.Pyramid(f) for f in frames]
        trace = []
        want = [kr.search_by_tracking_harris(pyr[a], pyr[b], q, m, trace) for (a, b), q, m in zip(pairs, pts, mask)]
        _HARRIS.update({"frames": frames, "pairs": pairs, "pts": pts, "masks": mask, "want": want, "trace": trace})
    return _HARRIS


def same_track(got, want):
    """byte for byte on next_pts, status and err (a dict: a SearchByTracking result, on every output)"""
    if isinstance(want, dict):
        return same_tracking(got, want) if "train_match" in want else same_harris(got, want)
    return all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def same_harris(got, want):
    return all(np.asarray(got[k]).dtype == np.asarray(want[k]).dtype and np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes()
               for k in ("kept", "pts", "object_id", "featuresklt_lastframe", "featuresklt_thisframe", "status", "err")) and \
        got["goodmatches"] == want["goodmatches"] and got["n_mask_outside"] == want["n_mask_outside"]


_CHAIN = {}


def dobs_lists(per_frame):
    """The dynamic-point observations of a window in the layout cs_ba_dyn_problem takes (dobs_cam, dobs_obj, dobs_point, dobs_uv): per_frame[f] = (map-point ids, object
    ids, pts) of frame f's mvpMapPointsHarris / keypoint_associate_objectID_harris / mvKeysHarris."""
    cam = np.concatenate([np.full(len(ids), f, np.int32) for f, (ids, _, _) in enumerate(per_frame)])
    return {"dobs_cam": cam, "dobs_point": np.concatenate([ids for ids, _, _ in per_frame]).astype(np.int32),
            "dobs_obj": np.concatenate([obj for _, obj, _ in per_frame]).astype(np.int32), "dobs_uv": np.concatenate([uv for _, _, uv in per_frame]).astype(np.float64)}


def chain_step(res, ids):
    """(map-point ids, object ids, pts) of the current frame from one SearchByTrackingHarris result and the last frame's ids."""
    return ids[res["kept"]], res["object_id"], res["pts"]


def chain_case():
    """Three frames of 128 x 96: a textured box of 44 x 40 moves by (3.25, 1.5) a frame over a still background; the object mask is the box (value 2 = object 1).  Points
    start on a grid over the box and a ring around it; SearchByTrackingHarris runs frame to frame on what the frame before kept."""
    if not _CHAIN:
        w, h = 128, 96
        frames, masks = [], []
        for f in range(3):
            ox, oy = 30 + 3.25 * f, 24 + 1.5 * f
            bg, box = texture(41, w, h), texture(42, w, h, ox, oy)
            x0, y0 = int(np.ceil(ox)), int(np.ceil(oy))
            m = np.zeros((h, w), np.uint8)
            m[y0:y0 + 40, x0:x0 + 44] = 2
            frames.append(np.where(m > 0, box, bg))
            masks.append(m)
        frames, masks = np.stack(frames), np.stack(masks)
        pts0 = np.array([[x, y] for y in range(18, 72, 6) for x in range(24, 82, 6)], f32)
        ids0 = np.arange(len(pts0), dtype=np.int32)
        inside = masks[0][pts0[:, 1].astype(int), pts0[:, 0].astype(int)] > 0
        per_frame = [(ids0[inside], np.ones(inside.sum(), np.int32), pts0[inside])]
        pyr = [kr.Pyramid(f) for f in frames]
        steps = []
        for f in (1, 2):
            ids, _, pts = per_frame[-1]
            r = kr.search_by_tracking_harris(pyr[f - 1], pyr[f], pts, masks[f])
            steps.append(r)
            per_frame.append(chain_step(r, ids))
        _CHAIN.update({"frames": frames, "masks": masks, "start": per_frame[0], "steps": steps, "lists": dobs_lists(per_frame)})
    return _CHAIN


def mirror_pairs():
    """The pairs tests/cpp/klt_mirror.cpp runs: (last, current, pts, mask or None, want) with `want` the restatement's (nextPts, status, err) or its Harris dict.  One
    pair has strided rows."""
    out = []
    for w, h in ((64, 48), (169, 169)):
        c = lk_case(w, h)
        out.append((c["frames"][0], c["frames"][1], c["pts"][0], None, c["want"][0]))
    e = edge_case()
    out.append((e["frames"][0], e["frames"][1], e["pts"][0], None, e["want"][0]))
    c = lk_case(42, 64)
    wide = np.full((2, 64, 50), 99, np.uint8)
    wide[:, :, :42] = c["frames"][1:]
    out.append((wide[0, :, :42], wide[1, :, :42], c["pts"][1], None, c["want"][1]))
    hc = harris_case()
    for (a, b), q, m, want in zip(hc["pairs"], hc["pts"], hc["masks"], hc["want"]):
        out.append((hc["frames"][a], hc["frames"][b], q, m, want))
    out.append((hc["frames"][0], hc["frames"][1], np.zeros((0, 2), f32), hc["masks"][0], kr.search_by_tracking_harris(hc["frames"][0], hc["frames"][1], np.zeros((0, 2), f32), hc["masks"][0])))
    for c in (tracking_still_case(), tracking_moving_case()):  # SearchByTracking records: `pts` is the case itself
        out.append((c["frames"][0], c["frames"][1], c, "tracking", c["want"]))
    return out


def write_mirror_input(path, pairs):
    with open(path, "wb") as f:
        f.write(np.int32(len(pairs)).tobytes())
        for last, cur, pts, mask, _ in pairs:
            h, w = last.shape
            stride = last.strides[0]
            assert cur.strides[0] == stride and last.strides[1] == 1
            tracking = isinstance(mask, str)
            f.write(np.array([w, h, stride, len(pts["last_pt"]) if tracking else len(pts), 2 if tracking else mask is not None], np.int32).tobytes())
            for im in (last, cur):
                rows = np.zeros((h, stride), np.uint8)
                rows[:, :w] = im
                f.write(rows.tobytes())
            if tracking:
                c = pts
                lk, ck = tracking_keys(c)
                f.write(np.array([len(ck), c["numobject"], 1, 1], np.int32).tobytes() + np.array([TH, *c["bounds"]], f32).tobytes() + SCALE_FACTORS.tobytes())
                f.write(lk.tobytes() + c["eligible"].tobytes() + c["object_id"].tobytes() + ck.tobytes() + c["keys_static"].tobytes() + c["had_map_point"].tobytes())
                continue
            f.write(np.ascontiguousarray(pts, f32).tobytes())
            if mask is not None:
                f.write(np.ascontiguousarray(mask, np.uint8).tobytes())


def read_mirror_output(path, pairs):
    """Per pair (nextPts, status, err) or the Harris dict, as the program wrote them."""
    buf, pos, out = open(path, "rb").read(), 0, []

    def take(n, dt):
        nonlocal pos
        a = np.frombuffer(buf, dt, n, pos).copy()
        pos += a.nbytes
        return a
    for _, _, pts, mask, _ in pairs:
        if isinstance(mask, str):
            k, c0, c1, c2, c3 = take(5, np.int32)
            out.append({"train_match": take(len(pts["cur_pt"]), np.int32), "lastptsinds": take(k, np.int32), "featuresklt_lastframe": take(2 * k, f32).reshape(-1, 2),
                        "featuresklt_thisframe": take(2 * k, f32).reshape(-1, 2), "kltmatches": int(c0), "goodmatches": int(c1), "findfeaturematches": int(c2), "uniquematches": int(c3)})
            continue
        n = len(pts)
        nxt, st, er = take(2 * n, f32).reshape(-1, 2), take(n, np.uint8), take(n, f32)
        if mask is None:
            out.append((nxt, st, er))
            continue
        good, outside = take(2, np.int32)
        out.append({"kept": take(good, np.int32), "pts": take(2 * good, f32).reshape(-1, 2), "object_id": take(good, np.int32), "goodmatches": int(good),
                    "n_mask_outside": int(outside), "featuresklt_lastframe": np.ascontiguousarray(pts, f32).reshape(-1, 2), "featuresklt_thisframe": nxt, "status": st, "err": er})
    assert pos == len(buf)
    return out


# ---- ORBmatcher::SearchByTracking ----
TRACKING_BRANCHES = {"direction_reject", "mean_flow_zero", "two_claims", "closest_tie", "no_feature"}
SCALE_FACTORS = (f32(1.2) ** np.arange(8, dtype=f32)).astype(f32)
TH = 15.0
_TRACKING = {}


def _tracking_want(c):
    grid = kr.FrameGrid(c["cur_pt"], c["cur_octave"], c["bounds"])
    trace = []
    c["want"] = kr.search_by_tracking(c["frames"][0], c["frames"][1], c["last_pt"], c["last_octave"], c["eligible"], c["object_id"], c["numobject"], TH, SCALE_FACTORS, grid,
                                      c["keys_static"], c["had_map_point"], trace)
    c["trace"] = trace[0] if trace else set()
    return c


def tracking_still_case():
    """A frame tracked onto itself, points on quarter pixels: every tracked point stays exactly where it is, so the object's mean flow is exactly zero (its 0 / 0
    direction is never read).  The current frame's key points are placed around the points: two at the same distance (the first in the cell walk wins), one key point
    between two points (both claim it, the later one keeps it), a static key point nearer than a dynamic one, a point with only a static key point in reach, a point
    with none, key points of octave 3 and below the point's own octave."""
    if "still" not in _TRACKING:
        w, h = 240, 120
        img = texture(51, w, h)
        # clusters 40 pixels apart: with th = 15 and octaves 0 - 2 the radius is 15 - 21.6
        last = [(30.0, 30.0, 0), (78.25, 30.0, 0), (82.25, 30.0, 0), (130.0, 30.5, 1), (180.0, 30.0, 0), (30.0, 85.75, 0), (80.0, 85.0, 2), (130.0, 85.0, 0), (180.0, 85.0, 3),
                (215.0, 60.0, 0), (216.5, 100.0, 1)]
        cur = [(31.0, 30.0, 0, 0), (29.0, 30.0, 0, 0),               # a tie around point 0
               (80.25, 30.5, 0, 0),                                  # between points 1 and 2
               (130.5, 30.5, 0, 0), (133.0, 31.0, 1, 0),             # point 3 has octave 1: the nearer key point of octave 0 does not count
               (180.5, 30.0, 0, 1), (184.0, 31.0, 0, 0),             # a static key point nearer than a dynamic one
               (30.0, 86.0, 0, 1),                                   # only a static one in reach of point 5
               (80.0, 86.0, 3, 0), (82.0, 88.0, 2, 0),               # octave 3 is above the limit
               (215.0, 61.0, 0, 0), (217.0, 101.0, 2, 0)]            # point 7 at (130, 85) has no key point in reach
        _TRACKING["still"] = _tracking_want({
            "frames": np.stack([img, img]), "last_pt": np.array([p[:2] for p in last], f32), "last_octave": np.array([p[2] for p in last], np.int32),
            "eligible": np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1], np.uint8), "object_id": np.array([0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1], np.int32), "numobject": 2,
            "cur_pt": np.array([p[:2] for p in cur], f32), "cur_octave": np.array([p[2] for p in cur], np.int32), "keys_static": np.array([p[3] for p in cur], np.uint8),
            "had_map_point": np.array([0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1], np.uint8), "bounds": (0.0, float(w), 0.0, float(h))})
    return _TRACKING["still"]


def tracking_moving_case():
    """256 x 224, four levels.  Object 0's points lie on a part of the frame that moves by (24, 0), two of them on a patch that moves by (17, 17): the mean flow is
    longer than 20 and the two are rejected by their direction.  Object 1 stands still.  The current frame's key points are a seeded scatter, with and without
    KeysStatic / earlier map points (None in the second variant)."""
    if "moving" not in _TRACKING:
        w, h = 256, 224
        a = texture(61, w, h)
        right, down = texture(61, w, h, 24.0, 0.0), texture(61, w, h, 17.0, 17.0)
        b = a.copy()
        b[:130, :] = right[:130, :]
        b[130:, :130] = down[130:, :130]
        last = [(x, y, 0) for y in (20, 38, 56, 74) for x in (40, 80, 120, 160)] + [(45, 178, 0), (80, 182, 0)] + [(170, 180, 1), (200, 190, 1), (230, 180, 1), (190, 165, 1)]
        rng = np.random.default_rng(9)
        cur_pt = rng.uniform([2, 2], [w - 2, h - 2], (400, 2)).astype(f32)
        _TRACKING["moving"] = _tracking_want({
            "frames": np.stack([a, b]), "last_pt": np.array([p[:2] for p in last], f32), "last_octave": np.array([(0, 1, 2, 0, 1, 3)[i % 6] if i < 16 else i % 3 for i in range(len(last))], np.int32),
            "eligible": np.ones(len(last), np.uint8), "object_id": np.array([p[2] for p in last], np.int32), "numobject": 3,
            "cur_pt": cur_pt, "cur_octave": rng.integers(0, 4, 400).astype(np.int32), "keys_static": (rng.random(400) < 0.2).astype(np.uint8),
            "had_map_point": (rng.random(400) < 0.3).astype(np.uint8), "bounds": (0.0, float(w), 0.0, float(h))})
    return _TRACKING["moving"]


def same_tracking(got, want):
    return all(np.asarray(got[k]).dtype == np.asarray(want[k]).dtype and np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes()
               for k in ("train_match", "lastptsinds", "featuresklt_lastframe", "featuresklt_thisframe")) and \
        all(got[k] == want[k] for k in ("kltmatches", "goodmatches", "findfeaturematches", "uniquematches"))


def tracking_keys(c):
    """(last frame's mvKeys, current frame's mvKeysUn) of a tracking case as KEYPOINT_DTYPE records"""
    from cube_slam_amd.orb import KEYPOINT_DTYPE
    out = []
    for pt, octv in ((c["last_pt"], c["last_octave"]), (c["cur_pt"], c["cur_octave"])):
        k = np.zeros(len(pt), KEYPOINT_DTYPE)
        k["x"], k["y"], k["octave"], k["size"], k["class_id"] = pt[:, 0], pt[:, 1], octv, 31.0, -1
        out.append(k)
    return out


# ---- the selection kernels past one wave and past one pass of a workgroup ----
_LARGE = {}
LARGE_HARRIS_SPECIAL = (70, 130, 200, 260, 300, 329)  # beyond-the-mask points: waves 1 - 3 of the first pass of 256, and the second pass


def harris_large_case():
    """One pair of 330 points on harris_case's frame tracked onto itself: every 64-lane wave of the selection's first pass of 256 and its second pass hold kept,
    mask-0 and beyond-the-mask points (x rounds to cols on the last row), so the counts of earlier waves and the carry between passes are all non-zero."""
    if "harris" not in _LARGE:
        c = harris_case()
        w, h = 96, 64
        rng = np.random.default_rng(23)
        pts = rng.uniform([2, 2], [w - 2, h - 2], (330, 2))
        beyond = [(w - 0.125, h - 1.0), (w - 0.375, h - 0.75), (w - 0.25, h - 0.875)]
        for k, i in enumerate(LARGE_HARRIS_SPECIAL):
            pts[i] = beyond[k % 3]
        pts = pts.astype(f32)
        trace = []
        want = kr.search_by_tracking_harris(c["frames"][0], c["frames"][1], pts, c["masks"][0], trace)
        _LARGE["harris"] = {"frames": c["frames"][:2], "pairs": [(0, 1)], "pts": [pts], "masks": c["masks"][:1], "want": [want], "trace": trace}
    return _LARGE["harris"]


def tracking_large_case():
    """SearchByTracking with 700 key points in the last frame, about half of them selected, and 600 in the current frame: three passes of the selection's ordered
    compaction, more than one pass of the per-point tail and of the per-key-point loops.  96 x 64, the second frame moved by (1.5, -2)."""
    if "tracking" not in _LARGE:
        w, h = 96, 64
        rng = np.random.default_rng(29)
        n_last, N = 700, 600
        c = {"frames": np.stack([texture(71, w, h), texture(71, w, h, 1.5, -2.0)]),
             "last_pt": (np.rint(rng.uniform([4, 4], [w - 4, h - 4], (n_last, 2)) * 4) / 4).astype(f32), "last_octave": rng.integers(0, 4, n_last).astype(np.int32),
             "eligible": (rng.random(n_last) < 0.65).astype(np.uint8), "object_id": rng.integers(0, 3, n_last).astype(np.int32), "numobject": 3,
             "cur_pt": rng.uniform([1, 1], [w - 1, h - 1], (N, 2)).astype(f32), "cur_octave": rng.integers(0, 4, N).astype(np.int32),
             "keys_static": (rng.random(N) < 0.3).astype(np.uint8), "had_map_point": (rng.random(N) < 0.4).astype(np.uint8), "bounds": (0.0, float(w), 0.0, float(h))}
        _LARGE["tracking"] = _tracking_want(c)
    return _LARGE["tracking"]
