"""TEST INFRASTRUCTURE: seeded and designed inputs for the corner detector and the new-Harris-feature loop (cs_klt_good_features, cs_track_new_harris_features and
their mirrors), each with what tests/gftt_restatement.py answers.  tests/test_gftt_patterns.py asserts on the restatement that every case takes the branch it was
designed for; the mirror and GPU tests compare byte for byte.  Every case is small: a GPU test over all of them takes a few seconds.

Most designed cases are built from DOTS: single bright pixels on a flat frame, at least 5 pixels apart and 3 from the border.  A dot's eig is a function of its
value alone (Sobel and box reach 2 pixels), peaks at the dot, and is the only candidate around it, so the candidates of a frame are its dots, ordered by value."""
import functools

import numpy as np

from tests import gftt_restatement as gr

f32 = np.float32
SIZES = [(3, 3), (2, 40), (33, 21), (64, 48), (70, 50), (127, 65)]  # (width, height): 70 is a multiple of the 10-pixel cell (the grid's last column is whole), 64, 33 and 127 are not
K4 = np.array([520.0, 510.0, 31.5, 23.25], f32)
TWC = np.array([[0.96, -0.28, 0.0, 0.5], [0.28, 0.96, 0.0, -1.25], [0.0, 0.0, 1.0, 2.0]], f32)


def texture(w, h, seed):
    """Random pixels smoothed by a 3 x 3 mean: corners everywhere, few exact ties."""
    rng = np.random.default_rng(seed)
    p = np.pad(rng.integers(0, 256, (h, w)).astype(np.int32), 1, mode="reflect") if min(w, h) >= 2 else None
    if p is None:
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    return (sum(p[j:j + h, k:k + w] for j in range(3) for k in range(3)) // 9).astype(np.uint8)


def dots(w, h, pts, base=40):
    """A flat frame with the pixels pts = [(x, y, value)]."""
    img = np.full((h, w), base, np.uint8)
    for x, y, v in pts:
        img[y, x] = v
    return img


def lattice(nx, ny, step, x0=3, y0=3):
    return [(x0 + step * i, y0 + step * j) for j in range(ny) for i in range(nx)]


def valued(pos, lo=120, span=100):
    """Distinct-ish values, all within a factor of 2 (eig goes with the square of the contrast: every dot stays above a tenth of the maximum)."""
    return [(x, y, lo + (i * 37) % span) for i, (x, y) in enumerate(pos)]


def case(img, mask=None, max_corners=200, quality=0.1, min_distance=10.0, **extra):
    c = {"img": np.ascontiguousarray(img, np.uint8), "mask": None if mask is None else np.ascontiguousarray(mask, np.uint8), "max_corners": max_corners, "quality": quality,
         "min_distance": min_distance}
    c["want"] = gr.good_features(c["img"], c["mask"], max_corners, quality, min_distance)
    c.update(extra)
    return c


def same_features(got, want):
    return got["corners"].tobytes() == want["corners"].tobytes() and got["quality"].tobytes() == want["quality"].tobytes() and got["n_candidates"] == want["n_candidates"]


@functools.lru_cache(maxsize=None)
def size_case(w, h):
    """A texture at one of SIZES with a random mask over 70 % of it; (3, 3) is searched for a frame whose one interior pixel is a corner."""
    if (w, h) == (3, 3):
        for seed in range(200):
            rng = np.random.default_rng(seed)
            img = (rng.integers(0, 2, (3, 3)) * rng.integers(50, 256)).astype(np.uint8)  # two values: with every border reflected, the sums of such a frame tie often
            if len(gr.good_features(img, None, 200, 0.1, 10.0)["corners"]) == 1:
                return case(img)
        raise AssertionError("no 3 x 3 frame with a corner")
    rng = np.random.default_rng(w * 1000 + h)
    return case(texture(w, h, w + h), (rng.random((h, w)) < 0.7).astype(np.uint8), quality=0.05, min_distance=3.0)


@functools.lru_cache(maxsize=None)
def border_corner_case():
    """Strong corners at (1, 1) and (w - 2, h - 2) whose Dx Dy have different signs, on a flat frame: searched among seeded 3 x 3 patches until both pixels are corners
    and the answer differs from the variant that reflects the image instead of cov."""
    w, h = 24, 20
    for seed in range(2000):
        rng = np.random.default_rng(seed)
        img = np.full((h, w), 60, np.uint8)
        img[0:3, 0:3] = rng.integers(0, 2, (3, 3)) * 180 + 20
        img[h - 3:, w - 3:] = rng.integers(0, 2, (3, 3)) * 180 + 20
        dx, dy = gr.derivatives(img)
        if not dx[1, 1] * dy[1, 1] * dx[h - 2, w - 2] * dy[h - 2, w - 2] < 0:
            continue
        c = case(img, min_distance=3.0)
        other = gr.good_features(img, None, 200, 0.1, 3.0, border="image")
        got = {tuple(p) for p in c["want"]["corners"]}
        if (1, 1) in got and (w - 2, h - 2) in got and not same_features(c["want"], other):
            c["image_variant"] = other
            return c
    raise AssertionError("no such frame")


@functools.lru_cache(maxsize=None)
def border_maximum_case():
    """The maximum of eig lies on a border pixel, which is inside the mask and cannot be a candidate: the threshold comes from it."""
    w, h = 40, 30
    for seed in range(500):  # a faint texture and a hard seeded patch on rows 0 and 1, until the maximum is on row 0
        img = texture(w, h, 5) // 4 + 100
        img[0:2, 16:20] = np.random.default_rng(seed).integers(0, 2, (2, 4)) * 255
        eig = gr.min_eigen(img)
        c = case(img, np.ones((h, w), np.uint8))
        if np.argmax(eig) < w and len(c["want"]["corners"]) >= 1:
            return c
    raise AssertionError("no such frame")


@functools.lru_cache(maxsize=None)
def masked_maximum_case():
    """The mask leaves out the 7 x 7 pixels around the global maximum of eig: the threshold is the masked maximum's."""
    w, h = 48, 36
    img = texture(w, h, 9)
    eig = gr.min_eigen(img)
    y, x = np.unravel_index(np.argmax(eig), eig.shape)
    mask = np.ones((h, w), np.uint8)
    mask[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] = 0
    return case(img, mask, open=case(img))


def empty_mask_case():
    return case(texture(40, 30, 3), np.zeros((30, 40), np.uint8))


def flat_case():
    return case(np.full((30, 40), 77, np.uint8))


@functools.lru_cache(maxsize=None)
def tie_case():
    """An 8 x 8 patch repeated over the frame: the tiles away from the border have bit-equal eig, so the raster index orders their corners."""
    patch = texture(8, 8, 21)
    return case(np.tile(patch, (5, 6)), min_distance=3.0)


@functools.lru_cache(maxsize=None)
def distance_case():
    """Dots at distance^2 exactly 100 from the strongest one, (6, 8) and (10, 0) away: both kept, the test is strict; and one at 98, (7, 7) away: dropped.  (99 is not a
    sum of two squares: no two pixels are at that distance.)  The dropped one is stronger than the kept ones, so it is walked before them."""
    a = (30, 30)
    return case(dots(64, 64, [(a[0], a[1], 250), (a[0] + 6, a[1] + 8, 200), (a[0] - 10, a[1], 190), (a[0] + 7, a[1] - 7, 230)]), at=a)


@functools.lru_cache(maxsize=None)
def seam_case():
    """64 pixels are six cells of 10 and one of 4.  Pairs too near each other across the seam x = 9 | 10, across x = 59 | 60 (the last, partial column of cells) and
    across both seams of one corner of four cells: the weaker of each pair is dropped although it lies in another cell."""
    pts = [(8, 12, 250), (13, 14, 150), (57, 30, 240), (62, 33, 140), (27, 18, 230), (32, 22, 130), (45, 45, 220), (45, 52, 120)]
    return case(dots(64, 60, pts))


@functools.lru_cache(maxsize=None)
def stop_case():
    """224 dots 6 pixels apart with minDistance 5: every one is acceptable, the walk stops at 200 in the middle of its fourth batch of 64."""
    return case(dots(16 * 6 + 4, 14 * 6 + 4, valued(lattice(16, 14, 6))), min_distance=5.0)


@functools.lru_cache(maxsize=None)
def count_case(n):
    """n dots: n candidates (64: one full batch, 65: a second batch of one)."""
    return case(dots(13 * 5 + 4, 5 * 5 + 4, valued(lattice(13, 5, 5)[:n])), min_distance=3.0)


@functools.lru_cache(maxsize=None)
def capacity_case(extra):
    """A fine lattice of equal dots, 5 pixels apart: gr.MAX_CANDIDATES + extra of them, every one a candidate, all of one value (8 192 ties)."""
    n = gr.MAX_CANDIDATES + extra
    pos = lattice(128, 65, 5)[:n]
    img = dots(128 * 5 + 4, 65 * 5 + 4, [(x, y, 200) for x, y in pos])
    if extra > 0:
        return {"img": img, "mask": None, "max_corners": 200, "quality": 0.1, "min_distance": 10.0, "want": None, "n_candidates": n}
    return case(img)


@functools.lru_cache(maxsize=None)
def batch_case():
    """Five frames of one size with 0, 1, 199, 200 and 224 acceptable corners (max_corners = 200, minDistance 5)."""
    w, h = 16 * 6 + 4, 14 * 6 + 4
    pos = valued(lattice(16, 14, 6))
    frames = [dots(w, h, pos[:k]) for k in (0, 1, 199, 200, 224)]
    return {"frames": np.stack(frames), "cases": [case(f, min_distance=5.0) for f in frames]}


def designed_cases():
    return {"border_corner": border_corner_case(), "border_maximum": border_maximum_case(), "masked_maximum": masked_maximum_case(), "empty_mask": empty_mask_case(),
            "flat": flat_case(), "tie": tie_case(), "distance": distance_case(), "seam": seam_case(), "stop": stop_case(), "count64": count_case(64), "count65": count_case(65)}


# ---- the mask and the new points ----
def harris_case(img, objmask, pts, obs, depth, K4=K4, Twc=TWC):
    c = {"img": np.ascontiguousarray(img, np.uint8), "objmask": np.ascontiguousarray(objmask, np.uint8), "pts": np.asarray(pts, f32).reshape(-1, 2), "obs": np.asarray(obs, np.int32),
         "depth": np.asarray(depth, f32), "K4": K4, "Twc": Twc, "trace": []}
    try:
        c["want"] = gr.new_harris_features(c["img"], c["objmask"], c["pts"], c["obs"], K4, Twc, c["depth"], c["trace"])
    except gr.BadObject:
        c["want"] = None
    return c


def same_harris(got, want):
    return all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in ("good", "pts", "object_id", "x3D", "x3D_valid")) and \
        got["n_mask_outside"] == want["n_mask_outside"] and got["n_candidates"] == want["n_candidates"]


MW, MH = 96, 72


def _objects():
    m = np.zeros((MH, MW), np.uint8)
    m[:, :40] = 1     # object 0 fills the left part, borders and corners included
    m[20:, 56:] = 2   # object 1 reaches the right and bottom borders
    return m


@functools.lru_cache(maxsize=None)
def mask_order_case(order):
    """Two existing points 6 pixels apart on object 0.  order 0: the first has more observations, draws, and erases the second's pixel; 1: the other way round; 2: equal
    counts, the lower index draws.  The discs differ, so do the masks."""
    obs = {0: [5, 2], 1: [2, 5], 2: [3, 3]}[order]
    return harris_case(texture(MW, MH, _order_seed()), _objects(), ORDER_PTS, obs, [2.5, 4.0])


ORDER_PTS = [[20.2, 30.4], [26.0, 30.0]]


@functools.lru_cache(maxsize=None)
def _order_seed():
    """The first texture on which the two orders also give different corners: one lies where only one of the two discs was drawn."""
    for seed in range(31, 131):
        a, b = (gr.new_harris_features(texture(MW, MH, seed), _objects(), np.array(ORDER_PTS, f32), obs, K4, TWC, [2.5, 4.0]) for obs in ([5, 2], [2, 5]))
        if a["pts"].tobytes() != b["pts"].tobytes():
            return seed
    raise AssertionError("no such texture")


@functools.lru_cache(maxsize=None)
def mask_edge_case():
    """Existing points: on the background (draws nothing); x rounding to cols (reads the next row's first pixel, which is on object 0, and draws a disc centred on
    column `cols`); an index beyond the image below and before it above (counted, skipped); discs clipped at the left, top, right and bottom borders and at the
    bottom-right corner; a half-way coordinate (30.5 rounds to 30, 31.5 to 32)."""
    pts = [[48.0, 10.0], [MW - 0.4, 33.0], [5.0, MH - 0.4], [-3.0, -0.2], [2.0, 40.0], [25.0, 1.0], [MW - 2.0, 45.0], [70.0, MH - 3.0], [MW - 3.0, MH - 2.0], [30.5, 55.5]]
    return harris_case(texture(MW, MH, 32), _objects(), pts, [9, 8, 7, 6, 5, 4, 3, 2, 1, 1], [2.5, 4.0])


@functools.lru_cache(maxsize=None)
def depth_case(kind):
    """The new points' depths.  "two": objects at 2.5 and 4.0; "behind": object 1 at z = 0 and object 0 behind the camera (x3D_valid = 0, zeros); "missing": object 1 has no
    cuboid (its id equals the cuboid count: CS_ERR_BAD_ARG)."""
    depth = {"two": [2.5, 4.0], "behind": [-1.0, 0.0], "missing": [2.5]}[kind]
    return harris_case(texture(MW, MH, 33), _objects(), np.zeros((0, 2), f32), np.zeros(0, np.int32), depth)


def harris_cases():
    return {"order0": mask_order_case(0), "order1": mask_order_case(1), "order2": mask_order_case(2), "edges": mask_edge_case(), "two": depth_case("two"), "behind": depth_case("behind")}


# ---- the chain: detect, track, detect again ----
@functools.lru_cache(maxsize=None)
def chain_frames():
    """Three frames of one texture moving by (2, 1) a frame, with two object masks that move with it."""
    w, h = 128, 96
    big = texture(w + 8, h + 8, 41)
    frames = np.stack([big[4 - f:4 - f + h, 4 - 2 * f:4 - 2 * f + w] for f in range(3)])
    masks = np.zeros((3, h, w), np.uint8)
    for f in range(3):
        masks[f, 10 + f:50 + f, 8 + 2 * f:60 + 2 * f] = 1
        masks[f, 40 + f:90 + f, 70 + 2 * f:120 + 2 * f] = 2
    return frames, masks


CHAIN_DEPTH = np.array([3.0, 5.0], f32)


def chain_new_features(frame, mask, tracked, detect):
    """One key frame of the chain: `tracked` = (map-point ids, object ids, pts) the frame has, detect(pts, obs) = the new-feature call (every tracked point has been
    observed twice).  Returns the frame's extended (ids, object ids, pts) and the call's dict."""
    ids, obj, pts = tracked
    r = detect(pts, np.full(len(pts), 2, np.int32))
    first = int(ids.max()) + 1 if len(ids) else 0
    new_ids = np.arange(first, first + len(r["pts"]), dtype=np.int32)
    return (np.concatenate([ids, new_ids]).astype(np.int32), np.concatenate([obj, r["object_id"]]).astype(np.int32), np.concatenate([pts, r["pts"]]).astype(f32)), r


@functools.lru_cache(maxsize=None)
def chain_case():
    """The chain the reference runs, on the restatements: new features on frame 0 from nothing, SearchByTrackingHarris 0 -> 1, new features on frame 1 with the kept
    points as existing ones; then the observation lists of the two frames in cs_ba_dyn_problem's layout."""
    from tests import klt_patterns as kp
    from tests import klt_restatement as kr
    frames, masks = chain_frames()
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), f32))
    f0, r0 = chain_new_features(frames[0], masks[0], none, lambda p, o: gr.new_harris_features(frames[0], masks[0], p, o, K4, TWC, CHAIN_DEPTH))
    step = kr.search_by_tracking_harris(kr.Pyramid(frames[0]), kr.Pyramid(frames[1]), f0[2], masks[1])
    trace = []
    f1, r1 = chain_new_features(frames[1], masks[1], kp.chain_step(step, f0[0]), lambda p, o: gr.new_harris_features(frames[1], masks[1], p, o, K4, TWC, CHAIN_DEPTH, trace))
    return {"frames": frames, "masks": masks, "new0": r0, "step": step, "new1": r1, "trace": trace, "per_frame": [f0, f1], "lists": kp.dobs_lists([f0, f1])}


# ---- the C++ mirror's files (tests/cpp/gftt_mirror.cpp) ----
def write_mirror_input(path, feats, harris):
    """int32 n_records; per record int32 kind (0 goodFeaturesToTrack, 1 CreateNewHarrisFeatures), width, height, then the image and
       kind 0: int32 has_mask, max_corners, float64 quality, min_distance, the mask when present;
       kind 1: the object mask, int32 n_exist, n_cuboids, the points (2 n floats), the observations (n int32), K4, Twc (12 floats), the depths."""
    with open(path, "wb") as f:
        f.write(np.int32(len(feats) + len(harris)).tobytes())
        for c in feats:
            h, w = c["img"].shape
            f.write(np.array([0, w, h], np.int32).tobytes() + c["img"].tobytes())
            f.write(np.array([c["mask"] is not None, c["max_corners"]], np.int32).tobytes() + np.array([c["quality"], c["min_distance"]], np.float64).tobytes())
            if c["mask"] is not None:
                f.write(c["mask"].tobytes())
        for c in harris:
            h, w = c["img"].shape
            f.write(np.array([1, w, h], np.int32).tobytes() + c["img"].tobytes() + c["objmask"].tobytes())
            f.write(np.array([len(c["pts"]), len(c["depth"])], np.int32).tobytes() + c["pts"].tobytes() + c["obs"].tobytes())
            f.write(np.asarray(c["K4"], f32).tobytes() + np.asarray(c["Twc"], f32).tobytes() + c["depth"].tobytes())


def read_mirror_output(path, feats, harris):
    """Per record int32 status (0 ok, 1 capacity, 2 bad object), then kind 0: int32 count, n_candidates, corners, quality; kind 1: int32 count, n_candidates,
    n_mask_outside, the mask, pts, object ids, x3D, x3D_valid."""
    raw = open(path, "rb").read()
    at = [0]

    def take(dt, n):
        a = np.frombuffer(raw, dt, n, at[0]).copy()
        at[0] += a.nbytes
        return a
    out = []
    for c in feats:
        st = int(take(np.int32, 1)[0])
        k, nc = (int(v) for v in take(np.int32, 2))
        out.append({"status": st, "corners": take(f32, 2 * k).reshape(-1, 2), "quality": take(f32, k), "n_candidates": nc})
    for c in harris:
        st = int(take(np.int32, 1)[0])
        k, nc, no = (int(v) for v in take(np.int32, 3))
        out.append({"status": st, "n_candidates": nc, "n_mask_outside": no, "good": take(np.uint8, c["img"].size).reshape(c["img"].shape), "pts": take(f32, 2 * k).reshape(-1, 2),
                    "object_id": take(np.int32, k), "x3D": take(f32, 3 * k).reshape(-1, 3), "x3D_valid": take(np.uint8, k)})
    assert at[0] == len(raw)
    return out
