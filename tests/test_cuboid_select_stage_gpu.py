"""GPU parity of the selection stage (cuboid_select_keep / _geom / _rank) against the CPU oracle at the sizes where its code takes another path.

Every case is one or two 640 x 480 synth.cuboid_scene frames, compared as tests/test_cuboid_gpu.py compares them.  The frames were chosen on the CPU with the
oracle alone: its debug rows give every unit's number of valid proposals and their two errors, fuse_normalize_scores the kept set.  Each case asserts from those
numbers that the condition it was chosen for is reached, so a change of the synthetic scenes cannot silently empty it.

Boxes: "scene" are the frame's own (tight boxes of the drawn cuboids: hundreds of valid proposals, no ties); ("rand", seed) are six seeded boxes that sit
anywhere in the frame (0 to some tens of valid proposals per unit, and ties in both errors, which the tight boxes never showed); "thin" are the boxes of
test_cuboid_gpu.py::test_edge_cases (a box 8 px wide: 1 001 identical top samples, none of which survives the reject tests on these frames -- 0 valid proposals --
and two boxes at the image border with 2 each)."""
import numpy as np
import pytest

from cube_slam_amd import synth
from cube_slam_amd.cuboid import CuboidBatch, detect_3d_cuboid

pytestmark = pytest.mark.gpu

REL = 1e-5  # as tests/test_cuboid_gpu.py

THIN = np.array([[300, 100, 8, 150, 0.5], [0, 0, 200, 300, 0.5], [440, 150, 199, 329, 0.5]], np.float64)


def _boxes(scene, how, W=640, H=480):
    if isinstance(how, str) and how == "scene":
        return np.asarray(scene["boxes"], np.float64)
    if isinstance(how, str) and how == "thin":
        return THIN
    rng = np.random.default_rng(how[1])
    out = []
    for _ in range(6):
        w, h = int(rng.integers(60, 260)), int(rng.integers(60, 260))
        out.append([int(rng.integers(12, W - 13 - w)), int(rng.integers(12, H - 13 - h)), w, h, 0.5])
    return np.array(out, np.float64)


def _frames(spec):
    scenes = [synth.cuboid_scene(seed, n_boxes=3) for seed, _ in spec]
    return scenes, [_boxes(s, how) for s, (_, how) in zip(scenes, spec)]


def _oracle_opts(po, det, stateful=0):
    o = po.cuboid_opts(consider_config_1=int(det.consider_config_1), consider_config_2=int(det.consider_config_2),
                       whether_sample_cam_roll_pitch=int(det.whether_sample_cam_roll_pitch),
                       whether_sample_bbox_height=int(det.whether_sample_bbox_height), max_cuboid_num=det.max_cuboid_num,
                       nominal_skew_ratio=det.nominal_skew_ratio, max_cut_skew=det.max_cut_skew,
                       yaw_range_deg=det.yaw_range_deg, yaw_step_deg=det.yaw_step_deg)
    o.stateful_cam_pose = stateful
    return o


def _cmp_cuboids(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert len(g) == len(r)
        for name in g.dtype.names:
            a, b = g[name], r[name]
            if name == "box_corners_2d":
                assert np.array_equal(a, b), name
            else:
                assert np.allclose(a, b, rtol=REL, atol=1e-9), (name, a, b)


def unit_stats(po, dbg, n_units):
    """Per unit, from the oracle's rows (column 4 the distance error, 5 the angle error): n valid proposals, n_kept of fuse_normalize_scores, whether the
    distance keys tie across the keep threshold (more ties than room: the first of them in index order are kept) and whether the angle keys of rank k - 1 and k
    tie (the angle criterion is dropped: the keep list is in distance order, `branch_b`)."""
    out, r0 = [], 0
    for n in dbg["row_count"][:n_units]:
        n = int(n)
        d, a = dbg["rows"][r0:r0 + n, 4], dbg["rows"][r0:r0 + n, 5]
        r0 += n
        st = {"n": n, "n_kept": n, "tie_d": False, "branch_b": False}
        if n > 4:
            k = int(round(float(np.float32(n)) / 3.0 * 2.0)) - 1  # breaking_num - 1, object_3d_util.cpp:505
            ds, as_ = np.sort(d), np.sort(a)
            st["tie_d"] = bool(ds[k - 1] == ds[k])
            st["branch_b"] = bool(as_[k - 1] == as_[k])
            st["n_kept"] = len(po.fuse_normalize_scores(d, a)[0])
        out.append(st)
    return out


def oracle_frames(po, scenes, boxes, oo):
    """(cuboids per box over all frames, unit_stats over all frames, units per box)"""
    ref, st = [], []
    per_box = 3 if oo.whether_sample_bbox_height else 1  # an upper bound: the oracle numbers its units consecutively
    for s, bx in zip(scenes, boxes):
        r, dbg = po.detect_cuboid(s["gray"], s["K"], s["Twc"], bx, s["lines"], opts=oo, debug=True)
        ref += r
        st.append(unit_stats(po, dbg, len(bx) * per_box))
    return ref, st


def _det(ctx, kw):
    det = detect_3d_cuboid(ctx)
    for k, v in kw.items():
        setattr(det, k, v)
    return det


def _run_batch(ctx, oracle, spec, kw):
    """The frames of `spec` as one batch against the oracle: cuboids, and every unit's n_valid.  Returns (oracle cuboids, flat unit statistics in unit order)."""
    det = _det(ctx, kw)
    scenes, boxes = _frames(spec)
    K = scenes[0]["K"]
    det.set_calibration(K)
    b = CuboidBatch(ctx, np.stack([s["gray"] for s in scenes]), K, np.stack([s["Twc"] for s in scenes]), boxes, [s["lines"] for s in scenes], det.opts())
    b.run()
    got = b.read()
    n_units = b.stats()["n_units"]
    dims = [b.unit(u) for u in range(n_units)]
    b.close()
    ref, st = oracle_frames(oracle, scenes, boxes, _oracle_opts(oracle, det))
    flat, u = [], 0
    for f, bx in enumerate(boxes):
        seg = 0
        for _ in range(len(bx)):
            for hs in range(dims[u]["n_hs"]):
                assert dims[u]["frame"] == f and dims[u]["hs"] == hs
                assert dims[u]["n_valid"] == st[f][seg]["n"], (u, dims[u]["n_valid"], st[f][seg])
                flat.append(dict(st[f][seg], box=dims[u]["box"], hs=hs))
                seg += 1
                u += 1
    assert u == n_units
    _cmp_cuboids(got, ref)
    return ref, flat


SMALL = [(8, ("rand", 1008)), (10, ("rand", 1010))]


@pytest.mark.parametrize("max_cuboid_num", [1, 5])
def test_units_with_zero_to_five_proposals(ctx, oracle, max_cuboid_num):
    """n = 0 (nothing to select, nothing to rank), 1-4 (all kept, no select), exactly 5 (the smallest select: k = 2) -- one of the 5s keeps NOTHING (the two keep
    sets do not meet), so its box has valid proposals and no cuboid.  With max_cuboid_num = 5 boxes have fewer candidates than records asked for."""
    ref, st = _run_batch(ctx, oracle, SMALL, {"yaw_step_deg": 15.0, "consider_config_2": False, "max_cuboid_num": max_cuboid_num})
    ns = [x["n"] for x in st]
    assert 0 in ns and 5 in ns and any(1 <= n <= 4 for n in ns) and any(n > 5 for n in ns)
    assert any(x["n"] == 5 and x["n_kept"] == 0 for x in st)
    if max_cuboid_num == 5:
        assert any(0 < len(r) < 5 for r in ref) and any(len(r) == 5 for r in ref)
    else:
        assert any(len(r) == 0 for r in ref) and any(len(r) == 1 for r in ref)


TIES = [(1, ("rand", 1001)), (7, "thin")]


@pytest.mark.parametrize("max_cuboid_num", [1, 3])
def test_ties_at_the_distance_threshold_and_in_the_angle_keys(ctx, oracle, max_cuboid_num):
    """A unit whose distance keys tie across the threshold (need_eq < ties: the first need_eq ties in index order are kept) and units whose angle keys tie at
    rank k (branch_b: the angle criterion is off and the keep list is in (distance, index) order, which the ranking then has to follow)."""
    ref, st = _run_batch(ctx, oracle, TIES, {"yaw_step_deg": 30.0, "consider_config_2": False, "max_cuboid_num": max_cuboid_num})
    assert any(x["tie_d"] for x in st) and any(x["branch_b"] for x in st) and any(x["tie_d"] and x["branch_b"] for x in st)
    assert any(x["n"] > 4 and not x["branch_b"] for x in st)
    assert sum(len(r) for r in ref) >= 4


@pytest.mark.parametrize("yaw_step_deg,max_cuboid_num,below,above", [(6.0, 1, 0, 64), (6.0, 5, 64, 256), (2.0, 3, 64, 256), (0.5, 5, 256, 1 << 30)])
def test_kept_lists_on_both_sides_of_the_wave_seams(ctx, oracle, yaw_step_deg, max_cuboid_num, below, above):
    """cuboid_select_geom takes the kept list 64 entries per wave, eight waves per unit: lists of at most 64 entries (one wave, seven leave at once; 64 exactly is
    among them), of 65-256, and above 512 (a wave takes a second stretch).  The case's (below, above] holds at least one unit's n_kept."""
    ref, st = _run_batch(ctx, oracle, [(3, "scene")], {"yaw_step_deg": yaw_step_deg, "max_cuboid_num": max_cuboid_num})
    kept = [x["n_kept"] for x in st]
    assert any(below < k <= above for k in kept), kept
    if yaw_step_deg == 6.0:
        assert 64 in kept and any(k > 64 for k in kept) and any(k < 64 for k in kept)
    if yaw_step_deg == 0.5:
        assert any(k > 512 for k in kept) and all(k > 256 for k in kept)
    assert all(len(r) == max_cuboid_num for r in ref)


def test_ranking_across_units_with_mixed_keep_orders(ctx, oracle):
    """whether_sample_bbox_height: three units per box, ranked together.  Boxes whose units disagree about the keep order (branch_b of one, not of the next:
    the distance enters the ranking key of some units only), one of them with a unit on the n <= 4 path, and ties at the distance threshold."""
    ref, st = _run_batch(ctx, oracle, [(2, ("rand", 1002)), (1, ("rand", 1001))], {"yaw_step_deg": 6.0, "whether_sample_bbox_height": True, "max_cuboid_num": 5})
    assert len(st) == 36 and all(x["hs"] == i % 3 for i, x in enumerate(st))
    mixed = [b for b in range(12) if len({x["branch_b"] for x in st[3 * b:3 * b + 3] if x["n_kept"] > 0}) == 2]
    assert len(mixed) >= 2, mixed
    assert any(any(0 < x["n"] <= 4 for x in st[3 * b:3 * b + 3]) for b in mixed)
    assert any(x["tie_d"] and x["branch_b"] for x in st)
    assert all(len(ref[b]) == 5 for b in mixed)


def test_roll_pitch_samples(ctx, oracle):
    """whether_sample_cam_roll_pitch: 25 camera samples per unit, the record's camera deltas; kept lists of several hundred entries."""
    ref, st = _run_batch(ctx, oracle, [(3, "scene")], {"yaw_step_deg": 6.0, "whether_sample_cam_roll_pitch": True, "max_cuboid_num": 3})
    assert all(x["n_kept"] > 256 for x in st) and any(x["n_kept"] > 512 for x in st)
    assert all(len(r) == 3 for r in ref)
    assert any(r["camera_roll_delta"].any() or r["camera_pitch_delta"].any() for r in ref)


@pytest.mark.parametrize("seed,yaw_step_deg,small", [(34, 30.0, 1), (22, 15.0, 0)])
def test_chained_call_carries_the_pose_of_few_and_of_many_proposals(ctx, oracle, seed, yaw_step_deg, small):
    """cs_cuboid_detect's chain (one batch per box, want_carry): the roll / pitch sample a box leaves behind when it has one valid proposal (n <= 4: the last of
    them in index order), none (the last sample of the loop) and hundreds (the last entry of the keep list), each handed to a box that follows.  On seed 34 the
    chain changes what a later box gives."""
    det = _det(ctx, {"whether_sample_cam_roll_pitch": True, "yaw_step_deg": yaw_step_deg, "consider_config_2": False, "max_cuboid_num": 2})
    scenes, boxes = _frames([(seed, ("rand", 1000 + seed))])
    s, bx = scenes[0], boxes[0]
    det.set_calibration(s["K"])
    got = det.detect_cuboid(s["gray"], s["Twc"], bx, s["lines"])
    ref, st = oracle_frames(oracle, scenes, boxes, _oracle_opts(oracle, det, stateful=1))
    ns = [x["n"] for x in st[0]]
    assert small in ns[:-1] and sum(n > 4 for n in ns[:-1]) >= 3, ns
    _cmp_cuboids(got, ref)
    assert sum(len(r) for r in ref) >= 9
    if seed == 34:
        other, _ = oracle_frames(oracle, scenes, boxes, _oracle_opts(oracle, det, stateful=0))
        assert any(len(a) != len(b) or any(not np.array_equal(a[f], b[f]) for f in a.dtype.names) for a, b in zip(ref, other))
