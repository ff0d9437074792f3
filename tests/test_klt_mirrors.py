"""CPU: the mirrors of the dynamic-object KLT on their path without a context against tests/klt_restatement.py, byte for byte on next_pts, status, err and every output
of SearchByTrackingHarris: the library's host statement over csrc/klt_math.h (calcOpticalFlowPyrLK / SearchByTrackingHarris with ctx=None), and the C++ mirror built with
g++ and -DCUBESLAM_HOST_ONLY from tests/cpp/klt_mirror.cpp, plain and a second time under the sanitizers, each run as a child process."""
import os
import subprocess

import numpy as np
import pytest

from cube_slam_amd import SearchByTrackingHarris, _lib, calcOpticalFlowPyrLK
from tests import klt_patterns as kp

f32 = np.float32


@pytest.mark.parametrize("w,h", kp.SIZES)
def test_host_path_equals_restatement(w, h):
    c = kp.lk_case(w, h)
    got = calcOpticalFlowPyrLK(c["frames"], c["pairs"], c["pts"])
    for p, (g, want) in enumerate(zip(got, c["want"])):
        assert kp.same_track(g, want), (p, np.flatnonzero((g[0] != want[0]).any(1) | (g[1] != want[1]) | (g[2] != want[2])))
    assert not kp.same_track(calcOpticalFlowPyrLK(c["frames"], [(1, 0)], c["pts"][:1])[0], c["want"][0])  # the pair the other way round is another answer


def test_host_path_edge_batches_and_strided_rows():
    e = kp.edge_case()
    assert kp.same_track(calcOpticalFlowPyrLK(e["frames"], e["pairs"], e["pts"])[0], e["want"][0])
    for counts in kp.BATCH_COUNTS:
        pairs, pts, want = kp.batch_call(counts)
        got = calcOpticalFlowPyrLK(kp.batch_case()["frames"], pairs, pts)
        assert all(kp.same_track(g, w) for g, w in zip(got, want)) and [len(g[0]) for g in got] == counts
    c = kp.lk_case(42, 64)
    wide = np.full((3, 64, 50), 99, np.uint8)
    wide[:, :, :42] = c["frames"]
    assert kp.same_track(calcOpticalFlowPyrLK(wide[:, :, :42], c["pairs"][:1], c["pts"][:1])[0], c["want"][0])


def test_host_search_by_tracking_harris():
    c = kp.harris_case()
    got = SearchByTrackingHarris(c["frames"], c["pairs"], c["pts"], c["masks"])
    assert all(kp.same_harris(g, w) for g, w in zip(got, c["want"]))
    ch = kp.chain_case()
    ids, _, pts = ch["start"]
    for f in (1, 2):
        r = SearchByTrackingHarris(ch["frames"], [(f - 1, f)], [pts], ch["masks"][f:f + 1])[0]
        assert kp.same_harris(r, ch["steps"][f - 1])
        ids, _, pts = kp.chain_step(r, ids)


def test_host_arguments():
    c = kp.lk_case(64, 48)
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG"):
        calcOpticalFlowPyrLK(c["frames"], [(0, 3)], c["pts"][:1])                    # no such frame
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG"):
        calcOpticalFlowPyrLK(c["frames"][:, :21], [(0, 1)], c["pts"][:1])            # no window fits 21 rows
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG"):
        calcOpticalFlowPyrLK(c["frames"], [(0, 1)], [np.array([[np.inf, 3.0]], f32)])
    assert [len(g[0]) for g in calcOpticalFlowPyrLK(c["frames"], [(0, 1), (1, 2)], [np.zeros((0, 2), f32)] * 2)] == [0, 0]


def test_cpp_mirror_without_the_library(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-DCUBESLAM_HOST_ONLY", "-I", root, os.path.join(root, "tests", "cpp", "klt_mirror.cpp")]
    subprocess.check_call(base + ["-O2", "-o", str(tmp_path / "mirror")])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(tmp_path / "mirror_san")])
    pairs = kp.mirror_pairs()
    kp.write_mirror_input(tmp_path / "in.bin", pairs)
    for exe in ("mirror", "mirror_san"):
        subprocess.check_call([str(tmp_path / exe), str(tmp_path / "in.bin"), str(tmp_path / (exe + ".out")), "host"], timeout=120)
        res = kp.read_mirror_output(tmp_path / (exe + ".out"), pairs)
        for i, ((_, _, _, mask, want), got) in enumerate(zip(pairs, res)):
            assert kp.same_track(got, want), (exe, i)
    assert subprocess.call([str(tmp_path / "mirror"), str(tmp_path / "in.bin"), str(tmp_path / "x.out")], stderr=subprocess.DEVNULL) == 2  # no device path in this build


def _tracking_host(c, keys_static, had_map_point):
    from cube_slam_amd import SearchByTracking
    lk, ck = kp.tracking_keys(c)
    return SearchByTracking(c["frames"][0], c["frames"][1], lk, c["eligible"], c["object_id"], c["numobject"], kp.TH, kp.SCALE_FACTORS, ck, c["bounds"], keys_static, had_map_point)


@pytest.mark.parametrize("case", ["still", "moving"])
def test_host_search_by_tracking(case):
    from tests import klt_restatement as kr
    c = kp.tracking_still_case() if case == "still" else kp.tracking_moving_case()
    assert kp.same_tracking(_tracking_host(c, c["keys_static"], c["had_map_point"]), c["want"])
    bare = kr.search_by_tracking(c["frames"][0], c["frames"][1], c["last_pt"], c["last_octave"], c["eligible"], c["object_id"], c["numobject"], kp.TH, kp.SCALE_FACTORS,
                                 kr.FrameGrid(c["cur_pt"], c["cur_octave"], c["bounds"]))
    got = _tracking_host(c, None, None)  # no KeysStatic, no earlier map points
    assert kp.same_tracking(got, bare) and got["uniquematches"] == (got["train_match"] >= 0).sum() and not kp.same_tracking(got, c["want"])


def test_host_search_by_tracking_arguments():
    c = dict(kp.tracking_still_case())
    c["object_id"] = np.where(np.arange(len(c["object_id"])) == 3, 2, c["object_id"]).astype(np.int32)  # a tracked point of object 2 with numobject = 2
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG"):
        _tracking_host(c, None, None)
    c["object_id"][3], c["object_id"][9] = 1, -5  # point 9 is not eligible: its id is never read
    assert kp.same_tracking(_tracking_host(c, c["keys_static"], c["had_map_point"]), kp.tracking_still_case()["want"])
    c["eligible"] = np.zeros(len(c["eligible"]), np.uint8)  # nothing to track
    r = _tracking_host(c, None, None)
    assert len(r["lastptsinds"]) == 0 and (r["train_match"] == -1).all() and r["kltmatches"] == 0


def test_tracking_track_harris_features_on_the_host():
    from cube_slam_amd import Tracking
    c = kp.harris_case()
    ids = np.arange(100, 100 + len(c["pts"][0]))
    pts, mps, obj, r = object.__new__(Tracking).TrackHarrisFeatures(c["frames"][0], c["frames"][1], c["pts"][0], ids, c["masks"][0])
    assert kp.same_harris(r, c["want"][0]) and np.array_equal(mps, ids[c["want"][0]["kept"]]) and pts.tobytes() == c["want"][0]["pts"].tobytes()


def test_host_large_cases():
    c = kp.harris_large_case()
    assert kp.same_harris(SearchByTrackingHarris(c["frames"], c["pairs"], c["pts"], c["masks"])[0], c["want"][0])
    t = kp.tracking_large_case()
    assert kp.same_tracking(_tracking_host(t, t["keys_static"], t["had_map_point"]), t["want"])
