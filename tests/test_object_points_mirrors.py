"""CPU: the host forms (ctx == NULL) of cs_triangulate_dynamic_points and cs_object_depth_points against the restatement on every pattern, bit for bit; the call-site wrappers
of cube_slam_amd/object_points.py; and csrc/object_points_math.h as a stand-alone program (tests/cpp/object_points_driver.cpp) built with g++ plainly and under
-fsanitize=address,undefined: both runs clean, both equal to the restatement.  No sanitizer goes near code loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import object_points_patterns as P
from tests import object_points_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", P.TRI_NAMES)
def test_triangulation_host_form(name):
    P.assert_equal(P.run_tri(None, P.case(name)), P.expected(name), P.TRI_KEYS, name)


@pytest.mark.parametrize("name", P.OD_NAMES)
def test_object_depth_host_form(name):
    for mode in P.MODES:
        P.assert_equal(P.run_od(None, P.case(name), mode), P.expected(name, mode), P.OD_KEYS, "%s mode %d" % (name, mode))


def test_call_site_wrappers():
    from cube_slam_amd.object_points import LocalMapping, Tracking
    c = P.case("od_more_than_80")
    args = (c["keys"], c["has_map_point"], c["object_id"], c["cuboid_depth"], c["K4"][0])
    idx, x = Tracking.MonoObjDepthInitialization(None, c["keys"], c["object_id"], c["cuboid_depth"], c["K4"][0], c["Twc"][0])
    w = P.expected("od_more_than_80", R.FIRST_FRAME)
    assert np.array_equal(idx, w["new_idx"]) and x.tobytes() == w["new_x3D"].tobytes()
    xy = np.stack([c["keys"]["x"], c["keys"]["y"]], 1)  # plain points do as well: the first-frame mode reads pt only
    assert np.array_equal(Tracking.MonoObjDepthInitialization(None, xy, c["object_id"], c["cuboid_depth"], c["K4"][0], c["Twc"][0])[0], w["new_idx"])
    P.assert_equal(Tracking.CreateNewKeyFrameObjectDepth(None, *args, c["bounds"][0], c["Twc"][0], c["draws"]), P.expected("od_more_than_80", R.TRACKING), P.OD_KEYS, "tracking")
    P.assert_equal(LocalMapping.CreateNewMapPointsObjectDepth(None, *args, c["Twc"][0], c["draws"]), P.expected("od_more_than_80", R.LOCAL_MAPPING), P.OD_KEYS, "local mapping")
    t = P.case("tri_statuses")
    got = Tracking.TriangulateDynamicPoints(None, t["Tcw_last"], t["Tcw_now"], t["K4"], t["cub_pose_last"], t["cub_pose_now"], t["kp1"], t["kp2"], t["obj_last"], t["obj_now"],
                                            t["idx_last"], t["world_pos"], t["tracklet_last"], t["tracklet_now"])
    P.assert_equal(got, P.expected("tri_statuses"), P.TRI_KEYS, "one pair")


def test_too_few_draws_is_an_error_of_the_mirror():
    from cube_slam_amd._lib import CubeSlamError
    c = dict(P.case("od_more_than_80"))
    c["draws"], c["draw_first"] = c["draws"][:79], np.array([0, 79], np.int32)
    with pytest.raises(CubeSlamError):
        P.run_od(None, c, R.TRACKING)
    with pytest.raises(R.OutOfDraws):
        R.object_depth_points(c, R.TRACKING)
    assert len(P.run_od(None, c, R.FIRST_FRAME)["new_idx"]) == 100  # the first-frame mode takes no draws


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("object_points_driver")
    src, inc = os.path.join(ROOT, "tests", "cpp", "object_points_driver.cpp"), os.path.join(ROOT, "cube_slam_amd", "csrc")
    plain, san = str(d / "driver"), str(d / "driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-ffp-contract=off", "-I", inc, src, "-o", plain])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc, src,
                           "-o", san])
    return plain, san


def _run(exe, tmp_path, data):
    (tmp_path / "in.bin").write_bytes(data)
    out = tmp_path / ("out_%s.bin" % os.path.basename(exe))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(out)], capture_output=True, text=True, timeout=120)
    return r, out


@pytest.mark.parametrize("name", P.NAMES)
def test_driver_plain_and_sanitized(drivers, tmp_path, name):
    c = P.case(name)
    for mode in (P.MODES if c["kind"] == "od" else (None,)):
        outs = []
        for exe in drivers:
            r, out = _run(exe, tmp_path, P.dump(c, mode))
            assert r.returncode == 0 and r.stderr == "", r.stderr
            outs.append(out.read_bytes())
        assert outs[0] == outs[1] == P.expected_bytes(c, P.expected(name, mode)), (name, mode)


def test_driver_refuses_too_few_draws(drivers, tmp_path):
    c = dict(P.case("od_more_than_80"))
    c["draws"], c["draw_first"] = c["draws"][:79], np.array([0, 79], np.int32)
    for exe in drivers:
        r, _ = _run(exe, tmp_path, P.dump(c, R.TRACKING))
        assert r.returncode == 3 and "returned -2" in r.stderr


@pytest.fixture(scope="module")
def mirror_exe(tmp_path_factory):
    from tests.test_object_points_host_cpp_gpu import build_mirror
    return build_mirror(tmp_path_factory.mktemp("object_points_mirror_host"))


@pytest.mark.parametrize("name", P.NAMES)
def test_cpp_mirror_over_the_host_forms(mirror_exe, tmp_path, name):
    """cubeslam::ObjectPoints (cube_slam_amd/host/object_points.hpp) without a context: the restatement's bytes on every pattern."""
    from tests.test_object_points_host_cpp_gpu import mirror_bytes
    c = P.case(name)
    for mode in (P.MODES if c["kind"] == "od" else (None,)):
        assert mirror_bytes(mirror_exe, "host", tmp_path, c, mode) == P.expected_bytes(c, P.expected(name, mode)), (name, mode)
