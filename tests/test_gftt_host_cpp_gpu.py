"""GPU: the C++ host mirrors cubeslam::goodFeaturesToTrack (cube_slam_amd/host/orb_slam_mirrors.hpp) and cubeslam::Tracking::CreateNewHarrisFeatures
(cube_slam_amd/host/tracking.hpp) compiled with g++ against the C-ABI library and run on the device; byte-identical to the same program on its path without a context
and to the restatement."""
import os
import subprocess

import pytest

from tests import gftt_patterns as gp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_gftt_mirror_on_the_device(ctx, tmp_path):
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "gftt_mirror.cpp"), "-o", str(tmp_path / "mirror"),
                           "-L", lib_dir, "-lcubeslam_hip", "-Wl,-rpath," + lib_dir])
    feats = [gp.size_case(w, h) for w, h in gp.SIZES] + list(gp.designed_cases().values())
    harris = list(gp.harris_cases().values()) + [gp.depth_case("missing")]
    gp.write_mirror_input(tmp_path / "in.bin", feats, harris)
    subprocess.check_call([str(tmp_path / "mirror"), str(tmp_path / "in.bin"), str(tmp_path / "device.out")], timeout=300)
    subprocess.check_call([str(tmp_path / "mirror"), str(tmp_path / "in.bin"), str(tmp_path / "host.out"), "host"], timeout=300)
    assert (tmp_path / "device.out").read_bytes() == (tmp_path / "host.out").read_bytes()
    for i, (c, got) in enumerate(zip(feats + harris, gp.read_mirror_output(tmp_path / "device.out", feats, harris))):
        if c["want"] is None:
            assert got["status"] == 2, i
            continue
        assert got["status"] == 0 and (gp.same_features if i < len(feats) else gp.same_harris)(got, c["want"]), i
