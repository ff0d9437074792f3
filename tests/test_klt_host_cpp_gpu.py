"""GPU: the C++ host mirror of the dynamic-object KLT (cubeslam::ORBmatcher::calcOpticalFlowPyrLK / SearchByTrackingHarris, cube_slam_amd/host/orb_slam_mirrors.hpp)
compiled with g++ against the C-ABI library and run on the device; byte-identical to the same program on its path without a context and to the restatement."""
import os
import subprocess

import pytest

from tests import klt_patterns as kp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_klt_mirror_on_the_device(ctx, tmp_path):
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "klt_mirror.cpp"), "-o", str(tmp_path / "mirror"),
                           "-L", lib_dir, "-lcubeslam_hip", "-Wl,-rpath," + lib_dir])
    pairs = kp.mirror_pairs()
    kp.write_mirror_input(tmp_path / "in.bin", pairs)
    subprocess.check_call([str(tmp_path / "mirror"), str(tmp_path / "in.bin"), str(tmp_path / "device.out")], timeout=300)
    subprocess.check_call([str(tmp_path / "mirror"), str(tmp_path / "in.bin"), str(tmp_path / "host.out"), "host"], timeout=300)
    assert (tmp_path / "device.out").read_bytes() == (tmp_path / "host.out").read_bytes()
    for i, ((_, _, _, mask, want), got) in enumerate(zip(pairs, kp.read_mirror_output(tmp_path / "device.out", pairs))):
        assert kp.same_track(got, want), i
