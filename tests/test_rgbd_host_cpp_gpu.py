"""GPU: the C++ host mirror of the RGB-D frame and of the close-point rule (cubeslam::Frame::ComputeStereoFromRGBD / UnprojectStereo / UpdatePoseMatrices and
cubeslam::ClosePoints, cube_slam_amd/host/orb_slam_mirrors.hpp) compiled with g++ against the C-ABI library and run on the device; byte-identical to the Python mirror
on the device, to the same program on its path without a context and to the program built with CUBESLAM_HOST_ONLY (tests/test_rgbd_mirrors.py runs that one under
the sanitizers on the CPU)."""
import os
import subprocess

import pytest

from cube_slam_amd.rgbd import ClosePoints, ComputeStereoFromRGBD
from tests import rgbd_restatement as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_rgbd_mirror_matches_python(ctx, tmp_path):
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    base = ["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "rgbd_mirror.cpp")]
    subprocess.check_call(base + ["-o", str(tmp_path / "mirror"), "-L", lib_dir, "-lcubeslam_hip", "-Wl,-rpath," + lib_dir])
    subprocess.check_call(base + ["-DCUBESLAM_HOST_ONLY", "-o", str(tmp_path / "mirror_host")])
    frames = rr.mirror_frames()
    rr.write_mirror_input(tmp_path / "in.bin", frames)
    subprocess.check_call([str(tmp_path / "mirror"), str(tmp_path / "in.bin"), str(tmp_path / "device.out")], timeout=300)
    subprocess.check_call([str(tmp_path / "mirror"), str(tmp_path / "in.bin"), str(tmp_path / "host.out"), "host"], timeout=300)
    subprocess.check_call([str(tmp_path / "mirror_host"), str(tmp_path / "in.bin"), str(tmp_path / "only.out"), "host"], timeout=300)
    device = (tmp_path / "device.out").read_bytes()
    assert device == (tmp_path / "host.out").read_bytes() == (tmp_path / "only.out").read_bytes()
    some = 0
    for fr, (ur, dep, counts, r, again) in zip(frames, rr.read_mirror_output(tmp_path / "device.out", frames)):
        pu, pd, pc = ComputeStereoFromRGBD(fr["image"], fr["keys"], fr["keysUn"], fr["bf"], fr["factor"], ctx=ctx, counts=True)
        assert ur.tobytes() == pu.tobytes() and dep.tobytes() == pd.tobytes() and counts == pc
        want = ClosePoints(pd, fr["keysUn"], fr["need_new"], fr["Tcw"], fr["K4"], fr["th"], fr["mode"], ctx=ctx)
        assert (r["n_valid"], r["n_walked"]) == (want["n_valid"], want["n_walked"])
        assert all(r[k].tobytes() == want[k].tobytes() for k in ("order", "new_idx", "new_x3D")) and again.tobytes() == r["new_x3D"].tobytes()
        some += 0 < len(r["new_idx"]) < r["n_valid"]
    assert some >= 2
