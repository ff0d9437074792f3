"""GPU: the C++ mirror (cubeslam::ObjectPoints, cube_slam_amd/host/object_points.hpp) compiled with g++ against the C-ABI library through tests/cpp/object_points_mirror.cpp, with a
context: the restatement's bytes on the largest patterns (the 257-point batch, the statuses, the batch of frames in all three modes).  Every pattern runs through the same
program without a context in tests/test_object_points_mirrors.py."""
import os
import subprocess

import pytest

from tests import object_points_patterns as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_mirror(directory):
    e = str(directory / "object_points_mirror")
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "object_points_mirror.cpp"), "-o", e, "-L", lib_dir, "-lcubeslam_hip",
                           "-Wl,-rpath," + lib_dir])
    return e


def mirror_bytes(exe, where, tmp_path, c, mode):
    (tmp_path / "in.bin").write_bytes(P.dump(c, mode))
    r = subprocess.run([exe, where, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return (tmp_path / "out.bin").read_bytes()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_mirror(tmp_path_factory.mktemp("object_points_mirror"))


@pytest.mark.parametrize("name,mode", [("tri_total_257", None), ("tri_statuses", None), ("od_batch", 0), ("od_batch", 1), ("od_batch", 2)])
def test_cpp_mirror_on_the_device(ctx, exe, tmp_path, name, mode):
    c = P.case(name)
    assert mirror_bytes(exe, "device", tmp_path, c, mode) == P.expected_bytes(c, P.expected(name, mode))
