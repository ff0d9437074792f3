"""GPU: the C++ mirror of Initializer (cubeslam::Initializer, cube_slam_amd/host/initializer.hpp) compiled with g++ against the C-ABI library through
tests/cpp/initializer_mirror.cpp, with a cubeslam::Context: evaluate_many is one cs_initializer_evaluate on the device for every pattern.  Its tables and Initialize results
equal those of the same program built with CUBESLAM_HOST_ONLY (no context, nothing of the library) and those of the Python mirror on the host path, byte for byte but for
the NaN of RH in the two cases without a model (a NaN equals any NaN: x86 and the device give NaNs of different sign)."""
import os
import subprocess

import numpy as np
import pytest

from tests import initializer_patterns as P
from tests.test_initializer_mirrors import driver_input, expected_output

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("initializer_mirror_device")
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    base = ["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "initializer_mirror.cpp")]
    subprocess.check_call(base + ["-o", str(d / "device"), "-L", lib_dir, "-lcubeslam_hip", "-Wl,-rpath," + lib_dir])
    subprocess.check_call(base + ["-DCUBESLAM_HOST_ONLY", "-o", str(d / "host")])
    return d


@pytest.mark.parametrize("mode", ["table", "draw"])
def test_cpp_mirror_with_a_context_equals_the_one_without(ctx, exes, tmp_path, mode):
    (tmp_path / "in.bin").write_bytes(driver_input(P.ALL))
    out = {}
    for exe in ("device", "host"):
        subprocess.check_call([str(exes / exe), str(tmp_path / "in.bin"), str(tmp_path / (exe + ".bin"))] + (["draw"] if mode == "draw" else []), timeout=120)
        out[exe] = (tmp_path / (exe + ".bin")).read_bytes()
    assert out["host"] == expected_output(P.ALL)
    dev, host = np.frombuffer(out["device"], np.uint8), np.frombuffer(out["host"], np.uint8)
    assert len(dev) == len(host)
    differ = np.nonzero(dev != host)[0]
    # RH of `no_model` and of `empty`, the only NaNs of the patterns: at most 4 bytes each, and where they differ both sides hold a NaN
    assert len(differ) <= 8
    for at in differ:
        lo = [k for k in range(at - 3, at + 1) if np.isnan(np.frombuffer(out["host"][k:k + 4], np.float32)[0]) and np.isnan(np.frombuffer(out["device"][k:k + 4], np.float32)[0])]
        assert lo, at
