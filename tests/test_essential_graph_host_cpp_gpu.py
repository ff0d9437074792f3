"""GPU: the C++ host mirror of the pose graph (cubeslam::OptimizeEssentialGraph, cube_slam_amd/host/essential_graph.hpp) compiled with g++ against the C-ABI library and run on
the 40-key-frame map with its 1 000 points; byte-identical to the Python mirror, which tests/test_essential_graph_gpu.py holds against the restatement."""
import os
import subprocess

import numpy as np
import pytest

from cube_slam_amd import optimizer as O
from tests import essential_graph_patterns as P
from tests import essential_graph_restatement as R
from tests.test_essential_graph_mirrors import parse, write_flat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_essential_graph_mirror_matches_python(ctx, tmp_path):
    mp, j = P.case("kf40"), P.judged("kf40")
    flat = R.flatten(mp)
    ids = [kf.mnId for kf in mp.all_kfs]
    nIDr = [ids[r] for r in j["ref"]]
    write_flat(tmp_path / "map.txt", flat, False, j["P"], nIDr)
    exe = tmp_path / "essential_graph_mirror"
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DWITH_DEVICE", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "essential_graph_mirror.cpp"), "-o", str(exe), "-L", lib_dir,
                           "-lcubeslam_hip", "-Wl,-rpath," + lib_dir])
    lines = subprocess.check_output([str(exe), str(tmp_path / "map.txt")], timeout=120).decode().split("\n")
    res = O.OptimizeEssentialGraph(flat, False, points=(j["P"], nIDr), ctx=ctx)
    g = res["graph"]
    for a, b in zip(parse(lines), [g["fixed_vertex"], g["mnId"], g["edge_i"], g["edge_j"], g["edge_kind"], g["Scw"].reshape(-1), g["Snc"].reshape(-1), g["has_nc"]]):
        assert np.array_equal(a, b)
    assert bytes.fromhex(lines[8]) == res["sim3"].tobytes() and bytes.fromhex(lines[9]) == res["Tiw"].tobytes() and bytes.fromhex(lines[10]) == res["points"].tobytes()
    assert lines[11] == "".join(str(s) for s in res["stats"]["sequence"]) and len(res["points"]) == 1000
