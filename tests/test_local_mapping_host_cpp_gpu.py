"""GPU: the C++ mirror of local mapping (cubeslam::LocalMapping, cube_slam_amd/host/local_mapping.hpp) compiled with g++ against the C-ABI library through
tests/cpp/local_mapping_mirror.cpp: byte-equal to the Python mirror (cube_slam_amd/local_mapping.py) on two patterns -- the neighbour loop with its baseline tests and its
prefix rule, the distinctive descriptors and the normals."""
import os
import subprocess

import numpy as np
import pytest

from tests import local_mapping_patterns as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("local_mapping_mirror") / "local_mapping_mirror")
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "local_mapping_mirror.cpp"), "-o", e, "-L", lib_dir,
                           "-lcubeslam_hip", "-Wl,-rpath," + lib_dir])
    return e


def _frame_bytes(f):
    i32 = lambda v: np.int32(v).tobytes()
    cam = np.concatenate([f.Rcw, f.tcw, f.Ow, [f.fx, f.fy, f.cx, f.cy, f.invfx, f.invfy, f.mbf, f.mb]]).astype(np.float32)
    return b"".join([i32(f.N), f.keysUn.tobytes(), f.keys_xy.astype(np.float32).tobytes(), f.u_right.tobytes(), f.depth.tobytes(), cam.tobytes(), i32(f.n_levels),
                     f.scale_factors.tobytes(), f.level_sigma2.tobytes(), np.float32(f.scale_factor).tobytes()])


@pytest.mark.parametrize("name,desc_kind,n_points", [("n3_mixed", "sizes", 65), ("statuses", "ties", 64)])
def test_cpp_mirror_equals_python_mirror(ctx, exe, tmp_path, name, desc_kind, n_points):
    from cube_slam_amd.local_mapping import ComputeDistinctiveDescriptors, KeyFrameView, LocalMapping, UpdateNormalAndDepth
    s = P.scene(name)
    doff, desc = P.descriptor_sets(desc_kind)
    c = P.normal_case(n_points)
    i32 = lambda v: np.asarray(v, np.int32).tobytes()
    blob = [i32(len(s["neighbours"])), _frame_bytes(s["kf"])] + [_frame_bytes(f) for f in s["neighbours"]] + [s["skip1"].astype(np.uint8).tobytes()]
    blob += [i32(t) for t in s["best2"]]
    blob += [i32(len(doff) - 1), i32(doff), desc.tobytes()]
    blob += [i32(n_points), c["pos"].tobytes(), i32(c["obs_off"]), i32(c["obs_kf"]), i32(c["n_kf"]), c["kf_Ow"].tobytes(), i32(c["ref_kf"]), i32(c["ref_octave"]), i32(P.N_LEVELS),
             P.SF.tobytes()]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=60)
    got = (tmp_path / "out.bin").read_bytes()

    view = lambda f: KeyFrameView(f.keysUn.copy(), f.keys_xy, f.u_right, f.depth, f.Rcw, f.tcw, f.Ow, f.fx, f.fy, f.cx, f.cy, f.invfx, f.invfy, f.mbf, f.mb, f.scale_factors,
                                  f.level_sigma2, f.scale_factor)
    views = [view(f) for f in s["neighbours"]]
    index = {id(v): i for i, v in enumerate(views)}
    lm = LocalMapping(ctx=ctx, monocular=False)
    r = lm.CreateNewMapPoints(view(s["kf"]), views, [None] * len(views), [None] * len(views),
                              search=lambda kf, nb, F12, epi: np.where(s["skip1"], -1, s["best2"][index[id(nb)]]).astype(np.int32))
    assert 0 < len(r["kept"]) < len(views) and r["nnew"] >= 3
    before = lm.points_before(r, r["kept"][-1])
    best = ComputeDistinctiveDescriptors(ctx, doff, desc)
    seven = lambda *shape: np.full(shape, 7.0, np.float32)
    nv, mn, mx, up = UpdateNormalAndDepth(ctx, c["pos"], c["obs_off"], c["obs_kf"], c["kf_Ow"], c["ref_kf"], c["ref_octave"], P.SF, seven(n_points, 3), seven(n_points), seven(n_points))
    want = b"".join([i32(r["kept"]), i32(r["pair_off"]), i32(r["idx1"]), i32(r["idx2"]), i32(r["pair_neighbour"]), r["x3D"].tobytes(), r["status"].tobytes(),
                     i32(r["new_pair_of_idx1"]), i32(r["nnew"]), i32(r["new_neighbour"]), i32(r["new_idx1"]), i32(r["new_idx2"]), r["new_x3D"].tobytes(), i32(len(before[0])),
                     i32(best), nv.tobytes(), mn.tobytes(), mx.tobytes(), up.tobytes()])
    assert got == want
