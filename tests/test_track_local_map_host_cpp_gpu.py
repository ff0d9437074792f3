"""GPU: the C++ mirror of Tracking::TrackLocalMap (cubeslam::Tracking, cube_slam_amd/host/tracking.hpp) compiled with g++ against the C-ABI library through
tests/cpp/tracking_mirror.cpp: byte-equal to the Python mirror (cube_slam_amd/tracking.py) on the seeded map of the chain test -- local key frames and points, the search's
outputs, the frame's map points, outlier flags, the pose, the counts and the visible / found statistics."""
import os
import subprocess

import numpy as np
import pytest

from tests import sim3_restatement as S
from tests import track_local_map_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("tracking_mirror") / "tracking_mirror")
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "tracking_mirror.cpp"), "-o", e, "-L", lib_dir,
                           "-lcubeslam_hip", "-Wl,-rpath," + lib_dir])
    return e


def test_cpp_mirror_equals_python_mirror(ctx, oracle, exe, tmp_path):
    from cube_slam_amd.tracking import Tracking
    frames = S.frames(oracle)
    cm = R.chain_map(frames)
    (tmp_path / "in.bin").write_bytes(R.pack(R.chain_arrays(frames, cm)))
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=60)
    m, F = R.chain_objects(frames, cm)
    t = Tracking(ctx=ctx)
    ok = t.TrackLocalMap(F, m)
    s = t.last_search
    t.close()
    assert s["nmatches"] >= 300 and t.mnMatchesInliers >= 100
    i32 = np.int32
    want = R.pack([t.mvpLocalKeyFrames.astype(i32), t.mvpLocalMapPoints.astype(i32), s["train_match"].astype(i32), s["in_view"].astype(np.uint8), s["pred_level"].astype(i32),
                   s["proj"].astype(np.float32), s["view_cos"].astype(np.float32), F.mvpMapPoints.astype(i32), F.mvbOutlier.astype(np.uint8), F.pose7.astype(np.float64),
                   np.asarray([s["nmatches"], s["n_to_match"], s["outside"], t.mnMatchesInliers, int(ok), t.mpReferenceKF], i32), m.visible.astype(np.int64), m.found.astype(np.int64)])
    assert (tmp_path / "out.bin").read_bytes() == want
