"""GPU: cs_triangulate_dynamic_points and cs_object_depth_points on the device, through the C-ABI, on every pattern of tests/object_points_patterns.py: bit-equal to the host form
(and so to the restatement, tests/test_object_points_mirrors.py): status bytes, x3D, PosToObj in both widths, the candidate lists before and after the draws, new_idx in
creation order and new_x3D.  The largest cases are the 257-point batch and the 100-candidate frame."""
import numpy as np
import pytest

from tests import object_points_patterns as P
from tests import object_points_restatement as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", P.TRI_NAMES)
def test_triangulation(ctx, name):
    c = P.case(name)
    got, host = P.run_tri(ctx, c), P.run_tri(None, c)
    P.assert_equal(got, host, P.TRI_KEYS, name + " against the host form")
    P.assert_equal(got, P.expected(name), P.TRI_KEYS, name + " against the restatement")


@pytest.mark.parametrize("name", P.OD_NAMES)
@pytest.mark.parametrize("mode", P.MODES)
def test_object_depth(ctx, name, mode):
    c = P.case(name)
    got, host = P.run_od(ctx, c, mode), P.run_od(None, c, mode)
    P.assert_equal(got, host, P.OD_KEYS, "%s mode %d against the host form" % (name, mode))
    P.assert_equal(got, P.expected(name, mode), P.OD_KEYS, "%s mode %d against the restatement" % (name, mode))


@pytest.mark.parametrize("mode", P.MODES)
def test_object_depth_compaction_seams(ctx, mode):
    """Both ordered compactions of od_frame at the seams of a wave and of a pass of 256 threads, nothing and everything flagged (P.od_compaction_seams)."""
    from tests import compaction_seams as cs
    c = P.case("od_compaction_seams")
    got = P.run_od(ctx, c, mode)
    P.assert_equal(got, P.run_od(None, c, mode), P.OD_KEYS, "mode %d against the host form" % mode)
    P.assert_equal(got, P.expected("od_compaction_seams", mode), P.OD_KEYS, "mode %d against the restatement" % mode)
    want_n = [k for n, _, fl in cs.cases() for k in (int(fl.sum()), n)]
    assert np.asarray(got["n_candidates"]).tolist() == want_n
    if mode == R.FIRST_FRAME:
        assert np.diff(got["new_first"]).tolist() == [int(fl.sum()) for _, _, fl in cs.cases() for _ in range(2)]


def test_c_abi_directly(ctx):
    """Both entry points with nothing of the Python mirror between: buffers sized by hand, canaries behind every output."""
    from cube_slam_amd._lib import lib, ptr
    c, want = P.case("tri_total_257"), P.expected("tri_total_257")
    n = 257
    st, x, o, d = np.full(n + 5, 77, np.uint8), np.full(3 * n + 5, 77, np.float32), np.full(3 * n + 5, 77, np.float32), np.full(3 * n + 5, 77, np.float64)
    r = lib().cs_triangulate_dynamic_points(ctx.ptr, 2, ptr(c["first"]), ptr(c["Tcw_last"]), ptr(c["Tcw_now"]), ptr(c["K4"]), ptr(c["cub_first_last"]), ptr(c["cub_pose_last"]),
                                            ptr(c["cub_first_now"]), ptr(c["cub_pose_now"]), None, None, ptr(c["kp1"]), ptr(c["kp2"]), ptr(c["obj_last"]), ptr(c["obj_now"]),
                                            ptr(c["idx_last"]), ptr(c["world_pos"]), ptr(st), ptr(x), ptr(o), ptr(d))
    assert r == 0
    for got, key in ((st, "status"), (x, "x3D"), (o, "pos_to_obj"), (d, "dpoints")):
        w = want[key].reshape(-1)
        assert got[:len(w)].tobytes() == w.tobytes() and (got[len(w):] == 77).all(), key
    c, want = P.case("od_batch"), P.expected("od_batch", R.TRACKING)
    F, nc, nn = len(c["first"]) - 1, len(want["candidates"]), len(want["new_idx"])
    i32 = lambda k: np.full(k + 4, -77, np.int32)
    outs = [i32(F), i32(F), i32(F), i32(F + 1), i32(int(c["first"][-1])), i32(int(c["first"][-1])), i32(F + 1), i32(int(c["first"][-1])), np.full(3 * int(c["first"][-1]) + 4, -77, np.float32)]
    r = lib().cs_object_depth_points(ctx.ptr, R.TRACKING, F, ptr(c["first"]), ptr(c["keys"]), ptr(c["has_map_point"]), ptr(c["object_id"]), ptr(c["cub_first"]), ptr(c["cuboid_depth"]),
                                     ptr(c["K4"]), ptr(c["bounds"]), ptr(c["Twc"]), ptr(c["draw_first"]), ptr(c["draws"]), *[ptr(a) for a in outs])
    assert r == 0
    for got, key in zip(outs, P.OD_KEYS):
        w = want[key].reshape(-1)
        assert got[:len(w)].tobytes() == w.tobytes() and (got[len(w):] == -77).all(), key  # (nothing is written behind the entries a frame has)
    assert nc == 121 and nn == 97


def test_bad_arguments_reach_no_kernel(ctx):
    """The checks of tests/test_object_points_cabi.py with a context: the error text names the function, nothing is written."""
    from cube_slam_amd._lib import CubeSlamError
    c = dict(P.case("tri_statuses"))
    c["obj_last"] = c["obj_last"].copy()
    c["obj_last"][3] = 2
    with pytest.raises(CubeSlamError, match="cs_triangulate_dynamic_points: an object row outside"):
        P.run_tri(ctx, c)
    c = dict(P.case("od_more_than_80"))
    c["draws"], c["draw_first"] = c["draws"][:79], np.array([0, 79], np.int32)
    with pytest.raises(CubeSlamError, match="fewer draws than max_initialize_pts"):
        P.run_od(ctx, c, R.TRACKING)
    P.assert_equal(P.run_od(ctx, c, R.FIRST_FRAME), P.expected("od_more_than_80", R.FIRST_FRAME), P.OD_KEYS, "the context is usable behind the error")
