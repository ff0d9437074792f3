"""GPU chain, the one the reference runs in dynamic mode: on three small frames of a shifted texture with two object masks, new Harris features on frame 0 from
nothing (cs_track_new_harris_features), ORBmatcher::SearchByTrackingHarris 0 -> 1 (cs_match_by_tracking_harris), new features on frame 1 with the kept points as
existing ones, all on one resident handle; then the observation lists in the layout cs_ba_dyn_problem consumes.  Everything equals the restatements run through the
same steps."""
import numpy as np
import pytest

from cube_slam_amd.klt import KLTTracker
from tests import gftt_patterns as gp
from tests import klt_patterns as kp

pytestmark = pytest.mark.gpu


def test_detect_track_detect_feeds_the_dynamic_ba_lists(ctx):
    c = gp.chain_case()
    frames, masks = c["frames"], c["masks"]
    t = KLTTracker(3, frames.shape[2], frames.shape[1], 256, ctx=ctx)

    def detect(f):
        return lambda p, o: t.new_harris_features([f], masks[f:f + 1], [p], [o], gp.K4, gp.TWC[None], [gp.CHAIN_DEPTH], good_masks=True)[0]
    try:
        t.set_frames(frames)
        none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32))
        f0, r0 = gp.chain_new_features(frames[0], masks[0], none, detect(0))
        assert gp.same_harris(r0, c["new0"]) and len(r0["pts"]) >= 20 and set(r0["object_id"]) == {0, 1}
        step = t.search_by_tracking_harris([(0, 1)], [f0[2]], masks[1:2])[0]
        assert kp.same_harris(step, c["step"]) and step["goodmatches"] >= 20
        f1, r1 = gp.chain_new_features(frames[1], masks[1], kp.chain_step(step, f0[0]), detect(1))
        assert gp.same_harris(r1, c["new1"]) and len(r1["pts"]) >= 1
    finally:
        t.close()
    drawn = [i for i, what in c["trace"] if what == "drawn"]
    assert len(drawn) >= 20 and any(what == "zero" for _, what in c["trace"])          # a tracked point inside an earlier disc draws nothing
    tracked = kp.chain_step(step, f0[0])[2]
    for x, y in r1["pts"]:
        assert r1["good"][int(y), int(x)] == 255                                        # no new corner in a drawn disc ...
        for i in drawn:
            rx, ry = int(np.rint(tracked[i][0])), int(np.rint(tracked[i][1]))
            assert abs(int(y) - ry) > 10 or abs(int(x) - rx) > (10, 9, 9, 9, 9, 8, 8, 7, 6, 4, 0)[abs(int(y) - ry)]
    for f, (ids, obj, pts) in enumerate((f0, f1)):
        new = pts[-len((r0, r1)[f]["pts"]):]
        assert (masks[f][new[:, 1].astype(int), new[:, 0].astype(int)] - 1 == obj[-len(new):]).all()     # ... and the ids match the masks
    got, want = kp.dobs_lists([f0, f1]), c["lists"]
    for key in ("dobs_cam", "dobs_point", "dobs_obj"):
        assert np.array_equal(got[key], want[key]), key
    assert got["dobs_uv"].tobytes() == want["dobs_uv"].tobytes() and got["dobs_uv"].shape == (len(f0[0]) + len(f1[0]), 2)
    assert len(set(f1[0])) == len(f1[0]) and set(f0[0]) <= set(f1[0]) | set(f0[0])
