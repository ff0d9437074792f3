"""GPU chain: ORBmatcher::SearchByTrackingHarris (cs_match_by_tracking_harris) over three consecutive synthetic frames of a moving textured box on one resident handle,
each step fed with what the step before kept, then the dynamic-point observation lists in the layout cs_ba_dyn_problem consumes (dobs_cam / dobs_obj / dobs_point /
dobs_uv).  Counts and indices are asserted against the same chain run on tests/klt_restatement.py; the bundle adjustment itself is covered by its own tests."""
import numpy as np
import pytest

from cube_slam_amd.klt import KLTTracker
from tests import klt_patterns as kp

pytestmark = pytest.mark.gpu


def test_harris_chain_feeds_the_dynamic_ba_lists(ctx):
    c = kp.chain_case()
    t = KLTTracker(3, 128, 96, 128, ctx=ctx)
    try:
        t.set_frames(c["frames"])
        per_frame = [c["start"]]
        for f in (1, 2):
            ids, _, pts = per_frame[-1]
            r = t.search_by_tracking_harris([(f - 1, f)], [pts], c["masks"][f:f + 1])[0]
            want = c["steps"][f - 1]
            assert r["goodmatches"] == want["goodmatches"] and np.array_equal(r["kept"], want["kept"]) and np.array_equal(r["object_id"], want["object_id"]), f
            per_frame.append(kp.chain_step(r, ids))
    finally:
        t.close()
    got, want = kp.dobs_lists(per_frame), c["lists"]
    assert len(got["dobs_cam"]) == len(want["dobs_cam"]) > 2 * len(c["start"][0])  # most points survive both steps
    for key in ("dobs_cam", "dobs_point", "dobs_obj"):
        assert np.array_equal(got[key], want[key]), key
    assert got["dobs_uv"].shape == (len(got["dobs_cam"]), 2) and (got["dobs_obj"] == 1).all()
    lost = [len(per_frame[f][0]) - len(per_frame[f + 1][0]) for f in range(2)]
    assert sum(lost) >= 1  # ... and some do not: the lists are not the identity
