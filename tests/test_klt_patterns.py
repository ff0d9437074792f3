"""CPU: the preconditions of tests/klt_patterns.py, asserted on the restatement's own trace so that no pattern is vacuous: every branch of the tracker and of
SearchByTrackingHarris' selection pass that the parity tests rely on is taken at least once."""
import numpy as np

from tests import klt_patterns as kp
from tests import klt_restatement as kr


def test_every_tracker_branch_is_taken():
    seen = set()
    for w, h in kp.SIZES:
        c = kp.lk_case(w, h)
        here = set().union(*c["trace"])
        seen |= here
        assert {"pad_left", "pad_right", "pad_top", "pad_bottom", "min_eig", "eps_stop", "prev_outside_level0", "weight_zero_fraction", "weight_round_tie"} <= here, (w, h)
        assert all(0 < want[1].sum() < len(want[1]) for want in c["want"]), (w, h)  # some points are tracked and some are not, in either pair
        top = kr.n_levels(w, h) - 1
        assert ("prev_outside_upper" in here) == (top > 0), (w, h)                  # out of range above level 0: no status change there
    e = kp.edge_case()
    seen |= set().union(*e["trace"])
    n_err = sum("err_outside" in s for s in e["trace"])
    print("err-stage rejections in the edge case: %d of %d points; branches over all cases: %s" % (n_err, len(e["trace"]), sorted(seen)))
    assert n_err >= 1 and e["want"][0][1].sum() >= 1
    assert kp.LK_BRANCHES <= seen, kp.LK_BRANCHES - seen


def test_flat_patch_is_rejected_by_min_eig():
    c = kp.lk_case(64, 48)
    i = len(c["pts"][0]) - 1  # the centre of the flat patch
    assert c["trace"][i] >= {"min_eig"} and c["want"][0][1][i] == 0


def test_batch_counts_cover_the_seams():
    assert sorted(set(sum(kp.BATCH_COUNTS, []))) == [0, 1, 63, 64, 65, 130]
    b = kp.batch_case()
    assert all(0 < w[1][:63].sum() < 63 for w in b["want"])


def test_harris_selection_branches():
    c = kp.harris_case()
    assert kp.HARRIS_BRANCHES <= set().union(*c["trace"])
    w0 = c["want"][0]
    assert w0["n_mask_outside"] >= 1        # x rounds to cols on the last row: the index is rows * cols
    assert 6 in w0["object_id"]             # x rounds to cols on another row: the next row's first pixel, which carries id 7
    assert all(0 < w["goodmatches"] < w["status"].sum() for w in c["want"])  # the mask's zero third drops tracked points
    ch = kp.chain_case()
    assert [s["goodmatches"] for s in ch["steps"]] == [len(s["kept"]) for s in ch["steps"]] and 0 < ch["steps"][1]["goodmatches"] < len(ch["start"][0])
    assert np.array_equal(ch["lists"]["dobs_cam"][:len(ch["start"][0])], np.zeros(len(ch["start"][0]), np.int32))


def test_search_by_tracking_branches():
    still, moving = kp.tracking_still_case(), kp.tracking_moving_case()
    assert {"mean_flow_zero", "two_claims", "closest_tie", "no_feature"} <= still["trace"] and "direction_reject" in moving["trace"]
    assert kp.TRACKING_BRANCHES <= still["trace"] | moving["trace"]
    w = still["want"]
    # The tie: key points 0 (31, 30) and 1 (29, 30) are equally far from point 0.  Bounds (0, 240) give cells 3.75 wide, so both lie in cell column 8; inside a cell the
    # indices ascend and the strict < keeps the first: key 0.  Key 2 lies between points 1 and 2 and keeps the later claim, 2.
    assert w["train_match"].tolist() == [0, -1, 2, -1, 3, -1, 4, -1, -1, 6, -1, 10]
    assert w["kltmatches"] == 9 and w["goodmatches"] == 9 and w["findfeaturematches"] == 7 and w["uniquematches"] == 3
    assert (w["featuresklt_thisframe"][[5, 7]] == 0).all() and (w["featuresklt_thisframe"][0] == still["last_pt"][0]).all()  # no feature: (0, 0); tracked: exactly in place
    m = moving["want"]
    assert m["kltmatches"] - m["goodmatches"] == 2 and m["uniquematches"] < m["findfeaturematches"] and 3 not in moving["last_octave"][m["lastptsinds"]]
    assert any(s for s in moving["keys_static"]) and any(moving["had_map_point"])


def test_large_cases_cross_waves_and_passes():
    """The selection kernels run 64-lane waves in passes of 256: the large cases put kept, mask-0 and beyond-the-mask points into every wave of the first pass and into
    the second, and select more points than one pass of the per-point tail holds."""
    c = kp.harris_large_case()
    w = c["want"][0]
    n = len(c["pts"][0])
    assert n > 256 and w["status"][list(kp.LARGE_HARRIS_SPECIAL)].all() and w["n_mask_outside"] == len(kp.LARGE_HARRIS_SPECIAL)
    for a in range(0, n, 64):
        idx = np.arange(a, min(a + 64, n))
        assert np.isin(idx, w["kept"]).any() and (~np.isin(idx, w["kept"]) & (w["status"][idx] > 0)).any(), a  # kept points and dropped ones in this wave
    assert max(kp.LARGE_HARRIS_SPECIAL) >= 256 and {i // 64 for i in kp.LARGE_HARRIS_SPECIAL} >= {1, 2, 3, 4, 5}
    t = kp.tracking_large_case()
    sel = t["want"]["lastptsinds"]
    assert len(t["last_pt"]) > 2 * 256 and len(sel) > 256 and len(t["cur_pt"]) > 2 * 256
    assert all(((sel >= a) & (sel < a + 256)).any() for a in (0, 256, 512)) and 0 < t["want"]["uniquematches"] < t["want"]["findfeaturematches"]
    assert "two_claims" in t["trace"] and (t["want"]["train_match"] >= 256).any()
