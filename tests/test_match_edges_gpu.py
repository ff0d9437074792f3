"""GPU parity of the matcher (cube_slam_amd/csrc/match.hip) on the designed inputs of tests/match_patterns.py: the device equals the oracle (tests/sim3_restatement.py for the
relocalisation search) on every case -- match vectors and counts are integers, compared with array_equal.  tests/test_match_patterns.py shows on the CPU that the oracle gives
what each case derives by construction and that the seams are reached."""
import numpy as np
import pytest

from cube_slam_amd._lib import CubeSlamError
from cube_slam_amd.matcher import ORBmatcher, hamming_knn2
from tests import match_patterns as mp
from tests.match_patterns import BOW, BOWKF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(ctx):
    m = ORBmatcher(ctx=ctx, max_keypoints=10000, max_queries=4096)  # (9 600 train key points: the first size match_resolve refuses)
    yield m
    m.close()


def _set(m, keys, desc=None):
    m.set_frame(keys, np.zeros((len(keys), 32), np.uint8) if desc is None else desc, mp.BOUNDS)


# ----------------------------------------------------------------------------------------------- match_grid, read back through GetFeaturesInArea
def test_grid_borders(matcher, oracle):
    keys, exp = mp.grid_borders()
    _set(matcher, keys)
    F = oracle.make_frame(keys, np.zeros((len(keys), 32), np.uint8), mp.BOUNDS)
    assert np.array_equal(matcher.GetFeaturesInArea(512.0, 384.0, 5000.0), oracle.get_features_in_area(F, 512.0, 384.0, 5000.0))
    for i in range(len(exp)):  # the region of every border point: both cells it could have been rounded into
        x, y = float(keys["x"][i]), float(keys["y"][i])
        assert np.array_equal(matcher.GetFeaturesInArea(x, y, 9.0), oracle.get_features_in_area(F, x, y, 9.0)), (x, y)


@pytest.mark.parametrize("N", mp.GRID_SIZES)
def test_grid_sizes(matcher, oracle, N):
    keys = mp.grid_scatter(N)
    _set(matcher, keys)
    F = oracle.make_frame(keys, np.zeros((len(keys), 32), np.uint8), mp.BOUNDS)
    assert np.array_equal(matcher.GetFeaturesInArea(512.0, 384.0, 5000.0), oracle.get_features_in_area(F, 512.0, 384.0, 5000.0))
    for cx, cy in ((0, 0), (31, 23), (63, 47), (5, 40)):  # cell regions: the lists of a 3 x 3 block around a cell, whole
        a = matcher.GetFeaturesInArea(16.0 * cx, 16.0 * cy, 24.0)
        assert np.array_equal(a, oracle.get_features_in_area(F, 16.0 * cx, 16.0 * cy, 24.0))


def test_grid_one_cell_and_corner_cells(matcher, oracle):
    keys = mp.grid_one_cell()
    _set(matcher, keys)
    assert np.array_equal(matcher.GetFeaturesInArea(160.0, 160.0, 20.0), np.arange(1500)), "1 500 key points of one cell, given in descending x, listed in ascending index"
    assert len(matcher.GetFeaturesInArea(192.0, 160.0, 15.0)) == 0
    keys = mp.grid_corner_cells()
    _set(matcher, keys)
    assert list(matcher.GetFeaturesInArea(512.0, 384.0, 5000.0)) == [0, 2, 4, 6, 8, 1, 3, 5, 7, 9]
    assert list(matcher.GetFeaturesInArea(0.0, 0.0, 8.0)) == [0, 2, 4, 6, 8] and list(matcher.GetFeaturesInArea(1010.0, 755.0, 8.0)) == [1, 3, 5, 7, 9]


# ----------------------------------------------------------------------------------------------- match_candidates
@pytest.fixture(scope="module")
def wframe(oracle):
    keys, desc = mp.window_frame()
    return keys, desc, mp.grid_lists(keys), oracle.make_frame(keys, desc, mp.BOUNDS)


def test_windows(matcher, oracle, wframe):
    keys, desc, grid, F = wframe
    _set(matcher, keys, desc)
    for x, y, r, lo, hi in mp.window_queries():
        assert np.array_equal(matcher.GetFeaturesInArea(x, y, r, lo, hi), oracle.get_features_in_area(F, x, y, r, lo, hi)), (x, y, r, lo, hi)


def _batches(wframe):
    keys, desc, grid, F = wframe
    return [mp.LocalBatch(keys, desc, grid, sf, q) for sf, q in mp.local_map_batches()] + [mp.LocalBatch(keys, desc, grid, mp.LOCAL_COUNT_SF, q) for _, q in mp.local_map_counts()]


def test_local_map_batches(matcher, oracle, wframe):
    """Every window in SearchByProjectionLocalMap calls that carry many queries at once: the 3072-cell window beside one-cell windows in one wave, 15 / 16 / 17 / 33 queries with
    invalid ones between."""
    _set(matcher, wframe[0], wframe[1])
    for B in _batches(wframe):
        got, ng = B.device(matcher)
        ref, nr = B.judge(oracle, wframe[3])
        assert np.array_equal(got, ref) and ng == nr and ng > 0
        assert matcher.last_candidate_stats() == {"queries": len(B.q), "candidates": B.candidates()}


def test_arena_exact_and_one_short(ctx, oracle, wframe):
    big, small = _batches(wframe)[0], _batches(wframe)[1]
    count = big.candidates()
    ref, nr = big.judge(oracle, wframe[3])
    m = ORBmatcher(ctx=ctx, max_keypoints=4096, max_queries=64, max_candidates=count)
    _set(m, wframe[0], wframe[1])
    got, ng = big.device(m)
    assert np.array_equal(got, ref) and ng == nr and m.last_candidate_stats()["candidates"] == count
    m.close()
    m = ORBmatcher(ctx=ctx, max_keypoints=4096, max_queries=64, max_candidates=count - 1)
    _set(m, wframe[0], wframe[1])
    with pytest.raises(CubeSlamError, match="CS_ERR_CAPACITY"):
        big.device(m)
    assert m.last_candidate_stats()["candidates"] == count, "the cursor reports what the arena should have held"
    got, ng = small.device(m)
    ref, nr = small.judge(oracle, wframe[3])
    assert np.array_equal(got, ref) and ng == nr and ng > 0 and small.candidates() < count
    m.close()


# ----------------------------------------------------------------------------------------------- match_resolve<V>
@pytest.mark.parametrize("variant", mp.VARIANTS)
def test_claims(matcher, oracle, variant):
    first, bad = None, []
    for S in mp.claim_cases(variant):
        if variant not in (BOW, BOWKF):
            _set(matcher, S.keys, S.desc)
        got, ng = mp.run_device(variant, S, matcher)
        ref, nr = mp.run_judge(variant, S, oracle)
        if not (np.array_equal(got, ref) and ng == nr):
            bad.append((S.name, ng, nr, np.flatnonzero(got != ref)[:8].tolist()))
        first = first or (S, ref, nr)
    assert not bad, (variant, bad)
    # one key point more than a workgroup's LDS holds: the capacity error, and the matcher goes on working
    S = mp.train_size(mp.LDS_LIMIT[variant] + 1)
    if variant not in (BOW, BOWKF):
        _set(matcher, S.keys, S.desc)
    with pytest.raises(CubeSlamError, match="CS_ERR_CAPACITY"):
        mp.run_device(variant, S, matcher)
    S, ref, nr = first
    if variant not in (BOW, BOWKF):
        _set(matcher, S.keys, S.desc)
    got, ng = mp.run_device(variant, S, matcher)
    assert np.array_equal(got, ref) and ng == nr


# ----------------------------------------------------------------------------------------------- the small kernels
def test_knn_tile_seams_and_ties(ctx, oracle):
    for nq in mp.KNN_SIZES:
        for nt in mp.KNN_SIZES:
            q, t, _ = mp.knn_case(nq, nt)
            bi, bd, sd = hamming_knn2(ctx, q, t)
            ri, rd, rs = oracle.hamming_knn2(q, t)
            assert np.array_equal(bi, ri) and np.array_equal(bd, rd) and np.array_equal(sd, rs), (nq, nt)


def _tri(m, oracle, c, check_ori):
    n1, n2 = len(c["k1"]), len(c["k2"])
    z1, z2, u1, u2 = np.zeros(n1, np.uint8), np.zeros(n2, np.uint8), np.full(n1, -1.0, np.float32), np.full(n2, -1.0, np.float32)
    sig = (mp.SF * mp.SF).astype(np.float32)
    m.mbCheckOrientation = check_ori
    got = m.SearchForTriangulation(c["k1"], c["d1"], c["node1"], z1, u1, c["k2"], c["d2"], c["node2"], z2, u2, c["F12"], -1e4, 100.0, mp.SF, sig, False)
    F1 = oracle.make_frame(c["k1"], c["d1"], mp.BOUNDS); F2 = oracle.make_frame(c["k2"], c["d2"], mp.BOUNDS)
    ref = oracle.search_for_triangulation(F1, c["node1"], z1, u1, F2, c["node2"], z2, u2, c["F12"], -1e4, 100.0, mp.SF, sig, False, check_ori)
    assert np.array_equal(got[0], ref[0]) and got[1] == ref[1]
    return got


def test_triangulation_strides_and_ties(matcher, oracle):
    for n_node, N1, zero_F in ((63, 4, False), (64, 1, False), (65, 5, False), (64, 4, True)):
        m12, n = _tri(matcher, oracle, mp.triangulation_case(n_node, N1, zero_F), False)
        assert n == (0 if zero_F else N1)
    assert _tri(matcher, oracle, mp.triangulation_threshold(), False)[1] == 1
    for N1 in (1023, 1024, 1025):  # match_orient_cut's 1 024-thread stride
        m12, n = _tri(matcher, oracle, mp.orientation_cut_case(N1), True)
        assert 0 < n < N1


def test_bow_node_sizes(matcher, oracle):
    S = mp.bow_nodes()
    for v in (BOW, BOWKF):
        got, ng = mp.run_device(v, S, matcher)
        ref, nr = mp.run_judge(v, S, oracle)
        assert np.array_equal(got, ref) and ng == nr == 2


# ----------------------------------------------------------------------------------------------- the window stream
def test_stream_pairs_do_not_interact(ctx, oracle):
    """ORBmatcherStream.search over three pairs of designed frames: a pair without a valid query between two that have some, a train frame of one key point, and a contested
    index on the last query of pair 0 and the first of pair 1."""
    from cube_slam_amd.matcher import ORBmatcherStream
    from cube_slam_amd.orb import ORBextractor
    imgs = mp.stream_images()
    orb = ORBextractor(*mp.STREAM_ORB, mp.STREAM_W, mp.STREAM_H, max_frames=len(imgs), ctx=ctx)
    frames = orb.extract_batch(imgs)
    e = oracle.ORBextractor(*mp.STREAM_ORB)
    for (k, d), img in zip(frames, imgs):
        rk, rd = e(img)
        assert k.tobytes() == rk.tobytes() and np.array_equal(d, rd)
    ms = ORBmatcherStream(False, ctx=ctx)
    for middle_valid in (False, True):
        c = mp.stream_case(frames, middle_valid)
        tm, nm = ms.search(orb, 0, 3, (1.0, 1.0, 0.0, 0.0), None, mp.STREAM_BOUNDS, np.concatenate(c["world_pos"]), np.concatenate(c["valid"]), np.concatenate(c["blocks"]), np.stack(c["Tcw"]),
                           1.0, 1.0, 0.0, 0.0, c["sf"], c["th"], 13, mp_desc=np.concatenate(c["mp_desc"]))
        off = 0
        for p in range(3):
            k, d = frames[p + 1]
            ref, nr = oracle.search_by_projection_frame(oracle.make_frame(k, d, mp.STREAM_BOUNDS), c["world_pos"][p], c["valid"][p], c["blocks"][p], c["mp_desc"][p], frames[p][0]["octave"],
                                                        frames[p][0]["angle"], c["Tcw"][p], 1.0, 1.0, 0.0, 0.0, c["sf"], c["th"], False)
            assert np.array_equal(tm[off:off + len(k)], ref) and nm[p] == nr, (middle_valid, p, tm, nm)
            assert np.array_equal(ref, c["expected"][p][0]) and nr == c["expected"][p][1]
            off += len(k)
        assert off == 13
    ms.close(); orb.close()
