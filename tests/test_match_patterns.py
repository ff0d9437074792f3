"""CPU: the designed matcher inputs of tests/match_patterns.py are what they claim to be -- the oracle (tests/sim3_restatement.py for the relocalisation search) gives the
result each case derives by construction, and every case reaches the seam it is built for."""
import numpy as np
import pytest

from tests import match_patterns as mp
from tests.match_patterns import BOW, BOWKF, CLAIM, INIT, LOCAL, PROJ


def _frame(oracle, keys, desc=None):
    return oracle.make_frame(keys, np.zeros((len(keys), 32), np.uint8) if desc is None else desc, mp.BOUNDS)


# ----------------------------------------------------------------------------------------------- grid
def test_grid_borders(oracle):
    keys, exp = mp.grid_borders()
    assert [mp.cell_of(keys["x"][i], keys["y"][i]) for i in range(len(exp))] == exp
    # the facts the case was built from, spelled out
    assert mp.cell_of(8.0, 16.0) == (1, 1) and mp.cell_of(7.999, 16.0) == (0, 1) and mp.cell_of(-8.0, 16.0) is None and mp.cell_of(1024.0, 16.0) is None
    assert mp.cell_of(1015.9, 16.0) == (63, 1) and mp.cell_of(1015.9, 767.0) is None and mp.cell_of(float(mp.above(-8.0)), 16.0) == (0, 1)
    F = _frame(oracle, keys)
    got = list(oracle.get_features_in_area(F, 512.0, 384.0, 5000.0))
    assert got == mp.whole_grid(keys)
    assert sum(e is None for e in exp) == 10 and len(got) == len(keys) - 10
    # per border point: a window that reaches into the cell the point would fall into if it were rounded the other way
    for i in range(len(exp)):
        x, y = float(keys["x"][i]), float(keys["y"][i])
        assert list(oracle.get_features_in_area(F, x, y, 9.0)) == mp.area(keys, mp.grid_lists(keys), x, y, 9.0)


@pytest.mark.parametrize("N", mp.GRID_SIZES)
def test_grid_sizes(oracle, N):
    keys = mp.grid_scatter(N)
    want = mp.whole_grid(keys)
    assert list(oracle.get_features_in_area(_frame(oracle, keys), 512.0, 384.0, 5000.0)) == want
    if N >= 1023:
        assert 0.8 * N < len(want) < N, "most points inside, some outside the grid"
        assert max(len(l) for l in mp.grid_lists(keys).values()) >= 2


def test_grid_one_cell_and_corner_cells(oracle):
    keys = mp.grid_one_cell()
    assert set(mp.grid_lists(keys)) == {(10, 10)} and np.all(np.diff(keys["x"]) < 0) and len(keys) == 1500
    assert list(oracle.get_features_in_area(_frame(oracle, keys), 160.0, 160.0, 20.0)) == list(range(1500))
    keys = mp.grid_corner_cells()
    g = mp.grid_lists(keys)
    assert g == {(0, 0): [0, 2, 4, 6, 8], (63, 47): [1, 3, 5, 7, 9]}
    assert list(oracle.get_features_in_area(_frame(oracle, keys), 512.0, 384.0, 5000.0)) == [0, 2, 4, 6, 8, 1, 3, 5, 7, 9]


# ----------------------------------------------------------------------------------------------- windows
@pytest.fixture(scope="module")
def wframe(oracle):
    keys, desc = mp.window_frame()
    return keys, desc, mp.grid_lists(keys), oracle.make_frame(keys, desc, mp.BOUNDS)


def test_windows(oracle, wframe):
    keys, desc, grid, F = wframe
    qs = mp.window_queries()
    assert len(qs) <= 36, "each one synchronises on the device"
    res = {}
    for x, y, r, lo, hi in qs:
        want = mp.area(keys, grid, x, y, r, lo, hi)
        assert list(oracle.get_features_in_area(F, x, y, r, lo, hi)) == want, (x, y, r, lo, hi)
        res[(x, y, r, lo, hi)] = want
    assert {mp.n_cells(x, y, r) for x, y, r, _ in mp.WINDOWS} >= mp.WINDOW_NCELLS
    lat = lambda c, r: r * mp.COLS + c
    assert res[(24.0, 24.0, 8.0, -1, -1)] == [] and res[(24.0, 24.0, float(mp.above(8.0)), -1, -1)] == [lat(1, 1), lat(1, 2), lat(2, 1), lat(2, 2)]
    assert res[(21.0, 16.0, 5.0, -1, -1)] == [] and res[(16.0, 21.0, 5.0, -1, -1)] == [] and res[(21.0, 16.0, float(mp.above(5.0)), -1, -1)] == [lat(1, 1)]
    assert res[(16.0, 16.0, 0.0, -1, -1)] == [] and mp.n_cells(16.0, 16.0, 0.0) == 1
    for q in ((-100.0, 100.0, 50.0), (1200.0, 100.0, 50.0), (100.0, -100.0, 50.0), (100.0, 900.0, 50.0)):
        assert mp.window_cells(*q) is None and res[q + (-1, -1)] == []
    assert res[(1014.0, 758.0, 4.0, -1, -1)] == [3075] and mp.window_cells(1014.0, 758.0, 4.0) == (63, 63, 47, 47)
    assert len(res[(512.0, 384.0, 5000.0, -1, -1)]) == 3097
    assert mp.window_cells(132.0, 865.0, 112.0)[2:] == (47, 47) and mp.window_cells(140.0, 873.0, 120.0)[2:] == (47, 47)
    assert res[(132.0, 865.0, 112.0, -1, -1)] == [3076 + c for c in range(2, 16)] and res[(140.0, 873.0, 120.0, -1, -1)] == [3076 + c for c in range(2, 17)], "the row at y = 758, not the centres at 752"
    assert res[(320.0, 320.0, 4.0, -1, -1)] == [lat(20, 20), 3072, 3073, 3074] and res[(320.0, 320.0, 4.0, 0, 0)] == [lat(20, 20), 3072, 3074], "ordered compaction: the record between is dropped"
    assert res[(320.0, 320.0, 4.0, 2, 2)] == [3073] and res[(320.0, 320.0, 4.0, 2, -1)] == [3073] and res[(320.0, 320.0, 4.0, 0, -1)] == res[(320.0, 320.0, 4.0, -1, -1)]
    assert mp.window_cells(-8.0, 8.0, 8.0)[:2] == (0, 0) and mp.window_cells(1024.0, 100.0, 16.0)[:2] == (63, 63)


def test_local_map_batches(oracle, wframe):
    keys, desc, grid, F = wframe
    batches = [mp.LocalBatch(keys, desc, grid, sf, q) for sf, q in mp.local_map_batches()] + [mp.LocalBatch(keys, desc, grid, mp.LOCAL_COUNT_SF, q) for _, q in mp.local_map_counts()]
    radii = set()
    for B in batches:
        want, n, st = mp.resolve(LOCAL, B)
        got, ng = B.judge(oracle, F)
        assert np.array_equal(got, want) and ng == n and n > 0
        radii |= {float(B.radius(q)) for q in range(len(B.q))}
    assert radii >= {r for _, _, r, _ in mp.WINDOWS}, "every window's radius arrives exactly"
    big = batches[0]
    assert [mp.n_cells(x, y, big.radius(q)) for q, (x, y, _, _) in enumerate(big.queries[:4])] == [3072, 1, 1, 1], "one wave: four queries with very different trip counts"
    assert [len(B.q) for B in batches[-4:]] == [15, 16, 17, 33] and all(0 < B.in_view.sum() < len(B.q) and B.in_view[0] and not B.in_view[1] for B in batches[-4:])
    assert big.candidates() > 500


# ----------------------------------------------------------------------------------------------- claims
def _cases():
    return [pytest.param(v, i, id="%s-%s" % (v, c.name)) for v in mp.VARIANTS for i, c in enumerate(mp.claim_cases(v))]


@pytest.mark.parametrize("variant,index", _cases())
def test_claims(oracle, variant, index):
    S = mp.claim_cases(variant)[index]
    want, n, st = mp.resolve(variant, S)
    got, ng = mp.run_judge(variant, S, oracle)
    assert np.array_equal(got, want) and ng == n, (S.name, variant, got, want, ng, n)
    assert n > 0, "no case matches nothing"
    if S.closed and variant in S.closed:
        assert np.array_equal(want, S.closed[variant][0]) and n == S.closed[variant][1], (want, S.closed[variant])
    for k, v in S.want.get(variant, {}).items():
        assert st[k] == v, (k, st[k], v)
    if S.name.startswith("train_size") and len(S.t) > 1:
        assert int(want.max()) >= 0 and (len(S.t) - 1 in want or len(S.t) - 2 in want or want[-1] >= 0 or want[-2] >= 0), "the contested pair is the end of the train arrays"


def test_claim_seams():
    """What the cases reach, in one place."""
    assert mp.LDS_SWITCH == {PROJ: 3071, LOCAL: 3071, INIT: 2456, BOW: 3071, BOWKF: 3071, CLAIM: 3071} and mp.LDS_LIMIT[PROJ] == 9599 and mp.LDS_LIMIT[INIT] == 7679
    for v in mp.VARIANTS:
        assert 3071 * 16 + 16 <= 48 * 1024 < 3072 * 16 + 16 and 9599 * 16 + 16 <= 150 * 1024 < 9600 * 16 + 16 and 2456 * 20 + 16 <= 48 * 1024 < 2457 * 20 + 16 and 7679 * 20 + 16 <= 150 * 1024 < 7680 * 20 + 16
        S = mp.domino(v)
        assert len(S.q) == 64 and mp.resolve(v, S)[2]["longest_list"] == 65
    assert [mp.counted(n).pair for n in mp.COUNTS[:4]] == [(61, 62), (62, 63), (63, 64), (64, 65)], "the contested pair inside batch 0, across the seam, inside batch 1"
    S = mp.rs_nc()
    L = S.lists(PROJ)
    assert sorted({len(l) for l in L}) == [7, 8, 9, 40]
    pos = {(len(l), [mp.hamming(S.desc[t], mp.bits(0)) for t in l].index(10)) for l in L}
    assert pos == {(7, 0), (7, 6), (8, 0), (8, 7), (9, 0), (9, 7), (9, 8), (40, 0), (40, 7), (40, 8), (40, 39)}
    sec = {(len(l), min(i for i, t in enumerate(l) if mp.hamming(S.desc[t], mp.bits(0)) in (19, 21))) for l in L}
    assert {(40, 3), (40, 10), (40, 38), (9, 3), (9, 7)} <= sec, "the second minimum in the registers and in the re-read part"
    for v in (LOCAL, INIT, BOW, BOWKF):
        assert mp.resolve(v, S)[2]["ratio_rejected"] == S.n_spots // 2
    for v in mp.ORIENTED:
        h = mp.resolve(v, mp.rotation_bins())[2]["histogram"]
        assert h[:3] == [5, 4, 3] and h[11] == 1 and h[12] == 2 and sum(h) == 15, h
    assert [mp.rot_bin(a, b) for a, b in mp.ANGLE_DIFFS] == [0, 1, 2, 11, 12, 12, 1, 0, 0]


def test_blocked_winner(oracle):
    for v in (PROJ, LOCAL, BOW, BOWKF, CLAIM):
        S = mp.train_size(65, blocked=True)
        want, n, _ = mp.resolve(v, S)
        free, _, _ = mp.resolve(v, mp.train_size(65))
        assert not np.array_equal(want, free) and n == 1 and (want[64] == 0 if v != BOWKF else list(want) == [64, -1])


# ----------------------------------------------------------------------------------------------- small kernels
@pytest.mark.parametrize("nq", mp.KNN_SIZES)
@pytest.mark.parametrize("nt", mp.KNN_SIZES)
def test_knn(oracle, nq, nt):
    q, t, (bi, bd, sd) = mp.knn_case(nq, nt)
    gi, gd, gs = oracle.hamming_knn2(q, t)
    assert np.array_equal(gi, bi) and np.array_equal(gd, bd) and np.array_equal(gs, sd)
    assert (sd[1::2] == bd[1::2]).all(), "duplicates: second == best, the first index wins"


def _tri(oracle, c, check_ori):
    n1, n2 = len(c["k1"]), len(c["k2"])
    F1 = oracle.make_frame(c["k1"], c["d1"], mp.BOUNDS); F2 = oracle.make_frame(c["k2"], c["d2"], mp.BOUNDS)
    return oracle.search_for_triangulation(F1, c["node1"], np.zeros(n1, np.uint8), np.full(n1, -1.0, np.float32), F2, c["node2"], np.zeros(n2, np.uint8), np.full(n2, -1.0, np.float32),
                                           c["F12"], -1e4, 100.0, mp.SF, (mp.SF * mp.SF).astype(np.float32), False, check_ori)


TRI_CASES = [(63, 4, False), (64, 1, False), (65, 5, False), (64, 4, True)]


@pytest.mark.parametrize("n_node,N1,zero_F", TRI_CASES)
def test_triangulation(oracle, n_node, N1, zero_F):
    c = mp.triangulation_case(n_node, N1, zero_F)
    m, n = _tri(oracle, c, False)
    assert np.array_equal(m, c["expected"][0]) and n == c["expected"][1]


def test_triangulation_threshold_and_orientation_cut(oracle):
    c = mp.triangulation_threshold()
    m, n = _tri(oracle, c, False)
    assert np.array_equal(m, c["expected"][0]) and n == 1
    for N1 in (1023, 1024, 1025):
        c = mp.orientation_cut_case(N1)
        m, n = _tri(oracle, c, True)
        assert np.array_equal(m, c["expected"][0]) and n == c["expected"][1] and 0 < n < N1


def test_bow_nodes(oracle):
    S = mp.bow_nodes()
    for v in (BOW, BOWKF):
        got, n = mp.run_judge(v, S, oracle)
        assert np.array_equal(got, S.closed[v][0]) and n == 2


# ----------------------------------------------------------------------------------------------- the window stream
def test_stream_case(oracle):
    e = oracle.ORBextractor(*mp.STREAM_ORB)
    frames = [e(img) for img in mp.stream_images()]
    for (k, d), dots in zip(frames, mp.STREAM_DOTS):
        assert sorted(zip(k["x"].tolist(), k["y"].tolist())) == sorted((float(x), float(y)) for x, y in dots) and (k["octave"] == 0).all()
        assert (d == frames[0][1][0]).all(), "one descriptor for every key point: every candidate of a window ties"
    for middle_valid in (False, True):
        c = mp.stream_case(frames, middle_valid)
        for p in range(3):
            k, d = frames[p + 1]
            F = oracle.make_frame(k, d, mp.STREAM_BOUNDS)
            tm, n = oracle.search_by_projection_frame(F, c["world_pos"][p], c["valid"][p], c["blocks"][p], c["mp_desc"][p], frames[p][0]["octave"], frames[p][0]["angle"], c["Tcw"][p], 1.0, 1.0, 0.0,
                                                      0.0, c["sf"], c["th"], False)
            assert np.array_equal(tm, c["expected"][p][0]) and n == c["expected"][p][1], (middle_valid, p, tm, n)
