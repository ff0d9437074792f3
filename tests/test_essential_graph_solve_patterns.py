"""CPU: the preconditions of tests/test_essential_graph_solve_gpu.py, asserted on the designed systems of tests/essential_graph_solve_patterns.py without a device: each graph
has the launch list, column and row lengths, roots and fill it was designed for (so a change cannot silently empty a case), every system is positive definite and within the
condition cap, the designed inputs are exact integers, and the judge sees what it is for: a block Cholesky over the solver's own structure that loses one update into one
fill block has a backward error above 1e-7 on every case with fill, against 4 k u <= 1e-12 for the clean solve."""
import numpy as np
import pytest

from tests import essential_graph_solve_patterns as SP

# name -> (launch list, longest column, longest row structure, roots, fill blocks, levels, l_blocks)
FIGURES = {
    "clique40": ([("seq", 40)], 39, 39, 1, 0, 40, 820),
    "two_cliques39": ([("par", 2)] * 39, 38, 38, 2, 0, 39, 1560),
    "path30": ([("seq", 30)], 1, 1, 1, 0, 30, 59),
    "star300": ([("par", 299), ("seq", 2)], 1, 299, 1, 0, 3, 601),
    "grid6x6": ([("par", 11), ("par", 4), ("par", 4), ("par", 3), ("par", 2), ("par", 2), ("seq", 10)], 6, 13, 1, 71, 16, 167),
    "forest": ([("par", 4), ("par", 3), ("par", 2), ("seq", 3)], 2, 2, 4, 0, 6, 21),
    "multi": ([("seq", 5)], 2, 4, 1, 2, 5, 12),
}


@pytest.mark.parametrize("name", SP.NAMES)
def test_the_graph_reaches_what_it_was_designed_for(name):
    c = SP.make(name)
    sy = c["sym"]
    print(name, {k: sy[k] for k in ("levels", "widths", "launches", "longest_column", "longest_row", "roots", "fill", "l_blocks", "h_blocks")})
    if name == "kf300_real":
        assert max(sy["widths"]) == 101 and sy["fill"] == 1069 and sy["longest_column"] == 16 and sy["roots"] == 1 and len(SP.fill_blocks(c)) == 1069
        return
    launches, col, row, roots, fill, levels, l_blocks = FIGURES[name]
    assert (sy["launches"], sy["longest_column"], sy["longest_row"], sy["roots"], sy["fill"], sy["levels"], sy["l_blocks"]) == (launches, col, row, roots, fill, levels, l_blocks)
    assert len(SP.fill_blocks(c)) == fill and sum(cnt for _, cnt in sy["launches"]) == c["n"] - 1
    T = 256  # EG_THREADS
    if name == "clique40":  # the first column: a second pass of the row-scaling loop, eight of the gather loop
        assert (col + 1 - 1) * 7 == 273 > T and -(-(col + 1) * 49 // T) == 8
    if name == "two_cliques39":  # the same second pass inside a parallel level, the fixed vertex between the two
        assert col * 7 == 266 > T and sy["widths"] == [2] * 39 and c["fixed"] == 39
    if name == "star300":  # the hub's incidence list: 300 leaves and the fixed vertex (and the anchor edge), on both sides
        assert sy["widths"] == [299, 1, 1] and int(np.sum(c["ei"] == 0)) + int(np.sum(c["ej"] == 0)) >= 301 and min(int(np.sum(c["ei"] == 0)), int(np.sum(c["ej"] == 0))) >= 100
    if name == "grid6x6":  # a chain that starts below parallel levels
        assert sy["widths"][:6] == [11, 4, 4, 3, 2, 2] and launches[-1] == ("seq", 10) and launches[-2][0] == "par"
    if name == "forest":  # an isolated free vertex, roots at four different levels
        assert 0 in [len(r) for r in sy["columns"]] and sy["widths"] == [4, 3, 2, 1, 1, 1]
        free_edges = [(int(a), int(b)) for a, b in zip(c["ei"], c["ej"]) if c["fixed"] not in (int(a), int(b))]
        assert not any(1 in e for e in free_edges)  # vertex 1 touches the fixed vertex alone
    if name == "multi":  # a pair with three edges in both orientations
        pair = [(int(a), int(b)) for a, b in zip(c["ei"], c["ej"]) if {int(a), int(b)} == {0, 1}]
        assert len(pair) == 3 and (0, 1) in pair and (1, 0) in pair


@pytest.mark.parametrize("name", SP.NAMES)
def test_positive_definite_and_within_the_condition_cap(name):
    c = SP.make(name)
    assert c["lambdas"] == (SP.LAMBDAS if c["designed"] else (1e-16,))
    for lam in c["lambdas"]:
        s = SP.system(c, lam)
        np.linalg.cholesky(s["A"])  # raises where A is not positive definite
        eta = SP.backward_errors(s, s["x_lapack"])
        print("%s lambda %g: cond %.3e, LAPACK eta %.2e (per block row %.2e), 4 k u %.2e, ceiling %.2e" % (name, lam, s["cond"], eta[0], eta[1], 4 * SP.tolerance_k(c) * SP.U, SP.higham_ceiling(c)))
        if c["designed"]:
            assert s["cond"] <= SP.COND_CAP
        assert np.isfinite(s["cond"]) and s["cond"] * 4 * SP.tolerance_k(c) * SP.U < 1e-3  # the comparison of x with the refined solution still says something
        assert max(eta[:2]) <= 4 * SP.tolerance_k(c) * SP.U <= SP.higham_ceiling(c)  # the dense solve passes the device's bound
        assert eta[0] < 2e-16
        # the refined reference is better than a float64 solve can be told from
        assert SP.backward_errors(s, s["x_ref"].astype(np.float64))[0] <= eta[0] + SP.U


@pytest.mark.parametrize("name", SP.DESIGNED)
def test_designed_inputs_are_exact_integers(name):
    c = SP.make(name)
    for a, bound in ((c["J"], 2), (c["err"], 3), (c["H"], 2.0 ** 53 - 1), (c["b"], 2.0 ** 53 - 1)):
        assert np.array_equal(a, np.rint(a)) and float(np.max(np.abs(a))) <= bound
    assert np.array_equal(c["H"], c["H"].T)
    # the fixed vertex's side of J is not zero: nothing may read it
    sides = np.concatenate([c["J"][c["ei"] == c["fixed"], 0].reshape(-1), c["J"][c["ej"] == c["fixed"], 1].reshape(-1)])
    assert np.count_nonzero(sides) > 0
    # exact whatever the order of the sums: the dense H of a permuted edge list is the same bytes
    perm = np.random.RandomState(1).permutation(len(c["ei"]))
    H2, b2 = SP.dense(c["n"], c["fixed"], c["ei"][perm], c["ej"][perm], c["J"][perm], c["err"][perm])
    assert H2.tobytes() == c["H"].tobytes() and b2.tobytes() == c["b"].tobytes()


@pytest.mark.parametrize("name", SP.NAMES)
def test_the_judge_sees_one_lost_update_into_one_fill_block(name):
    c = SP.make(name)
    fill = SP.fill_blocks(c)
    assert (len(fill) > 0) == (name in ("grid6x6", "multi", "kf300_real"))
    for lam in c["lambdas"]:
        s = SP.system(c, lam)
        bound = 4 * SP.tolerance_k(c) * SP.U
        clean = SP.backward_errors(s, SP.block_cholesky_solve(c, lam))
        assert max(clean[:2]) <= bound  # the same algorithm, nothing lost
        for drop in (fill[:1] + fill[-1:]):
            x = SP.block_cholesky_solve(c, lam, drop=drop)
            eta = SP.backward_errors(s, x)
            dx = float(np.max(np.abs(x - s["x_ref"].astype(np.float64))) / np.max(np.abs(s["x_ref"])))
            print("%s lambda %g: block %s lost its last update: eta %.2e (per block row %.2e at %d), x off by %.2e; clean %.2e, bound %.2e" % (name, lam, drop, eta[0], eta[1], eta[2], dx, clean[0], bound))
            assert eta[0] > 1e-7 and eta[1] > 1e-7 and eta[0] > 1e4 * bound
