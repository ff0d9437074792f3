"""Sim3Solver on the device against the restatement (tests/sim3_solver_restatement.py): cs_sim3_solver_hypotheses on the cases of tests/sim3_solver_patterns.py.  No tolerance
anywhere: counts and mask words equal entry for entry, the 13 floats of every hypothesis equal as bit patterns, a NaN equal to any NaN (the bit class: x86 and the device give
NaNs of different sign and payload for 0 / 0).  Every output array is prefilled with a sentinel, so equality also shows that every entry is written; the refusals leave the
sentinels in place.  The shapes are the smallest at which the kernel can go wrong: N = 20 (the one-iteration branch of SetRansacParameters), 21, 32 / 33 (one mask word with lane 31 the last, and the first N
with a second word: the condition under which the upper ballot half is stored; with 5 hypotheses no correspondence is an inlier and the words must be written as zeros, with
300 the last bit -- 31 and 32 -- is set in dozens of them), 63 / 64 / 65 (the wave seam and
the seam of the second mask word), 129 (a fifth mask word: the upper ballot half of the last pass is not stored), 200 (several passes per lane); 1, 5 and 300 hypotheses (less
than one workgroup, a partly filled one, many); 1, 3 and 16 problems of different N and hypothesis counts in one call (the offset seams), one of them without hypotheses."""
import numpy as np
import pytest

from tests import sim3_solver_patterns as P
from tests import sim3_solver_restatement as R

pytestmark = pytest.mark.gpu

SENT_I, SENT_F, SENT_M = -77, np.float32(-12345.5), 0xA5A5A5A5


def _call(ctx, cases):
    """One cs_sim3_solver_hypotheses over the cases -> n_inliers, sRt, mask (sentinel-filled before the call), and whatever the call raised."""
    from cube_slam_amd.sim3_solver import solver_hypotheses
    co = np.concatenate([[0], np.cumsum([len(c["X1"]) for c in cases])]).astype(np.int32)
    ho = np.concatenate([[0], np.cumsum([len(c["triples"]) for c in cases])]).astype(np.int32)
    words = sum(len(c["triples"]) * ((len(c["X1"]) + 31) // 32) for c in cases)
    ni = np.full(max(int(ho[-1]), 1), SENT_I, np.int32); sRt = np.full((max(int(ho[-1]), 1), 13), SENT_F, np.float32); mk = np.full(max(words, 1), SENT_M, np.uint32)
    cat = lambda k, w, dt: np.concatenate([np.asarray(c[k], dt).reshape(-1, w) for c in cases])
    err = None
    try:
        solver_hypotheses(ctx, co, cat("X1", 3, np.float32), cat("X2", 3, np.float32), cat("e1", 1, np.float32), cat("e2", 1, np.float32), cat("K8", 8, np.float32),
                          [c["fix_scale"] for c in cases], ho, cat("triples", 3, np.int32), n_inliers=ni, sRt=sRt, mask=mk)
    except Exception as e:  # noqa: BLE001 (handed to the caller)
        err = e
    return ni[:ho[-1]], sRt[:ho[-1]], mk[:words], err


def _check(got, judged_list):
    ni, sRt, mk, err = got
    assert err is None, err
    assert np.array_equal(ni, np.concatenate([j["n_inliers"] for j in judged_list]))
    assert R.same_floats(sRt, np.concatenate([j["sRt"] for j in judged_list]))
    assert np.array_equal(mk, np.concatenate([j["mask"].reshape(-1) for j in judged_list]))


@pytest.mark.parametrize("N,H", [(20, 5), (21, 5), (32, 5), (33, 5), (63, 5), (64, 5), (65, 5), (129, 5), (200, 5), (65, 1), (32, 300), (33, 300), (64, 300), (129, 300), (200, 300)])
def test_one_problem(ctx, N, H):
    _check(_call(ctx, [P.raw_case(N, H, N)]), [P.raw_judged(N, H, N)])


@pytest.mark.parametrize("name", P.ALL)
def test_solver_cases(ctx, name):
    """The cases with LoopClosing's RANSAC parameters: mRansacMaxIts hypotheses each (1 for N = 20, none for N = 15 < minInliers), fix_scale in n64_fix."""
    c = P.solver_case(name)
    got = _call(ctx, [c])
    if c["max_its"] == 0:
        assert got[3] is None and len(got[0]) == 0
        return
    _check(got, [P.judged(name)])


BATCHES = {1: [(65, 5, 31, False)],
           3: [(63, 5, 32, False), (129, 300, 33, True), (21, 1, 34, False)],
           16: [(20 + 13 * k, (1, 5, 7, 0, 300, 2)[k % 6], 40 + k, bool(k % 3 == 1)) for k in range(16)]}


@pytest.mark.parametrize("n_problems", [1, 3, 16])
def test_many_problems_in_one_call(ctx, n_problems):
    """Different N and hypothesis counts per problem, fix_scale 0 and 1 in one call, problems without hypotheses in the middle (k = 3, 9, 15 of the 16)."""
    spec = BATCHES[n_problems]
    if n_problems == 16:
        assert any(s[1] == 0 for s in spec[1:-1]) and {s[3] for s in spec} == {False, True}
    _check(_call(ctx, [P.raw_case(*s) for s in spec]), [P.raw_judged(*s) for s in spec])


@pytest.mark.parametrize("kind", ["coincident", "identical", "den0", "z0"])
def test_degenerate(ctx, kind):
    """Hypothesis 0 of each case: a coincident triple, Pr1 == Pr2 exactly (a zero imaginary part), Pr2 == 0 -- a NaN transform and no inlier, as in the reference --
    and a correspondence that the transform puts on z == 0, whose error is not finite and which is no inlier.  The other three hypotheses are ordinary."""
    c, j = P.degenerate(kind), P.degenerate_judged(kind)
    if kind == "z0":
        assert np.isfinite(j["sRt"][0]).all() and not np.isfinite(j["err"][0, 0, c["z0_index"]]) and j["n_inliers"][0] == 3
    else:
        assert np.isnan(j["sRt"][0]).all() and j["n_inliers"][0] == 0 and not j["mask"][0].any()
        assert np.isfinite(j["sRt"][1:]).all()
    _check(_call(ctx, [c]), [j])


def _untouched(got):
    from cube_slam_amd._lib import CubeSlamError
    ni, sRt, mk, err = got
    assert isinstance(err, CubeSlamError) and "CS_ERR_BAD_ARG" in str(err)
    assert (ni == SENT_I).all() and (sRt == SENT_F).all() and (mk == SENT_M).all()


@pytest.mark.parametrize("what", ["index_high", "index_negative", "repeated", "n_below_3"])
def test_refusals(ctx, what):
    """CS_ERR_BAD_ARG before anything is launched, the outputs untouched; the offending entry sits in the last problem of three, behind valid ones."""
    cases = [dict(P.raw_case(63, 5, 32)), dict(P.raw_case(21, 1, 34)), dict(P.raw_case(65, 5, 31))]
    t = cases[2]["triples"].copy()
    if what == "index_high":
        t[4, 1] = 65
    elif what == "index_negative":
        t[0, 2] = -1
    elif what == "repeated":
        t[3, 2] = t[3, 0]
    else:
        for k in ("X1", "X2", "e1", "e2"):
            cases[2][k] = cases[2][k][:2]
        t = np.array([[0, 1, 0]], np.int32)
    cases[2]["triples"] = t
    _untouched(_call(ctx, cases))


def test_nothing_to_do(ctx):
    from cube_slam_amd.sim3_solver import solver_hypotheses
    ni, sRt, mk = solver_hypotheses(ctx, [0], [], [], [], [], [], [], [0], [])
    assert len(ni) == 0 and len(sRt) == 0 and len(mk) == 0
    c = dict(P.raw_case(63, 5, 32)); c["triples"] = np.zeros((0, 3), np.int32)
    ni, sRt, mk, err = _call(ctx, [c])
    assert err is None and len(ni) == 0


def test_mirror_device_equals_host_and_transcription(ctx):
    """Sim3Solver.evaluate_many on the device for the candidates of one ComputeSim3, against the same solvers evaluated on the host (ctx=None, the CPU path over the same
    header) -- every table byte-equal -- and a scripted round-robin with a rejected success walked by both and by the literal transcription of :138-205."""
    from cube_slam_amd.sim3_solver import Sim3Solver
    names = ["n65", "n100_no_consensus", "n15_too_few", "n129", "n20"]

    def make(c_ctx):
        out = []
        for nm in names:
            c = P.solver_case(nm)
            s = Sim3Solver(c["X1"], c["X2"], c["e1"], c["e2"], P.K1, P.K2, c["idx1"], c["mN1"], c["fix_scale"], ctx=c_ctx)
            s.SetRansacParameters(P.PROB, P.MIN_INLIERS, P.MAX_ITS)
            assert s.mRansacMaxIts == c["max_its"]
            if s.mRansacMaxIts:
                s.set_triples(c["triples"])
            out.append(s)
        return out

    dev, host = make(ctx), make(None)
    Sim3Solver.evaluate_many(dev)
    Sim3Solver.evaluate_many(host)
    for nm, a, b in zip(names, dev, host):
        if a.mRansacMaxIts == 0:
            continue
        j = P.judged(nm)
        for t in (a._table, b._table):
            assert np.array_equal(t[0], j["n_inliers"]) and R.same_floats(t[1], j["sRt"]) and np.array_equal(t[2], j["mask"])
    reject = {(0, P.first_success("n65"))}
    assert P.first_success("n65") >= 0
    la, lb = P.round_robin(dev, reject), P.round_robin(host, reject)
    assert la == lb and sum(e[1] for e in la) >= 2  # the rejected success and the one that ends the loop
    # the transcription over the judged tables
    tr = []
    for nm in names:
        c = P.solver_case(nm)
        tr.append(R.IterateTranscription(len(c["X1"]), c["mN1"], c["idx1"], P.MIN_INLIERS, c["max_its"]))
    k = 0
    disc, match, n_cand = [False] * len(names), False, len(names)
    while n_cand > 0 and not match:
        for i, nm in enumerate(names):
            if disc[i]:
                continue
            j = P.judged(nm) if P.solver_case(nm)["max_its"] else None
            bits = None if j is None else [np.unpackbits(m.view(np.uint8), bitorder="little") for m in j["mask"]]
            h, nomore, vb, nin = tr[i].iterate(5, None if j is None else j["n_inliers"], bits)
            e = la[k]; k += 1
            assert e[:6] == (i, int(h >= 0), int(nomore), nin, tr[i].mnIterations, tr[i].mnBestInliers) and e[7] == np.array(vb, np.uint8).tobytes()
            if nomore:
                disc[i] = True; n_cand -= 1
            if h >= 0 and (i, h) not in reject:
                match = True
                break
    assert k == len(la) and match
