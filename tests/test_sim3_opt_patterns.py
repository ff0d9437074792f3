"""Preconditions of the Sim3 refinement's tests, checked on the CPU from the restatement alone (tests/sim3_opt_restatement.py): exact equality of flags and counts is a
fair demand only where no chi2 at a cut sits on the threshold, and a case that claims a path of Optimizer::OptimizeSim3 must take it."""
import numpy as np
import pytest

from tests import sim3_opt_restatement as R


@pytest.mark.parametrize("name", list(R.CASES))
def test_no_chi2_sits_on_the_threshold(name):
    _, _, _, st = R.judged(name)
    assert st["margin"] > 1e-3


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_takes_the_path_it_claims(name):
    c = R.case(name)
    pose, removed, n_in, st = R.judged(name)
    claims = R.CASES[name][1]
    assert claims
    n = len(removed)
    for claim in claims:
        if claim == "early":
            assert st["early"] and not st["stage2"] and n_in == 0 and n - st["nbad1"] < 10 and pose.tobytes() == np.ascontiguousarray(c["sim3_in"], np.float64).tobytes()
        elif claim == "stage2":
            assert st["stage2"] and not st["early"] and n_in == n - st["nbad1"] - st["nbad2"] and n_in >= 10 - st["nbad2"]
        elif claim == "nbad0":
            assert st["nbad1"] == 0
        elif claim == "nbad>0":
            assert st["nbad1"] > 0
        elif claim == "nbad2>0":
            assert st["nbad2"] > 0
        elif claim == "outliers_exact":
            assert len(c["outliers"]) == 3 and np.array_equal(np.nonzero(removed)[0], c["outliers"])
        else:
            raise AssertionError(claim)
    assert int(removed.sum()) == st["nbad1"] + st["nbad2"]


def test_the_set_covers_every_path():
    st = {name: R.judged(name)[3] for name in R.CASES}
    assert any(s["rejected"] > 0 for s in st.values())  # a rejected LM trial
    assert any(s["nbad2"] > 0 for s in st.values())  # stage 2 flags a pair
    assert any(s["stage2"] and s["nbad1"] == 0 for s in st.values()) and any(s["stage2"] and s["nbad1"] > 0 for s in st.values())  # 5 and 10 more iterations
    assert any(s["early"] and s["nbad1"] > 0 for s in st.values())  # the early return keeps its flags
    sizes = {len(R.judged(name)[1]) for name in R.CASES}
    assert {0, 9, 10, 11, 12, R.THREADS - 1, R.THREADS, R.THREADS + 1, 2000} <= sizes


def test_the_cases_are_what_the_issue_asks():
    for name, (kw, _) in R.CASES.items():
        c = R.case(name)
        n = kw["n"]
        assert c["P1c"].shape == (n, 3) and c["P2c"].shape == (n, 3)
        if n:
            assert 2.0 <= c["P1c"][:, 2].min() and c["P1c"][:, 2].max() <= 20.0 and 2.0 <= c["P2c"][:, 2].min() and c["P2c"][:, 2].max() <= 20.0
            for k in ("P1c", "P2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "intrinsics"):  # what the reference holds in floats
                assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k
        if not kw.get("same_k"):
            assert not np.array_equal(c["intrinsics"][:4], c["intrinsics"][4:])
        for i in c["outliers"]:
            clean = R.make_case(**dict(kw, n_outliers=0))
            assert max(np.linalg.norm(c["obs1"][i] - clean["obs1"][i]), np.linalg.norm(c["obs2"][i] - clean["obs2"][i])) >= 29.9
    assert [R.CASES[k][0]["s"] for k in ("scale_0.5", "scale_1", "scale_2")] == [0.5, 1.0, 2.0]
    batch_n = [R.CASES[k][0]["n"] for k in R.BATCH]
    assert len(R.BATCH) == 7 and len(set(batch_n)) == 7 and 0 in batch_n and any(R.judged(k)[3]["early"] and R.CASES[k][0]["n"] > 0 for k in R.BATCH)
    assert R.CASES["fix_scale_on"][0]["fix_scale"] and R.judged("fix_scale_on")[0][7] == R.case("fix_scale_on")["sim3_in"][7]
    assert R.judged("fix_scale_off")[0][7] != R.case("fix_scale_off")["sim3_in"][7]
