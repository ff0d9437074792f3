"""GPU parity: the pose graph on the device (cs_essential_graph_create / _optimize, cs_sim3_correct_points, cs_sim3_log) through cube_slam_amd.optimizer against the restatement
of Optimizer::OptimizeEssentialGraph (tests/essential_graph_restatement.py, pinned to the reference's own text by tests/test_essential_graph_restatement_pins.py) on every case of
tests/essential_graph_patterns.py.  The iteration count and the accepted / undone sequence of the LM trials must be equal; the estimates, the recovered float poses and the
corrected points must agree within R.TOL_* = 10 x D_REF_*, the reference's own sensitivity to the order of its key frames.  The reference is not read here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cube_slam_amd import _lib
from cube_slam_amd import optimizer as O
from tests import essential_graph_patterns as P
from tests import essential_graph_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


def test_the_library_exports_the_entries_and_the_header_declares_them():
    header = open(os.path.join(ROOT, "include", "cubeslam_hip.h")).read()
    for name in ("cs_essential_graph_create", "cs_essential_graph_optimize", "cs_essential_graph_destroy", "cs_sim3_correct_points", "cs_sim3_log"):
        assert hasattr(_lib.lib(), name) and re.search(r"\b%s\s*\(" % name, header), name
    assert "Optimizer::OptimizeEssentialGraph" in header and "Optimizer.cc:2575-2836" in header and _lib.header_version() == 108


_runs = {}


def _device(ctx, name):
    """One device run per case, shared by the tests below."""
    if name not in _runs:
        g = O.build_essential_graph(R.flatten(P.case(name)))
        eg = O.EssentialGraph(g, P.CASES[name][1], ctx=ctx)
        _runs[name] = (g,) + eg.optimize(g["Scw"], g["Snc"], g["has_nc"])
        eg.close()
    return _runs[name]


@gpu
@pytest.mark.parametrize("name", list(P.CASES))
def test_device_equals_the_restatement(ctx, name):
    g, sim3, Tiw, st = _device(ctx, name)
    j = P.judged(name)
    ds, dt = R.sim3_distance(sim3, j["sim3"]), R.abs_distance(Tiw, j["Tiw"])
    print("%s: n %d m %d levels %d L blocks %d (H %d) launches / trial %d; iterations %d / %d, sequence %s / %s, chi2 %.6g -> %.6g (restatement %.6g -> %.6g); sim3 %.3e (TOL %.3e), Tiw %.3e (TOL %.3e)"
          % (name, len(sim3), len(g["edge_i"]), st["levels"], st["l_blocks"], st["h_blocks"], st["launches_per_trial"], st["iterations"], j["stats"]["iterations"], st["sequence"],
             j["stats"]["sequence"], st["chi2_first"], st["chi2_last"], j["stats"]["chi2_first"], j["stats"]["chi2_last"], ds, R.TOL_SIM3, dt, R.TOL_TIW))
    sy = P.symbolic(len(sim3), g["edge_i"], g["edge_j"], g["fixed_vertex"])
    assert (st["levels"], st["l_blocks"], st["h_blocks"]) == (sy["levels"], sy["l_blocks"], sy["h_blocks"])
    assert st["iterations"] == j["stats"]["iterations"] and st["sequence"] == j["stats"]["sequence"]
    assert st["accepted"] == sum(st["sequence"]) and st["rejected"] == len(st["sequence"]) - st["accepted"] and st["trials"] == len(st["sequence"])
    assert ds <= R.TOL_SIM3 and dt <= R.TOL_TIW
    assert sim3[g["fixed_vertex"]].tobytes() == g["Scw"][g["fixed_vertex"]].tobytes()  # pLoopKF does not move
    assert Tiw.tobytes() == R.recover_se3(sim3).tobytes()  # the SE3 recovery is a handful of products in a fixed order
    if P.CASES[name][1]:  # fix_scale: the scale coefficients leave exactly as they came, the rest moved
        assert sim3[:, 7].tobytes() == g["Scw"][:, 7].tobytes() and sim3.tobytes() != g["Scw"].tobytes()
    elif name == "ring12":
        assert sim3[:, 7].tobytes() != g["Scw"][:, 7].tobytes()


@gpu
def test_point_correction(ctx):
    g, sim3, _, _ = _device(ctx, "kf40")
    j = P.judged("kf40")
    assert len(j["P"]) == 1000 and np.array_equal(g["Scw"], j["Scw"])
    got = O.correct_points(j["P"], j["ref"], g["Scw"], sim3, ctx=ctx)
    assert got.tobytes() == R.correct_points(j["P"], j["ref"], g["Scw"], sim3).tobytes()  # the restatement on the device's own sim3_out: equality
    d = R.abs_distance(got, j["points"])
    print("corrected points against the restatement's: %.3e (TOL %.3e)" % (d, R.TOL_POINTS))
    assert d <= R.TOL_POINTS
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG"):
        O.correct_points(j["P"][:2], [0, len(sim3)], g["Scw"], sim3, ctx=ctx)


@gpu
def test_the_whole_call_on_a_flattened_map(ctx):
    mp, j = P.case("kf40"), P.judged("kf40")
    ids = {kf: kf.mnId for kf in mp.all_kfs}
    pts = [p for p in mp.points if not p.bad]
    nIDr = [p.mnCorrectedReference if p.mnCorrectedByKF == mp.cur_kf.mnId else ids[p.ref_kf] for p in pts]
    res = O.OptimizeEssentialGraph(R.flatten(mp), False, points=(j["P"], nIDr), ctx=ctx)
    _, sim3, Tiw, _ = _device(ctx, "kf40")
    assert res["sim3"].tobytes() == sim3.tobytes() and res["Tiw"].tobytes() == Tiw.tobytes()  # and a second run of the same graph gives the same bytes
    assert res["points"].tobytes() == R.correct_points(j["P"], j["ref"], j["Scw"], sim3).tobytes()


@gpu
def test_runs_are_reproducible_and_do_not_depend_on_what_ran_before(ctx):
    g, sim3, Tiw, st = _device(ctx, "ring12")
    for other in ("kf40", None):
        if other:
            _runs.pop(other, None)
            _device(ctx, other)  # a different graph on the same context in between
        eg = O.EssentialGraph(g, False, ctx=ctx)
        a = eg.optimize(g["Scw"], g["Snc"], g["has_nc"])
        b = eg.optimize(g["Scw"], g["Snc"], g["has_nc"])  # the same handle again
        eg.close()
        for r in (a, b):
            assert r[0].tobytes() == sim3.tobytes() and r[1].tobytes() == Tiw.tobytes() and r[2] == st


@gpu
def test_sim3_log_branches(ctx):
    """identity, angle 1e-6 (d > 1 - eps), angle 3.0 (acos), each with |sigma| below and above 1e-5.  Held to the restatement's Sim3::log within 64 units of the last place of
    max(1, |value|): the two sides differ in acos / sin / cos / log of libm and the device's math library (a unit or two each), which the angle-3.0 branch multiplies by
    theta / (2 sqrt(1 - d^2)) ~ 11 and the 3 x 3 solve by the condition of W (below 4 here)."""
    rows = []
    for ang in (0.0, 1e-6, 3.0):
        for s in (1.0, 1.0 + 3e-6, 1.7, 0.4):
            q = R.S3._rot((0.3, -0.5, 0.8), np.degrees(ang))
            rows.append([0.7, -1.3, 2.1, q[0], q[1], q[2], q[3], s])
    S = np.array(rows)
    got, want = O.sim3_log(S, ctx=ctx), R.sim3_log(R._arr(S))
    d = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
    print("sim3_log: %.3e" % d)
    assert np.all(np.isfinite(got)) and d <= 64 * 2.220446049250313e-16
    assert got[0, :3].tobytes() == np.zeros(3).tobytes() and got[0, 6] == 0.0 and np.array_equal(got[0, 3:6], S[0, :3])  # identity rotation and scale: W = I


@gpu
def test_bad_arguments_are_errors_and_launch_nothing(ctx):
    g = O.build_essential_graph(R.flatten(P.case("chain5")))
    n = len(g["Scw"])

    def create(**kw):
        a = dict(g)
        a.update(kw)
        return O.EssentialGraph(a, False, ctx=ctx)

    ctx.timing(True)
    ctx.timing_reset()
    bad_i = g["edge_i"].copy(); bad_i[1] = n
    neg_j = g["edge_j"].copy(); neg_j[0] = -1
    same = g["edge_j"].copy(); same[2] = g["edge_i"][2]
    for kw in (dict(edge_i=bad_i), dict(edge_j=neg_j), dict(fixed_vertex=n), dict(fixed_vertex=-1), dict(edge_j=same),
               dict(edge_i=g["edge_i"][:0], edge_j=g["edge_j"][:0], edge_kind=g["edge_kind"][:0])):
        with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG"):
            create(**kw)
    for k in ("eg_measure", "eg_error", "eg_linearize", "eg_assemble", "eg_factor"):
        assert ctx.timing_get(k)[1] == 0
    ctx.timing(False)
    with pytest.raises(ValueError):
        create(edge_kind=g["edge_kind"][:-1])


# ---------------------------------------------------------------------------------------------------------------------------------- graph-level cases (P.GRAPH_CASES)
def test_no_trial_of_the_fans_is_near_a_tie():
    """CPU: the restatement alone.  fan256 has exactly 512 edges and 257 vertices, fan255 510 and 256; every trial's decision is far from a tie, so equal sequences can be asked."""
    for name, n, m in (("fan256", 257, 512), ("fan255", 256, 510)):
        g, (_, _, st) = P.graph_case(name), P.graph_judged(name)
        assert (len(g["Scw"]), len(g["edge_i"])) == (n, m) and st["iterations"] == 2 and len(st["margins"]) == len(st["sequence"])
        assert min(st["margins"]) > 1e-6 and 1 in st["sequence"] and st["chi2_last"] < 1e-3 * st["chi2_first"]
        free = set(range(n)) - {g["fixed_vertex"]}
        spokes = {int(a) if int(b) == g["fixed_vertex"] else int(b) for a, b in zip(g["edge_i"], g["edge_j"]) if g["fixed_vertex"] in (int(a), int(b))}
        assert spokes == free  # every free vertex has an edge to the fixed vertex


@gpu
@pytest.mark.parametrize("name", ["fan256", "fan255"])
def test_full_last_blocks_of_the_per_edge_and_per_vertex_kernels(ctx, name):
    g, (want, want_T, j) = P.graph_case(name), P.graph_judged(name)
    eg = O.EssentialGraph(g, False, ctx=ctx)
    sim3, Tiw, st = eg.optimize(g["Scw"], g["Snc"], g["has_nc"], iterations=P.GRAPH_CASES[name][1])
    eg.close()
    ds, dt = R.sim3_distance(sim3, want), R.abs_distance(Tiw, want_T)
    print("%s: n %d m %d; iterations %d / %d, sequence %s / %s, chi2 %.6g -> %.6g (restatement %.6g -> %.6g); sim3 %.3e (TOL %.3e), Tiw %.3e (TOL %.3e)"
          % (name, len(sim3), len(g["edge_i"]), st["iterations"], j["iterations"], st["sequence"], j["sequence"], st["chi2_first"], st["chi2_last"], j["chi2_first"], j["chi2_last"], ds,
             R.TOL_SIM3, dt, R.TOL_TIW))
    assert len(g["edge_i"]) % 256 == (0 if name == "fan256" else 254) and len(sim3) % 256 == (1 if name == "fan256" else 0)
    assert st["iterations"] == j["iterations"] and st["sequence"] == j["sequence"]
    assert ds <= R.TOL_SIM3 and dt <= R.TOL_TIW
    assert sim3[g["fixed_vertex"]].tobytes() == g["Scw"][g["fixed_vertex"]].tobytes()
    assert Tiw.tobytes() == R.recover_se3(sim3).tobytes()


@gpu
def test_a_nan_estimate_fails_every_solve_and_gives_the_estimates_back(ctx):
    """chain5 with one NaN in a free vertex's translation: chi2 is NaN, the factor meets a NaN pivot on every trial (rec[3], the host's "solve failed" trial, the zero step of
    eg_update), rho is NaN, so each iteration has one undone trial and none of the stop rules of optimization_algorithm_levenberg.cpp applies: 20 iterations, nothing accepted."""
    g, (want, _, j) = P.graph_case("nan_vertex"), P.graph_judged("nan_vertex")
    assert j["iterations"] == 20 and j["sequence"] == [0] * 20 and want.tobytes() == g["Scw"].tobytes() and np.isnan(g["Scw"]).sum() == 1
    eg = O.EssentialGraph(g, False, ctx=ctx)
    sim3, Tiw, st = eg.optimize(g["Scw"], g["Snc"], g["has_nc"], iterations=P.GRAPH_CASES["nan_vertex"][1])
    eg.close()
    print("nan_vertex: iterations %d / %d, sequence %s, lambda %.6g / %.6g" % (st["iterations"], j["iterations"], st["sequence"], st["lambda_last"], j["lambda_last"]))
    assert st["iterations"] == j["iterations"] and st["sequence"] == j["sequence"] and (st["accepted"], st["rejected"]) == (0, 20)
    assert sim3.tobytes() == g["Scw"].tobytes()
    assert st["lambda_last"] == j["lambda_last"]
