"""PnPsolver on the device against the host path of the same headers (cs_pnp_solver_evaluate with and without a context) on the cases of tests/pnp_solver_patterns.py, and both
against the recorded run of the reference's own text (tests/golden/pnp_solver.npz, written by tests/test_pnp_solver_reference_pins.py; the reference tree is not read here).  No
tolerance anywhere: counts, status and mask words equal entry for entry, the 12 doubles of every pose equal as bit patterns, a NaN equal to any NaN (the bit class: x86 and the
device give NaNs of different sign and payload).  The shapes are the smallest at which the kernels can go wrong: N = 4 (the minimal set is N), 15, 33 (the second mask word),
63 / 64 / 65 and 129 (the lane stride and the ballot halves), refinements over 4 to 88 inliers (less than a wave, more than one), problems with several records, none, and
without hypotheses in one batch."""
import os

import numpy as np
import pytest
import torch

# torch's copy of the HIP runtime must be the first in the process (the ctx fixture of tests/conftest.py), and importing this module loads libcubeslam_hip.so: P.case below
# evaluates on the host.  In a run of the whole suite another module has imported torch by then; in a run of this file alone none has.
torch.cuda.is_available()

from tests import pnp_solver_patterns as P

pytestmark = pytest.mark.gpu

KEYS = ("n_inliers", "Rt", "status", "mask", "refined_n", "refined_Rt", "refined_mask")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_solver.npz")


def same(a, b):
    """Equal as bit patterns, a NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def _assert_same(got, want):
    for k in KEYS:
        assert same(got[k], want[k]), k


def _concat(judged):
    return {k: np.concatenate([j[k].reshape((-1, 12) if k.endswith("Rt") else -1) for j in judged]) for k in KEYS}


WITH_QUADS = [n for n in P.ALL if len(P.case(n)["quads"])]


@pytest.mark.parametrize("name", WITH_QUADS)
def test_single_equals_host(ctx, name):
    _assert_same(P.evaluate([P.case(name)], ctx=ctx), P.judged(name))


SEAM_SEED = 70  # at N = 32 hypothesis 4 and at N = 33 hypothesis 0 reach min_inliers = 16: pnp_refine runs at both sizes


@pytest.mark.parametrize("N", [32, 33])
def test_second_mask_word_seam_equals_host(ctx, N):
    """One mask word with lane 31 the last (N = 32) and the first N with a second word (N = 33), where the upper ballot half starts to be stored: five quads drawn for the size,
    min_inliers of the relocalisation parameters, best_in 0; the seven outputs of the device against the host path.  Not a pattern of P.ALL: the golden file has no part in it."""
    c = P.correspondences(N, SEAM_SEED)
    c["min_inliers"], c["max_its"], _ = P.parameters(P.RELOC, N)
    c["max_err"] = c["sigma2"] * np.float32(P.RELOC[5])
    c["quads"] = P.draw(N, 5, 100 + SEAM_SEED)
    host = P.evaluate([c], best_in=[0])
    assert c["min_inliers"] == 16 and (host["refined_n"] >= 0).any() and len(host["mask"]) == 5 * (1 if N == 32 else 2)
    _assert_same(P.evaluate([c], ctx=ctx, best_in=[0]), host)


def test_batch_equals_host(ctx):
    """All patterns in one call; too_few has no hypotheses and lies between two others."""
    assert "too_few" in P.ALL[1:-1] and not len(P.case("too_few")["quads"])
    got = P.evaluate([P.case(n) for n in P.ALL], ctx=ctx)
    _assert_same(got, _concat([P.judged(n) for n in WITH_QUADS]))


def test_equals_recorded_reference(ctx):
    """Device and host path against the reference's own text as recorded in tests/golden/pnp_solver.npz."""
    g = np.load(GOLDEN)
    for name in [n for n in P.SCRIPT_NAMES if n in WITH_QUADS]:  # (coincident4 is not pinned: the reference is undefined on it)
        for got in (P.evaluate([P.case(name)], ctx=ctx), P.judged(name)):
            for k in KEYS:
                assert same(got[k], g[name + "/" + k]), (name, k)


@pytest.mark.parametrize("name,cut", [("planted", 20), ("planted", 30), ("n63", 7), ("coincident", 3)])
def test_split_table_with_best_in(ctx, name, cut):
    """A table split across two calls, the second with best_in = mnBestInliers after the first, evaluates to the single call: the same records, the same refinements."""
    c, whole = P.case(name), P.judged(name)
    a = P.evaluate([c], ctx=ctx, quads=[c["quads"][:cut]])
    best = max([0] + [int(n) for n in a["n_inliers"] if n >= c["min_inliers"]])
    b = P.evaluate([c], ctx=ctx, quads=[c["quads"][cut:]], best_in=[best])
    _assert_same(_concat([a, b]), whole)
    assert len(P.records(whole["n_inliers"], c["min_inliers"])) >= 2


def test_two_runs_byte_identical(ctx):
    cases = [P.case(n) for n in P.ALL]
    a, b = P.evaluate(cases, ctx=ctx), P.evaluate(cases, ctx=ctx)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
