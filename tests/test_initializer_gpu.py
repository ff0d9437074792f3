"""Initializer on the device against the host path of the same headers (cs_initializer_evaluate with and without a context) on the cases of tests/initializer_patterns.py.  No
tolerance anywhere: every output array equal as bit patterns, a NaN equal to any NaN (the bit class: x86 and the device give NaNs of different sign and payload; the only NaN of
the patterns is RH where no hypothesis scores).  The shapes are the smallest at which the kernels can go wrong: N = 8 (the set is the whole problem), 31 / 32 / 33 (the second
mask word), 63 / 64 / 65 and 130 (the lane stride and the ballot halves), 1 to 24 hypotheses, 0, 4 and 8 candidates, fewer and more than 51 good points, problems without a
model and without matches inside a batch."""
import os

import numpy as np
import pytest
import torch

# torch's copy of the HIP runtime must be the first in the process (the ctx fixture of tests/conftest.py), and importing the patterns loads libcubeslam_hip.so.
torch.cuda.is_available()

from tests import initializer_patterns as P

pytestmark = pytest.mark.gpu


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
    for k in P.KEYS:
        assert same(got[k], want[k]), k


@pytest.mark.parametrize("name", P.ALL)
def test_single_equals_host(ctx, name):
    _assert_same(P.evaluate([P.case(name)], ctx=ctx)[0], P.judged(name))


@pytest.mark.parametrize("batch", P.BATCHES, ids=["-".join(b) for b in P.BATCHES])
def test_batch_equals_singles_equals_rerun(ctx, batch):
    cases = [P.case(n) for n in batch]
    got = P.evaluate(cases, ctx=ctx)[0]
    _assert_same(got, P.concat([P.judged(n) for n in batch]))
    again = P.evaluate(cases, ctx=ctx)[0]
    for k in P.KEYS:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_mirror_with_context_equals_without(ctx):
    """Initializer.evaluate_many on the device for three frame pairs at once against the same on the host: every table byte-equal, and the same Initialize result."""
    from cube_slam_amd.initializer import Initializer
    names = ["general", "plane", "few"]

    def run(c_ctx):
        its = []
        for n in names:
            c = P.case(n)
            it = Initializer(c["keys1"], c["K"], c["sigma"], len(c["sets"]), ctx=c_ctx)
            it.set_sets(c["sets"])
            it.prepare(c["keys2"], c["vMatches12"])
            its.append(it)
        Initializer.evaluate_many(its)
        return its, [it.result() for it in its]

    dev, rdev = run(ctx)
    host, rhost = run(None)
    for d, h, n in zip(dev, host, names):
        for k in P.KEYS:
            assert same(d._table[k], h._table[k]), (n, k)
    for a, b in zip(rdev, rhost):
        assert a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            assert (x is None and y is None) or same(x, y)
    assert [r[0] for r in rdev] == [True, True, False]


@pytest.mark.parametrize("what", ["index_high", "index_negative", "repeated", "n_below_8", "match_outside", "no_keys"])
def test_refusals(ctx, what):
    """CS_ERR_BAD_ARG before anything is launched, the outputs untouched; the offending entry sits in the last problem of three, behind valid ones."""
    cases = [dict(P.case("n33")), dict(P.case("empty")), dict(P.case("n65"))]
    c = cases[2]
    c["sets"] = P.case("n64")["sets"].copy()
    if what == "index_high":
        c["sets"][4, 1] = 65
    elif what == "index_negative":
        c["sets"][0, 2] = -1
    elif what == "repeated":
        c["sets"][3, 7] = c["sets"][3, 0]
    elif what == "n_below_8":
        c["matches"], c["N"] = c["matches"][:7], 7
        c["sets"] = np.arange(8, dtype=np.int32).reshape(1, 8) % 7
    elif what == "match_outside":
        c["matches"] = c["matches"].copy(); c["matches"][64, 1] = len(c["keys2"])
    else:
        c["keys1"] = c["keys1"][:0]  # (with the matches kept: every match is outside)
    ctx.timing(True); ctx.timing_reset()
    rc, err, out = P.raw_call(ctx, cases)
    launches = sum(ctx.timing_get(k)[1] for k in ("init_normalize", "init_hypotheses", "init_select", "init_check_rt"))
    ctx.timing(False)
    assert rc == -2 and "cs_initializer_evaluate" in err
    assert launches == 0
    for k, v in out.items():
        assert (v.view(np.uint8) == 0x5A).all(), k


def test_launches_are_counted(ctx):
    """The counter the refusals rely on does count: one valid call, one launch of each kernel."""
    ctx.timing(True); ctx.timing_reset()
    rc, _, _ = P.raw_call(ctx, [P.case("n33")])
    n = [ctx.timing_get(k)[1] for k in ("init_normalize", "init_hypotheses", "init_select", "init_check_rt")]
    ctx.timing(False)
    assert rc == 0 and n == [1, 1, 1, 1]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "initializer.npz")


@pytest.mark.parametrize("name", P.ALL)
def test_equals_recorded_reference(ctx, name):
    """The device against the recorded run of the reference's own text (tests/golden/initializer.npz, written by tests/test_initializer_reference_pins.py; the reference tree
    is not read here): per hypothesis the score and, where the reference keeps one, the matrix and the mask; SH, SF; and through the mirror with a context the return value,
    R21, t21, vP3D and vbTriangulated."""
    from cube_slam_amd._ransac import mask_bits
    from cube_slam_amd.initializer import Initializer
    g = np.load(GOLDEN)
    c = P.case(name)
    got = P.evaluate([c], ctx=ctx)[0]
    H, N = len(c["sets"]), c["N"]
    W = (N + 31) // 32
    assert got["score"].tobytes() == g[name + "/score"].tobytes()
    mask = np.unpackbits(g[name + "/mask"], axis=-1)[..., :N].astype(bool) if H and N else np.zeros((2, H, N), bool)
    for m in range(2):
        for h in range(H):
            if g[name + "/kept"][m, h]:
                assert got["matrix"][m, h].tobytes() == g[name + "/matrix"][m, h].tobytes(), (m, h)
                assert np.array_equal(mask_bits(got["mask"][m, h * W:(h + 1) * W], N), mask[m, h]), (m, h)
    assert got["S"][0].tobytes() == g[name + "/S"].tobytes()
    branch, ret = g[name + "/branch_ret"]
    if ret < 0:
        return  # (Initialize was not run on the reference's side: no model, or fewer than 8 matches)
    assert got["model"][0] == branch
    it = Initializer(c["keys1"], c["K"], c["sigma"], H, ctx=ctx)
    it.set_sets(c["sets"])
    ok, R21, t21, vP3D, vb = it.Initialize(c["keys2"], c["vMatches12"])
    assert int(ok) == ret
    if ok:
        assert R21.tobytes() == g[name + "/R21"].tobytes() and t21.tobytes() == g[name + "/t21"].tobytes()
    assert vP3D.tobytes() == g[name + "/vP3D"].tobytes()
    assert np.array_equal(vb, np.unpackbits(g[name + "/vbTriangulated"])[:len(vb)].astype(bool))
