"""CPU: the cases of tests/local_mapping_patterns.py hold what their names promise, judged by tests/local_mapping_restatement.py alone -- and the restatement's own pieces hold
against independent forms: its f64 Jacobi against numpy.linalg.svd, its array forms against its scalar forms."""
import collections

import numpy as np
import pytest

from tests import local_mapping_patterns as P
from tests import local_mapping_restatement as R


def test_jacobi_against_numpy_svd():
    """The stated definition of cv::SVD (:448): the vector is numpy's last right singular vector up to sign, to the accuracy the gap between the two smallest singular values
    allows in double."""
    worst = 0.0
    n = 0
    for name in ("n3_mixed", "n3_mono_gap", "claim_0_2", "statuses"):
        s = P.scene(name)
        for nb_i, nb in enumerate(s["neighbours"]):
            for idx1 in np.nonzero(s["best2"][nb_i] >= 0)[0]:
                info = {}
                R.triangulate_pair(s["kf"], int(idx1), nb, int(s["best2"][nb_i][idx1]), info)
                if info["branch"] != "svd":
                    continue
                A = info["A"].astype(np.float64)
                v = np.array(R.jacobi_vmin4(A.tolist()))
                sv = np.linalg.svd(A)
                ref = sv[2][3]
                d = min(np.abs(v - ref).max(), np.abs(v + ref).max())
                bound = 64 * 2.0 ** -52 * sv[1][0] / (sv[1][2] - sv[1][3])
                worst = max(worst, d / bound)
                assert abs(np.linalg.norm(v) - 1) < 1e-14 and d <= bound, (name, nb_i, idx1, d, bound)
                n += 1
    print("%d matrices, worst distance / bound %.3f" % (n, worst))
    assert n >= 250


@pytest.mark.parametrize("name", P.ALL)
def test_scene_shapes(name):
    s, j = P.scene(name), P.judged(name)
    assert len(s["neighbours"]) <= 32
    for n, tab in enumerate(s["best2"]):
        assert tab.min() >= -1 and tab.max() < s["neighbours"][n].N
    counts = np.diff(j["pair_off"])
    if name in P.SCENES:
        want = P.SCENES[name][2]
        shared = sum(1 for c in want if c >= 2)
        assert list(counts) == want, "the table of every neighbour names its count of key points without a map point"
        assert j["nnew"] >= 0.3 * min(counts.sum(), 300) - shared
        mode = P.SCENES[name][3]
        ur = np.concatenate([s["kf"].u_right] + [f.u_right for f in s["neighbours"]])
        assert {"mono": (ur < 0).all(), "stereo": (ur >= 0).all(), "mixed": (ur < 0).any() and (ur >= 0).any()}[mode]
    hist = collections.Counter(int(x) for x in j["status"])
    print(name, "pairs", int(counts.sum()), "new", j["nnew"], {R.STATUS_NAMES[k]: v for k, v in sorted(hist.items())})


@pytest.mark.parametrize("name", P.ALL)
def test_marginal_pairs_stay_under_two_percent(name):
    """A pair is marginal where the reference's float SVD or libm cosine may decide it otherwise than the stated definitions do (R.marginal_pairs: the status moves with x3D
    within R.TOL_X3D = 10 x D_REF_X3D, or cosParallaxRays lies within D_COS of cosParallaxStereo).  The pin test exempts such pairs, so a case may hold few of them."""
    s, j = P.scene(name), P.judged(name)
    m = R.marginal_pairs(s["kf"], s["neighbours"], j["matches12"])
    assert len(m) == j["pair_off"][-1]
    k = sum(m.values())
    print(name, "pairs", len(m), "marginal", k)
    assert k <= 0.02 * len(m)
    assert R.TOL_X3D == 10 * R.D_REF_X3D


def test_large_scenes_take_every_branch():
    for name, need in (("n20_mixed", {"svd", "stereo1", "stereo2", None}), ("n20_mono", {"svd", None}), ("n3_stereo", {"svd"})):
        s = P.scene(name)
        seen = set()
        for n, nb in enumerate(s["neighbours"]):
            for idx1 in np.nonzero((s["best2"][n] >= 0) & ~s["skip1"])[0][:80]:
                info = {}
                R.triangulate_pair(s["kf"], int(idx1), nb, int(s["best2"][n][idx1]), info)
                seen.add(info["branch"])
        assert need <= seen, (name, seen)
    j = P.judged("n20_mixed")
    assert (j["status"] == R.CLAIMED).sum() >= 50 and len(set(j["status"].tolist())) >= 6


def test_shared_idx2():
    for name in ("n3_mixed", "claim_0_2"):
        tab = P.scene(name)["best2"][0]
        vals = tab[tab >= 0]
        assert len(vals) > len(set(vals.tolist())), "two key points of the current key frame share a best match"


def test_claim_0_2():
    s = P.scene("claim_0_2")
    st = [R.triangulate_pair(s["kf"], 5, s["neighbours"][n], int(s["best2"][n][5]))[0] for n in range(3)]
    assert st[0] == R.CREATED and st[1] != R.CREATED and st[2] == R.CREATED
    j = P.judged("claim_0_2")
    pairs5 = [p for p in range(len(j["idx1"])) if j["idx1"][p] == 5]
    assert len(pairs5) == 3 and j["status"][pairs5[0]] == R.CREATED and j["status"][pairs5[1]] == R.CLAIMED and j["status"][pairs5[2]] == R.CLAIMED
    assert j["new_pair_of_idx1"][5] == pairs5[0]


def test_statuses_hit_every_status_and_branch():
    s, j = P.scene("statuses"), P.judged("statuses")
    got = {}
    for n in range(len(s["neighbours"])):
        for p in range(j["pair_off"][n], j["pair_off"][n + 1]):
            got[(n, int(j["idx1"][p]))] = int(j["status"][p])
    assert got == P.STATUS_ROWS
    assert set(got.values()) == set(range(11)) - {R.W_ZERO}
    for (n, i), branch in P.STATUS_BRANCH.items():
        info = {}
        R.triangulate_pair(s["kf"], i, s["neighbours"][n], i, info)
        assert info["branch"] == branch, (n, i, info["branch"])
    a, b = {}, {}
    R.triangulate_pair(s["kf"], 14, s["neighbours"][0], 14, a); R.triangulate_pair(s["kf"], 15, s["neighbours"][0], 15, b)
    assert 0.9998 <= float(a["cosParallaxRays"]) < 0.99985 and 0.99975 < float(b["cosParallaxRays"]) < 0.9998
    assert s["kf"].depth[10] < 0 <= s["kf"].u_right[10]  # the stereo key point without depth
    z = P.judged("w_zero")
    assert z["status"].tolist() == [R.W_ZERO] and z["nnew"] == 0 and not z["x3D"].any()
    c, d = {}, {}
    cz = P.scene("cos_zero")
    R.triangulate_pair(cz["kf"], 0, cz["neighbours"][0], 0, c); R.triangulate_pair(cz["kf"], 0, cz["neighbours"][1], 0, d)
    assert 0 < float(c["cosParallaxRays"]) < 0.02 and -0.02 < float(d["cosParallaxRays"]) < 0 and c["branch"] == "svd" and d["branch"] is None


@pytest.mark.parametrize("kind", ["sizes", "equal", "ties"])
def test_descriptor_sets(kind):
    off, desc = P.descriptor_sets(kind)
    assert tuple(np.diff(off)) == P.DESC_N
    fast = R.distinctive_descriptors(off, desc)
    for p in range(len(off) - 1):
        d = desc[off[p]:off[p + 1]]
        assert R.distinctive_descriptor(d) == fast[p]
        if kind == "equal":
            assert fast[p] == 0
        if kind == "ties":
            assert len({bytes(r) for r in d}) <= 3
    if kind == "sizes":
        assert (fast[3:] > 0).any(), "a case where the answer is not the first row"


def test_descriptor_mixed():
    off, desc = P.descriptor_sets("mixed")
    n = np.diff(off)
    assert len(n) == 2000 and (n == 0).sum() >= 2 and n.max() == 130 and n[n <= 40].max() == 40
    best = R.distinctive_descriptors(off, desc)
    assert (best[n == 0] == -1).all() and (best[n > 0] >= 0).all() and len(set(best.tolist())) > 10
    for p in (0, 5, 7, 1000):
        assert R.distinctive_descriptor(desc[off[p]:off[p + 1]]) == best[p]


@pytest.mark.parametrize("n_points", [1, 64, 65])
def test_normal_cases(n_points):
    c = P.normal_case(n_points)
    normal, mind, maxd, upd = P.normal_judged(n_points)
    runs = np.diff(c["obs_off"])
    assert runs.max() <= 40 and c["obs_kf"][c["obs_off"][1] - 1] == c["ref_kf"][0], "point 0 has its reference key frame last in its run"
    if n_points > 1:
        assert runs[-1] == 0 and upd[-1] == 0 and (normal[-1] == 7).all() and runs[1] == 40 and runs[2] == 1
    for p in range(n_points):  # the array form against the scalar form, bit for bit
        r = R.update_normal_and_depth(c["pos"][p], c["obs_kf"][c["obs_off"][p]:c["obs_off"][p + 1]], c["kf_Ow"], c["ref_kf"][p], c["ref_octave"][p], P.SF)
        if r is None:
            assert upd[p] == 0
            continue
        assert np.array(r[0], np.float32).tobytes() == normal[p].tobytes() and np.float32(r[1]).tobytes() == mind[p].tobytes() and np.float32(r[2]).tobytes() == maxd[p].tobytes()
        assert 0.5 < np.linalg.norm(normal[p]) <= 1.0001 and mind[p] < maxd[p]
