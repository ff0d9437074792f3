"""Local mapping on the device against the restatement (tests/local_mapping_restatement.py): cs_create_new_map_points, cs_mappoint_distinctive_descriptors and
cs_mappoint_update_normal_and_depth on the cases of tests/local_mapping_patterns.py.  No tolerance anywhere: x3D, normals and distances equal as bit patterns, statuses, claims and
indices equal entry for entry.  Every index a case hands in is inside its table, except where the test is that the call refuses it before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from tests import local_mapping_patterns as P
from tests import local_mapping_restatement as R

pytestmark = pytest.mark.gpu


def _view(f):
    from cube_slam_amd.local_mapping import KeyFrameView
    return KeyFrameView(f.keysUn.copy(), f.keys_xy, f.u_right, f.depth, f.Rcw, f.tcw, f.Ow, f.fx, f.fy, f.cx, f.cy, f.invfx, f.invfy, f.mbf, f.mb, f.scale_factors, f.level_sigma2, f.scale_factor)


def _equal(got, j):
    assert np.array_equal(got["pair_off"], j["pair_off"]) and np.array_equal(got["idx1"], j["idx1"]) and np.array_equal(got["idx2"], j["idx2"])
    bad = np.nonzero(got["status"] != j["status"])[0]
    assert len(bad) == 0, [(int(p), int(got["status"][p]), int(j["status"][p])) for p in bad[:10]]
    assert got["x3D"].tobytes() == j["x3D"].astype(np.float32).tobytes()
    assert np.array_equal(got["new_pair_of_idx1"], j["new_pair_of_idx1"]) and got["nnew"] == j["nnew"]


@pytest.mark.parametrize("name", P.ALL)
def test_create_new_map_points(ctx, name):
    from cube_slam_amd.local_mapping import create_new_map_points
    s, j = P.scene(name), P.judged(name)
    got = create_new_map_points(ctx, _view(s["kf"]), [_view(f) for f in s["neighbours"]], j["matches12"])
    _equal(got, j)


@pytest.mark.parametrize("name", ["n3_mixed", "statuses"])
def test_mirror_loop(ctx, name):
    """LocalMapping.CreateNewMapPoints with the table search in the matcher's place: the baseline tests drop what the reference drops (the neighbours closer than their mb), the
    points come in the reference's creation order, and the prefix rule holds against the loop stopped early."""
    from cube_slam_amd.local_mapping import LocalMapping
    s = P.scene(name)
    views = [_view(f) for f in s["neighbours"]]
    lm = LocalMapping(ctx=ctx, monocular=False)
    kept = [i for i, f in enumerate(s["neighbours"]) if not np.float32(R.norm64([f.Ow[k] - s["kf"].Ow[k] for k in range(3)])) < f.mb]
    assert 0 < len(kept) < len(views)
    tables = {id(v): s["best2"][i] for i, v in enumerate(views)}
    search = lambda kf, nb, F12, epi: np.where(s["skip1"], -1, tables[id(nb)]).astype(np.int32)
    res = lm.CreateNewMapPoints(_view(s["kf"]), views, [None] * len(views), [None] * len(views), search=search)
    assert res["kept"] == kept
    want, _ = R.create_new_map_points(s["kf"], [s["neighbours"][i] for i in kept], R.table_search([s["best2"][i] for i in kept]), s["skip1"])
    assert [(kept[a[0]], a[1], a[2]) for a in want] == list(zip(res["new_neighbour"].tolist(), res["new_idx1"].tolist(), res["new_idx2"].tolist()))
    assert np.array([a[3] for a in want], np.float32).tobytes() == res["new_x3D"].tobytes()
    stop = kept[-1]  # CheckNewKeyFrames() turns true before the last surviving neighbour
    early, _ = R.create_new_map_points(s["kf"], [s["neighbours"][i] for i in kept[:-1]], R.table_search([s["best2"][i] for i in kept[:-1]]), s["skip1"])
    nb_, i1_, i2_, x_ = lm.points_before(res, stop)
    assert [(kept[a[0]], a[1], a[2]) for a in early] == list(zip(nb_.tolist(), i1_.tolist(), i2_.tolist())) and np.array([a[3] for a in early], np.float32).reshape(-1, 3).tobytes() == x_.tobytes()


def test_mirror_through_the_matcher(ctx):
    """The neighbour loop with the real search: two copies of one frame's descriptors a baseline apart, so SearchForTriangulation matches key point i with key point i; what it
    returns is handed to cs_create_new_map_points as it is and judged by the restatement on the same matches."""
    from cube_slam_amd.local_mapping import KeyFrameView, LocalMapping
    s = P.scene("n1_mixed_63")
    f1, f2 = s["kf"], s["neighbours"][0]
    tab = s["best2"][0]
    i1 = np.nonzero(tab >= 0)[0]
    rng = np.random.RandomState(5)
    d1 = rng.randint(0, 256, (f1.N, 32)).astype(np.uint8); d2 = rng.randint(0, 256, (f2.N, 32)).astype(np.uint8)
    d2[tab[i1]] = d1[i1]
    mk = lambda f, d, skip: KeyFrameView(f.keysUn, f.keys_xy, f.u_right, f.depth, f.Rcw, f.tcw, f.Ow, f.fx, f.fy, f.cx, f.cy, f.invfx, f.invfy, f.mbf, f.mb, f.scale_factors,
                                         f.level_sigma2, f.scale_factor, desc=d, node=np.zeros(f.N, np.int32), skip=skip)
    v1, v2 = mk(f1, d1, s["skip1"].astype(np.uint8)), mk(f2, d2, np.zeros(f2.N, np.uint8))
    R1, R2 = f1.Rcw.reshape(3, 3).astype(np.float64), f2.Rcw.reshape(3, 3).astype(np.float64)
    R12 = R1 @ R2.T
    t12 = -R12 @ f2.tcw.astype(np.float64) + f1.tcw.astype(np.float64)
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    K = np.array([[P.FX, 0, P.CX], [0, P.FY, P.CY], [0, 0, 1.0]])
    F12 = np.linalg.inv(K).T @ tx @ R12 @ np.linalg.inv(K)  # LocalMapping::ComputeF12
    c2 = R2 @ f1.Ow.astype(np.float64) + f2.tcw.astype(np.float64)
    epi = (P.FX * c2[0] / c2[2] + P.CX, P.FY * c2[1] / c2[2] + P.CY)
    lm = LocalMapping(ctx=ctx, monocular=False)
    res = lm.CreateNewMapPoints(v1, [v2], [F12.astype(np.float32)], [epi])
    m12 = np.full(f1.N, -1, np.int32)
    m12[res["idx1"]] = res["idx2"]
    assert len(res["idx1"]) >= 20 and (m12[i1][m12[i1] >= 0] == tab[i1][m12[i1] >= 0]).all() and not (m12[s["skip1"]] >= 0).any()
    j = R.expected_outputs(f1, [f2], R.table_search([m12]), np.zeros(f1.N, bool))
    _equal(res, j)
    assert res["nnew"] >= 10


def _call(ctx, kf, nbs, m, cap=None, outs=None, null=None):
    """The C-ABI call on output arrays filled with marks, one element longer than needed; null: the name of one argument to pass as NULL."""
    from cube_slam_amd._lib import lib
    from cube_slam_amd.local_mapping import CsLmFrame
    n = len(nbs)
    cap = int((m >= 0).sum()) if cap is None else cap
    o = outs or {"off": np.full(n + 1, -7, np.int32), "i1": np.full(cap + 1, -7, np.int32), "i2": np.full(cap + 1, -7, np.int32), "x": np.full(3 * cap + 3, -7, np.float32),
                 "st": np.full(cap + 1, 77, np.uint8), "new": np.full(kf.N + 1, -7, np.int32), "nnew": C.c_int(-7)}
    p = lambda k, a, t: None if null == k else a.ctypes.data_as(C.POINTER(t))
    arr = (CsLmFrame * max(n, 1))(*[f.c_struct() for f in nbs])
    cur = kf.c_struct()
    r = lib().cs_create_new_map_points(ctx.ptr, None if null == "kf" else C.byref(cur), None if null == "nbs" else arr, n, p("m", m, C.c_int), cap, p("off", o["off"], C.c_int),
                                       p("i1", o["i1"], C.c_int), p("i2", o["i2"], C.c_int), p("x", o["x"], C.c_float), p("st", o["st"], C.c_uint8), p("new", o["new"], C.c_int),
                                       None if null == "nnew" else C.byref(o["nnew"]))
    return r, o


def _untouched(o):
    return (o["off"] == -7).all() and (o["i1"] == -7).all() and (o["i2"] == -7).all() and (o["x"] == -7).all() and (o["st"] == 77).all() and (o["new"] == -7).all() and o["nnew"].value == -7


def test_bad_arguments_create(ctx):
    from cube_slam_amd._lib import lib
    s, j = P.scene("n3_mixed"), P.judged("n3_mixed")
    kf, nbs = _view(s["kf"]), [_view(f) for f in s["neighbours"]]
    m = j["matches12"].copy()
    first = tuple(np.argwhere(m >= 0)[0])

    def refused(kf_, nbs_, m_, what, **kw):
        r, o = _call(ctx, kf_, nbs_, np.ascontiguousarray(m_, np.int32), **kw)
        assert r == -2 and _untouched(o), what
        assert what in lib().cs_last_error(ctx.ptr).decode(), (what, lib().cs_last_error(ctx.ptr).decode())

    bad = m.copy(); bad[first] = nbs[first[0]].N
    refused(kf, nbs, bad, "matches12")
    bad = m.copy(); bad[first] = -2
    refused(kf, nbs, bad, "matches12")
    k = _view(s["kf"]); k.keysUn["octave"][first[1]] = k.scale_factors.size
    refused(k, nbs, m, "octave")
    n0 = _view(s["neighbours"][first[0]]); n0.keysUn["octave"][m[first]] = -1
    refused(kf, [n0 if i == first[0] else v for i, v in enumerate(nbs)], m, "octave")
    refused(kf, [nbs[i % 3] for i in range(33)], np.full((33, kf.N), -1, np.int32), "n_neigh")
    for null in ("keysUn", "keys_xy", "u_right", "depth", "scale_factors", "level_sigma2"):  # a NULL array of a frame
        k = _view(s["kf"]); setattr(k, null, np.zeros(0, np.float32))
        st = k.c_struct(); setattr(st, null, None)
        k.c_struct = lambda st=st: st
        refused(k, nbs, m, "NULL")
        n1 = _view(s["neighbours"][1]); st1 = n1.c_struct(); setattr(st1, null, None)
        n1.c_struct = lambda st1=st1: st1
        refused(kf, [nbs[0], n1, nbs[2]], m, "NULL")
    for null in ("off", "i1", "i2", "x", "st", "new", "nnew", "m", "kf", "nbs"):  # a NULL argument of the call
        r, o = _call(ctx, kf, nbs, m, null=null)
        assert r == -2 and _untouched(o) and "NULL" in lib().cs_last_error(ctx.ptr).decode(), null
    r, o = _call(ctx, kf, nbs, m, cap=int((m >= 0).sum()) - 1)  # one pair more than there is room for: only pair_off is written
    assert r == -4 and np.array_equal(o["off"], j["pair_off"]) and (o["i1"] == -7).all() and (o["st"] == 77).all() and (o["new"] == -7).all()
    r, o = _call(ctx, kf, nbs, m)  # the context is as usable as before
    assert r == 0 and np.array_equal(o["st"][:-1], j["status"]) and o["st"][-1] == 77 and o["new"][-1] == -7 and (o["x"][-3:] == -7).all()


# ---- ComputeDistinctiveDescriptors
@pytest.mark.parametrize("kind", ["sizes", "equal", "ties", "mixed"])
def test_distinctive_descriptors(ctx, kind):
    from cube_slam_amd.local_mapping import ComputeDistinctiveDescriptors
    off, desc = P.descriptor_sets(kind)
    want = R.distinctive_descriptors(off, desc)
    got = ComputeDistinctiveDescriptors(ctx, off, desc)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(p), int(off[p + 1] - off[p]), int(got[p]), int(want[p])) for p in bad[:10]]


def test_distinctive_descriptors_no_points_and_bad_arguments(ctx):
    from cube_slam_amd._lib import lib
    from cube_slam_amd.local_mapping import ComputeDistinctiveDescriptors
    assert len(ComputeDistinctiveDescriptors(ctx, np.zeros(1, np.int32), np.zeros((0, 32), np.uint8))) == 0
    assert ComputeDistinctiveDescriptors(ctx, np.zeros(3, np.int32), np.zeros((0, 32), np.uint8)).tolist() == [-1, -1]
    off, desc = P.descriptor_sets("sizes")
    best = np.full(len(off) - 1, -7, np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    for bad in (off[::-1].copy(), off + 1):
        assert lib().cs_mappoint_distinctive_descriptors(ctx.ptr, len(off) - 1, p(np.ascontiguousarray(bad, np.int32), C.c_int), p(desc, C.c_uint8), p(best, C.c_int)) == -2
        assert (best == -7).all() and b"obs_off" in lib().cs_last_error(ctx.ptr)
    assert lib().cs_mappoint_distinctive_descriptors(ctx.ptr, len(off) - 1, p(off, C.c_int), None, p(best, C.c_int)) == -2 and (best == -7).all()


# ---- UpdateNormalAndDepth
@pytest.mark.parametrize("n_points", P.NORMAL_N)
def test_update_normal_and_depth(ctx, n_points):
    from cube_slam_amd.local_mapping import UpdateNormalAndDepth
    c = P.normal_case(n_points)
    normal, mind, maxd, upd = P.normal_judged(n_points)
    seven = lambda *shape: np.full(shape, 7.0, np.float32)
    got = UpdateNormalAndDepth(ctx, c["pos"], c["obs_off"], c["obs_kf"], c["kf_Ow"], c["ref_kf"], c["ref_octave"], P.SF, seven(n_points, 3), seven(n_points), seven(n_points))
    assert np.array_equal(got[3], upd) and (upd == 0).sum() == (1 if n_points > 1 else 0)
    assert got[0].tobytes() == normal.tobytes() and got[1].tobytes() == mind.tobytes() and got[2].tobytes() == maxd.tobytes()  # (an empty run keeps its sevens)


def test_update_normal_and_depth_bad_arguments(ctx):
    """Through the C-ABI, so that the caller's own output arrays are what is looked at: refused with a message, nothing written."""
    from cube_slam_amd._lib import lib
    from cube_slam_amd.local_mapping import UpdateNormalAndDepth
    c = P.normal_case(65)
    seven = lambda *shape: np.full(shape, 7.0, np.float32)
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))

    def refused(what, **change):
        a = dict(c, sf=P.SF, n_levels=P.N_LEVELS, normal=seven(65, 3)); a.update(change)
        for k in ("obs_off", "obs_kf", "ref_kf", "ref_octave"):
            a[k] = None if a[k] is None else np.ascontiguousarray(a[k], np.int32)
        nv, mn, mx, up = a["normal"], seven(65), seven(65), np.full(65, 9, np.uint8)
        r = lib().cs_mappoint_update_normal_and_depth(ctx.ptr, 65, p(a["pos"], C.c_float), p(a["obs_off"], C.c_int), p(a["obs_kf"], C.c_int), a["n_kf"], p(a["kf_Ow"], C.c_float),
                                                      p(a["ref_kf"], C.c_int), p(a["ref_octave"], C.c_int), p(a["sf"], C.c_float), a["n_levels"], p(nv, C.c_float), p(mn, C.c_float),
                                                      p(mx, C.c_float), p(up, C.c_uint8))
        assert r == -2, what
        assert what in lib().cs_last_error(ctx.ptr).decode(), (what, lib().cs_last_error(ctx.ptr).decode())
        assert (nv is None or (nv == 7).all()) and (mn == 7).all() and (mx == 7).all() and (up == 9).all(), what

    obs = c["obs_kf"].copy(); obs[3] = c["n_kf"]
    refused("observation", obs_kf=obs)
    obs = c["obs_kf"].copy(); obs[-1] = -1
    refused("observation", obs_kf=obs)
    rk = c["ref_kf"].copy(); rk[0] = c["n_kf"]
    refused("reference key frame", ref_kf=rk)
    ro = c["ref_octave"].copy(); ro[5] = P.N_LEVELS
    refused("reference octave", ref_octave=ro)
    off = c["obs_off"].copy(); off[4] = off[3] - 1
    refused("obs_off", obs_off=off)
    refused("NULL", pos=None)
    refused("NULL", ref_kf=None)
    refused("NULL", normal=None)
    refused("NULL", sf=None)
    refused("n_levels", n_levels=0)
    refused("obs_off", obs_kf=None)
    rk = c["ref_kf"].copy(); rk[-1] = 10 ** 6  # the empty run reads neither: not an error
    ro = c["ref_octave"].copy(); ro[-1] = 99
    got = UpdateNormalAndDepth(ctx, c["pos"], c["obs_off"], c["obs_kf"], c["kf_Ow"], rk, ro, P.SF, seven(65, 3), seven(65), seven(65))
    assert got[0].tobytes() == P.normal_judged(65)[0].tobytes()
