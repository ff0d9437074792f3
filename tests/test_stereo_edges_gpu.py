"""GPU parity of the stereo association on designed key points (tests/stereo_patterns.py) through cs_stereo_match_from_keys: mvuRight, mvDepth and n_matched byte for
byte against tests/stereo_restatement.py, fed the same keys and what cs_orb_get_level returns for every level of the same run.  No tolerance: the arithmetic is integer
or single float operations in a fixed order.  Every designed pair is uploaded once, to two extractors, and the restatement runs once per pair; the conditions of
tests/test_stereo_patterns.py are repeated on the real levels, so that agreement on all -1 cannot pass."""
import ctypes as C

import numpy as np
import pytest

from cube_slam_amd import _lib
from cube_slam_amd.orb import ORBextractor
from cube_slam_amd.stereo import StereoMatcher
from tests import stereo_patterns as sp
from tests import stereo_restatement as sr

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD_ARG, CAPACITY = -2, -4
CAP = 300


class _Designed:
    pass


@pytest.fixture(scope="module")
def designed(ctx):
    """Every pair of the batch on two extractors (frame p = pair p), and the restatement's answer for each, computed once."""
    d = _Designed()
    d.pairs = sp.batch()
    d.index = {p.name: i for i, p in enumerate(d.pairs)}
    n = len(d.pairs)
    d.extL = ORBextractor(500, sp.SCALE, sp.NLEVELS, 20, 7, sp.W, sp.H, max_frames=n, ctx=ctx)
    d.extR = ORBextractor(500, sp.SCALE, sp.NLEVELS, 20, 7, sp.W, sp.H, max_frames=n, ctx=ctx)
    d.extL.upload(np.stack([p.left for p in d.pairs])); d.extL.run()
    d.extR.upload(np.stack([p.right for p in d.pairs])); d.extR.run()
    assert np.array_equal(d.extL.GetScaleFactors(), sp.SF) and np.array_equal(d.extL.GetInverseScaleFactors(), sp.ISF)
    d.want = []
    for i, p in enumerate(d.pairs):
        lvL, lvR = [d.extL.level(i, l) for l in range(sp.NLEVELS)], [d.extR.level(i, l) for l in range(sp.NLEVELS)]
        assert np.array_equal(lvL[0], p.left) and np.array_equal(lvR[0], p.right)  # level 0 is the designed image
        assert [a.shape for a in lvL] == list(zip(sp.LEVEL_H, sp.LEVEL_W))
        st = {}
        uR, dep, kept = sr.compute_stereo_matches(p.kl, p.dl, p.kr, p.dr, lvL, lvR, sp.SF, sp.ISF, p.bf, p.b, stats=st)
        print(p.name, "nl %d nr %d" % (len(p.kl), len(p.kr)), {k: v for k, v in st.items() if k not in ("best", "sad")})
        d.want.append((st, uR, dep, kept))
    yield d
    d.extL.close(); d.extR.close()


def _same(got, nm, want, what=""):
    (gu, gd), (st, wu, wd, kept) = got, want
    assert gu.dtype == np.float32 and gd.dtype == np.float32 and len(gu) == len(wu) == len(gd)
    assert gu.tobytes() == wu.tobytes(), "%s mvuRight: %d of %d differ" % (what, int((gu != wu).sum()), len(gu))
    assert gd.tobytes() == wd.tobytes(), "%s mvDepth: %d of %d differ" % (what, int((gd != wd).sum()), len(gd))
    assert int(nm) == kept, what


def _single(d, m, i):
    p = d.pairs[i]
    m.match_keys(d.extL, d.extR, [p.kl], [p.dl], [p.kr], [p.dr], p.bf, p.b, left_first=i, right_first=i)
    (got,), nm = m.read()
    return got, nm[0]


@pytest.mark.parametrize("group", ["cut", "disparity", "window", "levels", "border", "descriptor"])
def test_group_equals_restatement(ctx, designed, group):
    """Each pair of the group in a call of its own, on one handle."""
    d = designed
    m = StereoMatcher(CAP, 1, ctx=ctx)
    for p in sp.groups()[group]:
        i = d.index[p.name]
        p = d.pairs[i]
        st, uR, dep, kept = d.want[i]
        sp.assert_reached(p, st, uR, dep, kept)  # the design holds on the real levels
        got, nm = _single(d, m, i)
        _same(got, nm, d.want[i], p.name)
    m.close()


def _call(d, m, idx):
    """Pairs idx (consecutive frames, one bf / b) in one call."""
    ps = [d.pairs[i] for i in idx]
    assert list(idx) == list(range(idx[0], idx[0] + len(idx))) and len({(p.bf, p.b) for p in ps}) == 1
    m.match_keys(d.extL, d.extR, [p.kl for p in ps], [p.dl for p in ps], [p.kr for p in ps], [p.dr for p in ps], ps[0].bf, ps[0].b, left_first=idx[0], right_first=idx[0])
    return m.read()


def _runs_of_equal_calibration(pairs):
    """The batch cut into the longest runs of consecutive pairs that share bf / b (one call has one calibration)."""
    runs, start = [], 0
    for i in range(1, len(pairs) + 1):
        if i == len(pairs) or (pairs[i].bf, pairs[i].b) != (pairs[start].bf, pairs[start].b):
            runs.append(list(range(start, i)))
            start = i
    return runs


def test_batch_equals_restatement_and_single_calls(ctx, designed):
    """The designed pairs in batched calls, pairs of nl == 0 or nr == 0 between them (stereo_prep's nr == 0 beside nr > 0 in one launch; a wrong median in one pair of a
    batch), against the restatement and against the single calls."""
    d = designed
    m = StereoMatcher(CAP, len(d.pairs), ctx=ctx)
    one = StereoMatcher(CAP, 1, ctx=ctx)
    runs = _runs_of_equal_calibration(d.pairs)
    assert max(len(r) for r in runs) >= 12
    seen_empty = 0
    for idx in runs:
        res, nm = _call(d, m, idx)
        pu, pd, first, pnm = m.read_packed()
        assert np.array_equal(pnm, nm) and first[-1] == sum(len(d.pairs[i].kl) for i in idx)
        for k, i in enumerate(idx):
            _same(res[k], nm[k], d.want[i], d.pairs[i].name)
            assert pu[first[k]:first[k + 1]].tobytes() == res[k][0].tobytes() and pd[first[k]:first[k + 1]].tobytes() == res[k][1].tobytes()
            got, nm1 = _single(d, one, i)
            assert got[0].tobytes() == res[k][0].tobytes() and got[1].tobytes() == res[k][1].tobytes() and nm1 == nm[k]
            if len(d.pairs[i].kl) == 0 or len(d.pairs[i].kr) == 0:
                seen_empty += 1
                assert nm[k] == 0 and np.all(res[k][0] == -1) and len(res[k][0]) == len(d.pairs[i].kl)
                assert len(idx) > 1
    assert seen_empty == 3
    m.close(); one.close()


def test_reused_handle_leaks_nothing(ctx, designed):
    """A large batch, then a smaller one, then from_orb after from_keys, then from_keys again: no stale best, SAD or level-table entry may show.  Each against a
    fresh handle (the restatement, for the designed pairs)."""
    d = designed
    m = StereoMatcher(max(d.extL.cap, d.extR.cap), len(d.pairs), ctx=ctx)  # room for what the extractors themselves found
    runs = _runs_of_equal_calibration(d.pairs)
    big = max(runs, key=len)
    res, nm = _call(d, m, big)
    for k, i in enumerate(big):
        _same(res[k], nm[k], d.want[i], d.pairs[i].name)
    # smaller: pairs with fewer key points and other level tables land where the large batch's first pairs were
    for name in ("levels_only7", "cut_n1", "levels_ends", "cut_all_rejected", "empty_left"):
        i = d.index[name]
        got, nm1 = _single(d, m, i)
        _same(got, nm1, d.want[i], name)
    # from_orb on the same handle against a fresh one
    m.match(d.extL, d.extR, sr.BF, sr.BF / sr.FX)
    after, nm_after = m.read()
    fresh = StereoMatcher(max(d.extL.cap, d.extR.cap), len(d.pairs), ctx=ctx)
    fresh.match(d.extL, d.extR, sr.BF, sr.BF / sr.FX)
    clean, nm_clean = fresh.read()
    assert np.array_equal(nm_after, nm_clean)
    for a, b in zip(after, clean):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # ... and from_keys once more
    res, nm = _call(d, m, big)
    for k, i in enumerate(big):
        _same(res[k], nm[k], d.want[i], d.pairs[i].name)
    m.close(); fresh.close()


def test_from_keys_equals_from_orb(ctx):
    """cs_stereo_match_from_keys fed with what cs_orb_read returned for a 640 x 480 pair equals cs_stereo_match_from_orb on the same run."""
    left, right, _ = sr.pair(1, 640, 480, sr.FIXED_BANDS)
    extL = ORBextractor(1000, 1.2, 8, 20, 7, 640, 480, ctx=ctx)
    extR = ORBextractor(1000, 1.2, 8, 20, 7, 640, 480, ctx=ctx)
    extL.upload(left); extL.run()
    extR.upload(right); extR.run()
    (kl, dl), = extL.read()
    (kr, dr), = extR.read()
    b = sr.BF / sr.FX
    m = StereoMatcher(max(extL.cap, extR.cap), 1, ctx=ctx)
    m.match(extL, extR, sr.BF, b)
    (orb,), nm_orb = m.read()
    m.match_keys(extL, extR, [kl], [dl], [kr], [dr], sr.BF, b)
    (keys,), nm_keys = m.read()
    assert len(kl) > 900 and nm_orb[0] >= 0.40 * len(kl) and nm_keys[0] == nm_orb[0]
    assert keys[0].tobytes() == orb[0].tobytes() and keys[1].tobytes() == orb[1].tobytes()
    m.close(); extL.close(); extR.close()


def test_error_codes(ctx, designed):
    """Every refusal of cs_stereo_match_from_keys; after each the handle still reads the previous result, and it then answers a good call."""
    d = designed
    lib = _lib.lib()
    i = d.index["cut_512"]
    p = d.pairs[i]
    m = StereoMatcher(len(p.kl), 2, ctx=ctx)  # exactly the pair's count: one more key point is over the capacity
    before = _single(d, m, i)
    _same(before[0], before[1], d.want[i])
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    pb = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))
    pk = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(fL, kl, dl, fR, kr, dr, n_pairs=1, left=d.extL, right=d.extR, lf=i, rf=i, bf=p.bf, b=p.b):
        fL, fR = np.asarray(fL, np.int32), np.asarray(fR, np.int32)
        r = lib.cs_stereo_match_from_keys(ctx.ptr, m._s, left._e, lf, right._e, rf, n_pairs, pi(fL), pk(kl), pb(dl), pi(fR), pk(kr), pb(dr), C.c_float(bf), C.c_float(b))
        if r != 0:  # a refused call leaves the previous result readable
            (got,), nm = m.read()
            assert got[0].tobytes() == before[0][0].tobytes() and got[1].tobytes() == before[0][1].tobytes() and nm[0] == before[1]
        return r, lib.cs_last_error(ctx.ptr).decode()

    kl, dl, kr, dr = np.ascontiguousarray(p.kl), np.ascontiguousarray(p.dl), np.ascontiguousarray(p.kr), np.ascontiguousarray(p.dr)
    nl, nr = len(kl), len(kr)
    assert call([0, nl], kl, dl, [0, nr], kr, dr)[0] == 0
    # NULL arrays
    assert call([0, nl], None, dl, [0, nr], kr, dr)[0] == BAD_ARG and call([0, nl], kl, None, [0, nr], kr, dr)[0] == BAD_ARG
    assert call([0, nl], kl, dl, [0, nr], None, dr)[0] == BAD_ARG and call([0, nl], kl, dl, [0, nr], kr, None)[0] == BAD_ARG
    assert lib.cs_stereo_match_from_keys(ctx.ptr, m._s, d.extL._e, i, d.extR._e, i, 1, None, pk(kl), pb(dl), pi(np.array([0, nr], np.int32)), pk(kr), pb(dr), C.c_float(p.bf),
                                         C.c_float(p.b)) == BAD_ARG
    assert lib.cs_stereo_match_from_keys(ctx.ptr, m._s, None, i, d.extR._e, i, 1, pi(np.array([0, nl], np.int32)), pk(kl), pb(dl), pi(np.array([0, nr], np.int32)), pk(kr), pb(dr),
                                         C.c_float(p.bf), C.c_float(p.b)) == BAD_ARG
    # first not non-decreasing from 0
    assert call([1, nl], kl, dl, [0, nr], kr, dr)[0] == BAD_ARG and call([0, nl], kl, dl, [1, nr], kr, dr)[0] == BAD_ARG
    assert call([0, 5, 3], kl, dl, [0, 2, 4], kr, dr, n_pairs=2, lf=0, rf=0)[0] == BAD_ARG and call([0, 2, 4], kl, dl, [0, 5, 3], kr, dr, n_pairs=2, lf=0, rf=0)[0] == BAD_ARG
    # a right frame whose octaves decrease, with a message
    bad = kr.copy(); bad["octave"][0] = 1
    r, msg = call([0, nl], kl, dl, [0, nr], bad, dr)
    assert r == BAD_ARG and "level-major" in msg
    bad = kr.copy(); bad["octave"][-1] = -1  # ... at the last key point, and below the first level
    r, msg = call([0, nl], kl, dl, [0, nr], bad, dr)
    assert r == BAD_ARG and "level-major" in msg
    up = kr.copy(); up["octave"][-1] = 3  # increasing octaves are in order
    assert call([0, nl], kl, dl, [0, nr], up, dr)[0] == 0
    assert call([0, nl], kl, dl, [0, nr], kr, dr)[0] == 0
    # coordinates
    for field, v in (("x", np.inf), ("y", np.nan), ("x", -3.0e7)):
        bad = kl.copy(); bad[field][2] = v
        r, msg = call([0, nl], bad, dl, [0, nr], kr, dr)
        assert r == BAD_ARG and "coordinate" in msg
    # capacity: left, then right
    more_k, more_d = np.concatenate([kl, kl[:1]]), np.concatenate([dl, dl[:1]])
    r, msg = call([0, nl + 1], more_k, more_d, [0, nr], kr, dr)
    assert r == CAPACITY and "more key points" in msg
    assert call([0, nl], kl, dl, [0, nl + 1], more_k, more_d)[0] == CAPACITY
    # geometry and ranges, as for cs_stereo_match_from_orb
    assert call([0, nl], kl, dl, [0, nr], kr, dr, lf=len(d.pairs))[0] == BAD_ARG and call([0, nl], kl, dl, [0, nr], kr, dr, rf=len(d.pairs))[0] == BAD_ARG
    assert call([0, nl, nl, nl], kl, dl, [0, nr, nr, nr], kr, dr, n_pairs=3, lf=0, rf=0)[0] == BAD_ARG  # above max_pairs
    assert call([0, nl], kl, dl, [0, nr], kr, dr, n_pairs=0)[0] == BAD_ARG
    assert call([0, nl], kl, dl, [0, nr], kr, dr, bf=0.0)[0] == BAD_ARG and call([0, nl], kl, dl, [0, nr], kr, dr, b=-1.0)[0] == BAD_ARG
    fresh = ORBextractor(500, sp.SCALE, sp.NLEVELS, 20, 7, sp.W, sp.H, ctx=ctx)  # no run yet
    assert call([0, nl], kl, dl, [0, nr], kr, dr, left=fresh, lf=0)[0] == BAD_ARG
    other = ORBextractor(500, sp.SCALE, sp.NLEVELS, 20, 7, sp.W + 64, sp.H, ctx=ctx)
    other.upload(np.zeros((sp.H, sp.W + 64), np.uint8)); other.run()
    r, msg = call([0, nl], kl, dl, [0, nr], kr, dr, right=other, rf=0)
    assert r == BAD_ARG and "cs_stereo_match_from_keys" in msg
    fresh.close(); other.close()
    # the Python wrapper raises
    with pytest.raises(_lib.CubeSlamError):
        bad = p.kr.copy(); bad["octave"][0] = 1
        m.match_keys(d.extL, d.extR, [p.kl], [p.dl], [bad], [p.dr], p.bf, p.b, left_first=i, right_first=i)
    with pytest.raises(ValueError):
        m.match_keys(d.extL, d.extR, [p.kl], [p.dl[:-1]], [p.kr], [p.dr], p.bf, p.b)
    # ... and the handle answers a good call: two pairs, the device pointers
    j = d.index["cut_255"]
    assert j == i + 1 and len(d.pairs[j].kl) <= len(p.kl)
    res, nm = _call(d, m, [i, j])
    _same(res[0], nm[0], d.want[i]); _same(res[1], nm[1], d.want[j])
    u, dd, n = m.device_pair(1)
    assert n == len(d.pairs[j].kl) and u and dd
    m.close()
