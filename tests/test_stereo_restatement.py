"""CPU tests that hold the stereo checker (tests/stereo_restatement.py, a restatement of Frame::ComputeStereoMatches, Frame.cc:611-783) to ground truth on
synthetic rectified pairs of known disparity, so that "the device equals the checker" (tests/test_stereo_gpu.py) means something; and the part of the
cs_stereo_* C-ABI that needs no device.

Floors (40 % matched, median disparity error 0.5 px) lie under what the checker gives on the CPU oracle's key points: 48.0 - 50.7 % and 0.246 - 0.262 px."""
import ctypes as C

import numpy as np
import pytest

from tests import stereo_restatement as sr

f32 = np.float32
B = sr.BF / sr.FX


def _run(oracle, left, right, nfeat, bf=sr.BF, b=B):
    eL, eR = oracle.ORBextractor(nfeat, 1.2, 8, 20, 7), oracle.ORBextractor(nfeat, 1.2, 8, 20, 7)
    kl, dl = eL(left)
    kr, dr = eR(right)
    sf, isf = sr.scale_tables(1.2, 8)
    st = {}
    uR, dep, kept = sr.compute_stereo_matches(kl, dl, kr, dr, [eL.level(i) for i in range(8)], [eR.level(i) for i in range(8)], sf, isf, bf, b, stats=st)
    return kl, kr, uR, dep, kept, st


@pytest.mark.parametrize("W,H,nfeat", [(1241, 376, 2000), (640, 480, 1000)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recovers_known_disparities(oracle, W, H, nfeat, seed):
    left, right, truth = sr.pair(seed, W, H, sr.FIXED_BANDS)
    kl, kr, uR, dep, kept, st = _run(oracle, left, right, nfeat)
    err = sr.disparity_error(kl, uR, truth)
    print("N %d Nr %d %s matched %.1f %% median error %.3f px p95 %.3f" % (len(kl), len(kr), st, 100.0 * kept / len(kl), np.median(err), np.percentile(err, 95)))
    assert kept == int((uR >= 0).sum()) == int((dep > 0).sum())
    assert kept >= 0.40 * len(kl)
    assert np.median(err) <= 0.5
    m = uR >= 0
    assert np.all(uR[~m] == -1) and np.all(dep[~m] == -1)
    m &= dep != f32(f32(sr.BF) / f32(0.01))  # not the clamp, whose u_right is uL - 0.01 in double
    assert np.array_equal(dep[m], (f32(sr.BF) / (kl["x"][m] - uR[m])).astype(f32))  # mvDepth = mbf / disparity


def test_identical_images_are_cut_to_nothing(oracle):
    left = sr.pair(1, 640, 480, [0.0], noise=0.0)[0]
    kl, kr, uR, dep, kept, st = _run(oracle, left, left, 1000)
    assert st["accepted"] > 100  # matches are found ...
    assert kept == 0 and np.all(uR == -1) and np.all(dep == -1)  # ... and the median SAD of 0 removes every one (thDist = 0, SAD >= 0)


def test_empty_sides(oracle):
    left = sr.pair(1, 640, 480, [5.0])[0]
    flat = np.full_like(left, 90)
    kl, kr, uR, dep, kept, st = _run(oracle, left, flat, 1000)
    assert len(kr) == 0 and len(uR) == len(kl) > 0 and kept == 0 and np.all(uR == -1) and np.all(dep == -1)
    kl, kr, uR, dep, kept, st = _run(oracle, flat, left, 1000)
    assert len(kl) == 0 and len(uR) == 0 and len(dep) == 0 and kept == 0


def test_zero_disparity_reaches_the_clamp(oracle):
    """Disparity 0 with noise, 640 x 480, seeds 1-24: `disparity <= 0` (Frame.cc:757-761) needs deltaR == 0 (dist1 == dist3), bestincR == 0 and a level whose
    scale reproduces uL exactly.  Measured with this generator: 5 key points in 4 of the 24 pairs (seeds 4, 9, 18, 20), so the clamp is asserted over the
    set, not per pair."""
    reached, seen = 0, 0
    for seed in range(1, 25):
        left, right, truth = sr.pair(seed, 640, 480, [0.0])
        kl, kr, uR, dep, kept, st = _run(oracle, left, right, 1000)
        clamped = dep == f32(f32(sr.BF) / f32(0.01))
        print(seed, st, int(clamped.sum()))
        assert int(clamped.sum()) <= st["clamp"]  # the cut may remove some of them
        assert np.array_equal(uR[clamped], (kl["x"][clamped].astype(np.float64) - 0.01).astype(f32))
        reached += st["clamp"]
        seen += int(clamped.sum())
    assert reached >= 1 and seen >= 1


def test_negative_disparities_are_rejected(oracle):
    left, right, truth = sr.pair(1, 640, 480, [-2.0, -1.0, 0.0, 0.5])
    kl, kr, uR, dep, kept, st = _run(oracle, left, right, 1000)
    print(st)
    assert st["disparity"] > 100  # disparity < 0 (Frame.cc:755)
    m = uR >= 0
    assert np.all(kl["x"][m] - uR[m] > 0)


# ---- the C-ABI without a device


def test_version_is_108():
    from cube_slam_amd import _lib
    assert _lib.lib().cs_version() == 108 == _lib.header_version()


def test_stereo_symbols_exported():
    from cube_slam_amd import _lib
    lib = _lib.lib()
    for name in ("cs_stereo_create", "cs_stereo_destroy", "cs_stereo_match_from_orb", "cs_stereo_match_from_keys", "cs_stereo_read", "cs_stereo_read_packed",
                 "cs_stereo_device_pair"):
        assert hasattr(lib, name), name


def test_bad_arguments_without_a_handle():
    from cube_slam_amd import _lib
    lib = _lib.lib()
    BAD = -2  # CS_ERR_BAD_ARG
    out = C.c_void_p()
    fake = C.c_void_p(1)  # never dereferenced: the NULL argument is found first
    assert lib.cs_stereo_create(None, 2000, 1, C.byref(out)) == BAD and not out.value  # NULL context
    assert lib.cs_stereo_create(fake, 2000, 1, None) == BAD  # NULL out-pointer
    assert lib.cs_stereo_match_from_orb(None, None, None, 0, None, 0, 1, C.c_float(sr.BF), C.c_float(B)) == BAD
    assert lib.cs_stereo_match_from_orb(fake, None, fake, 0, fake, 0, 1, C.c_float(sr.BF), C.c_float(B)) == BAD  # NULL handle
    first = np.zeros(2, np.int32)
    key, dsc = np.zeros(28, np.uint8), np.zeros(32, np.uint8)
    pfirst, keys, desc = first.ctypes.data_as(C.POINTER(C.c_int)), C.c_void_p(key.ctypes.data), dsc.ctypes.data_as(C.POINTER(C.c_uint8))
    from_keys = lambda ctx, s, l, r: lib.cs_stereo_match_from_keys(ctx, s, l, 0, r, 0, 1, pfirst, keys, desc, pfirst, keys, desc, C.c_float(sr.BF), C.c_float(B))
    assert from_keys(None, None, None, None) == BAD
    assert from_keys(fake, None, fake, fake) == BAD  # NULL handle
    buf = np.zeros(4, np.float32)
    cnt = np.zeros(4, np.int32)
    pf, pi = buf.ctypes.data_as(C.POINTER(C.c_float)), cnt.ctypes.data_as(C.POINTER(C.c_int))
    total = C.c_long()
    assert lib.cs_stereo_read(None, None, pf, pf, 4, pi, pi) == BAD
    assert lib.cs_stereo_read(fake, None, pf, pf, 4, pi, pi) == BAD
    assert lib.cs_stereo_read_packed(None, None, pf, pf, C.c_long(4), pi, C.byref(total), pi) == BAD
    assert lib.cs_stereo_read_packed(fake, None, pf, pf, C.c_long(4), pi, C.byref(total), pi) == BAD
    u, d, n = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_int()
    assert lib.cs_stereo_device_pair(None, 0, C.byref(u), C.byref(d), C.byref(n)) == BAD
    lib.cs_stereo_destroy(None, None)  # a no-op, like its neighbours


def test_python_mirror_is_exported():
    import cube_slam_amd
    assert callable(cube_slam_amd.ComputeStereoMatches) and callable(cube_slam_amd.StereoMatcher)
