"""The stated definitions of cv::SVDecomp on CV_32F and of Mat::inv() (cube_slam_amd/csrc/initializer_math.h over cv_svd_math.h: a one-sided Hestenes Jacobi with float
storage; the closed-form inverse) against numpy.linalg in float64 (LAPACK, the only independent SVD here), on the matrices the patterns of tests/initializer_patterns.py
actually hand them: the 16 x 9 of ComputeH21 and the 8 x 9 of ComputeF21 of every hypothesis, the 3 x 3 Fpre of every hypothesis and the 3 x 3 that ReconstructH /
ReconstructF decompose, and the inverses of T2, H21i and K.

The distances are measured, not chosen: every maximum over the patterns is a named constant D_* (the measured value rounded up) and 4 D is asserted.  The patterns are seeded,
so the margin covers only another LAPACK build.  Singular values and vectors are relative to the largest singular value; a last right vector is compared up to sign, and for
the 8 x 9 -- whose vt.row(8) is no Jacobi row but the completion of the other rows' span -- it is asked to lie in LAPACK's null space."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import initializer_patterns as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, DP = C.POINTER(C.c_float), C.POINTER(C.c_double)
F32 = np.float32

# measured with this file (measure()): the largest value over all matrices of the patterns -- in the comments -- rounded up
D_SV_16x9 = 2.7e-7  # 2.60e-07  |W - s| / s_max
D_ORTHO_16x9 = 8e-7  # 7.81e-07  max |Vt Vt^T - I|
D_VLAST_16x9 = 7.5e-8  # 7.22e-08  vt.row(8) against LAPACK's up to sign, times (s_7 - s_8) / s_max: the distance a perturbation of float size leaves at that gap
D_SV_8x9 = 2.5e-7  # 2.42e-07
D_ORTHO_8x9 = 2.6e-7  # 2.55e-07  the 8 unit rows and the completion
D_NULL_8x9 = 3.2e-8  # 3.17e-08  |(I - n n^T) vt.row(8)|, n = LAPACK's null vector, times s_7 / s_max (as above)
D_SV_3x3 = 2.6e-7  # 2.58e-07
D_ORTHO_3x3 = 3.8e-7  # 3.71e-07  U and Vt
D_RECON_3x3 = 3.5e-7  # 3.47e-07  max |A - U diag(w) Vt| / s_max
D_INV = 5.8e-8  # 5.72e-08  max |Ainv - inv| / max |inv|
D_VLAST_16x9_WELL = 5.3e-7  # 5.29e-07  the same vector distance unscaled, over the matrices whose last gap is above WELL of the largest value
D_NULL_8x9_WELL = 9.7e-6    # 9.67e-06  the same null-space distance unscaled, over the matrices with s_7 above WELL of the largest value
WELL = 1e-3
TOL = 4.0
NAMES = [n for n in P.ALL if len(P.case(n)["sets"])]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("initializer_svd")), "libinitializer_svd_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-shared", "-I", ROOT, "-o", so, os.path.join(ROOT, "tests", "cpp", "initializer_svd_probe.cpp")])
    lb = C.CDLL(so)
    lb.probe_det3.restype = C.c_double
    return lb


def _f(a):
    return a.ctypes.data_as(FP)


def _ortho(M):
    M = M.astype(np.float64)
    return np.abs(M @ M.T - np.eye(len(M))).max()


def measure(lib):
    d = dict.fromkeys(("sv16", "ortho16", "vlast16", "vlast16_abs", "sv8", "ortho8", "null8", "null8_abs", "sv3", "ortho3", "recon3", "inv"), 0.0)
    well = {"vlast16_abs": 0, "null8_abs": 0}

    def upd(k, v):
        assert np.isfinite(v), k
        d[k] = max(d[k], float(v))

    def svd3(A):
        U, w, Vt = np.zeros(9, F32), np.zeros(3, F32), np.zeros(9, F32)
        lib.probe_svd3(_f(np.ascontiguousarray(A, F32)), _f(U), _f(w), _f(Vt))
        A64 = np.asarray(A, np.float64).reshape(3, 3)
        s = np.linalg.svd(A64, compute_uv=False)
        upd("sv3", np.abs(w - s).max() / s[0])
        upd("ortho3", max(_ortho(U.reshape(3, 3)), _ortho(Vt.reshape(3, 3))))
        upd("recon3", np.abs(A64 - U.reshape(3, 3).astype(np.float64) @ np.diag(w.astype(np.float64)) @ Vt.reshape(3, 3)).max() / s[0])
        assert (np.diff(w) <= 0).all()

    def inv3(A):
        Ai = np.zeros(9, F32)
        lib.probe_inv3(_f(np.ascontiguousarray(A, F32).reshape(-1)), _f(Ai))
        ref = np.linalg.inv(np.asarray(A, np.float64).reshape(3, 3))
        upd("inv", np.abs(Ai.reshape(3, 3) - ref).max() / np.abs(ref).max())

    for name in NAMES:
        c, j = P.case(name), P.judged(name)
        pn1, pn2, T1, T2 = np.zeros_like(c["keys1"]), np.zeros_like(c["keys2"]), np.zeros(9, F32), np.zeros(9, F32)
        lib.probe_normalize(_f(c["keys1"]), len(c["keys1"]), _f(pn1), _f(T1))
        lib.probe_normalize(_f(c["keys2"]), len(c["keys2"]), _f(pn2), _f(T2))
        inv3(T2); inv3(c["K"])
        for h, s8 in enumerate(c["sets"]):
            p1 = np.ascontiguousarray(pn1[c["matches"][s8, 0]]); p2 = np.ascontiguousarray(pn2[c["matches"][s8, 1]])
            A, W, Vt = np.zeros((16, 9), F32), np.zeros(9), np.zeros((9, 9), F32)
            lib.probe_h21(_f(p1), _f(p2), _f(A), W.ctypes.data_as(DP), _f(Vt))
            _, s, vt = np.linalg.svd(A.astype(np.float64))
            upd("sv16", np.abs(W - s).max() / s[0])
            upd("ortho16", _ortho(Vt))
            v = Vt[8].astype(np.float64)
            upd("vlast16", min(np.abs(v - vt[8]).max(), np.abs(v + vt[8]).max()) * (s[7] - s[8]) / s[0])
            if (s[7] - s[8]) > WELL * s[0]:  # a well separated last value: the vector itself, no scaling
                upd("vlast16_abs", min(np.abs(v - vt[8]).max(), np.abs(v + vt[8]).max())); well["vlast16_abs"] += 1
            A8, W8, vt9, U3, w3, Vt3, Fn = np.zeros((8, 9), F32), np.zeros(8), np.zeros((9, 9), F32), np.zeros(9, F32), np.zeros(3, F32), np.zeros(9, F32), np.zeros(9, F32)
            lib.probe_f21(_f(p1), _f(p2), _f(A8), W8.ctypes.data_as(DP), _f(vt9), _f(U3), _f(w3), _f(Vt3), _f(Fn))
            _, s, vt = np.linalg.svd(A8.astype(np.float64))
            upd("sv8", np.abs(W8 - s).max() / s[0])
            upd("ortho8", _ortho(vt9))
            r = vt9[8].astype(np.float64)
            if s[7] > 1e-6 * s[0]:  # the 8 rows are independent: the null space is a line
                upd("null8", np.linalg.norm(r - (r @ vt[8]) * vt[8]) * s[7] / s[0])
                if s[7] > WELL * s[0]:
                    upd("null8_abs", np.linalg.norm(r - (r @ vt[8]) * vt[8])); well["null8_abs"] += 1
            else:  # a noise-free rotation: the rows have rank 6 and the null space is no line; what holds is ortho8
                assert name == "plane_d1d2"
            svd3(vt9[8])
            Hm, Fm = j["matrix"][0, h], j["matrix"][1, h]
            assert Fn.tobytes() != b"" and np.isfinite(Fn).all()
            inv3(Hm)
            for model, M in ((0, Hm), (1, Fm)):
                A3 = np.zeros(9, F32)
                lib.probe_recon_matrix(model, _f(np.ascontiguousarray(M)), _f(np.ascontiguousarray(c["K"]).reshape(-1)), _f(A3))
                svd3(A3)
    assert min(well.values()) >= 20, well  # the unscaled bounds are held on enough matrices
    return d


def test_float_svd_and_inverse_against_lapack(lib):
    d = measure(lib)
    print("measured:", {k: "%.3g" % v for k, v in d.items()})
    for k, D in (("sv16", D_SV_16x9), ("ortho16", D_ORTHO_16x9), ("vlast16", D_VLAST_16x9), ("vlast16_abs", D_VLAST_16x9_WELL), ("null8_abs", D_NULL_8x9_WELL), ("sv8", D_SV_8x9), ("ortho8", D_ORTHO_8x9), ("null8", D_NULL_8x9),
                 ("sv3", D_SV_3x3), ("ortho3", D_ORTHO_3x3), ("recon3", D_RECON_3x3), ("inv", D_INV)):
        assert d[k] <= TOL * D, (k, d[k], D)


def _completion_attempt(rows, signs):
    """One attempt of the 8 x 9 completion in numpy float32, as csrc/initializer_math.h states it -> the row before its normalisation."""
    row = (np.array(signs, F32) * F32(1.0 / 9)).astype(F32)
    for _ in range(2):
        for j in range(8):
            pd = np.float64(0)
            for k in range(9):
                pd += np.float64(F32(row[k] * rows[j, k]))
            row = (row.astype(np.float64) - pd * rows[j].astype(np.float64)).astype(F32)
            asum = F32(0)
            for k in range(9):
                asum = F32(asum + abs(row[k]))
            row = (row * (F32(1) / asum if asum > F32(2.384185791015625e-07) * F32(100) else F32(0))).astype(F32)
    return row


def _draws(n):
    state, out = 0x12345678, []
    for _ in range(n):
        state = ((state & 0xFFFFFFFF) * 4294883355 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
        out.append(1.0 if (state & 0xFFFFFFFF) & 256 else -1.0)
    return out


def test_completion_draws_again_where_the_first_start_vector_fails(lib):
    """Pattern `redraw`, set 0: the first nine draws give a start vector that the projections wipe out (its remainder's L1 norm falls below 200 FLT_EPSILON), the next nine
    do not, and the library's vt.row(8) is the second attempt's row, normalised -- bit for bit."""
    c = P.case("redraw")
    pn1, pn2, T = np.zeros_like(c["keys1"]), np.zeros_like(c["keys2"]), np.zeros(9, F32)
    lib.probe_normalize(_f(c["keys1"]), len(c["keys1"]), _f(pn1), _f(T))
    lib.probe_normalize(_f(c["keys2"]), len(c["keys2"]), _f(pn2), _f(T))
    s8 = c["sets"][0]
    p1 = np.ascontiguousarray(pn1[c["matches"][s8, 0]]); p2 = np.ascontiguousarray(pn2[c["matches"][s8, 1]])
    A8, W8, vt9, U3, w3, Vt3, Fn = np.zeros((8, 9), F32), np.zeros(8), np.zeros((9, 9), F32), np.zeros(9, F32), np.zeros(3, F32), np.zeros(9, F32), np.zeros(9, F32)
    lib.probe_f21(_f(p1), _f(p2), _f(A8), W8.ctypes.data_as(DP), _f(vt9), _f(U3), _f(w3), _f(Vt3), _f(Fn))
    d = _draws(18)
    first, second = _completion_attempt(vt9[:8], d[:9]), _completion_attempt(vt9[:8], d[9:])
    assert not first.any() and second.any()
    n = np.sqrt((second.astype(np.float64) ** 2).sum())
    assert (second * F32(1 / n)).astype(F32).tobytes() == vt9[8].tobytes()
    assert np.abs(Fn).max() > 0 and P.judged("redraw")["score"][1, 0] > 1000  # and the hypothesis is a good one: most matches are its inliers


def test_completion_start_vector_and_sign_dependence(lib):
    """The start vector of the 8 x 9 completion is the stated generator's: +-1/9 with the signs of its first nine draws; and the determinant is the closed form."""
    state, signs = 0x12345678, []
    for _ in range(9):
        state = ((state & 0xFFFFFFFF) * 4294883355 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
        signs.append(1.0 if (state & 0xFFFFFFFF) & 256 else -1.0)
    assert len(set(signs)) == 2  # (a vector of one sign would be the mean direction)
    A = np.array([[2, 0, 1], [1, 3, 0], [0, 1, 4]], F32)
    assert lib.probe_det3(_f(A)) == np.linalg.det(A.astype(np.float64)).round(9) == 25.0
    Z = np.zeros(9, F32); out = np.ones(9, F32)
    lib.probe_inv3(_f(Z), _f(out))
    assert (out == 0).all()  # a zero determinant gives the zero matrix
