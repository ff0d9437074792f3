"""Judge of the batched Sim3 refinement (cs_sim3_optimization): a statement-by-statement float64 restatement of ORB_SLAM2::Optimizer::OptimizeSim3 (reference
orb_object_slam/src/Optimizer.cc:2838-3033) over flat arrays, and the seeded generator of the problems the tests run.  A helper, not a test module.

What is restated, each in the association the reference's text gives it:
  * g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h): the exponential with its four branches, the product, the inverse and map; the quaternion is never renormalised.
    Quaterniond(Matrix3d), quaternion * quaternion and quaternion * vector are Eigen's generic code (RotationBase / Quaternion.h).
  * EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError with VertexSim3Expmap::cam_map1 / cam_map2 and project (types_seven_dof_expmap.h, se3_ops.hpp).
  * BaseBinaryEdge::linearizeOplusXj (core/base_binary_edge.hpp:269-320): central differences, delta = 1e-9, through VertexSim3Expmap::oplusImpl (which zeroes update[6]
    under _fix_scale), and constructQuadraticForm's robust branch (:91-113) with RobustKernelHuber (core/robust_kernel_impl.cpp:65-91; its dsqr member is a float).
  * BlockSolverX over LinearSolverDense (solvers/linear_solver_dense.h): one 7 x 7 block, L D L^T reading the lower triangle, no pivoting (for these positive definite
    systems Eigen's pivoted form differs by rounding only), success where every D is positive.
  * OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:61-164) under SparseOptimizer::optimize (core/sparse_optimizer.cpp:354-419).
Sums over edges (H, b, the robust chi2) run in the optimizer's edge order: e12 of correspondence 0, e21 of 0, e12 of 1, ...  Per-edge work is elementwise numpy float64,
the 7-dof state is Python floats; exp / sin / cos / pow are libm's through `math`."""
import ctypes as C
import glob
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"

DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
EPS = 0.00001
DBL_MAX = float(np.finfo(np.float64).max)

# D_REF: the largest change of the reference's own eight output numbers, relative to max(1, |value|), when only the order of its correspondences is reversed, over all CASES
# (measured by tests/test_sim3_opt_restatement_pins.py::test_reference_order_sensitivity, which asserts that this constant is what it measures: 4.807e-07, from the case
# "stride_p1"; the other cases lie between 1e-09 and 2e-08).  With delta = 1e-9 Jacobians a last-bit change of a sum moves the next iterate by far more than a bit.
D_REF = 4.807275137963529e-07
# restatement vs reference and device vs restatement: 10 x D_REF (the device's strided partials and shuffle tree are a third summation order over up to 15 LM iterations)
TOL = 10 * D_REF


# ---------------------------------------------------------------------------------------------------------------------------------- g2o::Sim3
def _mat3_mul(a, b):
    r = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            s = a[i][0] * b[0][j]
            s += a[i][1] * b[1][j]
            s += a[i][2] * b[2][j]
            r[i][j] = s
    return r


def _skew(v):  # se3_ops.hpp:27-38
    return [[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]]


def quat_from_matrix(m):
    """Eigen's quaternionbase_assign_impl<Matrix3d>: (x, y, z, w)."""
    q = [0.0] * 4
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return tuple(q)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz)


def quat_rot(q, v):
    """QuaternionBase::_transformVector; v's components may be arrays."""
    x, y, z, w = q
    v0, v1, v2 = v
    uv0 = y * v2 - z * v1
    uv1 = z * v0 - x * v2
    uv2 = x * v1 - y * v0
    uv0 = uv0 + uv0
    uv1 = uv1 + uv1
    uv2 = uv2 + uv2
    return (v0 + w * uv0 + (y * uv2 - z * uv1), v1 + w * uv1 + (z * uv0 - x * uv2), v2 + w * uv2 + (x * uv1 - y * uv0))


def sim3_exp(u):
    """Sim3(const Vector7d &update) (sim3.h:70-142) -> (q, t, s)."""
    omega = [u[0], u[1], u[2]]
    upsilon = [u[3], u[4], u[5]]
    sigma = u[6]
    theta = math.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    Om = _skew(omega)
    s = math.exp(sigma)
    Om2 = _mat3_mul(Om, Om)
    I = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]

    def rodrigues():
        a = math.sin(theta) / theta
        b = (1 - math.cos(theta)) / (theta * theta)
        return [[I[i][j] + a * Om[i][j] + b * Om2[i][j] for j in range(3)] for i in range(3)]

    def small():
        return [[I[i][j] + Om[i][j] + Om2[i][j] for j in range(3)] for i in range(3)]

    if math.fabs(sigma) < EPS:
        C = 1.0
        if theta < EPS:
            A = 1. / 2.
            B = 1. / 6.
            R = small()
        else:
            theta2 = theta * theta
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
            R = rodrigues()
    else:
        C = (s - 1) / sigma
        if theta < EPS:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = small()
        else:
            R = rodrigues()
            a = s * math.sin(theta)
            b = s * math.cos(theta)
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    q = quat_from_matrix(R)
    W = [[A * Om[i][j] + B * Om2[i][j] + C * I[i][j] for j in range(3)] for i in range(3)]
    t = []
    for i in range(3):
        acc = W[i][0] * upsilon[0]
        acc += W[i][1] * upsilon[1]
        acc += W[i][2] * upsilon[2]
        t.append(acc)
    return (q, tuple(t), s)


def sim3_map(S, p):
    q, t, s = S
    r = quat_rot(q, p)
    return (s * r[0] + t[0], s * r[1] + t[1], s * r[2] + t[2])


def sim3_inverse(S):
    q, t, s = S
    qc = (-q[0], -q[1], -q[2], q[3])
    k = -1. / s
    return (qc, quat_rot(qc, (k * t[0], k * t[1], k * t[2])), 1. / s)


def sim3_mul(a, b):
    qa, ta, sa = a
    r = quat_rot(qa, b[1])
    return (quat_mul(qa, b[0]), (sa * r[0] + ta[0], sa * r[1] + ta[1], sa * r[2] + ta[2]), sa * b[2])


def sim3_from8(v):
    """tx ty tz qx qy qz qw s -> (q, t, s), Python floats."""
    v = [float(x) for x in v]
    return ((v[3], v[4], v[5], v[6]), (v[0], v[1], v[2]), v[7])


def sim3_to8(S):
    q, t, s = S
    return np.array([t[0], t[1], t[2], q[0], q[1], q[2], q[3], s], np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------- the graph
class _Problem:
    def __init__(self, c):
        f = lambda a, k: np.ascontiguousarray(a, np.float64).reshape(-1, k)
        self.P1, self.P2, self.o1, self.o2 = f(c["P1c"], 3), f(c["P2c"], 3), f(c["obs1"], 2), f(c["obs2"], 2)
        self.w1, self.w2 = np.ascontiguousarray(c["inv_sigma2_1"], np.float64), np.ascontiguousarray(c["inv_sigma2_2"], np.float64)
        self.K = [float(x) for x in c["intrinsics"]]
        self.fix = bool(c["fix_scale"])
        self.th2 = float(np.float32(c["th2"]))
        self.delta = float(np.float32(np.sqrt(np.float32(c["th2"]))))  # const float deltaHuber = sqrt(th2)
        self.dsqr = float(np.float32(self.delta * self.delta))  # RobustKernelHuber::dsqr is a float
        self.n = len(self.w1)

    def errors(self, S, Sinv, idx):
        """computeError of both edges of the correspondences idx at the estimate S (Sinv = S.inverse()): (n, 4) = e12 x, y, e21 x, y."""
        fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = self.K
        P1, P2 = self.P1[idx], self.P2[idx]
        with np.errstate(all="ignore"):
            a = sim3_map(S, (P2[:, 0], P2[:, 1], P2[:, 2]))
            b = sim3_map(Sinv, (P1[:, 0], P1[:, 1], P1[:, 2]))
            return np.stack([self.o1[idx, 0] - (a[0] / a[2] * fx1 + cx1), self.o1[idx, 1] - (a[1] / a[2] * fy1 + cy1),
                             self.o2[idx, 0] - (b[0] / b[2] * fx2 + cx2), self.o2[idx, 1] - (b[1] / b[2] * fy2 + cy2)], axis=1)

    def chi2(self, E, idx):
        """BaseEdge::chi2 = _error.dot(information() * _error) of e12 and of e21."""
        w1, w2 = self.w1[idx], self.w2[idx]
        return E[:, 0] * (w1 * E[:, 0]) + E[:, 1] * (w1 * E[:, 1]), E[:, 2] * (w2 * E[:, 2]) + E[:, 3] * (w2 * E[:, 3])

    def robust_chi2(self, E, idx):
        """SparseOptimizer::activeRobustChi2, in edge order."""
        with np.errstate(all="ignore"):
            c = np.stack(self.chi2(E, idx), axis=1).reshape(-1)
            r = np.where(c <= self.dsqr, c, 2 * np.sqrt(c) * self.delta - self.dsqr)
        s = 0.0
        for v in r:
            s += float(v)
        return s

    def build(self, S, E, idx):
        """BlockSolver::buildSystem: numeric Jacobians and the robust quadratic form of every active edge, summed in edge order -> H (7 x 7), b (7)."""
        pert = []
        for d in range(7):
            pair = []
            for step in (DELTA, -DELTA):
                u = [0.0] * 7
                u[d] = step
                if self.fix:
                    u[6] = 0.0
                T = sim3_mul(sim3_exp(u), S)
                pair.append(self.errors(T, sim3_inverse(T), idx))
            pert.append(pair)
        with np.errstate(all="ignore"):
            J = np.stack([SCALAR * (p[0] - p[1]) for p in pert], axis=2)  # (n, 4, 7): rows e12 x, y, e21 x, y
            n = len(idx)
            contrib = np.zeros((n, 2, 56))
            c12, c21 = self.chi2(E, idx)
            for e, (chi, w) in enumerate(((c12, self.w1[idx]), (c21, self.w2[idx]))):
                rho1 = np.where(chi <= self.dsqr, 1.0, self.delta / np.sqrt(chi))
                e0, e1 = E[:, 2 * e], E[:, 2 * e + 1]
                r0, r1 = (-(w * e0)) * rho1, (-(w * e1)) * rho1  # omega_r = -omega * _error; omega_r *= rho[1]
                wo = rho1 * w  # robustInformation
                J0, J1 = J[:, 2 * e, :], J[:, 2 * e + 1, :]
                for a in range(7):
                    contrib[:, e, 49 + a] = J0[:, a] * r0 + J1[:, a] * r1
                    for c in range(7):
                        contrib[:, e, a * 7 + c] = (J0[:, a] * wo) * J0[:, c] + (J1[:, a] * wo) * J1[:, c]
            tot = np.add.accumulate(contrib.reshape(2 * n, 56), axis=0)[-1]
        return tot[:49].reshape(7, 7).copy(), tot[49:].copy()


def ldlt_solve(H, lam, b):
    """LinearSolverDense::solve on H + lam * I: L D L^T from the lower triangle; (isPositive, x)."""
    n = 7
    a = [[float(H[i][j]) for j in range(n)] for i in range(n)]
    for i in range(n):
        a[i][i] += lam
    L = [[0.0] * n for _ in range(n)]
    D = [0.0] * n
    positive = True
    for j in range(n):
        d = a[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k] * D[k]
        D[j] = d
        if not d > 0.0:
            positive = False
        if d == 0.0:
            continue
        for i in range(j + 1, n):
            s = a[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k] * D[k]
            L[i][j] = s / d
    if not positive:
        return False, [0.0] * n
    x = [0.0] * n
    for i in range(n):
        s = float(b[i])
        for k in range(i):
            s -= L[i][k] * x[k]
        x[i] = s
    for i in range(n):
        x[i] = x[i] / D[i]
    for i in range(n - 1, -1, -1):
        s = x[i]
        for k in range(i + 1, n):
            s -= L[k][i] * x[k]
        x[i] = s
    return True, x


def _optimize(P, S, idx, iterations, st):
    """SparseOptimizer::optimize(iterations) over the correspondences idx from the estimate S -> (S, the _error every edge is left with)."""
    lam, ni, n_bad = 0.0, 2.0, 0
    E = None
    for it in range(iterations):
        E = P.errors(S, sim3_inverse(S), idx)
        current = P.robust_chi2(E, idx)
        ini = current
        H, b = P.build(S, E, idx)
        if it == 0:
            mx = 0.0
            for j in range(7):
                mx = max(math.fabs(H[j][j]), mx)
            lam, ni, n_bad = 1e-5 * mx, 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            backup = S
            ok, x = ldlt_solve(H, lam, b)
            if P.fix:
                x[6] = 0.0  # VertexSim3Expmap::oplusImpl writes through to the solver's x
            S = sim3_mul(sim3_exp(x), S)
            E = P.errors(S, sim3_inverse(S), idx)
            temp = P.robust_chi2(E, idx)
            if not ok:
                temp = DBL_MAX
            rho = current - temp
            scale = 0.0
            for j in range(7):
                scale += x[j] * (lam * x[j] + float(b[j]))
            scale += 1e-3
            rho /= scale
            if rho > 0 and math.isfinite(temp):
                alpha = 1. - math.pow((2 * rho - 1), 3)
                alpha = min(alpha, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                current = temp
            else:
                lam *= ni
                ni *= 2
                S = backup
                st["rejected"] += 1
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        st["iterations"] += 1
        if qmax == 10 or rho == 0:
            break
        if (ini - current) * 1e3 < ini:
            n_bad += 1
        else:
            n_bad = 0
        if n_bad >= 3:
            break
    return S, E


def optimize_sim3(c):
    """Optimizer::OptimizeSim3 on one problem (a dict as make_case returns) -> (sim3_out (8,), removed (n,) u8, n_inliers, stats).
    stats: early (the < 10 return), nbad1 / nbad2 (pairs flagged by the first / second cut), rejected (LM trials undone), margin (the smallest relative distance of any
    chi2 at either cut from th2)."""
    P = _Problem(c)
    st = {"early": False, "nbad1": 0, "nbad2": 0, "rejected": 0, "iterations": 0, "margin": float("inf"), "stage2": False}
    sim3_in = np.ascontiguousarray(c["sim3_in"], np.float64).copy()
    removed = np.zeros(P.n, np.uint8)
    if P.n == 0:  # optimize() finds no vertex to optimise; nCorrespondences - nBad < 10
        st["early"] = True
        return sim3_in, removed, 0, st
    idx = np.arange(P.n)
    S, E = _optimize(P, sim3_from8(sim3_in), idx, 5, st)

    def cut(E, idx):
        c12, c21 = P.chi2(E, idx)
        both = np.concatenate([c12, c21])
        with np.errstate(all="ignore"):
            st["margin"] = min(st["margin"], float(np.min(np.abs(both - P.th2) / P.th2)))
        return (c12 > P.th2) | (c21 > P.th2)

    bad = cut(E, idx)
    removed[idx[bad]] = 1
    st["nbad1"] = int(bad.sum())
    if P.n - st["nbad1"] < 10:
        st["early"] = True
        return sim3_in, removed, 0, st
    idx = idx[~bad]
    st["stage2"] = True
    S, E = _optimize(P, S, idx, 10 if st["nbad1"] > 0 else 5, st)
    bad = cut(E, idx)
    removed[idx[bad]] = 1
    st["nbad2"] = int(bad.sum())
    return sim3_to8(S), removed, int(len(idx) - st["nbad2"]), st


# ---------------------------------------------------------------------------------------------------------------------------------- the problems
K1 = (525.0, 520.5, 319.5, 239.5)
K2 = (481.25, 483.0, 305.75, 248.25)
N_LEVELS = 8


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(deg) / 2
    return (a[0] * math.sin(h), a[1] * math.sin(h), a[2] * math.sin(h), math.cos(h))


def make_case(seed, n, s=1.0, n_outliers=0, noise=1.0, fix_scale=False, th2=10.0, same_k=False):
    """One OptimizeSim3 problem: two cameras (K1, K2), n points 2 - 20 units deep in both, pixel noise of `noise` level-sigmas, n_outliers pairs with an observation moved
    by 30 - 60 px, and the initial Sim3 perturbed from the truth (scale s) by a few degrees, a few percent of translation and +-5 % of scale (none under fix_scale).
    Everything the reference holds in floats (points as cv::Mat, key points, invSigma2, K, th2) is float-valued."""
    rng = np.random.RandomState(seed)
    k1, k2 = K1, (K1 if same_k else K2)
    truth = (_rot(rng.normal(size=3), rng.uniform(4, 10)), tuple(rng.uniform(-0.4, 0.4, 3) * s), float(s))  # S12: frame 2 -> frame 1
    z2 = rng.uniform(2.0 * max(1.0, 1.0 / s) * 1.15, 20.0 * min(1.0, 1.0 / s) * 0.85, n)
    u2 = rng.uniform(60, 560, n)
    v2 = rng.uniform(50, 420, n)
    P2 = np.stack([(u2 - k2[2]) / k2[0] * z2, (v2 - k2[3]) / k2[1] * z2, z2], axis=1).astype(np.float32).astype(np.float64).reshape(n, 3)
    a = sim3_map(truth, (P2[:, 0], P2[:, 1], P2[:, 2]))
    P1 = np.stack(a, axis=1).astype(np.float32).astype(np.float64).reshape(n, 3)
    lv1, lv2 = rng.randint(0, N_LEVELS, n), rng.randint(0, N_LEVELS, n)
    sigma = 1.2 ** np.arange(N_LEVELS)
    inv_sigma2 = (np.float32(1.0) / (np.float32(1.2) ** np.arange(N_LEVELS, dtype=np.float32)) ** 2).astype(np.float32)
    o1 = np.stack([P1[:, 0] / P1[:, 2] * k1[0] + k1[2], P1[:, 1] / P1[:, 2] * k1[1] + k1[3]], axis=1).reshape(n, 2) + rng.normal(size=(n, 2)) * (noise * sigma[lv1])[:, None]
    o2 = np.stack([P2[:, 0] / P2[:, 2] * k2[0] + k2[2], P2[:, 1] / P2[:, 2] * k2[1] + k2[3]], axis=1).reshape(n, 2) + rng.normal(size=(n, 2)) * (noise * sigma[lv2])[:, None]
    outliers = np.sort(rng.choice(n, n_outliers, replace=False)) if n_outliers else np.zeros(0, np.int64)
    for i in outliers:
        ang, r = rng.uniform(0, 2 * math.pi), rng.uniform(30, 60)
        (o1 if rng.rand() < 0.5 else o2)[i] += (r * math.cos(ang), r * math.sin(ang))
    ds = 1.0 if fix_scale else float(rng.choice([-1, 1]) * rng.uniform(0.02, 0.05) + 1.0)
    pert = (_rot(rng.normal(size=3), rng.uniform(1, 3)), tuple(rng.uniform(-0.03, 0.03, 3) * s), ds)
    init = sim3_mul(pert, truth)
    return {"seed": seed, "P1c": P1, "P2c": P2, "obs1": o1.astype(np.float32).astype(np.float64), "obs2": o2.astype(np.float32).astype(np.float64),
            "inv_sigma2_1": inv_sigma2[lv1].astype(np.float64), "inv_sigma2_2": inv_sigma2[lv2].astype(np.float64),
            "intrinsics": np.array(k1 + k2, np.float32).astype(np.float64), "sim3_in": sim3_to8(init), "th2": np.float32(th2), "fix_scale": bool(fix_scale),
            "outliers": outliers, "truth": sim3_to8(truth)}


THREADS = 256  # the workgroup's stride over the correspondences

# name -> (make_case arguments, the paths the case claims).  Seeds are chosen so that in the restatement no chi2 at either cut lies within a relative 1e-3 of th2
# (tests/test_sim3_opt_patterns.py asserts it, and that every claim holds).
CASES = {}


def _case(name, claims=(), **kw):
    CASES[name] = (kw, tuple(claims))


_case("n0", ("early",), seed=1, n=0)
_case("n9", ("early",), seed=2, n=9, noise=0.3)
_case("n10", ("stage2", "nbad0"), seed=3, n=10, noise=0.3)
_case("n11", ("stage2", "nbad0"), seed=4, n=11, noise=0.3)
_case("n12_3out", ("early", "outliers_exact"), seed=100, n=12, n_outliers=3, noise=0.3)
_case("stride_m1", ("stage2",), seed=103, n=THREADS - 1, n_outliers=25)
_case("stride", ("stage2",), seed=7, n=THREADS, n_outliers=25)
_case("stride_p1", ("stage2",), seed=8, n=THREADS + 1, n_outliers=25)
_case("n2000", ("stage2", "nbad>0"), seed=9, n=2000, n_outliers=300)
_case("clean_5_more", ("stage2", "nbad0"), seed=10, n=120, noise=0.3)
_case("outliers_10_more", ("stage2", "nbad>0"), seed=11, n=150, n_outliers=30)
_case("fix_scale_on", ("stage2",), seed=12, n=140, n_outliers=20, fix_scale=True, s=2.0)
_case("fix_scale_off", ("stage2",), seed=12, n=140, n_outliers=20, fix_scale=False, s=2.0)
_case("scale_0.5", ("stage2",), seed=13, n=130, n_outliers=15, s=0.5)
_case("scale_1", ("stage2",), seed=14, n=130, n_outliers=15, s=1.0)
_case("scale_2", ("stage2",), seed=15, n=130, n_outliers=15, s=2.0)
_case("stage2_flags", ("stage2", "nbad>0", "nbad2>0"), seed=207, n=200, n_outliers=30)
_case("same_k", ("stage2",), seed=16, n=90, n_outliers=10, same_k=True)
BATCH = ("stride_p1", "n0", "n11", "n12_3out", "outliers_10_more", "fix_scale_on", "scale_0.5")  # seven problems of different sizes, one empty, one taking the early return

_made, _judged = {}, {}


def case(name):
    if name not in _made:
        _made[name] = make_case(**CASES[name][0])
    return _made[name]


def judged(name):
    """The restatement's result for a case, computed once."""
    if name not in _judged:
        _judged[name] = optimize_sim3(case(name))
    return _judged[name]


def pose_distance(a, b):
    """Largest difference of the eight numbers relative to max(1, |value|), the quaternion's sign aligned."""
    a, b = np.asarray(a, np.float64).copy(), np.asarray(b, np.float64)
    if np.dot(a[3:7], b[3:7]) < 0:
        a[3:7] = -a[3:7]
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


# ---------------------------------------------------------------------------------------------------------------------------------- the reference's own text
def _cut(text, sig):
    """The function definition that starts with `sig`, up to the brace that closes its body."""
    a = text.index(sig)
    i = text.index("{", a)
    depth = 0
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
        if depth == 0:
            return text[a:i]


def reference_available():
    return os.path.isdir(REF) and bool(glob.glob(os.path.join(ROOT, "oracle", "_ref", "gg_core_*.o")))


def build_reference(directory):
    """Optimizer::OptimizeSim3 cut out of the reference into `directory` (outside the repository), compiled there around tests/cpp/ref_sim3_opt_standins.cpp with
    types_seven_dof_expmap.cpp, under the flags of oracle/Makefile.ref's g2o build, and linked with the g2o core / types / stuff objects of oracle/_ref."""
    d = str(directory)
    assert not os.path.abspath(d).startswith(ROOT + os.sep)
    text = open(os.path.join(REF, "orb_object_slam", "src", "Optimizer.cc")).read()
    with open(os.path.join(d, "ref_sim3_opt_extracted.inc"), "w") as f:
        f.write(_cut(text, "int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale)") + "\n")
    shim = os.path.join(ROOT, "oracle", "ref_shim")
    flags = ["-O3", "-ffp-contract=off", "-fno-fast-math", "-std=c++14", "-fPIC", "-w", "-fvisibility=hidden", "-fvisibility-inlines-hidden",
             "-I" + os.path.join(shim, "eigen_full"), "-I" + os.path.join(shim, "g2o_shadow"), "-I" + os.path.join(REF, "orb_object_slam"), "-I" + shim, "-I" + d]
    objs = []
    for src, name in ((os.path.join(ROOT, "tests", "cpp", "ref_sim3_opt_standins.cpp"), "standins.o"),
                      (os.path.join(REF, "orb_object_slam", "Thirdparty", "g2o", "g2o", "types", "types_seven_dof_expmap.cpp"), "types_seven_dof_expmap.o")):
        objs.append(os.path.join(d, name))
        subprocess.check_call(["g++"] + flags + ["-c", src, "-o", objs[-1]])
    ref_objs = sorted(glob.glob(os.path.join(ROOT, "oracle", "_ref", "gg_core_*.o")) + glob.glob(os.path.join(ROOT, "oracle", "_ref", "gg_types_*.o")) +
                      glob.glob(os.path.join(ROOT, "oracle", "_ref", "gg_stuff_*.o")) + [os.path.join(ROOT, "oracle", "_ref", "gg_os_specific.o")])
    so = os.path.join(d, "libref_sim3_opt.so")
    subprocess.check_call(["g++", "-shared", "-o", so] + objs + ref_objs + ["-Wl,--no-undefined", "-Wl,-Bsymbolic"])
    lib = C.CDLL(so)
    lib.pin_optimize_sim3.restype = C.c_int
    return lib


def run_reference(lib, c, order=None, repeats=1):
    """The reference's function on one problem, its correspondences in `order` (default: as they are) -> (sim3_out, removed in the case's own order, return value)."""
    n = len(c["inv_sigma2_1"])
    order = np.arange(n) if order is None else np.asarray(order)
    dp = lambda a, k: np.ascontiguousarray(np.asarray(a, np.float64).reshape(n, k)[order])
    arrs = [dp(c["P1c"], 3), dp(c["P2c"], 3), dp(c["obs1"], 2), dp(c["obs2"], 2), dp(c["inv_sigma2_1"], 1), dp(c["inv_sigma2_2"], 1),
            np.ascontiguousarray(c["intrinsics"], np.float64), np.ascontiguousarray(c["sim3_in"], np.float64)]
    out, rem = np.zeros(8), np.zeros(max(n, 1), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    r = lib.pin_optimize_sim3(n, *[ptr(a) for a in arrs], C.c_float(float(c["th2"])), int(c["fix_scale"]), int(repeats), ptr(out), rem.ctypes.data_as(C.POINTER(C.c_uint8)))
    removed = np.zeros(n, np.uint8)
    removed[order] = rem[:n]
    return out, removed, r
