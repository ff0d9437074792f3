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
# "stride_p1"; the other seeded cases lie between 1e-09 and 2e-08, the designed ones below 2.1e-07, "th2_7.815").  With delta = 1e-9 Jacobians a last-bit change of a sum moves the next iterate by far more than a bit.
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


EXP_BRANCHES = ("sigma0_theta0", "sigma0_theta", "sigma_theta0", "sigma_theta")  # |sigma| < eps or not, theta < eps or not, in the order sim3.h:83-128 writes them


def sim3_exp_branch(u):
    """The branch of sim3_exp an update takes: the two comparisons are IEEE operations on theta as sim3_exp computes it."""
    theta = math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    return EXP_BRANCHES[(0 if math.fabs(u[6]) < EPS else 2) + (0 if theta < EPS else 1)]


def sim3_exp_longdouble(u):
    """The formulas of sim3_exp in numpy.longdouble, on the branch the float64 comparisons choose -> the eight numbers tx ty tz qx qy qz qw s (longdouble)."""
    L = np.longdouble
    branch = EXP_BRANCHES.index(sim3_exp_branch(u))
    small_sigma, small_theta = branch < 2, branch % 2 == 0
    w = [L(u[0]), L(u[1]), L(u[2])]
    ups, sigma = [L(u[3]), L(u[4]), L(u[5])], L(u[6])
    theta = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Om = [[L(0), -w[2], w[1]], [w[2], L(0), -w[0]], [-w[1], w[0], L(0)]]
    Om2 = [[Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j] for j in range(3)] for i in range(3)]
    I = [[L(1 if i == j else 0) for j in range(3)] for i in range(3)]
    s = np.exp(sigma)
    if small_theta:
        R = [[I[i][j] + Om[i][j] + Om2[i][j] for j in range(3)] for i in range(3)]
    else:
        a, b = np.sin(theta) / theta, (1 - np.cos(theta)) / (theta * theta)
        R = [[I[i][j] + a * Om[i][j] + b * Om2[i][j] for j in range(3)] for i in range(3)]
    if small_sigma:
        C = L(1)
        if small_theta:
            A, B = L(1) / 2, L(1) / 6
        else:
            A, B = (1 - np.cos(theta)) / (theta * theta), (theta - np.sin(theta)) / (theta * theta * theta)
    else:
        C = (s - 1) / sigma
        if small_theta:
            A, B = ((sigma - 1) * s + 1) / (sigma * sigma), ((L(0.5) * sigma * sigma - sigma + 1) * s) / (sigma * sigma * sigma)
        else:
            a, b, c = s * np.sin(theta), s * np.cos(theta), theta * theta + sigma * sigma
            A, B = (a * sigma + (1 - b) * theta) / (theta * c), (C - ((b - 1) * sigma + a * theta) / c) / (theta * theta)
    q = [L(0)] * 4
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0:
        t = np.sqrt(t + 1)
        q[3] = t / 2
        t = L(0.5) / t
        q[0], q[1], q[2] = (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
        q[i] = t / 2
        t = L(0.5) / t
        q[3], q[j], q[k] = (R[k][j] - R[j][k]) * t, (R[j][i] + R[i][j]) * t, (R[k][i] + R[i][k]) * t
    W = [[A * Om[i][j] + B * Om2[i][j] + C * I[i][j] for j in range(3)] for i in range(3)]
    tr = [W[i][0] * ups[0] + W[i][1] * ups[1] + W[i][2] * ups[2] for i in range(3)]
    return np.array(tr + q + [s], np.longdouble)


def quat_branch(u):
    """Which branch of Quaterniond(Matrix3d) the rotation of an update takes: "t>0", or the largest diagonal entry "i0" / "i1" / "i2"."""
    o = sim3_exp_longdouble(u)[3:7]
    R = [[1 - 2 * (o[1] ** 2 + o[2] ** 2), 0, 0], [0, 1 - 2 * (o[0] ** 2 + o[2] ** 2), 0], [0, 0, 1 - 2 * (o[0] ** 2 + o[1] ** 2)]]  # the diagonal of the rotation q stands for
    if R[0][0] + R[1][1] + R[2][2] > 0:
        return "t>0"
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    return "i%d" % i


def _exp_updates():
    """Designed updates for cs_sim3_exp: both comparisons at eps, one ulp either side and well away, with and without a translation (without one t is exactly zero and the
    quaternion alone is judged, which is where the two theta branches differ most: R's Omega^2 term has the factor 1 in one and 1/2 in the other); rotations of pi - 1e-3
    for the three written-out cases of the quaternion's second branch; the zero update."""
    lo, hi = float(np.nextafter(EPS, 0.0)), float(np.nextafter(EPS, 1.0))
    ups = [(0.0, 0.0, 0.0), (0.3, -0.2, 0.5)]
    out = [[0.0] * 7]
    axes = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1 / math.sqrt(2), 1 / math.sqrt(2), 0.0), (0.6, -0.48, 0.64)]
    for theta in (0.0, 1e-6, lo, EPS, hi, 2e-5, 0.3, 2.0):
        for sigma in (0.0, 1e-6, -1e-6, lo, -lo, EPS, -EPS, hi, -hi, 2e-5, -0.4, 0.7):
            for a, axis in enumerate(axes[2:] if theta not in (lo, EPS, hi) else axes):
                for up in ups:
                    out.append([axis[0] * theta, axis[1] * theta, axis[2] * theta, up[0], up[1], up[2], sigma])
    for axis in axes[:4]:
        for sigma in (0.0, 0.2):
            th = math.pi - 1e-3
            out.append([axis[0] * th, axis[1] * th, axis[2] * th, 0.3, -0.2, 0.5, sigma])
    return np.array(out, np.float64)


EXP_UPDATES = _exp_updates()


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
    def __init__(self, c, mutate=None):
        assert mutate in (None,) + MUTANTS
        self.mutate = mutate
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
                wo = w if self.mutate == "no_rho1_in_H" else rho1 * w  # robustInformation
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


MUTANTS = ("no_rho1_in_H", "lambda0_1e-4", "keep_rejected")  # the deliberately wrong variants of optimize_sim3(mutate=...): see there
EXITS = ("qmax", "rho0", "nbad3", "full")  # how a stage's optimize() ends: ten trials of one iteration, rho == 0, three iterations of little gain, the budget spent
TRACE_RECORD = 7  # stage, iteration, currentChi before the trial, tempChi as computed, lambda used, solved, accepted (include/cubeslam_hip/sim3_opt_trace.h)


def _optimize(P, S, idx, iterations, st, stage=0):
    """SparseOptimizer::optimize(iterations) over the correspondences idx from the estimate S -> (S, the _error every edge is left with)."""
    lam, ni, n_bad = 0.0, 2.0, 0
    E = None
    way_out = "full"
    for it in range(iterations):
        E = P.errors(S, sim3_inverse(S), idx)
        current = P.robust_chi2(E, idx)
        ini = current
        H, b = P.build(S, E, idx)
        if it == 0:
            mx = 0.0
            for j in range(7):
                mx = max(math.fabs(H[j][j]), mx)
            lam, ni, n_bad = (1e-4 if P.mutate == "lambda0_1e-4" else 1e-5) * mx, 2.0, 0
            if stage == 0:
                st["system0"] = np.array([H[a][c] for a in range(7) for c in range(a + 1)] + [float(v) for v in b] + [current], np.float64)
        rho, qmax = 0.0, 0
        while True:
            backup = S
            ok, x = ldlt_solve(H, lam, b)
            if P.fix:
                x[6] = 0.0  # VertexSim3Expmap::oplusImpl writes through to the solver's x
            S = sim3_mul(sim3_exp(x), S)
            E = P.errors(S, sim3_inverse(S), idx)
            temp = P.robust_chi2(E, idx)
            record = [float(stage), float(it), current, temp, lam, 1.0 if ok else 0.0, 0.0]
            st["trace"].append(record)
            if ok:
                st["branches"].append(sim3_exp_branch(x))
            else:
                st["failed_solves"] += 1
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
                record[6] = 1.0
            else:
                lam *= ni
                ni *= 2
                if P.mutate != "keep_rejected":
                    S = backup
                st["rejected"] += 1
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        st["iterations"] += 1
        if qmax == 10 or rho == 0:
            way_out = "qmax" if qmax == 10 else "rho0"
            break
        if (ini - current) * 1e3 < ini:
            n_bad += 1
        else:
            n_bad = 0
        if n_bad >= 3:
            way_out = "nbad3"
            break
    st["exits"].append(way_out)
    st["stage_iterations"].append(st["iterations"] - sum(st["stage_iterations"]))
    return S, E


def optimize_sim3(c, stage2_budget=None, mutate=None):
    """Optimizer::OptimizeSim3 on one problem (a dict as make_case returns) -> (sim3_out (8,), removed (n,) u8, n_inliers, stats).
    stats: early (the < 10 return), nbad1 / nbad2 (pairs flagged by the first / second cut), rejected (LM trials undone), margin (the smallest relative distance of any
    chi2 at either cut from th2); and what the probe cs_sim3_optimization_trace shows of the way: trace ((trials, 7): one record per LM trial in the probe's layout, see
    TRACE_RECORD), system0 (36: the 28 lower-triangle entries of H in row order, b and chi2 of the first linearisation of stage one; zeros without correspondences), exits
    (one of EXITS per stage that ran), stage_iterations (iterations entered per stage), branches (the sim3_exp branch of every solved step, in order), failed_solves.
    The two keyword arguments exist for the preconditions that tests/test_sim3_opt_patterns.py checks on the CPU; their defaults restate the reference.
      stage2_budget  the iterations of the second optimize() in place of nBad > 0 ? 10 : 5
      mutate         one of MUTANTS, each a bug the end pose forgives: "no_rho1_in_H" builds H from the plain information (b keeps rho[1]), "lambda0_1e-4" starts from
                     lambda = 1e-4 * max |diag H|, "keep_rejected" does not restore the estimate after a rejected trial"""
    P = _Problem(c, mutate)
    st = {"early": False, "nbad1": 0, "nbad2": 0, "rejected": 0, "iterations": 0, "margin": float("inf"), "stage2": False,
          "trace": [], "system0": np.zeros(36), "exits": [], "stage_iterations": [], "branches": [], "failed_solves": 0}

    def done(*result):
        st["trace"] = np.array(st["trace"], np.float64).reshape(-1, TRACE_RECORD)
        return result + (st,)

    sim3_in = np.ascontiguousarray(c["sim3_in"], np.float64).copy()
    removed = np.zeros(P.n, np.uint8)
    if P.n == 0:  # optimize() finds no vertex to optimise; nCorrespondences - nBad < 10
        st["early"] = True
        return done(sim3_in, removed, 0)
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
        return done(sim3_in, removed, 0)
    idx = idx[~bad]
    st["stage2"] = True
    S, E = _optimize(P, S, idx, (10 if st["nbad1"] > 0 else 5) if stage2_budget is None else stage2_budget, st, stage=1)
    bad = cut(E, idx)
    removed[idx[bad]] = 1
    st["nbad2"] = int(bad.sum())
    return done(sim3_to8(S), removed, int(len(idx) - st["nbad2"]))


# ---------------------------------------------------------------------------------------------------------------------------------- the problems
K1 = (525.0, 520.5, 319.5, 239.5)
K2 = (481.25, 483.0, 305.75, 248.25)
N_LEVELS = 8


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(deg) / 2
    return (a[0] * math.sin(h), a[1] * math.sin(h), a[2] * math.sin(h), math.cos(h))


def make_case(seed, n, s=1.0, n_outliers=0, noise=1.0, fix_scale=False, th2=10.0, same_k=False, weights=None, moved=(), start=None, k2_claimed=None, fix_flag=None, behind=()):
    """One OptimizeSim3 problem: two cameras (K1, K2), n points 2 - 20 units deep in both, pixel noise of `noise` level-sigmas, n_outliers pairs with an observation moved
    by 30 - 60 px, and the initial Sim3 perturbed from the truth (scale s) by a few degrees, a few percent of translation and +-5 % of scale (none under fix_scale).
    Everything the reference holds in floats (points as cv::Mat, key points, invSigma2, K, th2) is float-valued.
    The designed departures, none of which draws from the generator (a case without them is what it was before they existed):
      weights     both invSigma2 arrays are this number (0.0: H = 0 and b = 0, every solve fails)
      moved       ((i, dx, dy), ...): obs1[i] is moved by (dx, dy) pixels, far beyond the 30 - 60 px of n_outliers
      start       (degrees, translation, scale factor): the initial Sim3 is this far from the truth in place of the few degrees and percent, about the drawn axis and
                  along the drawn signs
      k2_claimed  the K2 the problem states in `intrinsics`, the points and observations staying those of K2: the same arrays under another camera
      fix_flag    the fix_scale the problem states, the start staying that of `fix_scale`: one problem with and without the flag
      behind      indices whose P2c is mirrored to negative depth (finite errors, a chi2 far beyond any th2)"""
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
    axis, deg, dt = rng.normal(size=3), rng.uniform(1, 3), rng.uniform(-0.03, 0.03, 3)
    pert = (_rot(axis, deg), tuple(dt * s), ds)
    if start is not None:
        pert = (_rot(axis, start[0]), tuple(np.sign(dt) * start[1] * s), float(start[2]))
    init = sim3_mul(pert, truth)
    for i, dx, dy in moved:
        o1[i] += (dx, dy)
    for i in behind:
        P2[i, 2] = -P2[i, 2]
    w = inv_sigma2 if weights is None else np.full(N_LEVELS, weights, np.float32)
    kc = k2 if k2_claimed is None else tuple(k2_claimed)
    return {"seed": seed, "P1c": P1, "P2c": P2, "obs1": o1.astype(np.float32).astype(np.float64), "obs2": o2.astype(np.float32).astype(np.float64),
            "inv_sigma2_1": w[lv1].astype(np.float64), "inv_sigma2_2": w[lv2].astype(np.float64),
            "intrinsics": np.array(k1 + kc, np.float32).astype(np.float64), "sim3_in": sim3_to8(init), "th2": np.float32(th2),
            "fix_scale": bool(fix_scale if fix_flag is None else fix_flag),
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

# The designed cases: the exits, budgets and per-problem parameters the seeded ones above never reach.  Claims beyond those above (each checked by
# tests/test_sim3_opt_patterns.py): "exits:a,b" the way out of each stage (* = any), "failed_solves" every trial's solve fails, "pose_unmoved" sim3_out is sim3_in bit for
# bit although stage two ran, "all_inliers" / "all_flagged", "ten_left" exactly 10 pairs enter stage two, "behind_flagged" the mirrored point is finite and flagged,
# "scale_kept" s leaves as it came, "stage2_its>=6" / "stage2_its==5", "budget_matters" the other stage-two budget lands further than 100 x TOL away or differs in a flag.
_case("zero_weights", ("stage2", "nbad0", "exits:qmax,qmax", "failed_solves", "pose_unmoved", "all_inliers"), seed=21, n=40, weights=0.0)
_case("all_outliers", ("early", "all_flagged"), seed=22, n=30, n_outliers=30, noise=0.3)
_case("n13_3out", ("stage2", "outliers_exact", "ten_left"), seed=100, n=13, n_outliers=3, noise=0.3)
_case("behind", ("stage2", "nbad>0", "behind_flagged"), seed=30, n=50, behind=(17,))
_case("fix_clean", ("stage2", "nbad0", "exits:qmax,*", "scale_kept"), seed=28, n=60, fix_scale=True)
_case("exact", ("stage2", "nbad0", "exits:*,rho0"), seed=42, n=80, noise=0.0)
_case("budget10", ("stage2", "nbad>0", "stage2_its>=6", "budget_matters"), seed=371, n=100, th2=1000.0, moved=((5, 900, -700), (41, 900, -700), (77, 900, -700)), start=(60, 1.0, 2.5))
_case("budget5", ("stage2", "nbad0", "exits:*,full", "stage2_its==5", "budget_matters"), seed=424, n=100, th2=1e5, start=(60, 1.0, 2.5))
_case("th2_5.991", ("stage2", "nbad>0"), seed=500, n=150, n_outliers=20, noise=1.3, th2=5.991)  # (float) (delta * delta) is th2 - 4.8e-7
_case("th2_7.815", ("stage2", "nbad>0"), seed=500, n=150, n_outliers=20, noise=1.3, th2=7.815)  # ... th2 + 4.8e-7
_case("th2_20", ("stage2", "nbad>0"), seed=500, n=150, n_outliers=20, noise=1.3, th2=20.0)  # ... th2
_case("k_a", ("stage2",), seed=700, n=120, n_outliers=10)
_case("k_b", ("stage2",), seed=700, n=120, n_outliers=10, k2_claimed=(495.0, 470.0, 300.0, 255.0))
_case("fix_a", ("stage2", "scale_kept"), seed=760, n=110, n_outliers=12, s=1.5, fix_flag=True)
_case("fix_b", ("stage2",), seed=760, n=110, n_outliers=12, s=1.5, fix_flag=False)
NEW_CASES = tuple(CASES)[18:]
PAIRS = (("th2_5.991", "th2_20"), ("k_a", "k_b"), ("fix_a", "fix_b"))  # one geometry each, differing in one per-problem parameter

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


# ---------------------------------------------------------------------------------------------------------------------------------- the way, not only the end
# How far the restatement's own first system and trace move when only the order of its correspondences changes (the way D_REF was obtained, over the four ORDERS below).  The first system is
# one sum and has one figure.  The trace has a figure per trial: with delta = 1e-9 Jacobians two summation orders drift apart from trial to trial (1e-15 at the first
# trial, 1e-6 after ten), and the tempChi of a rejected trial -- chi2 after a step far outside the trust region -- moves by up to 3e-2 where the chi2 that is kept moves
# by 1e-9, so one figure for all trials would either fail the first kind or see nothing in the second.  For trial i of a case (order_figures):
#   chi_i     the larger of: the largest relative change of currentChi over the trials 0 .. i (what has accumulated in the estimate), the relative change of tempChi of
#             trial i itself, and D_SYS0 (two orders may agree to the bit by luck)
#   lambda_i  the largest relative change of lambda over the trials 0 .. i, and D_SYS0
# Tolerances are 10 x the figure, the factor TOL uses for a third summation order.  A trial is decisive where its solve failed (tempChi is then replaced by DBL_MAX
# whatever it was) or |currentChi - tempChi| / currentChi >= 100 x chi_i; the decisive prefix of a case ends before its first trial that is not, and at the latest where the
# two orders stop agreeing in (stage, iteration, solved, accepted).  tests/test_sim3_opt_patterns.py::test_order_sensitivity_constants asserts each constant:
#   D_SYS0    system0 over TRACED: the entries of H relative to the largest |H|, those of b to the largest |b|, chi2 to itself
#   D_CHI     the largest chi_i inside a decisive prefix, over TRACED          D_LAMBDA  the largest lambda_i inside a decisive prefix
#   D_EXP     sim3_exp in float64 against the same formulas in numpy.longdouble on EXP_UPDATES, as pose_distance measures
D_SYS0 = 4.168467699661468e-15  # "n2000"
D_CHI = 0.009703636592577617  # a rejected trial's tempChi in "budget10"; the chi2 of an accepted trial moves by 1.4e-04 at most ("budget5")
D_LAMBDA = 7.359614434272237e-06  # "budget5"
D_EXP = 5.142225566797526e-12  # theta = 1e-5, sigma = 2e-5: (1 - cos(theta)) / theta^2 and its like cancel; the median over EXP_UPDATES is 1e-16
SYS0_TOL, EXP_TOL = 10 * D_SYS0, 10 * D_EXP
TRACED = tuple(k for k in CASES if k != "n0")  # every case that runs a trial
MAX_TRIALS = 150  # 15 iterations of at most 10 trials
STRUCTURE = [0, 1, 5, 6]  # stage, iteration, solved, accepted


# The orders a case is summed in beside its own.  Reversal alone is one draw of what another order does, and at a trial whose step is itself amplified rounding (a
# rejected trial at convergence) that draw scatters by more than the factor ten: a trial's figure is the largest over these four.
ORDERS = {"reversed": lambda n: np.arange(n)[::-1], "halves swapped": lambda n: np.roll(np.arange(n), n // 2),
          "evens then odds": lambda n: np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)]), "odds reversed then evens": lambda n: np.concatenate([np.arange(1, n, 2)[::-1], np.arange(0, n, 2)])}


def reordered_case(c, order="reversed"):
    """The same problem with its correspondences in another order."""
    r = dict(c)
    idx = ORDERS[order](len(np.asarray(c["inv_sigma2_1"]).reshape(-1)))
    for k in ("P1c", "P2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
        r[k] = np.ascontiguousarray(np.asarray(c[k])[idx])
    return r


def _rel(a, b):
    a, b = float(a), float(b)
    if a == b:
        return 0.0
    return abs(a - b) / abs(b) if b != 0 else float("inf")


def system0_distance(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = []
    for lo, hi in ((0, 28), (28, 35)):
        m = np.max(np.abs(want[lo:hi]))
        d.append(float(np.max(np.abs(got[lo:hi] - want[lo:hi]))) / m if m > 0 else (0.0 if np.array_equal(got[lo:hi], want[lo:hi]) else float("inf")))
    return max(d[0], d[1], _rel(got[35], want[35]))


def common_prefix(a, b):
    """The number of leading trials of two traces that agree in stage, iteration, solved and accepted."""
    k = 0
    while k < min(len(a), len(b)) and np.array_equal(a[k][STRUCTURE], b[k][STRUCTURE]):
        k += 1
    return k


_figures = {}


def order_figures(name, other=None):
    """-> {"sys0", "chi" (per trial), "lambda" (per trial), "prefix" (the decisive prefix), "common", "gain" (per trial: |currentChi - tempChi| / currentChi)} of a case,
    from its trace and those of the same problem in the ORDERS."""
    if name in _figures:
        return _figures[name]
    st = judged(name)[3]
    others = [optimize_sim3(reordered_case(case(name), o))[3] for o in ORDERS]
    t = st["trace"]
    kc = min(common_prefix(rs["trace"], t) for rs in others)
    chi, lam, gain, carry_c, carry_l, prefix, open_ = [], [], [], D_SYS0, D_SYS0, 0, True
    for i in range(kc):
        carry_c = max([carry_c] + [_rel(rs["trace"][i][2], t[i][2]) for rs in others])
        carry_l = max([carry_l] + [_rel(rs["trace"][i][4], t[i][4]) for rs in others])
        chi.append(max([carry_c] + [_rel(rs["trace"][i][3], t[i][3]) for rs in others]))
        lam.append(carry_l)
        gain.append(abs(t[i][2] - t[i][3]) / t[i][2] if t[i][2] > 0 else 0.0)
        if open_ and (t[i][5] == 0.0 or gain[i] >= 100 * chi[i]):
            prefix = i + 1
        else:
            open_ = False
    f = _figures[name] = {"sys0": max(system0_distance(rs["system0"], st["system0"]) for rs in others), "chi": chi, "lambda": lam, "prefix": prefix, "common": kc, "gain": gain}
    return f


def compare_way(name, system0, trace):
    """A first system and a trace (the device's, or a mutant's) against the restatement's of the case -> {"sys0": distance of the systems, "same": stage, iteration, solved
    and accepted equal on the decisive prefix, "chi" / "lambda": the largest relative difference on the prefix, "chi_ratio" / "lambda_ratio": the largest difference as a
    multiple of its trial's tolerance (<= 1 passes), "chi_trial": the trial of "chi_ratio", "prefix"}."""
    f, want = order_figures(name), judged(name)[3]
    k, t = f["prefix"], want["trace"]
    g = np.asarray(trace, np.float64).reshape(-1, TRACE_RECORD)
    out = {"sys0": system0_distance(system0, want["system0"]), "prefix": k, "same": len(g) >= k and bool(np.array_equal(g[:k][:, STRUCTURE], t[:k][:, STRUCTURE])),
           "chi": 0.0, "lambda": 0.0, "chi_ratio": 0.0, "lambda_ratio": 0.0, "chi_trial": -1}
    for i in range(min(k, len(g))):
        dc, dl = max(_rel(g[i][2], t[i][2]), _rel(g[i][3], t[i][3])), _rel(g[i][4], t[i][4])
        out["chi"], out["lambda"] = max(out["chi"], dc), max(out["lambda"], dl)
        if dc / (10 * f["chi"][i]) > out["chi_ratio"]:
            out["chi_ratio"], out["chi_trial"] = dc / (10 * f["chi"][i]), i
        out["lambda_ratio"] = max(out["lambda_ratio"], dl / (10 * f["lambda"][i]))
    return out


_exp = {}


def exp_judged():
    """-> (sim3_exp of every row of EXP_UPDATES as eight numbers (n, 8), its distance from the longdouble formulas per row, the tolerance per row).  A row's tolerance is 10 x
    its own distance, and at least 10 x 2^-52 (a float64 result may be the longdouble one rounded, which says nothing about a second libm): never more than EXP_TOL."""
    if not _exp:
        want = np.array([sim3_to8(sim3_exp(list(u))) for u in EXP_UPDATES])
        ld = [sim3_exp_longdouble(list(u)) for u in EXP_UPDATES]
        d = np.array([float(np.max(np.abs(np.asarray(w, np.longdouble) - l) / np.maximum(1, np.abs(l)))) for w, l in zip(want, ld)])
        _exp["r"] = (want, d, 10 * np.maximum(d, 2.0 ** -52))
    return _exp["r"]


def measure_order_sensitivity():
    """-> (D_SYS0, D_CHI, D_LAMBDA as defined above)."""
    fs = [order_figures(name) for name in TRACED]
    return (max(f["sys0"] for f in fs), max(max(f["chi"][:f["prefix"]] + [0.0]) for f in fs), max(max(f["lambda"][:f["prefix"]] + [0.0]) for f in fs))


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
