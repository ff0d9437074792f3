"""Named inputs of the PoseOptimization edge tests (tests/test_pose_patterns.py on the CPU, tests/test_pose_edges_gpu.py on the device) and the seeded generator that makes
them.  A helper, not a test module.  The judge is the oracle's orc_pose_optimization (oracle/ba_oracle.cpp), which tests/test_ref_graph_pins.py holds to the reference's own
Optimizer::PoseOptimization; orc_pose_optimization_trace is the same run with its counts, and says which paths of the routine a case reaches.

A case is fit for the device test where, in the oracle alone,
  * no chi2 at any classification lies within a relative MARGIN of its threshold (the cut compares floats: 1e-6 is about 16 float ulps, and far above the 1e-12 that the
    device and the oracle differ by), so equal flags are a fair demand, and
  * the pose moves by at most D_REF_FIT when only the order of the edges changes (PERMUTATION_SEEDS): no LM decision flips under reordering.  A flip sends the run elsewhere
    (synth.pose_frame(10, n=800, outlier_frac=0.15) moves by 1.9e-9 that way), and then no tolerance derived from round-off is fair.
Both are conditions on the inputs; test_pose_patterns.py asserts them for every case, and seeds are chosen to meet them."""
import math

import numpy as np

KITTI = (721.5377, 721.5377, 609.5593, 172.854, 386.1448)  # fx fy cx cy bf: synth.K_KITTI, the stereo rig of the sequences
TUM = (517.3, 516.5, 318.6, 255.3, 40.0)  # a 640 x 480 RGB-D camera
THREADS = 256  # the workgroup's stride over a frame's edges; block_reduce sums 64-lane trees, then (w0 + w1) + (w2 + w3)

MARGIN = 1e-6
PERMUTATION_SEEDS = (1, 2, 3, 4)
D_REF_FIT = 1e-12
# D_REF: the largest change of the oracle's seven output numbers over all CASES when only the order of the edges changes (measured by
# tests/test_pose_patterns.py::test_order_sensitivity, which asserts that no case exceeds this constant).
D_REF = 2.1094237467877974e-14  # the case "n3"; the cases of ten edges and more lie between 0 and 2.2e-15
# device vs oracle: 100 x D_REF, the margin the BA edge tests give the device over the oracle's own reordering figure.  The device differs by more than a permutation:
# another summation tree in all 28 sums of every iteration, and its own sqrt / sin / cos.
TOL = 100 * D_REF


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 1:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def _quat(R):
    """(x, y, z, w) of a rotation whose trace is positive (every rotation here is a few degrees)."""
    s = math.sqrt(np.trace(R) + 1.0) * 2
    return np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def make_frame(seed, n, cam=KITTI, outliers=0.2, stereo=0.0, noise_px=1.0, start="predicted", obs_bf=None, zero_weights=False, mirror=0.0, quat_scale=1.0, one_point=False,
               far=(6.0, -2.0, 5.0)):
    """One frame for Optimizer::PoseOptimization under the camera `cam` (fx, fy, cx, cy, bf): n map points 4 - 60 m deep, drawn in normalised image coordinates so that the
    geometry (points, true pose, start pose, which edges are stereo / outliers, the pixel noise) depends on the seed alone and not on the camera.
      outliers      share of the edges (rounded to a count) whose observation is moved by 15 - 80 px in u and 15 - 60 px in v
      stereo        share of the edges that carry u_right = u - bf / z (1.0: all of them)
      start         "predicted": the true pose perturbed like a constant-velocity prediction; "exact": the true pose; "far": its translation moved by `far` metres
      obs_bf        the bf that u_right is made with where it is not the camera's (the frame then optimises against another rig than it was observed with)
      zero_weights  every invSigma2 = 0
      mirror        share of the points mirrored through the world's origin, their observations kept: they lie behind the camera
      quat_scale    the start pose's quaternion is multiplied by this
      one_point     every edge is edge 0 over again
    Points, observations and weights are float-valued, as the reference reads them."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = cam
    R = _rot(1, rng.uniform(-0.2, 0.2)) @ _rot(0, rng.uniform(-0.05, 0.05))
    t = rng.uniform(-1, 1, 3)
    xn, yn, z = rng.uniform(-0.5, 0.8, n), rng.uniform(-0.2, 0.25, n), rng.uniform(4, 60, n)
    Xc = np.stack([xn * z, yn * z, z], axis=1)
    Xw = _f32((R.T @ (Xc - t).T).T)  # Tcw = [R t]
    octave = rng.integers(0, 8, n)
    sig = 1.2 ** octave
    noise = rng.normal(0, noise_px, (n, 3)) * sig[:, None]
    is_stereo = rng.random(n) < stereo
    k = int(round(outliers * n))
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:k]] = True
    shift = np.stack([rng.uniform(15, 80, n) * rng.choice([-1, 1], n), rng.uniform(15, 60, n) * rng.choice([-1, 1], n)], axis=1)
    dR = _rot(1, rng.normal(0, 0.01)) @ _rot(0, rng.normal(0, 0.005)) @ _rot(2, rng.normal(0, 0.005))
    dt = rng.normal(0, 0.05, 3)
    mirrored = np.zeros(n, bool)
    mirrored[rng.permutation(n)[:int(round(mirror * n))]] = True
    # everything random is drawn; from here on the camera comes in
    Xc = (R @ Xw.T).T + t
    u, v = Xc[:, 0] / Xc[:, 2] * fx + cx, Xc[:, 1] / Xc[:, 2] * fy + cy
    obs = np.stack([u + noise[:, 0], v + noise[:, 1], np.full(n, -1.0)], axis=1)
    obs[is_stereo, 2] = u[is_stereo] - (bf if obs_bf is None else obs_bf) / Xc[is_stereo, 2] + noise[is_stereo, 2]
    obs[bad, :2] += shift[bad]
    assert np.all(obs[is_stereo, 2] >= 0)  # u_right < 0 means monocular
    Xw[mirrored] = -Xw[mirrored]
    w = np.zeros(n) if zero_weights else 1.0 / (sig * sig)
    if one_point:
        Xw[:], obs[:], w[:], bad[:], is_stereo[:] = Xw[0], obs[0], w[0], bad[0], is_stereo[0]
    pose_true = np.concatenate([t, _quat(R)])
    if start == "predicted":
        pose = np.concatenate([dR @ t + dt, _quat(dR @ R)])
    elif start == "exact":
        pose = pose_true.copy()
    elif start == "far":
        pose = np.concatenate([t + np.array(far, np.float64), _quat(R)])
    else:
        raise ValueError(start)
    pose[3:] *= quat_scale
    return {"Xw": Xw, "obs": _f32(obs), "inv_sigma2": _f32(w), "intr": np.array(cam, np.float64), "pose": pose, "pose_true": pose_true, "is_outlier": bad,
            "is_stereo": is_stereo, "shift": shift, "mirrored": mirrored}


def normalised(pose):
    """SE3Quat::normalizeRotation of a start pose: w >= 0, unit norm -- what the routine returns where it does not move."""
    p = np.array(pose, np.float64)
    if p[6] < 0:
        p[3:] *= -1
    p[3:] /= math.sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6])
    return p


# name -> (make_frame arguments, the paths the case claims).  Claims (tests/test_pose_patterns.py::test_case_takes_the_path_it_claims):
#   untouched / one_round / four_rounds   n < 3, n < 10, n >= 10
#   exit_qmax / exit_rho0 / exit_nbad / exit_iterations   some round ends that way
#   rejected / failed_solve / failed_every_round / empty_round   an LM trial undone; a 6 x 6 solve failed; in every round; a round that starts with no active edge
#   none_flagged / all_flagged / stays   the flags; the pose is the normalised start pose
#   behind   a point with pc[2] <= 0 was evaluated
#   flips_quat   the start quaternion has w < 0 and is not of unit length
CASES = {}
SIZES = (3, 4, 9, 10, 11, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2049)


def _case(name, claims=(), **kw):
    CASES[name] = (kw, tuple(claims))


_case("n0", ("untouched", "stays"), seed=100, n=0)
_case("n2", ("untouched", "stays"), seed=101, n=2, outliers=0.0, cam=TUM)
# the sizes: about 20 % gross outliers; of every seam triple one is monocular, one mixed, one all stereo
_case("n3", ("one_round",), seed=103, n=3, stereo=1.0)
_case("n4", ("one_round",), seed=104, n=4, stereo=0.5)
_case("n9", ("one_round",), seed=109, n=9)
_case("n10", ("four_rounds", "rejected"), seed=110, n=10, stereo=0.5)
_case("n11", ("four_rounds",), seed=111, n=11, stereo=1.0)
_case("n63", ("four_rounds",), seed=163, n=63, stereo=0.5)
_case("n64", ("four_rounds",), seed=164, n=64, stereo=1.0)
_case("n65", ("four_rounds",), seed=165, n=65)
_case("n255", ("four_rounds",), seed=1255, n=255, stereo=1.0)
_case("n256", ("four_rounds",), seed=1256, n=256)
_case("n257", ("four_rounds",), seed=1257, n=257, stereo=0.3)
_case("n511", ("four_rounds",), seed=1511, n=511)
_case("n512", ("four_rounds", "rejected", "exit_nbad"), seed=1512, n=512, stereo=0.5)
_case("n513", ("four_rounds",), seed=1513, n=513, stereo=1.0)
_case("n2049", ("four_rounds",), seed=3049, n=2049, stereo=0.4)
# paths of the routine
_case("all_outliers", ("four_rounds", "empty_round", "failed_solve", "exit_qmax", "all_flagged", "stays"), seed=200, n=300, outliers=1.0)
_case("zero_weights", ("four_rounds", "failed_every_round", "exit_qmax", "none_flagged", "stays"), seed=201, n=120, stereo=0.3, zero_weights=True)
_case("far_start", ("four_rounds", "exit_iterations", "none_flagged"), seed=237, n=200, outliers=0.0, noise_px=0.0, stereo=0.5, start="far", far=(-8.0, 0.0, 0.0))
_case("behind_camera", ("four_rounds", "behind"), seed=203, n=200, stereo=0.5, mirror=0.1)
_case("quat_unnormalised", ("four_rounds", "flips_quat"), seed=204, n=150, stereo=0.2, quat_scale=-2.5)
_case("exact_start", ("four_rounds", "none_flagged"), seed=205, n=150, outliers=0.0, noise_px=0.0, stereo=0.3, start="exact")
_case("one_point", ("four_rounds", "exit_rho0", "none_flagged"), seed=206, n=20, outliers=0.0, one_point=True)
# cameras: one geometry under two cameras; one stereo frame under two rigs
_case("cam_kitti", ("four_rounds",), seed=300, n=300, stereo=0.5, cam=KITTI)
_case("cam_tum", ("four_rounds",), seed=300, n=300, stereo=0.5, cam=TUM)
_case("bf_a", ("four_rounds",), seed=301, n=120, stereo=1.0, cam=KITTI)
_case("bf_b", ("four_rounds",), seed=301, n=120, stereo=1.0, cam=KITTI[:4] + (380.0,), obs_bf=KITTI[4])

# One call of the library: neighbours under different cameras, a frame without edges and one with two between large ones, and (the first size being odd, the others even)
# every edge offset after the first odd.
BATCH = ("n257", "cam_tum", "n0", "n512", "n2", "cam_kitti", "bf_b", "n10", "all_outliers", "n64", "bf_a")

_made, _judged, _sensitivity = {}, {}, {}


def case(name):
    if name not in _made:
        _made[name] = make_frame(**CASES[name][0])
    return _made[name]


def run(oracle, fr, order=None):
    """The oracle on a frame, its edges in `order` (default: as they are) -> (pose, flags in the frame's own order, n_inliers, trace)."""
    if order is None:
        return oracle.pose_optimization_trace(fr["Xw"], fr["obs"], fr["inv_sigma2"], fr["intr"], fr["pose"])
    pose, flags, n_in, tr = oracle.pose_optimization_trace(fr["Xw"][order], fr["obs"][order], fr["inv_sigma2"][order], fr["intr"], fr["pose"])
    back = np.zeros_like(flags)
    back[order] = flags
    return pose, back, n_in, tr


def judged(oracle, name):
    """The oracle's result for a case, computed once and never changed."""
    if name not in _judged:
        pose, flags, n_in, tr = run(oracle, case(name))
        pose.setflags(write=False)
        flags.setflags(write=False)
        _judged[name] = (pose, flags, n_in, tr)
    return _judged[name]


def pose_distance(a, b):
    """Largest absolute difference of the seven numbers (translations are metres of order one, the quaternion has unit length and w >= 0 on both sides)."""
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def order_sensitivity(oracle, name):
    """(d_ref, flags equal, counts equal) of a case: the oracle again with the edges permuted under each of PERMUTATION_SEEDS, against the oracle on the case as it is."""
    if name not in _sensitivity:
        pose, flags, n_in, _ = judged(oracle, name)
        d, same_flags, same_count = 0.0, True, True
        n = len(flags)
        for s in PERMUTATION_SEEDS:
            p, f, k, _ = run(oracle, case(name), np.random.default_rng(s).permutation(n))
            d = max(d, pose_distance(p, pose))
            same_flags &= bool(np.array_equal(f, flags))
            same_count &= k == n_in
        _sensitivity[name] = (d, same_flags, same_count)
    return _sensitivity[name]
