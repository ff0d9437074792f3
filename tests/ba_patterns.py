"""Graph transforms over the dict of synth.ba_problem (plain numpy): the shapes of the reduced camera system that a chain with k_obs <= 9 never
produces -- wide bands, scrambled camera order, loop edges, fixed cameras in the middle, starved landmarks, dead cuboid blocks, gross outliers.
Every transform returns a new dict and leaves its input untouched.  CASES names the graphs that tests/test_ba_patterns.py (CPU, oracle only) vets
and tests/test_ba_edges_gpu.py (device vs oracle) runs, each with the (C, Bc) it is built to have."""
import numpy as np

from cube_slam_amd import synth

_OBS_KEYS = ("obs_cam", "obs_point", "obs_uv", "obs_inv_sigma2", "obs_ur")
_COBS_KEYS = ("cobs_cam", "cobs_cuboid", "cobs_bbox", "cobs_info")


def free_index(d):
    """index of every camera among the free ones (-1: fixed), as cs_ba_create numbers the pose blocks"""
    fixed = np.asarray(d["cam_fixed"]).astype(int)  # uint8 would wrap in the cumsum
    idx = np.cumsum(1 - fixed) - 1
    return np.where(fixed != 0, -1, idx)


def band_shape(d):
    """(C, Bc) as cs_ba_create computes them: C free cameras; Bc the largest distance, in free-camera indices, between two free cameras that share
    a landmark or a cuboid (edges of fixed cameras are dead and do not count).  This is the graph's own half-width: where it is 0 (one free camera,
    or free cameras that share nothing) the library solves with a band of half-width 1 whose extra block is zero."""
    idx = free_index(d)
    C = int((idx >= 0).sum())
    Bc = 0
    for cams, owner in ((d["obs_cam"], d["obs_point"]), (d["cobs_cam"], d["cobs_cuboid"])):
        i = idx[np.asarray(cams, int)]
        o = np.asarray(owner, int)[i >= 0]
        i = i[i >= 0]
        if len(i) == 0:
            continue
        n = int(o.max()) + 1
        lo = np.full(n, C, int); hi = np.full(n, -1, int)
        np.minimum.at(lo, o, i); np.maximum.at(hi, o, i)
        seen = hi >= 0
        Bc = max(Bc, int((hi[seen] - lo[seen]).max()))
    return C, Bc


def permute_cameras(d, seed):
    """The same optimisation problem with the cameras relabelled: camera i becomes camera perm[i].  Un-permute a result with cam[perm]."""
    n = len(d["cam_pose"])
    perm = np.random.default_rng(seed).permutation(n)
    inv = np.argsort(perm)
    d2 = dict(d)
    for k in ("cam_pose", "cam_fixed", "cam_true"):
        d2[k] = np.ascontiguousarray(np.asarray(d[k])[inv])
    d2["obs_cam"] = perm[np.asarray(d["obs_cam"], int)].astype(np.int32)
    d2["cobs_cam"] = perm[np.asarray(d["cobs_cam"], int)].astype(np.int32)
    return d2, perm


def _rot_of_quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def add_loop_edges(d, n_landmarks, cams, seed, last=3, noise_px=1.0):
    """A loop closure with correct geometry: n_landmarks landmarks that the last `last` observing key frames see are also observed by every camera of
    `cams`, projected from cam_true / points_true (pose layout t, qx qy qz qw of Tcw) plus pixel noise.  Positive depth is all that is asked.
    (synth.ba_problem starts no landmark at its last ~k_obs + 5 key frames, so those observe nothing: "last" counts the key frames that observe.)"""
    rng = np.random.default_rng(seed)
    tail = np.unique(np.asarray(d["obs_cam"]))[-last:]
    cand = np.unique(np.asarray(d["obs_point"])[np.isin(d["obs_cam"], tail)])
    pick = np.sort(rng.choice(cand, n_landmarks, replace=False))
    oc, op, ou, ow = [], [], [], []
    for c in cams:
        t, R = d["cam_true"][c, :3], _rot_of_quat(d["cam_true"][c, 3:])
        Xc = d["points_true"][pick] @ R.T + t
        assert (Xc[:, 2] > 0).all()
        uv = np.stack([d["fx"] * Xc[:, 0] / Xc[:, 2] + d["cx"], d["fy"] * Xc[:, 1] / Xc[:, 2] + d["cy"]], axis=1) + rng.normal(0, noise_px, (len(pick), 2))
        octave = rng.integers(0, 8, len(pick))
        oc.append(np.full(len(pick), c)); op.append(pick); ou.append(uv); ow.append(1.0 / (1.2 ** octave) ** 2)
    d2 = dict(d)
    new = {"obs_cam": np.concatenate(oc), "obs_point": np.concatenate(op), "obs_uv": np.concatenate(ou), "obs_inv_sigma2": np.concatenate(ow)}
    if d.get("obs_ur") is not None:
        new["obs_ur"] = np.full(len(new["obs_cam"]), -1.0)
    for k, v in new.items():
        d2[k] = np.concatenate([np.asarray(d[k]), v.astype(np.asarray(d[k]).dtype)])
    order = np.lexsort((d2["obs_cam"], d2["obs_point"]))  # landmark-major, as synth.ba_problem leaves it
    for k in new:
        d2[k] = np.ascontiguousarray(d2[k][order])
    return d2


def fix_cameras(d, idx):
    d2 = dict(d)
    f = np.array(d["cam_fixed"], np.uint8)
    f[np.asarray(idx, int)] = 1
    d2["cam_fixed"] = f
    return d2


def keep_observations(d, mask):
    mask = np.asarray(mask, bool)
    d2 = dict(d)
    for k in _OBS_KEYS:
        if d.get(k) is not None:
            d2[k] = np.ascontiguousarray(np.asarray(d[k])[mask])
    return d2


def cuboids_seen_only_by(d, cams, cuboids=None):
    """Drops the camera-cuboid edges of the listed cuboids (default: all) whose camera is not in `cams`, so that fixing `cams` leaves those cuboids
    with dead Schur blocks only."""
    cc, cq = np.asarray(d["cobs_cam"]), np.asarray(d["cobs_cuboid"])
    hit = np.ones(len(cq), bool) if cuboids is None else np.isin(cq, cuboids)
    keep = ~hit | np.isin(cc, cams)
    d2 = dict(d)
    for k in _COBS_KEYS:
        d2[k] = np.ascontiguousarray(np.asarray(d[k])[keep])
    return d2


def with_outliers(d, frac, sigma_px, seed):
    """A share `frac` of the observations moved by N(0, sigma_px) in u and v: wrong matches that the Huber kernel has to hold down."""
    rng = np.random.default_rng(seed)
    n = len(d["obs_cam"])
    hit = rng.choice(n, int(round(frac * n)), replace=False)
    uv = np.array(d["obs_uv"], np.float64)
    uv[hit] += rng.normal(0, sigma_px, (len(hit), 2))
    d2 = dict(d)
    d2["obs_uv"] = uv
    return d2


# ----------------------------------------------------------------------------------------------- the graphs of the two test files
def ladder(k_obs, n_kf=48, n_points=600):
    """cuboid-free chain whose landmarks are seen by k_obs consecutive key frames: (C, Bc) = (n_kf - 1, k_obs - 1)"""
    return synth.ba_problem(70 + k_obs, n_kf=n_kf, n_points=n_points, n_cuboids=0, k_obs=k_obs)


def chain30(n_cuboids=0):
    return synth.ba_problem(5, n_kf=30, n_points=500, n_cuboids=n_cuboids)


def chain14(n_cuboids=3):
    """14 key frames, landmarks seen by up to 10 of them (a short chain of synth.ba_problem starts nearly every landmark at key frame 0, so k_obs = 5 would
    leave key frames 5.. almost unobserved); of the three cuboids one is seen by key frames 0-7, one by 0-3 and one by none (point-cuboid edges only)"""
    return synth.ba_problem(11, n_kf=14, n_points=300, n_cuboids=n_cuboids, k_obs=10)


def _dead_cuboid():
    """cuboid 0 keeps two of its camera edges and both cameras are fixed: its Schur blocks are all dead, beside two live cuboids"""
    d = chain14()
    cams = np.unique(np.asarray(d["cobs_cam"])[np.asarray(d["cobs_cuboid"]) == 0])
    cams = cams[cams > 0][:2]
    assert len(cams) == 2
    return fix_cameras(cuboids_seen_only_by(d, cams, cuboids=[0]), cams)


def _starved():
    """every third landmark cut to one observation, every seventh to none"""
    d = chain14(0)
    pt = np.asarray(d["obs_point"])
    first = np.ones(len(pt), bool); first[1:] = pt[1:] != pt[:-1]  # landmark-major order: the first observation of each landmark
    keep = np.ones(len(pt), bool)
    keep[(pt % 3 == 0) & ~first] = False
    keep[pt % 7 == 0] = False
    return keep_observations(d, keep)


# name -> (builder, (C, Bc)); the builders are cheap, the tests call them once each
CASES = {
    **{"ladder_Bc%d" % (k - 1): ((lambda k=k: ladder(k)), (47, k - 1)) for k in (2, 4, 10, 11, 12, 17, 18, 21, 22)},
    "long_Bc20": (lambda: ladder(21, n_kf=127, n_points=2000), (126, 20)),          # C >= 6 * (Bc + 1): the two-sided chain, ba_band_mid at N = 120
    "cr_C36_Bc9": (lambda: ladder(10, n_kf=37, n_points=500), (36, 9)),             # C = 4 * Bc: the least nested dissection takes
    "cr_C35_Bc9": (lambda: ladder(10, n_kf=36, n_points=500), (35, 9)),             # C = 4 * Bc - 1: =cr falls to a band kernel
    # either side of C = 6 * (Bc + 1) = 30; the chain's last six key frames observe next to nothing and are fixed, so every free camera has observations
    "twist_C29_Bc4": (lambda: fix_cameras(synth.ba_problem(41, n_kf=36, n_points=500, n_cuboids=0), range(30, 36)), (29, 4)),
    "twist_C30_Bc4": (lambda: fix_cameras(synth.ba_problem(41, n_kf=37, n_points=500, n_cuboids=0), range(31, 37)), (30, 4)),
    "chain30": (chain30, (29, 4)),
    "chain30_scrambled": (lambda: permute_cameras(chain30(), 1)[0], (29, 26)),
    "chain30_cub4": (lambda: chain30(4), (29, 8)),
    "chain30_cub4_scrambled": (lambda: permute_cameras(chain30(4), 1)[0], (29, 26)),
    "chain30_loop": (lambda: add_loop_edges(chain30(), 25, (1, 2, 3), 2, last=5), (29, 22)),
    # every landmark seen by every key frame: the band is the whole matrix (C = Bc + 1, fewer columns than the LDS ring has slots)
    **{"tiny_kf%d" % n: ((lambda n=n: synth.ba_problem(50 + n, n_kf=n, n_points=120, n_cuboids=0, k_obs=n)), (n - 1, n - 2)) for n in (2, 3, 4, 7)},
    "fixed_mid": (lambda: fix_cameras(chain14(), [3, 4, 9]), (10, 6)),
    "one_free": (lambda: fix_cameras(chain14(), [i for i in range(14) if i != 6]), (1, 0)),
    "all_fixed_cuboids_only": (lambda: fix_cameras(chain14(), range(14)), (0, 0)),
    "dead_cuboid": (_dead_cuboid, (11, 9)),
    "starved_landmarks": (_starved, (13, 9)),
    "outliers": (lambda: with_outliers(chain14(0), 0.2, 40.0, 3), (13, 9)),
    "outliers_scrambled": (lambda: permute_cameras(with_outliers(chain14(0), 0.2, 40.0, 3), 4)[0], (13, 12)),
}
# metamorphic pairs: the second member is the first with its cameras relabelled (permutation seed)
PAIRS = {"chain30": ("chain30_scrambled", 1), "chain30_cub4": ("chain30_cub4_scrambled", 1), "outliers": ("outliers_scrambled", 4)}


def build(name):
    return CASES[name][0]()


def perm_of(name):
    """the permutation that made PAIRS[name]'s second member"""
    return np.random.default_rng(PAIRS[name][1]).permutation(len(build(name)["cam_pose"]))
