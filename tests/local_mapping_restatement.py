"""TEST INFRASTRUCTURE: the judge of the local-mapping tests.  LocalMapping::CreateNewMapPoints (orb_object_slam/src/LocalMapping.cc:319-570) restated literally in numpy scalars
-- the neighbours one after the other, skip1 (pKF1->GetMapPoint(idx1) != NULL) updated after every created point, every statement of :410-549 in the reference's float
arithmetic -- and MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (MapPoint.cc:381-446, :469-510).

np.float32 scalars are the reference's floats, Python floats its doubles; every conversion is written out (F(...) rounds to float, float(...) widens).  A cv::Mat product is one
gemm per row with double accumulation and one rounding; Mat::dot and cv::norm accumulate in double.  Two operations are the library's stated definitions, because
the reference's result depends on the OpenCV and libm it was built with:
  * cv::SVD::compute (:448) -> jacobi_vmin4: one-sided Jacobi in double, fixed sweep order and convergence test, + - * / sqrt only; compared against numpy.linalg.svd in
    tests/test_local_mapping_patterns.py;
  * cos(2 * atan2(mb / 2, depth)) (:431, :433) -> (d^2 - h^2) / (d^2 + h^2), h = mb / 2, in double, rounded once.
The same goes for the cv::MatExpr scale operations x3D / w, normali / cv::norm(normali) and normal / n: float(v_k * (1.0 / s))."""
import math

import numpy as np

F = np.float32

CREATED, PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE, CLAIMED, STEREO_NO_DEPTH = range(11)
STATUS_NAMES = ["created", "parallax", "w_zero", "z1", "z2", "reproj1", "reproj2", "zero_dist", "scale", "claimed", "stereo_no_depth"]

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

JACOBI_MAX_SWEEPS = 30
JACOBI_EPS = 8.8817841970012523e-16  # 2^-50


def jacobi_vmin4(A):
    """Right singular vector of the smallest singular value of the 4x4 A (rows of Python floats): Hestenes' one-sided Jacobi on the columns, pairs (0,1) (0,2) (0,3) (1,2) (1,3)
    (2,3) per sweep, a pair rotated unless |a_p . a_q| <= 2^-50 sqrt(|a_p|^2 |a_q|^2), until a sweep rotates nothing (at most 30); the smallest column norm, the first among equals."""
    W = [[float(A[r][c]) for c in range(4)] for r in range(4)]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(JACOBI_MAX_SWEEPS):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                alpha = beta = gamma = 0.0
                for r in range(4):
                    alpha += W[r][p] * W[r][p]
                    beta += W[r][q] * W[r][q]
                    gamma += W[r][p] * W[r][q]
                ag = -gamma if gamma < 0 else gamma
                if ag <= JACOBI_EPS * math.sqrt(alpha * beta):
                    continue
                rotated = True
                zeta = (beta - alpha) / (2.0 * gamma)
                az = -zeta if zeta < 0 else zeta
                t = (-1.0 if zeta < 0 else 1.0) / (az + math.sqrt(1.0 + zeta * zeta))
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = c * t
                for M in (W, V):
                    for r in range(4):
                        mp, mq = M[r][p], M[r][q]
                        M[r][p] = c * mp - s * mq
                        M[r][q] = s * mp + c * mq
        if not rotated:
            break
    best, nbest = 0, 0.0
    for k in range(4):
        n = 0.0
        for r in range(4):
            n += W[r][k] * W[r][k]
        if k == 0 or n < nbest:
            best, nbest = k, n
    return [V[r][best] for r in range(4)]


def dot64(a, b):
    s = 0.0
    for k in range(3):
        s += float(a[k]) * float(b[k])
    return s


def norm64(v):
    return math.sqrt(dot64(v, v))


def gemm3(R, p, t):
    """R * p + t: double accumulation over k ascending, one rounding (R: 9 floats row-major)."""
    o = []
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += float(R[r * 3 + k]) * float(p[k])
        o.append(F(s * 1.0 + float(t[r]) * 1.0))
    return o


def cos_stereo(mb, depth):
    h, d = float(mb) / 2.0, float(depth)
    return F((d * d - h * h) / (d * d + h * h))


class Frame:
    """The flat view of a KeyFrame (cs_lm_frame): keysUn (KEYPOINT_DTYPE), keys_xy (N, 2), u_right, depth, Rcw (9), tcw, Ow, the intrinsics, the level tables, mfScaleFactor."""

    def __init__(self, keysUn, keys_xy, u_right, depth, Rcw, tcw, Ow, fx, fy, cx, cy, mbf, mb, scale_factors, level_sigma2, scale_factor, invfx=None, invfy=None):
        self.keysUn = np.ascontiguousarray(keysUn, KEYPOINT_DTYPE)
        self.keys_xy = np.ascontiguousarray(keys_xy, np.float32).reshape(-1, 2)
        self.u_right = np.ascontiguousarray(u_right, np.float32)
        self.depth = np.ascontiguousarray(depth, np.float32)
        self.N = len(self.keysUn)
        self.Rcw = np.ascontiguousarray(Rcw, np.float32).reshape(9)
        self.tcw = np.ascontiguousarray(tcw, np.float32).reshape(3)
        self.Ow = np.ascontiguousarray(Ow, np.float32).reshape(3)
        self.fx, self.fy, self.cx, self.cy, self.mbf, self.mb = F(fx), F(fy), F(cx), F(cy), F(mbf), F(mb)
        self.invfx = F(1.0) / self.fx if invfx is None else F(invfx)  # invfx = 1.0f / fx (Frame.cc)
        self.invfy = F(1.0) / self.fy if invfy is None else F(invfy)
        self.scale_factors = np.ascontiguousarray(scale_factors, np.float32)
        self.level_sigma2 = np.ascontiguousarray(level_sigma2, np.float32)
        self.n_levels = len(self.scale_factors)
        self.scale_factor = F(scale_factor)
        self.Rwc = self.Rcw.reshape(3, 3).T.copy().reshape(9)  # Rcw.t(): a copy


def _reproj_fails(f, kp, ur, stereo, x3D, z, mbf):
    x = F(dot64(f.Rcw[0:3], x3D) + float(f.tcw[0]))
    y = F(dot64(f.Rcw[3:6], x3D) + float(f.tcw[1]))
    invz = F(1.0 / float(z))
    u = f.fx * x * invz + f.cx
    v = f.fy * y * invz + f.cy
    errX, errY = u - kp["x"], v - kp["y"]
    sigma2 = f.level_sigma2[kp["octave"]]
    if not stereo:
        return float(errX * errX + errY * errY) > 5.991 * float(sigma2)
    u_r = u - mbf * invz
    errX_r = u_r - ur
    return float(errX * errX + errY * errY + errX_r * errX_r) > 7.8 * float(sigma2)


def triangulate_pair(f1, idx1, f2, idx2, info=None):
    """:410-549 for one pair -> (status, x3D as three np.float32; 0 0 0 where the reference has none).  info (a dict) receives cosParallaxRays, the branch taken and A."""
    zero3 = [F(0), F(0), F(0)]
    with np.errstate(all="ignore"):
        ratioFactor = F(1.5) * f1.scale_factor
        kp1, kp2 = f1.keysUn[idx1], f2.keysUn[idx2]
        kp1_ur, kp2_ur = f1.u_right[idx1], f2.u_right[idx2]
        bStereo1, bStereo2 = bool(kp1_ur >= 0), bool(kp2_ur >= 0)
        xn1 = [(kp1["x"] - f1.cx) * f1.invfx, (kp1["y"] - f1.cy) * f1.invfy, F(1.0)]
        xn2 = [(kp2["x"] - f2.cx) * f2.invfx, (kp2["y"] - f2.cy) * f2.invfy, F(1.0)]
        ray1, ray2 = gemm3(f1.Rwc, xn1, zero3), gemm3(f2.Rwc, xn2, zero3)
        cosParallaxRays = F(dot64(ray1, ray2) / (norm64(ray1) * norm64(ray2)))
        cosParallaxStereo = cosParallaxRays + F(1)
        cosParallaxStereo1 = cosParallaxStereo2 = cosParallaxStereo
        if bStereo1:
            cosParallaxStereo1 = cos_stereo(f1.mb, f1.depth[idx1])
        elif bStereo2:
            cosParallaxStereo2 = cos_stereo(f2.mb, f2.depth[idx2])
        cosParallaxStereo = cosParallaxStereo2 if cosParallaxStereo2 < cosParallaxStereo1 else cosParallaxStereo1
        if info is not None:
            info.update(cosParallaxRays=cosParallaxRays, cosParallaxStereo=cosParallaxStereo, stereo=(bStereo1, bStereo2), branch=None)
        if cosParallaxRays < cosParallaxStereo and cosParallaxRays > 0 and (bStereo1 or bStereo2 or float(cosParallaxRays) < 0.9998):
            T1 = [[f1.Rcw[r * 3 + 0], f1.Rcw[r * 3 + 1], f1.Rcw[r * 3 + 2], f1.tcw[r]] for r in range(3)]
            T2 = [[f2.Rcw[r * 3 + 0], f2.Rcw[r * 3 + 1], f2.Rcw[r * 3 + 2], f2.tcw[r]] for r in range(3)]
            A = [[xn1[0] * T1[2][k] - T1[0][k] for k in range(4)], [xn1[1] * T1[2][k] - T1[1][k] for k in range(4)],
                 [xn2[0] * T2[2][k] - T2[0][k] for k in range(4)], [xn2[1] * T2[2][k] - T2[1][k] for k in range(4)]]
            x4 = [F(c) for c in jacobi_vmin4(A)]
            if info is not None:
                info.update(branch="svd", A=np.array(A, np.float32))
            if x4[3] == 0:
                return W_ZERO, zero3
            invw = 1.0 / float(x4[3])
            x3D = [F(float(x4[k]) * invw) for k in range(3)]
        elif bStereo1 and cosParallaxStereo1 < cosParallaxStereo2:
            if info is not None:
                info["branch"] = "stereo1"
            z = f1.depth[idx1]
            if not z > 0:
                return STEREO_NO_DEPTH, zero3
            u, v = f1.keys_xy[idx1]
            x3D = gemm3(f1.Rwc, [(u - f1.cx) * z * f1.invfx, (v - f1.cy) * z * f1.invfy, z], f1.Ow)
        elif bStereo2 and cosParallaxStereo2 < cosParallaxStereo1:
            if info is not None:
                info["branch"] = "stereo2"
            z = f2.depth[idx2]
            if not z > 0:
                return STEREO_NO_DEPTH, zero3
            u, v = f2.keys_xy[idx2]
            x3D = gemm3(f2.Rwc, [(u - f2.cx) * z * f2.invfx, (v - f2.cy) * z * f2.invfy, z], f2.Ow)
        else:
            return PARALLAX, zero3
        return _checks(f1, kp1, kp1_ur, bStereo1, f2, kp2, kp2_ur, bStereo2, x3D, ratioFactor), x3D


def _checks(f1, kp1, kp1_ur, bStereo1, f2, kp2, kp2_ur, bStereo2, x3D, ratioFactor):
    """:469-549 for a given x3D (also what tells whether a pair's status moves with x3D: marginal_pairs)."""
    with np.errstate(all="ignore"):
        z1 = F(dot64(f1.Rcw[6:9], x3D) + float(f1.tcw[2]))
        if z1 <= 0:
            return Z1
        z2 = F(dot64(f2.Rcw[6:9], x3D) + float(f2.tcw[2]))
        if z2 <= 0:
            return Z2
        if _reproj_fails(f1, kp1, kp1_ur, bStereo1, x3D, z1, f1.mbf):
            return REPROJ1
        if _reproj_fails(f2, kp2, kp2_ur, bStereo2, x3D, z2, f1.mbf):  # mpCurrentKeyFrame->mbf, :524
            return REPROJ2
        dist1 = F(norm64([x3D[k] - f1.Ow[k] for k in range(3)]))
        dist2 = F(norm64([x3D[k] - f2.Ow[k] for k in range(3)]))
        if dist1 == 0 or dist2 == 0:
            return ZERO_DIST
        ratioDist = dist2 / dist1
        ratioOctave = f1.scale_factors[kp1["octave"]] / f2.scale_factors[kp2["octave"]]
        if ratioDist * ratioFactor < ratioOctave or ratioDist > ratioOctave * ratioFactor:
            return SCALE
        return CREATED


def checks_at(f1, idx1, f2, idx2, x3D):
    x = [F(c) for c in x3D]
    return _checks(f1, f1.keysUn[idx1], f1.u_right[idx1], bool(f1.u_right[idx1] >= 0), f2, f2.keysUn[idx2], f2.u_right[idx2], bool(f2.u_right[idx2] >= 0), x, F(1.5) * f1.scale_factor)


def table_search(best2):
    """The stand-in for ORBmatcher(0.6, false).SearchForTriangulation: per neighbour a table of best matches, consulted with the skip1 of the moment of the call."""
    def search(n, skip1):
        return np.where(np.asarray(skip1, bool), -1, best2[n]).astype(np.int32)
    return search


def create_new_map_points(kf, neighbours, search, skip1):
    """The reference's loop (:349-569 without the baseline tests, which the caller has applied): neighbours in order, one search each with the skip1 of that moment, the pairs in
    idx1 order, skip1[idx1] set where a point is created (AddMapPoint).  Returns the created points [(neighbour, idx1, idx2, x3D)] in creation order and, per neighbour, the
    visited pairs [(idx1, idx2, status, x3D)]."""
    skip1 = np.array(skip1, bool)
    points, visited = [], []
    for n, f2 in enumerate(neighbours):
        m = search(n, skip1.copy())
        rows = []
        for idx1 in range(kf.N):
            idx2 = int(m[idx1])
            if idx2 < 0:
                continue
            st, x = triangulate_pair(kf, idx1, f2, idx2)
            rows.append((idx1, idx2, st, x))
            if st == CREATED:
                points.append((n, idx1, idx2, x))
                skip1[idx1] = True
        visited.append(rows)
    return points, visited


def expected_outputs(kf, neighbours, search, skip1):
    """What cs_create_new_map_points has to return for the searches made with the INITIAL skip1, derived from the sequential loop above: a pair the loop visited has the loop's
    status and x3D; a pair it never saw -- its idx1 had received a point from an earlier neighbour -- is CLAIMED, with the x3D its own triangulation gives."""
    points, visited = create_new_map_points(kf, neighbours, search, skip1)
    pair_off, idx1s, idx2s, xs, sts = [0], [], [], [], []
    new_pair = np.full(kf.N, -1, np.int32)
    matches12 = np.stack([search(n, np.array(skip1, bool)) for n in range(len(neighbours))]) if neighbours else np.zeros((0, kf.N), np.int32)
    for n, f2 in enumerate(neighbours):
        seen = {r[0]: r for r in visited[n]}
        for idx1 in range(kf.N):
            idx2 = int(matches12[n, idx1])
            if idx2 < 0:
                assert idx1 not in seen
                continue
            if idx1 in seen:
                assert seen[idx1][1] == idx2
                st, x = seen[idx1][2], seen[idx1][3]
                if st == CREATED:
                    new_pair[idx1] = len(sts)
            else:
                assert new_pair[idx1] >= 0  # the only reason the loop's search leaves out a pair of the initial search
                st, x = CLAIMED, triangulate_pair(kf, idx1, f2, idx2)[1]
            idx1s.append(idx1); idx2s.append(idx2); sts.append(st); xs.append(x)
        pair_off.append(len(sts))
    return {"matches12": matches12.astype(np.int32), "pair_off": np.array(pair_off, np.int32), "idx1": np.array(idx1s, np.int32), "idx2": np.array(idx2s, np.int32),
            "x3D": np.array(xs, np.float32).reshape(-1, 3), "status": np.array(sts, np.uint8), "new_pair_of_idx1": new_pair, "nnew": len(points), "points": points}


def factorised(kf, neighbours, search, skip1):
    """The three steps cs_create_new_map_points is built from: every neighbour searched with the initial skip1, every pair triangulated on its own, per idx1 the first accepted
    pair in neighbour order.  Returns the created points in the reference's creation order (pair order)."""
    skip1 = np.array(skip1, bool)
    pairs = []
    for n, f2 in enumerate(neighbours):
        m = search(n, skip1.copy())
        for idx1 in range(kf.N):
            if m[idx1] >= 0:
                pairs.append((n, idx1, int(m[idx1])) + triangulate_pair(kf, idx1, f2, int(m[idx1])))
    claimed, points = set(), []
    for n, idx1, idx2, st, x in pairs:  # (pairs are in neighbour order: the first accepted pair of an idx1 comes first)
        if st == CREATED and idx1 not in claimed:
            claimed.add(idx1)
            points.append((n, idx1, idx2, x))
    return points


# ---- MapPoint
def descriptor_distance(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def distinctive_descriptor(desc):
    """MapPoint::ComputeDistinctiveDescriptors :411-440 over the descriptors of the observations (N x 32 bytes, bad key frames left out): BestIdx, -1 for none."""
    N = len(desc)
    if N == 0:
        return -1
    D = [[0] * N for _ in range(N)]
    for i in range(N):
        for j in range(i + 1, N):
            D[i][j] = D[j][i] = descriptor_distance(desc[i], desc[j])
    BestMedian, BestIdx = 2 ** 31 - 1, 0
    for i in range(N):
        vDists = sorted(D[i])
        median = vDists[int(0.5 * (N - 1))]
        if median < BestMedian:
            BestMedian, BestIdx = median, i
    return BestIdx


def distinctive_descriptors(obs_off, desc):
    """The same for many points, with the distance matrix from numpy's bit counts (the per-point loop above is the definition; this is what large cases are judged by, and
    tests/test_local_mapping_patterns.py holds the two against each other)."""
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    out = np.full(len(obs_off) - 1, -1, np.int32)
    for p in range(len(obs_off) - 1):
        b = bits[obs_off[p]:obs_off[p + 1]]
        N = len(b)
        if N == 0:
            continue
        D = b @ (1 - b).T
        D = D + D.T
        med = np.sort(D, axis=1)[:, int(0.5 * (N - 1))]
        out[p] = int(np.argmin(med))  # the first minimum
    return out


def update_normal_and_depth(pos, obs, kf_Ow, ref_kf, ref_octave, scale_factors):
    """MapPoint::UpdateNormalAndDepth :487-509: (mNormalVector, mfMinDistance, mfMaxDistance), None for an empty run."""
    if len(obs) == 0:
        return None
    with np.errstate(all="ignore"):
        pos = [F(c) for c in pos]
        normal = [F(0), F(0), F(0)]
        n = 0
        for k in obs:
            normali = [pos[c] - F(kf_Ow[k][c]) for c in range(3)]
            inv = 1.0 / norm64(normali)
            normal = [normal[c] + F(float(normali[c]) * inv) for c in range(3)]
            n += 1
        PC = [pos[c] - F(kf_Ow[ref_kf][c]) for c in range(3)]
        dist = F(norm64(PC))
        maxd = dist * F(scale_factors[ref_octave])
        mind = maxd / F(scale_factors[len(scale_factors) - 1])
        invn = 1.0 / float(n)
        return [F(float(normal[c]) * invn) for c in range(3)], mind, maxd


def update_normal_and_depth_many(pos, obs_off, obs_kf, kf_Ow, ref_kf, ref_octave, scale_factors, normal, mind, maxd, updated):
    """The same for many points with numpy arrays: the points side by side, the observations of each still one after the other, every operation the scalar one above (numpy's
    elementwise float and double arithmetic is IEEE; tests/test_local_mapping_patterns.py holds the two against each other).  Fills the rows of non-empty runs."""
    pos = np.asarray(pos, np.float32); kf_Ow = np.asarray(kf_Ow, np.float32); sf = np.asarray(scale_factors, np.float32)
    cnt = np.diff(obs_off)
    acc = np.zeros((len(pos), 3), np.float32)

    def norm64_rows(v):
        d = v.astype(np.float64)
        return np.sqrt((0.0 + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])

    with np.errstate(all="ignore"):
        for j in range(int(cnt.max()) if len(cnt) else 0):
            rows = np.nonzero(cnt > j)[0]
            normali = pos[rows] - kf_Ow[obs_kf[obs_off[rows] + j]]
            inv = 1.0 / norm64_rows(normali)
            acc[rows] = acc[rows] + (normali.astype(np.float64) * inv[:, None]).astype(np.float32)
        rows = np.nonzero(cnt > 0)[0]
        dist = norm64_rows(pos[rows] - kf_Ow[ref_kf[rows]]).astype(np.float32)
        mx = dist * sf[ref_octave[rows]]
        maxd[rows] = mx
        mind[rows] = mx / sf[len(sf) - 1]
        normal[rows] = (acc[rows].astype(np.float64) * (1.0 / cnt[rows].astype(np.float64))[:, None]).astype(np.float32)
        updated[rows] = 1
    return normal, mind, maxd, updated


# ---- the distance of x3D from the reference's own float SVD and libm cosine (tests/test_local_mapping_restatement_pins.py measures it), and the pairs it makes undecidable
D_REF_X3D = 7.0  # the largest |x3D(reference) - x3D(restatement)| / x3d_scale over the created points of every pinned case; the pin test asserts 0.5 x this <= measured <= this
TOL_X3D = 10 * D_REF_X3D
D_COS = 6e-8     # the largest |cos_stereo(mb, depth) - cosf(2 * atan2f(mb / 2, depth))| over the stereo key points of every pinned case


def x3d_scale(A, x3D):
    """2^-24 * sigma_1 / (sigma_3 - sigma_4) * |x3D| with numpy's singular values of A: what one float rounding of A's entries moves the smallest singular vector by."""
    s = np.linalg.svd(np.asarray(A, np.float64), compute_uv=False)
    return 2.0 ** -24 * s[0] / (s[2] - s[3]) * float(np.linalg.norm(np.asarray(x3D, np.float64)))


def cos_stereo_libm(mb, depth):
    """:431 / :433 as the reference's text reads with float overloads: cosf(2 * atan2f(mb / 2, depth))."""
    return F(np.cos(F(2) * np.arctan2(F(mb) / F(2), F(depth), dtype=np.float32), dtype=np.float32))


def marginal_pairs(kf, neighbours, matches12):
    """Per (neighbour, idx1) of matches12: True where the reference, with its float SVD and libm cosine, may decide the pair otherwise than the restatement -- the status changes
    when x3D is moved by TOL_X3D * x3d_scale along any axis (triangulated pairs), or cosParallaxRays lies within D_COS of cosParallaxStereo (stereo pairs: the branch may differ)."""
    out = {}
    for n, f2 in enumerate(neighbours):
        for idx1 in range(kf.N):
            idx2 = int(matches12[n][idx1])
            if idx2 < 0:
                continue
            info = {}
            st, x = triangulate_pair(kf, idx1, f2, idx2, info)
            m = False
            if (info["stereo"][0] or info["stereo"][1]) and abs(float(info["cosParallaxRays"]) - float(info["cosParallaxStereo"])) <= D_COS:
                m = True
            if info["branch"] == "svd" and st not in (W_ZERO,):
                step = TOL_X3D * x3d_scale(info["A"], x)
                for axis in range(3):
                    for sign in (-1.0, 1.0):
                        y = [float(c) for c in x]
                        y[axis] += sign * step
                        if checks_at(kf, idx1, f2, idx2, y) != st:
                            m = True
            out[(n, idx1)] = m
    return out


def reference_available():
    import os
    return os.path.isdir("/root/reference")


def build_reference_loop(directory):
    """LocalMapping::CreateNewMapPoints (:319-570, up to the line that prints nnew) and KeyFrame::UnprojectStereo cut out of the reference into `directory` and compiled there
    around tests/cpp/ref_local_mapping_loop_standins.cpp.  Nothing is written inside the repository."""
    import ctypes as C
    import os
    import subprocess
    from tests.test_sim3_restatement_pins import _cut
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t = open("/root/reference/orb_object_slam/src/LocalMapping.cc").read()
    a = t.index("void LocalMapping::CreateNewMapPoints()")
    b = t.index("\n", t.index("New Triangulated pt num", a))
    k = open("/root/reference/orb_object_slam/src/KeyFrame.cc").read()
    with open(os.path.join(str(directory), "ref_local_mapping_loop_extracted.inc"), "w") as f:
        f.write(t[a:b] + "\n}\n\n" + _cut(k, "cv::Mat KeyFrame::UnprojectStereo(int i)") + "\n")
    so = os.path.join(str(directory), "libref_local_mapping_loop.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-I" + str(directory), "-o", so,
                           os.path.join(root, "tests", "cpp", "ref_local_mapping_loop_standins.cpp")])
    return C.CDLL(so)


def run_reference_loop(lib, kf, neighbours, best2, skip1, monocular=False, median_depths=None):
    """-> (the pairs the reference's searches returned [(neighbour, idx1, idx2)], the created points [(neighbour, idx1, idx2, x3D)] in creation order).
    monocular with median depths of 0 (the default here) makes the baseline test :356-372 keep every neighbour; monocular=False is the reference's test against pKF2->mb."""
    import ctypes as C

    class FrameIn(C.Structure):
        _fields_ = [("N", C.c_int)] + [(k, C.c_void_p) for k in ("ux", "uy", "kx", "ky", "ur", "depth", "octave", "pose", "cam")] + [("n_levels", C.c_int), ("sf", C.c_void_p),
                                                                                                                                  ("sigma2", C.c_void_p), ("scale_factor", C.c_float)]
    keep = []

    def ptr(a, dt):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data

    def frame(f):
        return FrameIn(f.N, ptr(f.keysUn["x"], np.float32), ptr(f.keysUn["y"], np.float32), ptr(f.keys_xy[:, 0], np.float32), ptr(f.keys_xy[:, 1], np.float32), ptr(f.u_right, np.float32),
                       ptr(f.depth, np.float32), ptr(f.keysUn["octave"], np.int32), ptr(np.concatenate([f.Rcw, f.tcw, f.Ow]), np.float32),
                       ptr([f.fx, f.fy, f.cx, f.cy, f.invfx, f.invfy, f.mbf, f.mb], np.float32), f.n_levels, ptr(f.scale_factors, np.float32), ptr(f.level_sigma2, np.float32),
                       float(f.scale_factor))
    n = len(neighbours)
    cur = frame(kf)
    arr = (FrameIn * max(n, 1))(*[frame(f) for f in neighbours])
    b2 = np.ascontiguousarray(np.stack(best2) if n else np.zeros((0, kf.N)), np.int32)
    sk = np.ascontiguousarray(skip1, np.uint8)
    md = np.ascontiguousarray(np.zeros(max(n, 1)) if median_depths is None else median_depths, np.float32)
    cap = max(n * kf.N, 1)
    n_pairs = C.c_int(); pairs3 = np.zeros((cap, 3), np.int32); new3 = np.zeros((max(kf.N, 1), 3), np.int32); newx = np.zeros((max(kf.N, 1), 3), np.float32)
    nnew = lib.pin_create_new_map_points(C.byref(cur), arr, n, int(monocular), md.ctypes.data_as(C.c_void_p), sk.ctypes.data_as(C.c_void_p), b2.ctypes.data_as(C.c_void_p), C.byref(n_pairs),
                                         pairs3.ctypes.data_as(C.c_void_p), new3.ctypes.data_as(C.c_void_p), newx.ctypes.data_as(C.c_void_p))
    return [tuple(int(v) for v in r) for r in pairs3[:n_pairs.value]], [(int(a), int(b), int(c), x.copy()) for (a, b, c), x in zip(new3[:nnew], newx[:nnew])]
