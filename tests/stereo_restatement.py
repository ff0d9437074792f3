"""Checker of the stereo association: a plain numpy restatement of ORB_SLAM2::Frame::ComputeStereoMatches (reference
orb_object_slam/src/Frame.cc:611-783), a direct loop with np.float32 at every float operation, and the generator of the synthetic rectified
pairs the stereo tests use.  A helper, not a test module; it reads nothing but its arguments.

What the reference leaves undefined ends here, as in the device code, as "unmatched": a left key point whose (int)y is outside [0, rows), a
right key point whose row span leaves [0, rows) or whose octave is not a level (it is entered nowhere), a patch / strip that leaves its level
image, and zero accepted matches.  None of it occurs for key points that come from the extractor."""
import math

import numpy as np

from cube_slam_amd import synth

f32 = np.float32
TH_HIGH = 100  # ORBmatcher.cc:42
BF = 386.1448  # the KITTI 00-02 calibration the tests use: Camera.bf, Camera.fx
FX = 718.856


def scale_tables(scaleFactor, nlevels):
    """mvScaleFactor / mvInvScaleFactor of the extractor's constructor (ORBextractor.cc:412-426): a running float product, not scaleFactor ** l."""
    sf = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        sf[i] = f32(sf[i - 1] * f32(scaleFactor))
    return sf, (f32(1) / sf).astype(f32)


def c_round(x):
    """C round() on a float: half away from zero."""
    x = float(x)
    return math.floor(x + 0.5) if x >= 0 else math.ceil(x - 0.5)


def compute_stereo_matches(kl, dl, kr, dr, pyrL, pyrR, sf, isf, bf, b, stats=None):
    """(mvuRight, mvDepth, n_matched).  kl / kr: key points (fields x, y, octave) in mvKeys order, dl / dr: their 32-byte descriptors,
    pyrL / pyrR: mvImagePyramid of both extractors, sf / isf: mvScaleFactors / mvInvScaleFactors, bf / b: mbf / mb."""
    N, Nr = len(kl), len(kr)
    sf = np.asarray(sf, f32)
    isf = np.asarray(isf, f32)
    bf, b = f32(bf), f32(b)
    uR = np.full(N, -1, f32)  # :613-614
    dep = np.full(N, -1, f32)
    st = {} if stats is None else stats  # how often each exit was taken
    st.update(cand=0, hamming=0, column_exit=0, edge_shift=0, parabola=0, disparity=0, clamp=0)
    # ... and the guarded exits (what the reference leaves undefined), the winner of every Hamming search as (iL, iR, distance, candidates), the (iL, SAD) pairs accepted
    # before the cut, and the median
    st.update(left_row=0, max_u=0, right_span=0, right_octave=0, left_octave=0, patch=0, empty=0, best=[], sad=[], median=None)
    nRows = pyrL[0].shape[0]  # :616
    nlevels = len(pyrL)
    rows = [[] for _ in range(nRows)]  # :619-636
    for iR in range(Nr):
        octv = int(kr["octave"][iR])
        if octv < 0 or octv >= nlevels:
            st["right_octave"] += 1
            continue
        kpY = f32(kr["y"][iR])
        r = f32(f32(2) * sf[octv])
        maxr = int(math.ceil(f32(kpY + r)))
        minr = int(math.floor(f32(kpY - r)))
        if minr < 0 or maxr >= nRows:
            st["right_span"] += 1
            continue
        for yi in range(minr, maxr + 1):
            rows[yi].append(iR)
    minD = f32(-3)  # :639-641
    maxD = f32(bf / b)
    krx, kro = kr["x"].astype(f32), kr["octave"].astype(np.int64)
    vDistIdx = []
    w, L = 5, 5
    for iL in range(N):  # :647
        levelL = int(kl["octave"][iL])
        vL, uL = f32(kl["y"][iL]), f32(kl["x"][iL])
        if not (vL >= 0 and vL < nRows):
            st["left_row"] += 1
            continue
        cand = rows[int(vL)]  # :654
        if not cand:
            continue
        minU = f32(uL - maxD)  # :659-660
        maxU = f32(uL - minD)
        if maxU < 0:
            st["max_u"] += 1
            continue
        c = np.asarray(cand)
        c = c[(kro[c] >= levelL - 1) & (kro[c] <= levelL + 1) & (krx[c] >= minU) & (krx[c] <= maxU)]  # :676, :681
        if len(c) == 0:
            continue
        st["cand"] += len(c)
        d = np.unpackbits(dr[c] ^ dl[iL][None, :], axis=1).sum(1)  # DescriptorDistance
        j = int(np.argmin(d))  # strict < over increasing iR (:686): the first minimum
        if d[j] >= TH_HIGH:  # :695
            continue
        st["hamming"] += 1
        st["best"].append((iL, int(c[j]), int(d[j]), len(c)))
        if levelL < 0 or levelL >= nlevels:
            st["left_octave"] += 1
            continue
        uR0 = krx[c[j]]
        s = isf[levelL]
        su, sv, sr = int(c_round(f32(uL * s))), int(c_round(f32(vL * s))), int(c_round(f32(uR0 * s)))  # :699-701
        imL, imR = pyrL[levelL], pyrR[levelL]
        h, wd = imL.shape
        if sv - w < 0 or sv + w >= h or su - w < 0 or su + w >= wd or sr - w - L < 0 or sr + w + L >= wd:
            st["patch"] += 1
            continue  # cv::Mat range checks in the reference
        IL = imL[sv - w:sv + w + 1, su - w:su + w + 1].astype(np.int32)  # :706-708
        IL = IL - IL[w, w]
        if sr + L - w < 0 or sr + L + w + 1 >= imR.shape[1]:  # :716-719
            st["column_exit"] += 1
            continue
        best, binc = 2 ** 31 - 1, 0
        vDists = np.zeros(2 * L + 1, f32)
        for inc in range(-L, L + 1):  # :721-735
            IR = imR[sv - w:sv + w + 1, sr + inc - w:sr + inc + w + 1].astype(np.int32)
            IR = IR - IR[w, w]
            dist = int(np.abs(IL - IR).sum())  # integers <= 121 * 510: exact in the reference's float sums too
            if dist < best:
                best, binc = dist, inc
            vDists[L + inc] = dist
        if binc == -L or binc == L:  # :737
            st["edge_shift"] += 1
            continue
        d1, d2, d3 = vDists[L + binc - 1], vDists[L + binc], vDists[L + binc + 1]
        with np.errstate(all="ignore"):
            deltaR = f32(f32(d1 - d3) / f32(f32(2) * f32(f32(d1 + d3) - f32(f32(2) * d2))))  # :745
        # Kept as written, but never taken: d2 is the strict first minimum of integer sums, so d1 > d2 and d3 >= d2; the denominator is >= 2 and
        # |d1 - d3| <= d1 + d3 - 2 * d2, every term exact in float (below 2^24), so |deltaR| <= 0.5 and neither NaN nor inf can arise.
        if deltaR < -1 or deltaR > 1:
            st["parabola"] += 1
            continue
        bestuR = f32(sf[levelL] * f32(f32(f32(sr) + f32(binc)) + deltaR))  # :751
        disparity = f32(uL - bestuR)
        if disparity >= 0 and disparity < maxD:  # :755
            if disparity <= 0:
                disparity = f32(0.01)
                bestuR = f32(float(uL) - 0.01)  # a double subtraction, as written at :760
                st["clamp"] += 1
            dep[iL] = f32(bf / disparity)
            uR[iL] = bestuR
            vDistIdx.append((best, iL))
        else:
            st["disparity"] += 1
    vDistIdx.sort()  # :769
    st["accepted"] = len(vDistIdx)
    st["sad"] = sorted((i, dist) for dist, i in vDistIdx)
    if N > 0 and not vDistIdx:
        st["empty"] += 1
    kept = 0
    if vDistIdx:
        median = f32(vDistIdx[len(vDistIdx) // 2][0])
        st["median"] = int(median)
        thDist = f32(f32(f32(1.5) * f32(1.4)) * median)
        kept = len(vDistIdx)
        for dist, i in reversed(vDistIdx):  # :773-782
            if f32(dist) < thDist:
                break
            uR[i] = -1
            dep[i] = -1
            kept -= 1
    st["kept"] = kept
    return uR, dep, kept


def pair(seed, W, H, disps, noise=2.0):
    """(left, right, truth): synth._texture_base(seed, W, H) cut at column 200 for the left image and at 200 + d for the right one (linear interpolation
    for a fractional d) in len(disps) horizontal bands of constant disparity d, Gaussian noise added to both before rounding.  truth[row] = d."""
    base = synth._texture_base(seed, W, H).astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    s = 200
    left = base[:, s:s + W].copy()
    right = np.zeros_like(left)
    band = H // len(disps)
    truth = np.zeros(H, np.float32)
    for k, d in enumerate(disps):
        r0, r1 = k * band, (H if k == len(disps) - 1 else (k + 1) * band)
        i = int(math.floor(d))
        fr = d - i
        right[r0:r1] = (1 - fr) * base[r0:r1, s + i:s + i + W] + fr * base[r0:r1, s + i + 1:s + i + 1 + W]
        truth[r0:r1] = d
    left += rng.normal(0, noise, left.shape)
    right += rng.normal(0, noise, right.shape)

    def q(a):
        return np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return q(left), q(right), truth


FIXED_BANDS = [3.0, 12.5, 40.25, 97.75]


def batch_bands(seed):
    """The four bands of pair `seed` of the 64-pair batch."""
    return [float(x) for x in np.random.default_rng(seed).uniform(2, 120, 4)]


def disparity_error(kl, uR, truth):
    """|(uL - u_right) - d(row)| of the matched key points."""
    m = uR >= 0
    return np.abs((kl["x"][m] - uR[m]) - truth[kl["y"][m].astype(int)])
