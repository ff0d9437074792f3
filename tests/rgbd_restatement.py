"""An independent numpy statement of the RGB-D frame and of the close-point rule, written from the reference's lines (orb_object_slam/src/Frame.cc:334-344, :546-576,
:785-822; src/Tracking.cc:388, :804-819, :1221-1273, :2075-2128), and the input generators of the RGB-D tests.  Scalar loops with numpy float32 / Python float (= double)
arithmetic, one operation at a time; the walk is the reference's loop, not a closed form."""
import math

import numpy as np

from cube_slam_amd.orb import KEYPOINT_DTYPE

f32 = np.float32
NEAREST, ALL = 0, 1
# TUM1.yaml: Camera.fx fy cx cy, k1 k2 p1 p2 k3, Camera.bf, ThDepth, DepthMapFactor
K4 = np.array([517.306408, 516.469215, 318.643040, 255.313989], f32)
DIST5 = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], f32)
BF = 40.0
TH_DEPTH = float(f32(BF) * f32(40.0) / K4[0])  # mThDepth = mbf * ThDepth / fx (Tracking.cc:216)
FACTOR = float(f32(1.0) / f32(5000.0))          # mDepthMapFactor = 1.0f / DepthMapFactor (Tracking.cc:223-227)


def small_K4(W, H):
    """TUM1's intrinsics scaled to a W x H image, so that the distortion model bends a small test image as it bends 640 x 480."""
    return np.array([K4[0] * W / 640, K4[1] * H / 480, K4[2] * W / 640, K4[3] * H / 480], f32)


def undistort_keypoints(keys, K4, dist5):
    """Frame::UndistortKeyPoints (Frame.cc:546-576): a copy when mDistCoef.at<float>(0) == 0, else cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) in its
    classic form: five fixed-point iterations in double, re-projection with P = K, rounding to float."""
    out = np.array(keys, KEYPOINT_DTYPE)
    if dist5 is None or dist5[0] == 0:
        return out
    fx, fy, cx, cy = (float(v) for v in K4)
    k1, k2, p1, p2, k3 = (float(v) for v in dist5)
    ifx, ify = 1.0 / fx, 1.0 / fy
    for i in range(len(out)):
        x = (float(keys["x"][i]) - cx) * ifx
        y = (float(keys["y"][i]) - cy) * ify
        x0, y0 = x, y
        for _ in range(5):
            r2 = x * x + y * y
            icdist = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            x = (x0 - dx) * icdist
            y = (y0 - dy) * icdist
        out["x"][i] = f32(fx * x + cx)
        out["y"][i] = f32(fy * y + cy)
    return out


def convert_sample(raw, factor):
    """What imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (Tracking.cc:388) leaves in one pixel: (float)raw * factor, one float multiply."""
    with np.errstate(all="ignore"):
        return f32(f32(raw) * f32(factor))


def compute_stereo_from_rgbd(im_raw, factor, keys, keysUn, bf):
    """Frame::ComputeStereoFromRGBD (Frame.cc:785-806) on the raw image: (mvuRight, mvDepth, n_with_depth, n_outside).  at<float>(v, u) with float arguments truncates
    both toward zero; a sample outside the Mat (undefined in the reference) leaves the key point without depth and is counted."""
    H, W = im_raw.shape
    N = len(keys)
    mvuRight, mvDepth = np.full(N, -1, f32), np.full(N, -1, f32)
    n_with, n_out = 0, 0
    for i in range(N):
        u, v = float(keys["x"][i]), float(keys["y"][i])
        if math.isnan(u) or math.isnan(v) or not (0 <= int(u) < W and 0 <= int(v) < H):
            n_out += 1
            continue
        d = convert_sample(im_raw[int(v), int(u)], factor)
        if d > 0:
            with np.errstate(all="ignore"):
                mvDepth[i] = d
                mvuRight[i] = f32(keysUn["x"][i]) - f32(bf) / d
            n_with += 1
    return mvuRight, mvDepth, n_with, n_out


def update_pose_matrices(Tcw):
    """Frame::UpdatePoseMatrices (Frame.cc:334-344): mRwc = mRcw.t(); mOw = -mRcw.t() * mtcw is one gemm with alpha = -1: double accumulation, one rounding."""
    Tcw = np.asarray(Tcw, f32).reshape(3, 4)
    Rwc = Tcw[:, :3].T.copy()
    Ow = np.zeros(3, f32)
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += float(Tcw[k, r]) * float(Tcw[k, 3])
        Ow[r] = f32(-s)
    return Rwc, Ow


def unproject_stereo(u, v, z, K4, Rwc, Ow):
    """Frame::UnprojectStereo (Frame.cc:808-822) for z > 0, u / v of mvKeysUn."""
    with np.errstate(all="ignore"):
        invfx, invfy = f32(1.0) / f32(K4[0]), f32(1.0) / f32(K4[1])
        xc = [(f32(u) - f32(K4[2])) * f32(z) * invfx, (f32(v) - f32(K4[3])) * f32(z) * invfy, f32(z)]
        out = np.zeros(3, f32)
        for r in range(3):
            s = 0.0
            for k in range(3):
                s += float(Rwc[r, k]) * float(xc[k])
            out[r] = f32(s + float(Ow[r]))
    return out


def walk(sorted_depths, th_depth):
    """The loop of Tracking.cc:1241-1273 / :2092-2128 over the sorted depths with its counters only: nPoints when it ends."""
    nPoints = 0
    for z in sorted_depths:
        nPoints += 1
        if z > th_depth and nPoints > 100:
            break
    return nPoints


def closed_form(n_valid, c):
    """nPoints without the loop: c = the sorted entries that are not beyond mThDepth."""
    return min(n_valid, max(c, 100) + 1)


def close_points(depth, keysUn, need_new, Tcw, K4, th_depth, mode):
    """The stereo / RGB-D block of UpdateLastFrame and CreateNewKeyFrame (mode NEAREST) or the loop of StereoInitialization (:804-819, mode ALL) for one frame."""
    Rwc, Ow = update_pose_matrices(Tcw)
    vDepthIdx = [(float(depth[i]), i) for i in range(len(depth)) if depth[i] > 0]
    if mode == NEAREST:
        vDepthIdx.sort()
    new_idx, new_x3D, nPoints = [], [], 0
    for z, i in vDepthIdx:
        if mode == ALL or need_new[i]:
            new_idx.append(i)
            new_x3D.append(unproject_stereo(keysUn["x"][i], keysUn["y"][i], depth[i], K4, Rwc, Ow))
        nPoints += 1
        if mode == NEAREST and z > th_depth and nPoints > 100:
            break
    return {"n_valid": len(vDepthIdx), "order": np.array([i for _, i in vDepthIdx], np.int32), "n_walked": nPoints, "new_idx": np.array(new_idx, np.int32),
            "new_x3D": np.array(new_x3D, f32).reshape(-1, 3)}


# ---- generators ----------------------------------------------------------------------------------------------------------------------------------------

HOLE_RATE = 0.25


def depth_image(seed, W, H, dtype):
    """A raw depth image with a quarter of its pixels empty: uint16 in the sensor's units (0.4 - 8 m at 1 / 5000) or float32 metres."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(2000, 40000, (H, W)).astype(np.uint16)
    raw[rng.random((H, W)) < HOLE_RATE] = 0
    return raw if dtype == np.uint16 else (raw.astype(f32) * f32(FACTOR)).astype(f32)


def keypoints(seed, n, W, H):
    """n key points with float coordinates inside the image, the other fields as an extractor would fill them."""
    rng = np.random.default_rng(seed)
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"] = rng.uniform(0, W - 0.01, n).astype(f32)
    k["y"] = rng.uniform(0, H - 0.01, n).astype(f32)
    k["size"], k["angle"], k["response"], k["octave"], k["class_id"] = 31.0, rng.uniform(0, 360, n), rng.uniform(20, 200, n), rng.integers(0, 8, n), -1
    return k


FRAME_SIZES = [64, 0, 257, 1, 63, 65]  # an empty frame between two full ones


def edge_keypoints(W, H):
    """The four corners, the last column's far end, one column outside, a row that truncates to 0 from below, NaN coordinates, rows / columns outside."""
    xy = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W - 1 + 0.999, 5), (W, 5), (7, -0.5), (-0.5, -0.999), (float("nan"), 3), (3, float("nan")), (-1.0, 3), (3, H),
          (3, -1.0), (1e9, 3), (3, -1e9), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0)]
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    k["x"], k["y"] = [p[0] for p in xy], [p[1] for p in xy]
    k["class_id"] = -1
    return k


def edge_image(W, H, dtype):
    """The image that goes with edge_keypoints: every pixel valid but for row 0, columns 1 - 5, which hold 0, NaN, +inf, 1, 65535 (uint16: 0, 0, 65535, 1, 65535)."""
    im = np.full((H, W), 5000 if dtype == np.uint16 else 1.5, dtype)
    im[0, 1:6] = [0, 0, 65535, 1, 65535] if dtype == np.uint16 else [0, np.nan, np.inf, 1, 65535]
    return im


def poses(n):
    """n poses [3, 4]: rotations about a slanted axis with a translation; every fourth is scaled and sheared (not orthonormal)."""
    out = np.zeros((n, 3, 4), f32)
    for f in range(n):
        a = 0.1 + 0.37 * f
        ax = np.array([0.3, -0.5 + 0.01 * f, 0.8])
        ax /= np.linalg.norm(ax)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * Kx @ Kx
        if f % 4 == 3:
            R = R @ np.array([[1.3, 0.2, 0], [0, 0.7, -0.1], [0.05, 0, 1.1]])
        out[f, :, :3] = R
        out[f, :, 3] = [0.5 * f - 1.0, 0.25, -0.125 * f]
    return out


def close_case(seed, n_valid, c, th_depth, kind="float"):
    """mvDepth of one frame: n_valid key points with z > 0 of which c are not beyond th_depth, between them n_valid // 3 + 2 without depth (-1, 0 or NaN), shuffled.
    kind: "float" (distinct), "u16" (raw * 1 / 5000 from a few raw values: heavy in ties), "equal" (all 1.0), "inf" (the far ones are +inf), "at_th" (the close ones sit
    exactly on th_depth)."""
    rng = np.random.default_rng(seed)
    th = f32(th_depth)
    if kind == "u16":
        lim = int(th / f32(FACTOR))
        near = rng.integers(max(lim - 40, 1), lim - 1, c).astype(f32) * f32(FACTOR)
        far = rng.integers(lim + 2, lim + 42, n_valid - c).astype(f32) * f32(FACTOR)
    elif kind == "equal":
        near, far = np.full(c, 1.0, f32), np.full(n_valid - c, 1.0, f32)
    else:
        near = rng.uniform(0.3, 0.999 * th, c).astype(f32)
        far = rng.uniform(1.001 * th, 3 * th, n_valid - c).astype(f32)
        if kind == "inf":
            far[:] = np.inf
        if kind == "at_th":
            near[:] = th
    junk = rng.choice(np.array([-1.0, 0.0, np.nan], f32), n_valid // 3 + 2)
    z = np.concatenate([near, far, junk]).astype(f32)
    rng.shuffle(z)
    return z


def need_new_pattern(which, n):
    return [np.zeros(n, np.uint8), np.ones(n, np.uint8), (np.arange(n) % 2).astype(np.uint8)][which % 3]


N_VALID = [0, 1, 2, 63, 64, 65, 99, 100, 101, 102, 127, 128, 129, 1000]


def close_cases(capacity, th_depth=TH_DEPTH):
    """The frames of one close-point call: [(name, depth)] over N_VALID and the capacity x c in {0, 99, 100, 101, n_valid}, then the special depth kinds.  (All depths equal AND beyond the
    threshold needs a call of its own with th_depth below 1.)"""
    out, seed = [], 1
    for n in N_VALID + [capacity]:
        for c in sorted({min(c, n) for c in (0, 99, 100, 101, n)}):
            nj = n // 3 + 2
            z = close_case(seed, n, c, th_depth)
            if n == capacity:  # the frame is exactly as long as the handle allows: no key point without depth
                z = z[z > 0]
            assert len(z) == (n if n == capacity else n + nj)
            out.append(("n%d_c%d" % (n, c), z))
            seed += 1
    for kind, n, c in (("equal", 150, 150), ("equal", 90, 90), ("u16", 400, 130), ("u16", 129, 60), ("at_th", 140, 120), ("at_th", 101, 101), ("inf", 130, 40), ("inf", 120, 0)):
        out.append(("%s_n%d_c%d" % (kind, n, c), close_case(seed, n, c, th_depth, kind)))
        seed += 1
    return out


# ---- the C++ mirror's driver (tests/cpp/rgbd_mirror.cpp) -----------------------------------------------------------------------------------------------

def mirror_frames():
    """[dict] of the frames the C++ driver runs: a strided uint16 image, the edge cases in float32, a tie-heavy frame with one key point per pixel, an empty frame."""
    W, H = 64, 48
    K, T = small_K4(W, H), poses(4)
    frames = []
    wide = np.full((H, 80), 777, np.uint16)
    wide[:, :W] = depth_image(3, W, H, np.uint16)
    k = keypoints(262, 257, W, H)
    frames.append(dict(image=wide[:, :W], factor=FACTOR, keys=k, keysUn=undistort_keypoints(k, K, DIST5), need_new=need_new_pattern(2, 257), mode=NEAREST, th=2.0))
    k = edge_keypoints(W, H)
    frames.append(dict(image=edge_image(W, H, f32), factor=1.0, keys=k, keysUn=undistort_keypoints(k, K, DIST5), need_new=need_new_pattern(1, len(k)), mode=ALL, th=TH_DEPTH))
    z = close_case(11, 400, 130, TH_DEPTH, "u16")
    im = np.zeros((H, W), f32)
    im.flat[:len(z)] = z
    k = np.zeros(len(z), KEYPOINT_DTYPE)
    k["x"], k["y"] = np.arange(len(z)) % W + 0.25, np.arange(len(z)) // W + 0.5
    frames.append(dict(image=im, factor=1.0, keys=k, keysUn=keypoints(12, len(z), W, H), need_new=need_new_pattern(2, len(z)), mode=NEAREST, th=TH_DEPTH))
    frames.append(dict(image=np.zeros((H, W), np.uint16), factor=FACTOR, keys=k[:0], keysUn=k[:0], need_new=np.zeros(0, np.uint8), mode=NEAREST, th=TH_DEPTH))
    for f, fr in enumerate(frames):
        fr.update(K4=K, Tcw=T[f], bf=BF)
    return frames


def write_mirror_input(path, frames):
    with open(path, "wb") as fh:
        fh.write(np.int32(len(frames)).tobytes())
        for fr in frames:
            im = fr["image"]
            H, W = im.shape
            fh.write(np.array([0 if im.dtype == np.uint16 else 1, W, H, im.strides[0], fr["mode"], len(fr["keys"])], np.int32).tobytes())
            fh.write(np.concatenate([[fr["factor"], fr["bf"], fr["th"]], fr["K4"], np.asarray(fr["Tcw"]).ravel()]).astype(f32).tobytes())
            rows = np.zeros((H, im.strides[0]), np.uint8)  # the rows with their padding
            rows[:, :W * im.itemsize] = np.ascontiguousarray(im).view(np.uint8).reshape(H, -1)
            fh.write(rows.tobytes())
            fh.write(np.ascontiguousarray(fr["keys"]).tobytes() + np.ascontiguousarray(fr["keysUn"]).tobytes() + np.ascontiguousarray(fr["need_new"], np.uint8).tobytes())


def read_mirror_output(path, frames):
    """Per frame (mvuRight, mvDepth, (n_with_depth, n_outside), the close-point dict, UnprojectStereo of every created point)."""
    raw = open(path, "rb").read()
    at, out = 0, []

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(raw, dtype, n, at)
        at += a.nbytes
        return a.copy()
    for fr in frames:
        N = len(fr["keys"])
        n_with, n_out = take(np.int32, 2)
        ur, dep = take(f32, N), take(f32, N)
        n_valid, n_walked, n_new = take(np.int32, 3)
        r = {"n_valid": int(n_valid), "n_walked": int(n_walked), "order": take(np.int32, n_valid), "new_idx": take(np.int32, n_new), "new_x3D": take(f32, 3 * n_new).reshape(-1, 3)}
        out.append((ur, dep, (int(n_with), int(n_out)), r, take(f32, 3 * n_new).reshape(-1, 3)))
    assert at == len(raw)
    return out
