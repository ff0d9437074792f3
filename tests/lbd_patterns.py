"""Inputs that put the LBD path (cube_slam_amd/csrc/lbd.hip) where a test wants it: frames whose size crosses a seam of lbd_blur5 / lbd_sobel, images that show a
shifted column or a missed clamp in every pixel, KeyLines that LSD never produces, and descriptor sets for the line matcher.  A helper, not a test module; it reads
nothing but its arguments and every generator is seeded.  tests/test_lbd_patterns.py proves on the CPU oracle that the inputs are what they claim to be.

The seams.  One wave of lbd_blur5 / lbd_sobel owns a strip of STRIP = 256 columns and a block of ROWS = 64 rows, every lane four columns; the right halo of a strip
comes from extra lanes, rows are fetched in groups of four, and the Sobel result leaves as one 16-byte store only where the pixel index is a multiple of four."""
import numpy as np

from cube_slam_amd import synth
from cube_slam_amd.lsd import KEYLINE_DTYPE

f32 = np.float32
STRIP, ROWS = 256, 64

# ----------------------------------------------------------------------------------------------- images


def texture(seed, W, H):
    return synth.texture_image(seed, W, H)


def saturated(W, H):
    """255 everywhere but for isolated zeros: the fixed-point blur has gain 257^2 / 65536, so a white neighbourhood reaches 257 before the clamp at 255."""
    img = np.full((H, W), 255, np.uint8)
    img[::7, ::5] = 0
    return img


def byte_pattern(W, H):
    """(7 x + 13 y) & 255: no two neighbouring columns or rows agree, so a column or a row shifted by one shows in every pixel; the wrap from 255 to 0 gives
    derivatives beyond +-255, which need the high byte of their 16-bit half of the interleaved map."""
    y, x = np.mgrid[0:H, 0:W]
    return ((7 * x + 13 * y) & 255).astype(np.uint8)


def flat(W, H, value=90):
    return np.full((H, W), value, np.uint8)


MAP_KINDS = ("texture", "saturated", "bytes")


def map_image(kind, W, H):
    return {"texture": lambda: texture(1000 + 7 * W + H, W, H), "saturated": lambda: saturated(W, H), "bytes": lambda: byte_pattern(W, H)}[kind]()


# widths around: the smallest frame, one lane group (4), a last strip of 1 .. 5 columns behind one and behind two strips; heights around: the smallest frame, one
# prefetch group, a last block of 1 .. 6 rows behind one and behind two blocks.  At H = 67 the last block has three rows (shorter than a prefetch group), at H = 9
# the frame is lower than a block; W = 257 has a last strip of one column, W = 13 is narrower than a strip and odd.
MAP_WIDTHS = (8, 9, 10, 11, 12, 13, 31) + tuple(range(252, 262)) + tuple(range(511, 517))
MAP_HEIGHTS = (8, 9, 11) + tuple(range(61, 71)) + tuple(range(127, 131))
MAP_SIZES = tuple(dict.fromkeys([(W, H) for H in (67, 9) for W in MAP_WIDTHS] + [(W, H) for W in (257, 13) for H in MAP_HEIGHTS]))
STRIDE_CASE = (257, 67, 13)  # W, H, padding bytes per row


def padded(img, pad, fill=0xFF):
    """(buffer, stride): img in rows of W + pad bytes, the padding filled with `fill`."""
    H, W = img.shape
    buf = np.full((H, W + pad), fill, np.uint8)
    buf[:, :W] = img
    return buf, W + pad


# ----------------------------------------------------------------------------------------------- KeyLines


def keylines(rows):
    """KEYLINE_DTYPE array from (x0, y0, x1, y1, numOfPixels or None): octave 0, the in-octave and the start / end points those values as float32, angle and
    lineLength from the float32 differences, class_id the index, numOfPixels (if None) int(max(|dx|, |dy|)) + 1 as a LineIterator would count."""
    kl = np.zeros(len(rows), KEYLINE_DTYPE)
    for i, (x0, y0, x1, y1, nop) in enumerate(rows):
        x0, y0, x1, y1 = f32(x0), f32(y0), f32(x1), f32(y1)
        dx, dy = f32(x1 - x0), f32(y1 - y0)
        k = kl[i]
        k["startPointX"] = k["sPointInOctaveX"] = x0; k["startPointY"] = k["sPointInOctaveY"] = y0
        k["endPointX"] = k["ePointInOctaveX"] = x1; k["endPointY"] = k["ePointInOctaveY"] = y1
        k["angle"] = f32(np.arctan2(dy, dx)); k["lineLength"] = f32(np.hypot(dx, dy))
        k["pt"] = (f32((x0 + x1) / f32(2)), f32((y0 + y1) / f32(2)))
        k["class_id"] = i; k["octave"] = 0; k["size"] = f32(abs(dx) * abs(dy)); k["response"] = 0
        k["numOfPixels"] = int(max(abs(dx), abs(dy))) + 1 if nop is None else nop
    return kl


DESC_FRAMES = ((257, 65), (300, 70), (513, 130))  # a last strip of one column and a last block of one row; narrower than two strips, W * H % 4 == 0; three strips, three blocks
DESC_SEED = {(257, 65): 21, (300, 70): 22, (513, 130): 23}
WALK_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 2000)  # around the walk's unroll of eight, and far longer than the frame
ANGLES = (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 1e-7, 7.0, -9.5, 4 * np.pi)  # the axes, +-pi, a denormal-free tiny angle, outside [-pi, pi]
RANDOM_SEED, RANDOM_LINES = 7, 400


def battery(W, H):
    """(names, keylines): the named lines, given in 300 x 70 coordinates and scaled to W x H (whole pixels; the .5 lines get their half afterwards)."""
    def X(x): return float(round(x * W / 300.0))
    def Y(y): return float(round(y * H / 70.0))
    names, rows, angle = [], [], {}

    def add(name, x0, y0, x1, y1, nop=None, ang=None):
        if ang is not None:
            angle[len(rows)] = ang
        names.append(name); rows.append((x0, y0, x1, y1, nop))
    add("diagonal", X(20), Y(10), X(280), Y(60))
    add("over_left_top", X(-20), Y(-15), X(40), Y(25))
    add("over_right_bottom", X(260), Y(45), X(320), Y(85))
    add("over_top_and_bottom", X(150), -30.0, X(150), H + 30.0)
    add("anti_diagonal", W - 1.0, 0.0, 0.0, H - 1.0)
    add("outside", X(400), Y(200), X(500), Y(300))
    for n in WALK_COUNTS:
        add("walk_%d" % n, X(100), Y(35), X(120), Y(35), nop=n)
    add("half_horizontal", X(100), Y(30) + 0.5, X(160), Y(30) + 0.5)
    add("half_vertical", X(150) + 0.5, Y(10), X(150) + 0.5, Y(60))
    add("forward", X(60), Y(20), X(200), Y(50))
    add("backward", X(200), Y(50), X(60), Y(20))
    for a in ANGLES:
        add("angle_%r" % float(f32(a)), X(80), Y(25), X(180), Y(45), ang=f32(a))
    kl = keylines(rows)
    for i, a in angle.items():
        kl["angle"][i] = a
    return names, kl


def random_lines(W, H, seed=RANDOM_SEED, n=RANDOM_LINES):
    """n segments with endpoints uniform in [-W/4, 5W/4] x [-H/4, 5H/4]: most of them leave the frame somewhere."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-W / 4, 5 * W / 4, (n, 2)); y = rng.uniform(-H / 4, 5 * H / 4, (n, 2))
    return keylines([(x[i, 0], y[i, 0], x[i, 1], y[i, 1], None) for i in range(n)])


def sample_extent(kl):
    """Largest |coordinate| a walk can reach, generously (the unrolled walk runs up to seven samples past numOfPixels): the reference casts to short, so it has to stay
    inside +-32000."""
    mx = np.abs(0.5 * (kl["sPointInOctaveX"].astype(np.float64) + kl["ePointInOctaveX"])); my = np.abs(0.5 * (kl["sPointInOctaveY"].astype(np.float64) + kl["ePointInOctaveY"]))
    return float((np.maximum(mx, my) + kl["numOfPixels"] / 2 + 8 + 32).max())


def support_start(oracle, k):
    """(sCorX, sCorY, dL0, dL1) of support-region row 0 in float32, as computeLBD :1272-1282 forms them."""
    s, c = oracle.sincos_f(float(k["angle"]))
    dL0, dL1 = f32(c), f32(s)
    hw, hh = f32((np.int16(k["numOfPixels"]) - 1) // 2 if k["numOfPixels"] > 0 else 0), f32(31)
    mx = f32(0.5 * (np.float64(k["sPointInOctaveX"]) + np.float64(k["ePointInOctaveX"]))); my = f32(0.5 * (np.float64(k["sPointInOctaveY"]) + np.float64(k["ePointInOctaveY"])))
    return f32(f32(f32(-dL0 * hw) + f32(dL1 * hh)) + mx), f32(f32(f32(-dL1 * hw) - f32(dL0 * hh)) + my), dL0, dL1


def same_vectors(fd, rfd):
    """The 72-float vectors agree: NaN at the same places (payload and sign not compared), the same bits everywhere else."""
    nan = np.isnan(rfd)
    return np.array_equal(np.isnan(fd), nan) and np.array_equal(fd.view(np.uint32)[~nan], rfd.view(np.uint32)[~nan])


# ----------------------------------------------------------------------------------------------- resident batch
BATCH_W, BATCH_H, BATCH_MAX = 261, 97, 8  # two strips (the last of five columns), two row blocks, W * H odd: every other frame's maps start off a 16-byte boundary
BATCH_SEEDS = tuple(range(3, 11))
BATCH_LINES_3_TO_6 = (53, 79, 68, 60)     # what the oracle finds on seeds 3 .. 6


def batch_frames():
    """Five of max_frames = 8: flat, three textures, flat."""
    fl = flat(BATCH_W, BATCH_H)
    return np.stack([fl] + [texture(s, BATCH_W, BATCH_H) for s in BATCH_SEEDS[:3]] + [fl])


def growth_batches():
    """(one frame, eight frames): the second batch has more lines than the buffers sized for the first can hold (lsd_run: nl + nl / 4 + 256)."""
    tex = np.stack([texture(s, BATCH_W, BATCH_H) for s in BATCH_SEEDS])
    return tex[:1], tex


# ----------------------------------------------------------------------------------------------- matcher
MATCH_NQ, MATCH_NT = (1, 255, 256, 257), (1, 255, 256, 257, 513)  # around the 256 queries of a workgroup and the 256 train rows of a tile
INT_MAX = 2 ** 31 - 1


def descriptors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def flip_bits(row, bits):
    out = row.copy()
    for b in bits:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def brute_knn(q, t):
    """(first index of the minimum, minimum, all distances) of the Hamming distances, numpy."""
    dist = np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(2).astype(np.int32)
    return dist.argmin(1).astype(np.int32), dist.min(1), dist


def brute_second(dist):
    """Second smallest distance per query counted with multiplicity (a tie for the best is its own second), INT_MAX with one train row."""
    if dist.shape[1] == 1:
        return np.full(len(dist), INT_MAX, np.int32)
    return np.partition(dist, 1, axis=1)[:, 1].astype(np.int32)


def duplicate_case(j=100, nt=513, seed=31):
    """(q, t, j): train row j copied to j + 256 (the same place of the next tile), the query equal to it."""
    t = descriptors(nt, seed)
    t[j + 256] = t[j]
    q = descriptors(5, seed + 1)
    q[2] = t[j]
    return q, t, j


def tie_case(j=37, k=300, nbits=9, nt=513, seed=33):
    """(q, t, j, nbits): train rows j (tile 0) and k (tile 1) both nbits away from query 1, in different bits; every other row is a random 256-bit string."""
    assert j < 256 <= k < 512
    t = descriptors(nt, seed); q = descriptors(3, seed + 1)
    t[j] = flip_bits(q[1], range(0, nbits)); t[k] = flip_bits(q[1], range(100, 100 + nbits))
    return q, t, j, nbits
