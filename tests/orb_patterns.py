"""Frames that put the ORB extractor's candidates where a test wants them: isolated single-pixel dots on a flat background, and uniform noise.
A helper, not a test module; it reads nothing but its arguments and every generator is seeded.

Why dots.  A pixel of value fg on a background bg, no other dot within 3 pixels (Chebyshev), has sixteen ring pixels equal to bg: it is a FAST-9/16
corner for every threshold below |fg - bg| with cornerScore |fg - bg| - 1, no background pixel is a corner (its ring holds isolated dots, never nine
in a row), and 3 x 3 non-maximum suppression has nothing to suppress.  So on level 0 the candidates ARE the dots -- every one with the same response
-- provided they lie inside the extractor's border (EDGE = 19 pixels).  All generators keep dots at least MIN_GAP = 4 apart and MARGIN = 24 from the
image border.  What the higher levels make of the resized dots is whatever the reference makes of it; the tests compare it like any other frame.

The grids below restate ORBextractor.cc:776-800 (cells) and :547-560 (root nodes) for level 0, so that a generator can aim at a cell or a root."""
import math

import numpy as np

f32 = np.float32
EDGE = 19      # EDGE_THRESHOLD
MINB = 16      # minBorderX = EDGE_THRESHOLD - 3
MARGIN = 24
MIN_GAP = 4


def dots(W, H, points, bg, fg):
    """H x W uint8 image of value bg with the pixels points[i] = (x, y) set to fg (one value, or one per point)."""
    img = np.full((H, W), bg, np.uint8)
    points = np.asarray(points, np.int64).reshape(-1, 2)
    assert len(points) == 0 or (points[:, 0].min() >= 0 and points[:, 0].max() < W and points[:, 1].min() >= 0 and points[:, 1].max() < H)
    img[points[:, 1], points[:, 0]] = np.asarray(fg, np.uint8)
    return img


def noise(W, H, seed):
    """Uniform random bytes: the dense case, tens of thousands of candidates per VGA frame."""
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def check_isolated(points):
    """Every dot at least MIN_GAP from every other (Chebyshev): what makes the candidates predictable."""
    p = np.asarray(points, np.int64)
    order = np.lexsort((p[:, 0], p[:, 1]))
    p = p[order]
    for i in range(len(p)):
        j = i + 1
        while j < len(p) and p[j, 1] - p[i, 1] < MIN_GAP:
            assert abs(p[j, 0] - p[i, 0]) >= MIN_GAP, (p[i], p[j])
            j += 1
    return True


def level0_grid(W, H):
    """(nCols, nRows, wCell, hCell) of level 0 (ORBextractor.cc:776-787)."""
    fw, fh = W - 2 * EDGE + 6, H - 2 * EDGE + 6  # maxBorderX - minBorderX
    nCols, nRows = int(f32(fw) / f32(30)), int(f32(fh) / f32(30))
    return nCols, nRows, int(math.ceil(f32(fw) / f32(nCols))), int(math.ceil(f32(fh) / f32(nRows)))


def level0_cell(W, H, points):
    """Cell index (row * nCols + col) of the level-0 cell whose FAST call reports a corner at each (x, y): cell (i, j) reports the
    pixels [MINB + j * wCell + 3, MINB + (j + 1) * wCell + 3) x (rows alike) (:790-826)."""
    nCols, nRows, wCell, hCell = level0_grid(W, H)
    p = np.asarray(points, np.int64).reshape(-1, 2)
    cj, ci = (p[:, 0] - MINB - 3) // wCell, (p[:, 1] - MINB - 3) // hCell
    assert len(p) == 0 or (cj.min() >= 0 and cj.max() < nCols and ci.min() >= 0 and ci.max() < nRows)
    return ci * nCols + cj


def level0_roots(W, H):
    """(nIni, hX, height) of DistributeOctTree's root nodes on level 0, in candidate coordinates (pixel - MINB) (:547-560)."""
    fw, fh = W - 2 * EDGE + 6, H - 2 * EDGE + 6
    nIni = int(math.floor(float(f32(fw) / f32(fh)) + 0.5))
    return nIni, float(f32(fw) / f32(nIni)), fh


def lattice(W, H, spacing, offset=(0, 0)):
    """Regular lattice: node sizes tie on every split and every response ties."""
    assert spacing >= MIN_GAP
    xs = np.arange(MARGIN + offset[0] % spacing, W - MARGIN, spacing)
    ys = np.arange(MARGIN + offset[1] % spacing, H - MARGIN, spacing)
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)


def jittered_lattice(W, H, spacing, jitter, seed):
    """The lattice with every dot moved by up to +-jitter pixels: node sizes differ a little, responses still tie."""
    assert spacing - 2 * jitter >= MIN_GAP
    p = lattice(W, H, spacing)
    p = p + np.random.default_rng(seed).integers(-jitter, jitter + 1, p.shape)
    keep = (p[:, 0] >= MARGIN) & (p[:, 0] < W - MARGIN) & (p[:, 1] >= MARGIN) & (p[:, 1] < H - MARGIN)
    return p[keep]


def cluster_and_sparse(W, H, seed, cluster=(24, 16), sparse_spacing=40):
    """One tight cluster (cluster[0] x cluster[1] dots MIN_GAP apart, at a seeded place) and a sparse lattice everywhere else: one node keeps most of the
    points while the others run out, so the largest-first phase keeps splitting the same lineage."""
    rng = np.random.default_rng(seed)
    cw, ch = (cluster[0] - 1) * MIN_GAP, (cluster[1] - 1) * MIN_GAP
    cx, cy = int(rng.integers(MARGIN, W - MARGIN - cw)), int(rng.integers(MARGIN, H - MARGIN - ch))
    c = np.stack(np.meshgrid(cx + MIN_GAP * np.arange(cluster[0]), cy + MIN_GAP * np.arange(cluster[1])), -1).reshape(-1, 2)
    s = lattice(W, H, sparse_spacing)
    far = (s[:, 0] < cx - MIN_GAP) | (s[:, 0] > cx + cw + MIN_GAP) | (s[:, 1] < cy - MIN_GAP) | (s[:, 1] > cy + ch + MIN_GAP)
    return np.concatenate([c, s[far]])


def one_quadrant(W, H, seed, spacing=6):
    """Every dot inside one quadrant of one root node of level 0 (root and quadrant seeded): every other child of that root's first split, and every
    other root, is empty."""
    rng = np.random.default_rng(seed)
    nIni, hX, fh = level0_roots(W, H)
    root, qx, qy = int(rng.integers(nIni)), int(rng.integers(2)), int(rng.integers(2))
    x0, x1 = int(f32(hX) * f32(root)), int(f32(hX) * f32(root + 1))
    mx, my = x0 + int(math.ceil((x1 - x0) / 2)), int(math.ceil(fh / 2))
    bx = (x0, mx) if qx == 0 else (mx, x1)
    by = (0, my) if qy == 0 else (my, fh)
    # two pixels inside the quadrant, and inside the image margin (candidate coordinates + MINB = pixels)
    lo_x, hi_x = max(bx[0] + 2 + MINB, MARGIN), min(bx[1] - 2 + MINB, W - MARGIN)
    lo_y, hi_y = max(by[0] + 2 + MINB, MARGIN), min(by[1] - 2 + MINB, H - MARGIN)
    return np.stack(np.meshgrid(np.arange(lo_x, hi_x, spacing), np.arange(lo_y, hi_y, spacing)), -1).reshape(-1, 2)


def two_classes(W, H, seed, spacing=10):
    """(points, strong): a lattice whose dots are strong (|fg - bg| above iniThFAST) or weak (between minThFAST and iniThFAST), chosen per level-0 cell: a third of
    the cells hold only weak dots (the cell falls back to minThFAST and reports them), a third only strong ones, a third both (the cell finds the strong ones at
    iniThFAST and never looks for the weak)."""
    rng = np.random.default_rng(seed)
    p = lattice(W, H, spacing)
    cell = level0_cell(W, H, p)
    kind = rng.integers(0, 3, cell.max() + 1)[cell]  # 0 weak only, 1 strong only, 2 mixed
    strong = (kind == 1) | ((kind == 2) & (rng.integers(0, 2, len(p)) == 1))
    return p, strong


def two_class_values(strong, bg, iniTh, minTh):
    """fg per dot: strong dots 3 * iniTh above bg, weak dots halfway between the two thresholds above bg."""
    weak = (iniTh + minTh) // 2
    assert minTh < weak < iniTh and bg + 3 * iniTh <= 255
    return np.where(strong, bg + 3 * iniTh, bg + weak).astype(np.uint8)


# ---- the first phase of DistributeOctTree as lists, and dots that bring one of its passes to a wanted length and pattern -------------------------------------------------
def quadtree_first_phase(cand, fw, fh):
    """DistributeOctTree's first phase (ORBextractor.cc:588-675) on one root of fw x fh over candidate coordinates (pixel - MINB), with a quota no pass reaches: per
    pass the list as [(box, points in the node)], until the list stops growing.  A node with more than one point is split (DivideNode, :483-538: halves rounded up)
    and its non-empty children are pushed to the front in the order they are made; the others keep their place."""
    nodes = [((0, 0, fw, fh), [tuple(c) for c in cand])]
    passes = []
    while True:
        passes.append(nodes)
        front, kept = [], []
        for box, pts in nodes:
            if len(pts) <= 1:
                kept.append((box, pts))
                continue
            x0, y0, x1, y1 = box
            mx, my = x0 + int(math.ceil((x1 - x0) / 2)), y0 + int(math.ceil((y1 - y0) / 2))
            boxes = [(x0, y0, mx, my), (mx, y0, x1, my), (x0, my, mx, y1), (mx, my, x1, y1)]
            ch = [[], [], [], []]
            for x, y in pts:
                ch[(0 if x < mx else 1) + (0 if y < my else 2)].append((x, y))
            front += [(b, c) for b, c in zip(boxes, ch) if c]
        new = front[::-1] + kept
        if len(new) == len(nodes):
            return passes
        nodes = new


def quadtree_seam_dots(W, H, flags):
    """Dots (pixels) of a W x H frame with one level-0 root whose sides divide by 32, for a pass of the first phase whose list has len(flags) nodes, expandable
    exactly where flags is set.  The nodes are sibling groups of four (one of three and one of two where the length asks for it) under parents of one depth; the
    parents are dealt to the quadrants of every depth in turn.  So every node above them holds two points or more, the list grows with every pass and nothing is
    kept at its tail, and the pass below the parents lists their children and nothing else, in an order that does not depend on which of them hold two dots (in
    different quadrants) and which one.  -> (dots, the passes of quadtree_first_phase, the index of that pass).  The order itself comes from the restated first
    phase, and the result is checked against flags."""
    fw, fh = W - 2 * EDGE + 6, H - 2 * EDGE + 6
    assert level0_roots(W, H)[0] == 1 and fw % 32 == 0 and fh % 32 == 0
    flags = [bool(f) for f in flags]
    S = len(flags)
    groups = [1] if S == 1 else [4] * (S // 4 - (S % 4 == 1)) + {0: [], 1: [3, 2], 2: [2], 3: [3]}[S % 4]
    assert sum(groups) == S and S >= 1
    e = 0  # depth of the parents: the first with room for them
    while 4 ** e < len(groups):
        e += 1
    D = e + (S > 1)
    assert D <= 5
    bw, bh = fw >> D, fh >> D

    def parent(m):  # the base-4 digits of m, lowest first, choose the quadrant from the root down
        i = j = 0
        for d in range(e):
            q = (m >> (2 * d)) & 3
            i, j = 2 * i + (q & 1), 2 * j + (q >> 1)
        return i, j
    cells = [(0, 0)] if S == 1 else [(2 * i + (q & 1), 2 * j + (q >> 1)) for (i, j), g in zip(map(parent, range(len(groups))), groups) for q in range(g)]
    clamp = lambda x, y: (min(max(x, MARGIN - MINB), fw - 1 - (MARGIN - MINB)), min(max(y, MARGIN - MINB), fh - 1 - (MARGIN - MINB)))
    first = [clamp(i * bw + 3, j * bh + 3) for i, j in cells]
    second = [clamp(i * bw + bw - 5, j * bh + bh - 4) for i, j in cells]
    two = [True] * S
    for _ in range(2):
        cand = first + [s for s, t in zip(second, two) if t]
        passes = quadtree_first_phase(cand, fw, fh)
        where = {pt: n for n, (_, pts) in enumerate(passes[D]) for pt in pts}
        assert len(passes[D]) == S and sorted(where[a] for a in first) == list(range(S))
        if [len(p) > 1 for _, p in passes[D]] == flags:
            dots = np.array(cand, np.int64).reshape(-1, 2) + MINB
            assert len(dots) < 2 or check_isolated(dots)
            return dots, passes, D
        two = [flags[where[a]] for a in first]
    raise AssertionError("no dot set for %d nodes" % S)
