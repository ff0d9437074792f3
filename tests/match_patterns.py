"""Designed inputs for the matcher (cube_slam_amd/csrc/match.hip): frames and queries that sit on the seams of match_grid, match_candidates, match_resolve<V> and the small
kernels, each with the result it must give.  A helper, not a test module; it imports neither the oracle nor the device library.  tests/test_match_patterns.py holds the
oracle to these expectations on the CPU and asserts that every seam is reached; tests/test_match_edges_gpu.py holds the device to the oracle on the same inputs.

Frame bounds are (0, 1024, 0, 768): wInv = hInv = 1 / 16, so every cell border and every product with wInv is exact in float.  bits(n) has its first n bits set: against
bits(0) the Hamming distance is n, and |bits(a) ^ bits(b)| = |a - b|.

The expectations come from three small models written here from the reference's rules, not from the oracle: cell_of / grid_lists (PosInGrid rounds half away from zero),
area (GetFeaturesInArea: floor / ceil of the window, strict |dx| < r, cells column-major, a cell's list ascending) and resolve (the sequential loop of each of the six
searches over candidate lists).  The headline cases also carry their result in closed form (`closed`)."""
import math

import numpy as np

from cube_slam_amd.orb import KEYPOINT_DTYPE

f32 = np.float32
BOUNDS = (0.0, 1024.0, 0.0, 768.0)
COLS, ROWS, CELL = 64, 48, 16.0
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30
SF = f32(1.2) ** np.arange(8, dtype=np.float32)
PROJ, LOCAL, INIT, BOW, BOWKF, CLAIM = "RV_PROJ", "RV_LOCAL", "RV_INIT", "RV_BOW", "RV_BOWKF", "RV_CLAIM"
VARIANTS = (PROJ, LOCAL, INIT, BOW, BOWKF, CLAIM)
ORIENTED = (PROJ, INIT, BOW, BOWKF, CLAIM)  # SearchByProjection(F, vpMapPoints) has no rotation check
RS_NC, MC_G, MC_Q = 8, 16, 16                # match.hip: candidates kept in registers; lanes per query; queries per workgroup
ORB_DIST = 70                                # the relocalisation search's ORBdist in these cases
# train-side state of match_resolve: 16 bytes per key point (20 for RV_INIT) + 16; dynamic LDS above 48 KiB, refused above 150 KiB (mt_resolve)
LDS_SWITCH = {v: (48 * 1024 - 16) // (20 if v == INIT else 16) for v in VARIANTS}      # the largest N2 that stays at or below 48 KiB: 3071 / 2456
LDS_LIMIT = {v: (150 * 1024 - 16) // (20 if v == INIT else 16) for v in VARIANTS}      # the largest N2 accepted: 9599 / 7679


def bits(n):
    d = np.zeros(32, np.uint8)
    d[:n // 8] = 255
    if n % 8:
        d[n // 8] = (1 << (n % 8)) - 1
    return d


def bit_range(a, b):
    return bits(b) ^ bits(a)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def make_keys(xy, octave=0, angle=0.0):
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    if len(xy):
        xy = np.asarray(xy, np.float32).reshape(-1, 2)
        k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["octave"] = octave; k["angle"] = angle; k["size"] = 31
    return k


def below(v):
    return f32(np.nextafter(f32(v), f32(-np.inf)))


def above(v):
    return f32(np.nextafter(f32(v), f32(np.inf)))


# ----------------------------------------------------------------------------------------------- the models
def c_round(v):
    v = float(v)
    return math.floor(v + 0.5) if v >= 0 else math.ceil(v - 0.5)


def cell_of(x, y):
    """Frame::PosInGrid: (column, row) or None outside the grid."""
    px, py = c_round(f32(f32(x) - f32(BOUNDS[0])) * f32(1 / CELL)), c_round(f32(f32(y) - f32(BOUNDS[2])) * f32(1 / CELL))
    return None if (px < 0 or px >= COLS or py < 0 or py >= ROWS) else (px, py)


def grid_lists(keys):
    """cell -> key point indices in ascending order (mGrid[x][y] in push_back order)."""
    g = {}
    for i in range(len(keys)):
        c = cell_of(keys["x"][i], keys["y"][i])
        if c is not None:
            g.setdefault(c, []).append(i)
    return g


def window_cells(x, y, r):
    """(nMinCellX, nMaxCellX, nMinCellY, nMaxCellY) of Frame::GetFeaturesInArea, or None where it returns early."""
    x, y, r, inv = f32(x), f32(y), f32(r), f32(1 / CELL)
    x0 = max(0, math.floor(f32(f32(f32(x - f32(BOUNDS[0])) - r) * inv)))
    if x0 >= COLS:
        return None
    x1 = min(COLS - 1, math.ceil(f32(f32(f32(x - f32(BOUNDS[0])) + r) * inv)))
    if x1 < 0:
        return None
    y0 = max(0, math.floor(f32(f32(f32(y - f32(BOUNDS[2])) - r) * inv)))
    if y0 >= ROWS:
        return None
    y1 = min(ROWS - 1, math.ceil(f32(f32(f32(y - f32(BOUNDS[2])) + r) * inv)))
    if y1 < 0:
        return None
    return x0, x1, y0, y1


def n_cells(x, y, r):
    w = window_cells(x, y, r)
    return 0 if w is None else (w[1] - w[0] + 1) * (w[3] - w[2] + 1)


def area(keys, grid, x, y, r, minLevel=-1, maxLevel=-1):
    w = window_cells(x, y, r)
    out = []
    if w is None:
        return out
    x, y, r = f32(x), f32(y), f32(r)
    check = minLevel > 0 or maxLevel >= 0
    for ix in range(w[0], w[1] + 1):
        for iy in range(w[2], w[3] + 1):
            for i in grid.get((ix, iy), ()):
                o = int(keys["octave"][i])
                if check and (o < minLevel or (maxLevel >= 0 and o > maxLevel)):
                    continue
                if abs(f32(keys["x"][i] - x)) < r and abs(f32(keys["y"][i] - y)) < r:
                    out.append(i)
    return out


def rot_bin(a1, a2):
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = c_round(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH))))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes):
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, i
        elif s > m3:
            m3, i3 = s, i
    if m2 < f32(0.1) * f32(m1):
        i2 = i3 = -1
    elif m3 < f32(0.1) * f32(m1):
        i3 = -1
    return i1, i2, i3


# ----------------------------------------------------------------------------------------------- 1. grid
def _lattice_refs():
    """One key point at the centre of every cell of row 1 and of column 1: the cell order of a whole-grid query then shows the cell of every other point."""
    return [(CELL * c, CELL) for c in range(COLS)] + [(CELL, CELL * r) for r in range(ROWS)]


def grid_borders():
    """Key points on and beside every rounding border of PosInGrid, in front of the reference points (lower indices: a point in a wrong cell changes place in the list).
    Returns (keys, expected cell per border point)."""
    xs = [(8.0, 1), (below(8.0), 0), (24.0, 2), (below(24.0), 1), (-8.0, None), (above(-8.0), 0), (below(-8.0), None), (0.0, 0), (1024.0, None), (1016.0, None),
          (below(1016.0), 63), (1015.9, 63), (7.999, 0), (below(1024.0), None), (-0.0, 0)]
    ys = [(8.0, 1), (below(8.0), 0), (-8.0, None), (above(-8.0), 0), (768.0, None), (760.0, None), (below(760.0), 47), (767.0, None), (759.9, 47), (744.0, 47), (below(744.0), 46)]
    pts = [(x, CELL) for x, _ in xs] + [(CELL, y) for y, _ in ys] + [(1015.9, 767.0)]
    exp = [None if c is None else (c, 1) for _, c in xs] + [None if r is None else (1, r) for _, r in ys] + [None]
    return make_keys(pts + _lattice_refs()), exp


def grid_scatter(N):
    """N key points scattered over the grid and a little beyond it (N around the 1 024-thread stride of match_grid)."""
    i = np.arange(N)
    return make_keys(np.stack([(i * 37 % 1060) - 18 + 0.25, (i * 91 % 800) - 16 + 0.5], axis=1).astype(np.float32) if N else [], octave=i % 4)


GRID_SIZES = (0, 1, 1023, 1024, 1025)


def grid_one_cell(n=1500):
    """n key points in cell (10, 10) in descending x."""
    return make_keys([(167.9 - 0.0105 * i, 160.0) for i in range(n)])


def grid_corner_cells():
    """Key points in cells 0 and 3071 only, their indices interleaved."""
    return make_keys([((1.0 + 0.5 * i, 2.0) if i % 2 == 0 else (1009.0 + 0.5 * i, 753.0)) for i in range(10)])


def whole_grid(keys):
    """What GetFeaturesInArea(512, 384, 5000) returns: every key point inside the grid in (column, row, index) order."""
    g = grid_lists(keys)
    return [i for c in sorted(g) for i in g[c]]


# ----------------------------------------------------------------------------------------------- 2. windows
def window_frame():
    """A key point at every cell centre, index row-major (so index order is not cell order), level (column + row) % 4, and extras: three records behind the centre of cell
    (20, 20) of which the first and third pass a level filter (0, 0); one in the last cell; 21 along the last row at y = 758, which a window that comes up from below the grid
    (one row of cells) reaches while the centres at y = 752 stay outside."""
    pts, octv = [], []
    for r in range(ROWS):
        for c in range(COLS):
            pts.append((CELL * c, CELL * r)); octv.append((c + r) % 4)
    pts += [(318.0, 320.0), (323.0, 320.0), (321.0, 320.0), (1012.0, 756.0)]; octv += [0, 2, 0, 1]
    pts += [(CELL * c, 758.0) for c in range(21)]; octv += [c % 4 for c in range(21)]
    keys = make_keys(pts, octave=np.array(octv))
    desc = np.stack([bits(1 + (7 * i) % 97) for i in range(len(keys))])  # every distance to bits(0) is at most TH_HIGH; neighbours differ
    return keys, desc


# (x, y, r, what it is there for)
WINDOWS = [
    (24.0, 24.0, 8.0, "x - r = 16 and x + r = 32: cells 1 .. 2; the four centres sit at |dx| == r and are excluded"),
    (24.0, 24.0, float(above(8.0)), "one ulp wider: the four centres"),
    (21.0, 16.0, 5.0, "|dx| == r"), (16.0, 21.0, 5.0, "|dy| == r"), (21.0, 16.0, float(above(5.0)), "|dx| one ulp inside r"),
    (16.0, 16.0, 0.0, "r = 0: one cell, nothing passes"),
    (-100.0, 100.0, 50.0, "left of the grid"), (1200.0, 100.0, 50.0, "right of the grid"), (100.0, -100.0, 50.0, "above"), (100.0, 900.0, 50.0, "below"),
    (1014.0, 758.0, 4.0, "one cell (the last), ny = 1"),
    (40.0, 40.0, 17.0, "16 cells, 4 x 4"), (132.0, 865.0, 112.0, "16 cells, ny = 1: the window comes up from below the grid"), (140.0, 873.0, 120.0, "17 cells, ny = 1"),
    (512.0, 384.0, 5000.0, "all 3072 cells"),
    (320.0, 320.0, 4.0, "three extras behind the centre of cell (20, 20)"),
    (-8.0, 8.0, 8.0, "x + r = 0: ceil gives cell 0"), (1024.0, 100.0, 16.0, "x - r = 1008: floor gives cell 63"),
]
LEVEL_FILTERS = ((-1, -1), (0, -1), (2, -1), (0, 3), (2, 2))
WINDOW_NCELLS = {1, 16, 17, 3072}


def window_queries():
    """(x, y, r, minLevel, maxLevel) for GetFeaturesInArea: every window without a level filter, and the level filters on three of them."""
    q = [(x, y, r, -1, -1) for x, y, r, _ in WINDOWS]
    for lo, hi in LEVEL_FILTERS[1:]:
        q += [(40.0, 40.0, 17.0, lo, hi), (320.0, 320.0, 4.0, lo, hi)]
    q.append((320.0, 320.0, 4.0, 0, 0))
    return q


def local_map_batches():
    """The windows as SearchByProjectionLocalMap calls: th = 1 and view_cos = 0 give r = 4 * scale_factors[level], so a call's scale table (rA, rB, rA, rB, rA) / 4 carries two radii
    exactly, each at levels of its parity.  Each batch is (scale table, queries (x, y, level, in_view)); the level filter is (level - 1, level), and a query takes the level of its
    radius that lets the key point at the nearest cell centre through.  Batch 0 puts the 3072-cell window beside three one-cell windows in one
    wave; the invalid queries of the last batch interleave with the valid ones."""
    radii = sorted({r for _, _, r, _ in WINDOWS})
    out = []
    for k in range(0, len(radii), 2):
        pair = radii[k:k + 2]
        q = []
        for x, y, r, _ in WINDOWS:
            if r in pair:
                o = (min(max(c_round(x / CELL), 0), COLS - 1) + min(max(c_round(y / CELL), 0), ROWS - 1)) % 4  # the level of the nearest centre
                q.append((x, y, o if o % 2 == pair.index(r) else o + 1, 1))
        out.append((np.array([f32((pair * 3)[k]) / f32(4) for k in range(5)], np.float32), q))
    big = (np.array([5000.0 / 4, 1.0], np.float32), [(512.0, 384.0, 0, 1), (1014.0, 758.0, 1, 1), (1014.0, 758.0, 1, 1), (1014.0, 758.0, 1, 1)] + [(16.0 * (3 + i), 160.0, 1, 1) for i in range(12)])
    return [big] + out


def local_map_counts():
    """(nq, queries) for nq in 15, 16, 17, 33 around MC_Q = 16 queries per workgroup: windows of 17 px over the lattice, every third query invalid."""
    return [(n, [(16.0 * (2 + i), 16.0 * (2 + i % 5), i % 2, int(i % 3 != 1)) for i in range(n)]) for n in (15, 16, 17, 33)]


LOCAL_COUNT_SF = np.array([17.0 / 4, 9.0 / 4], np.float32)


class LocalBatch:
    """One SearchByProjectionLocalMap call over the window frame, in the form `resolve` reads: no query blocks (a later claim overwrites an earlier one), nnratio 1 (the ratio
    rule never rejects), descriptor bits(0) for every query -- the match of a query is the nearest key point of its window, first in the reference's order."""

    def __init__(self, keys, desc, grid, sf, queries):
        self.keys, self.desc, self.grid, self.sf, self.queries = keys, desc, grid, np.asarray(sf, np.float32), queries
        self.t, self.q = range(len(keys)), queries
        nq = len(queries)
        self.qdesc = np.zeros((nq, 32), np.uint8); self.blocks = np.zeros(nq, np.uint8); self.tblocked = np.zeros(len(keys), np.uint8)
        self.qangle = np.zeros(nq, np.float32); self.nnratio, self.check_ori = 1.0, False
        self.qxy = np.array([(x, y) for x, y, _, _ in queries], np.float32).reshape(nq, 2)
        self.qlevel = np.array([l for _, _, l, _ in queries], np.int32); self.in_view = np.array([v for _, _, _, v in queries], np.uint8)

    def radius(self, q):
        return f32(f32(4.0) * self.sf[self.qlevel[q]])

    def lists(self, variant=None):
        return [area(self.keys, self.grid, x, y, self.radius(q), l - 1, l) if v else None for q, (x, y, l, v) in enumerate(self.queries)]

    def candidates(self):
        return sum(len(l) for l in self.lists() if l is not None)

    def device(self, m):
        m.mfNNratio = self.nnratio
        return m.SearchByProjectionLocalMap(self.qxy, np.zeros(len(self.q), np.float32), self.qlevel, self.in_view, self.blocks, self.qdesc, self.sf, 1.0)

    def judge(self, oracle, F):
        return oracle.search_local_map(F, self.qxy, np.zeros(len(self.q), np.float32), self.qlevel, self.in_view, self.blocks, self.qdesc, self.sf, 1.0, self.nnratio)


# ----------------------------------------------------------------------------------------------- 4. claims: one description, six searches
class Search:
    """Train key points and queries grouped in `spots`: a spot is one grid cell centre, far from every other spot, and doubles as the vocabulary node of the two BoW searches.  A
    query's candidates are the train key points of its spot in ascending index, in every variant (window radius 10 around the spot's centre; the node's features)."""

    def __init__(self, name, nnratio=0.9, check_ori=False, r=10.0):
        self.name, self.nnratio, self.check_ori, self.r = name, nnratio, check_ori, r
        self.t, self.q = [], []  # (spot, desc, angle, level, blocked) / (spot, desc, angle, level, blocks)
        self.n_filler = 0
        self.closed = None       # the result in closed form where the case has one: {variant: (match vector, nmatches)}
        self.want = {}           # what the case must reach: {variant: {statistic: value}}

    def train(self, spot, desc, angle=0.0, level=0, blocked=0):
        self.t.append((spot, desc, angle, level, blocked)); return len(self.t) - 1

    def query(self, spot, desc, angle=0.0, level=0, blocks=1):
        assert not self.q or spot >= self.q[-1][0], "queries by ascending spot: index order is then the visiting order of the BoW searches too"
        self.q.append((spot, desc, angle, level, blocks)); return len(self.q) - 1

    def filler(self, n):
        """n train key points in FRONT of the spots' (lower indices), along the bottom rows where no window reaches, in a node no query has."""
        assert not self.t
        self.n_filler = n
        for _ in range(n):
            self.t.append((-1, bits(255), 0.0, 0, 0))

    @staticmethod
    def centre(spot):
        assert 0 <= spot < 140
        return CELL * (4 + 4 * (spot % 14)), CELL * (4 + 4 * (spot // 14))

    def build(self):
        nt, nq = len(self.t), len(self.q)
        xy, seen = [], {}
        for i, (s, *_rest) in enumerate(self.t):
            if s < 0:
                xy.append((8.0 + i % 1000, 700.0 + 2.0 * (i // 1000)))
            else:
                k = seen.get(s, 0); seen[s] = k + 1
                cx, cy = self.centre(s)
                xy.append((cx + 0.5 * (k % 15 - 7), cy + 0.5 * ((k // 15) % 15 - 7)))
        self.keys = make_keys(xy, octave=np.array([t[3] for t in self.t], np.int32), angle=np.array([t[2] for t in self.t], np.float32))
        self.desc = np.stack([t[1] for t in self.t]) if nt else np.zeros((0, 32), np.uint8)
        self.tnode = np.array([t[0] if t[0] >= 0 else 9999 for t in self.t], np.int32)
        self.tblocked = np.array([t[4] for t in self.t], np.uint8)
        self.qxy = np.array([self.centre(q[0]) for q in self.q], np.float32).reshape(nq, 2)
        self.qdesc = np.stack([q[1] for q in self.q]); self.qangle = np.array([q[2] for q in self.q], np.float32)
        self.qlevel = np.array([q[3] for q in self.q], np.int32); self.qnode = np.array([q[0] for q in self.q], np.int32)
        self.blocks = np.array([q[4] for q in self.q], np.uint8)
        self.qkeys = make_keys(self.qxy, octave=self.qlevel, angle=self.qangle)
        self.grid = grid_lists(self.keys)
        return self

    # the window of query q as the entry of `variant` opens it
    def window(self, variant, q):
        L = int(self.qlevel[q])
        if variant == PROJ:
            return f32(f32(self.r) * SF[L]), L - 1, L + 1
        if variant == LOCAL:
            th = f32(self.r) / f32(4)
            return f32(f32(f32(4.0) * th if th != 1.0 else f32(4.0)) * SF[L]), L - 1, L
        if variant == INIT:
            return f32(int(self.r)), L, L
        return f32(self.r), -1, 1  # CLAIM: predicted level 0, levels [-1, 1]

    def lists(self, variant):
        out = []
        for q in range(len(self.q)):
            if variant in (BOW, BOWKF):
                out.append([i for i in range(len(self.t)) if self.tnode[i] == self.qnode[q]])
            elif variant == INIT and self.qlevel[q] > 0:
                out.append(None)
            else:
                r, lo, hi = self.window(variant, q)
                out.append(area(self.keys, self.grid, self.qxy[q, 0], self.qxy[q, 1], r, lo, hi))
        return out


def resolve(variant, S):
    """The sequential loop of the search `variant` over S's candidate lists -> (match vector, nmatches, statistics).  The match vector is per train key point (the query that holds
    it) for RV_PROJ, RV_LOCAL, RV_BOW, RV_CLAIM and per query (its train key point) for RV_INIT, RV_BOWKF."""
    lists, nt, nq = S.lists(variant), len(S.t), len(S.q)
    dist = lambda q, t: hamming(S.qdesc[q], S.desc[t])
    ratio = f32(S.nnratio)
    ori = S.check_ori and variant != LOCAL
    hist = [[] for _ in range(HISTO_LENGTH)]
    st = {"overwritten": 0, "displaced": 0, "cut": 0, "ratio_rejected": 0, "moved_on": 0, "longest_list": max([len(l) for l in lists if l is not None] + [0]), "histogram": None}
    tb = S.tblocked if variant != INIT else np.zeros(nt, np.uint8)
    owner = [-1] * nt
    q_match = [-1] * nq
    mdist = [2 ** 31 - 1] * nt
    n = 0
    for q in range(nq):
        if lists[q] is None:
            continue
        big = 2 ** 31 - 1 if variant == INIT else 256
        best = best2 = big
        bidx = blev = blev2 = -1
        skipped_better = False
        for t in lists[q]:
            d = dist(q, t)
            if variant in (PROJ, LOCAL):
                skip = tb[t] or (owner[t] >= 0 and S.blocks[owner[t]])
            elif variant == INIT:
                skip = mdist[t] <= d
            else:
                skip = tb[t] or owner[t] >= 0
            if skip:
                skipped_better = skipped_better or (owner[t] >= 0 and d < best)
                continue
            if d < best:
                best2, best, blev2, blev, bidx = best, d, blev, int(S.keys["octave"][t]), t
            elif d < best2:
                best2, blev2 = d, int(S.keys["octave"][t])
        if variant == PROJ:
            ok = best <= TH_HIGH
        elif variant == LOCAL:
            ok = best <= TH_HIGH
            if ok and blev == blev2 and f32(best) > ratio * f32(best2):
                ok = False; st["ratio_rejected"] += 1
        elif variant == CLAIM:
            ok = best <= ORB_DIST
        else:
            ok = best < TH_LOW if variant == BOWKF else best <= TH_LOW
            if ok and not (f32(best) < (f32(best2) * ratio if variant == INIT else ratio * f32(best2))):
                ok = False; st["ratio_rejected"] += 1
        if not ok or bidx < 0:
            continue
        st["moved_on"] += bool(skipped_better)
        if owner[bidx] >= 0:
            if variant == INIT:
                q_match[owner[bidx]] = -1; n -= 1; st["displaced"] += 1
            else:
                st["overwritten"] += 1
        owner[bidx] = q; q_match[q] = bidx; mdist[bidx] = best; n += 1
        if ori:
            hist[rot_bin(S.qangle[q], S.keys["angle"][bidx])].append(q if variant in (INIT, BOWKF) else bidx)
    if ori:
        st["histogram"] = [len(h) for h in hist]
        keep = three_maxima(st["histogram"])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for e in hist[b]:
                if variant in (INIT, BOWKF):
                    if variant == BOWKF or q_match[e] >= 0:
                        q_match[e] = -1; n -= 1; st["cut"] += 1
                else:
                    owner[e] = -1; n -= 1; st["cut"] += 1
    return np.array(q_match if variant in (INIT, BOWKF) else owner, np.int32), n, st


def domino(variant):
    """A full batch of 64 queries in which query k's best key point is the one query k - 1 ends on: train t_j = bits(4 j), queries bits(off), bits(off), bits(4 + off), ...
    With off = 1 query k + 1 is 1 bit from t_k and 3 bits from t_(k+1); the first two queries are equal, so query 1 moves from t_0 to t_1, which moves query 2 on, and so
    forth: lane k is final only in round k + 1.  SearchForInitialization skips a key point matched at a smaller OR EQUAL distance: off = 2 puts t_k and t_(k+1) both at 2 bits
    (nnratio 2 lets the tie pass the ratio test), so every move rests on the equality.  Result: query i holds t_i."""
    off = 2 if variant == INIT else 1
    S = Search("domino", nnratio=2.0 if variant == INIT else 0.9)
    for j in range(65):
        S.train(0, bits(4 * j))
    S.query(0, bits(off))
    for k in range(63):
        S.query(0, bits(4 * k + off))
    S.build()
    m = np.full(64 if variant in (INIT, BOWKF) else 65, -1, np.int32); m[:64] = np.arange(64)
    S.closed = {variant: (m, 64)}
    S.want = {variant: {"moved_on": 63, "displaced": 0}}
    return S


COUNTS = (63, 64, 65, 66, 128, 129)


def counted(nq):
    """nq queries, one per spot with one key point each, and the last two sharing a spot of two key points u, w: both are nearest to u, the later one nearer (2 bits against 4).
    The pair sits at lanes (nq - 2, nq - 1): (62, 63) inside a batch, (63, 64) across the seam, (64, 65) inside the next one.  The claim-once searches send the later query on
    to w; SearchForInitialization lets it displace the earlier one, which ends without a match."""
    S = Search("counted%d" % nq)
    for s in range(nq - 2):
        S.train(s, bits(0))
    u = S.train(nq - 2, bits(0)); w = S.train(nq - 2, bit_range(100, 120))
    for s in range(nq - 2):
        S.query(s, bits(3))
    a = S.query(nq - 2, bits(4)); b = S.query(nq - 2, bits(2))
    S.build()
    S.closed = {}
    for v in VARIANTS:
        if v == INIT:
            m = np.arange(nq, dtype=np.int32); m[a] = -1; m[b] = u
            S.closed[v] = (m, nq - 1)
        elif v == BOWKF:
            S.closed[v] = (np.arange(nq, dtype=np.int32), nq)
        else:
            S.closed[v] = (np.arange(nq, dtype=np.int32), nq)  # train key point i (u = nq - 2, w = nq - 1) is held by query i
    S.want = {v: ({"displaced": 1} if v == INIT else {"moved_on": 1}) for v in VARIANTS}
    S.pair = (a, b)
    return S


def proj_overwrite():
    """SearchByProjection(CurrentFrame, LastFrame): query A, whose map point has no observations (blocks = 0), claims u; query B takes u from it.  Both claims count and both
    enter the rotation histogram: A's entry lies alone in bin 5, behind bins 0 (B and 20 others), 1 and 2 (3 each), so bin 5 is cut -- and the cut clears u, which B holds.  nmatches is 28 claims less the one cut
    entry = 27 while only 26 key points stay matched: the reference's count, kept as it is.  A second pair A2, B2 on
    another key point u2 lies in bin 0 with both entries: u2 stays with B2, the later claim."""
    S = Search("proj_overwrite", check_ori=True)
    u = S.train(0, bits(0))
    spot = 1
    for b, cnt in ((0, 20), (1, 3), (2, 3)):
        for _ in range(cnt):
            S.train(spot, bits(0)); spot += 1
    S.train(spot, bits(0))
    A = S.query(0, bits(4), angle=150.0, blocks=0); B = S.query(0, bits(2), angle=0.0)
    spot = 1
    for b, cnt in ((0, 20), (1, 3), (2, 3)):
        for _ in range(cnt):
            S.query(spot, bits(3), angle=30.0 * b); spot += 1
    S.query(spot, bits(4), blocks=0); S.query(spot, bits(2))
    S.build()
    m = np.arange(-1, 27, dtype=np.int32) + 2; m[u] = -1; m[27] = 29
    S.closed = {PROJ: (m, 29)}
    S.want = {PROJ: {"overwritten": 2, "cut": 1}}
    return S


def init_displacement():
    """SearchForInitialization, 80 queries on one train key point at distances 45, 45, 44, 44, ..., 6, 6: a strictly smaller distance displaces, an equal one does not, inside a
    batch and across the seam at queries 63 / 64.  Only query 78 keeps the key point."""
    S = Search("init_displacement")
    S.train(0, bits(0))
    for i in range(80):
        S.query(0, bits(45 - i // 2))
    S.build()
    m = np.full(80, -1, np.int32); m[78] = 0
    S.closed = {INIT: (m, 1)}
    S.want = {INIT: {"displaced": 39}}
    return S


def init_equal():
    """40 queries at one distance from one train key point: only the first is matched."""
    S = Search("init_equal")
    S.train(0, bits(0))
    for i in range(40):
        S.query(0, bits(7))
    S.build()
    m = np.full(40, -1, np.int32); m[0] = 0
    S.closed = {INIT: (m, 1)}
    S.want = {INIT: {"displaced": 0}}
    return S


def init_stale_histogram():
    """SearchForInitialization keeps a displaced query's entry in rotHist.  Twelve queries displace each other on one key point, all in bin 7; bins 0, 1, 2, 3 hold 5, 4, 3, 2
    undisturbed matches.  With the eleven stale entries bin 7 is the largest and bins 7, 0, 1 survive: the five matches of bins 2 and 3 are cut.  Counting live entries only
    would keep bins 0, 1, 2 and cut bin 7.  One query of level 1 has a perfect candidate and takes no part."""
    S = Search("init_stale_histogram", check_ori=True)
    S.train(0, bits(0))
    spot = 1
    for b, cnt in ((0, 5), (1, 4), (2, 3), (3, 2)):
        for _ in range(cnt):
            S.train(spot, bits(0)); spot += 1
    S.train(spot, bits(0))
    for i in range(12):
        S.query(0, bits(30 - i), angle=210.0)
    spot = 1
    for b, cnt in ((0, 5), (1, 4), (2, 3), (3, 2)):
        for _ in range(cnt):
            S.query(spot, bits(3), angle=30.0 * b); spot += 1
    S.query(spot, bits(0), level=1)
    S.build()
    m = np.full(27, -1, np.int32); m[11] = 0; m[12:21] = np.arange(1, 10)
    S.closed = {INIT: (m, 10)}
    S.want = {INIT: {"displaced": 11, "cut": 5}}
    return S


def rs_nc():
    """Candidate lists of 7, 8, 9 and 40 with the minimum (10 bits) at positions 0, 7, 8 and last, and the second minimum on either side of position 8, once at 19 bits (nnratio
    0.5: 10 < 9.5 fails where a ratio test applies) and once at 21 (passes).  Every other candidate is 60 bits away."""
    S = Search("rs_nc", nnratio=0.5)
    spot = 0
    for n in (7, 8, 9, 40):
        for p in sorted({0, 7, 8, n - 1}):
            if p >= n:
                continue
            for s in (3, 10, n - 2):
                if s >= n or s == p or s < 0:
                    continue
                for second in (19, 21):
                    for c in range(n):
                        S.train(spot, bits(10 if c == p else second if c == s else 60))
                    spot += 1
    S.n_spots = spot
    for s in range(spot):
        S.query(s, bits(0))
    return S.build()


def thresholds():
    """One query per spot at the accept thresholds of every search and on the ratio test's equality: a single candidate at 49, 50, 51, ORB_DIST, ORB_DIST + 1, 100, 101 bits; a
    best of 10 with the second best at 20 (nnratio 0.5: best2 = 2 best, exact in float), 19 and 21."""
    S = Search("thresholds", nnratio=0.5)
    spot = 0
    for d in (49, 50, 51, ORB_DIST, ORB_DIST + 1, 100, 101):
        S.train(spot, bits(d)); spot += 1
    for second in (20, 19, 21):
        S.train(spot, bits(10)); S.train(spot, bits(second)); spot += 1
    for s in range(spot):
        S.query(s, bits(0))
    S.build()
    S.closed = {}
    accept = {PROJ: 100, LOCAL: 100, INIT: 50, BOW: 50, BOWKF: 49, CLAIM: ORB_DIST}
    for v in VARIANTS:
        single = [i if d <= accept[v] else -1 for i, d in enumerate((49, 50, 51, ORB_DIST, ORB_DIST + 1, 100, 101))]
        # best 10 / second 20: RV_LOCAL rejects only when best > ratio * best2 (10 > 10 is false); the others need best < ratio * best2 (10 < 10 is false); no ratio test in RV_PROJ / RV_CLAIM
        r20, r19, r21 = {PROJ: (1, 1, 1), CLAIM: (1, 1, 1), LOCAL: (1, 0, 1)}.get(v, (0, 0, 1))
        if v in (INIT, BOWKF):
            m = single + [7 if r20 else -1, 9 if r19 else -1, 11 if r21 else -1]
        else:
            m = single + [7 if r20 else -1, -1, 8 if r19 else -1, -1, 9 if r21 else -1, -1]
        S.closed[v] = (np.array(m, np.int32), int(sum(x >= 0 for x in m)))
    return S


def local_levels():
    """SearchByProjection(F, vpMapPoints): the ratio test applies only when best and second best are on one level.  Queries of predicted level 1 see levels 0 and 1.  Spots: best and
    second on level 1 (10 against 19: rejected), best on level 1 and second on level 0 (accepted), the same two with the second best in FRONT of the best in the list, and a
    level-2 key point that is nearest but outside the level window."""
    S = Search("local_levels", nnratio=0.5)
    S.train(0, bits(10), level=1); S.train(0, bits(19), level=1)
    S.train(1, bits(10), level=1); S.train(1, bits(19), level=0)
    S.train(2, bits(19), level=1); S.train(2, bits(10), level=1)
    S.train(3, bits(19), level=0); S.train(3, bits(10), level=1)
    S.train(4, bits(1), level=2); S.train(4, bits(10), level=1)
    for s in range(5):
        S.query(s, bits(0), level=1)
    S.build()
    S.closed = {LOCAL: (np.array([-1, -1, 1, -1, -1, -1, -1, 3, -1, 4], np.int32), 3)}
    S.want = {LOCAL: {"ratio_rejected": 2}}
    return S


ANGLE_DIFFS = ((0.0, -0.0), (15.0, 0.0), (45.0, 0.0), (344.9, 0.0), (345.0, 0.0), (359.9, 0.0), (10.0, 350.0), (0.0, 359.9), (359.9, 359.9))


def rotation_bins():
    """One match per spot with the angle pairs of ANGLE_DIFFS (query, train): differences -0.0, 15 (bin 0.5 -> 1), 45 (1.5 -> 2), 344.9, 345 (11.5 -> 12), 359.9 and negative
    differences that wrap.  Bins 0, 1, 2 are reached first by three matches each, so they survive and every other bin's single match is cut."""
    S = Search("rotation_bins", check_ori=True)
    n = len(ANGLE_DIFFS)
    for s, (_, ta) in enumerate(ANGLE_DIFFS):
        S.train(s, bits(0), angle=ta)
    for s in range(n, n + 6):
        S.train(s, bits(0))
    for s, (qa, _) in enumerate(ANGLE_DIFFS):
        S.query(s, bits(3), angle=qa)
    for s in range(n, n + 6):
        S.query(s, bits(3), angle=30.0 * ((s - n) % 3))
    return S.build()


HISTOGRAM_SHAPES = ((10, 1), (20, 1), (10, 10, 10, 10), (5, 5, 0, 5))
HISTOGRAM_CUT = {(10, 1): 0, (20, 1): 1, (10, 10, 10, 10): 10, (5, 5, 0, 5): 0}  # 1 < 0.1f * 10 is false, 1 < 0.1f * 20 is true; of four equal bins the first three stay


def rotation_histogram(shape):
    """Independent matches, shape[k] of them in bin 2 + 2 k."""
    S = Search("rotation_histogram%s" % (shape,), check_ori=True)
    spot = 0
    for cnt in shape:
        for _ in range(cnt):
            S.train(spot, bits(0)); spot += 1
    spot = 0
    for k, cnt in enumerate(shape):
        for _ in range(cnt):
            S.query(spot, bits(3), angle=30.0 * (2 + 2 * k)); spot += 1
    S.build()
    S.want = {v: {"cut": HISTOGRAM_CUT[shape]} for v in ORIENTED}
    return S


def train_sizes(variant):
    return (1, 63, 64, 65, LDS_SWITCH[variant], LDS_SWITCH[variant] + 1, LDS_LIMIT[variant])


def train_size(N2, blocked=False):
    """N2 train key points, the contested pair u, w of `counted` at the END (indices N2 - 2, N2 - 1: the top of the LDS arrays), N2 - 2 fillers in front.  blocked: u may not be
    matched (train_blocked / skipF / skip2), so the first query takes w and the second nothing it wants."""
    S = Search("train_size%d%s" % (N2, "_blocked" if blocked else ""))
    if N2 == 1:
        S.train(0, bits(0)); S.query(0, bits(4))
        return S.build()
    S.filler(N2 - 2)
    S.train(0, bits(0), blocked=int(blocked)); S.train(0, bit_range(100, 120))
    S.query(0, bits(4)); S.query(0, bits(2))
    return S.build()


# how each entry point is called on a Search: the same for the device (cube_slam_amd.matcher.ORBmatcher `m`, frame set) and the CPU judges
def world_points(S):
    """Map points that project onto the queries' centres with fx = fy = 1, cx = cy = 0 and the identity pose: (x, y, 1)."""
    return np.concatenate([S.qxy, np.ones((len(S.q), 1), np.float32)], axis=1).astype(np.float32)


def reloc_points(S):
    """The relocalisation search's map points: max_distance = |p|, so PredictScale gives ceil(log(1) / log(1.2)) = level 0 and the radius is th."""
    wp = world_points(S)
    d = np.sqrt((wp.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    return {"world_pos": wp, "normal": np.zeros_like(wp), "min_distance": (d * f32(0.5)).astype(np.float32), "max_distance": d, "skip": np.zeros(len(wp), np.uint8), "mp_desc": S.qdesc}


EYE = np.eye(4, dtype=np.float32)[:3]
LOG_SF = float(np.float32(math.log(1.2)))


def run_device(variant, S, m):
    """-> (match vector, nmatches); `m` has S's train frame set (the BoW searches take both sides as arguments)."""
    m.mfNNratio, m.mbCheckOrientation = S.nnratio, S.check_ori
    tb = S.tblocked if S.tblocked.any() else None
    if variant == PROJ:
        return m.SearchByProjectionFrame(world_points(S), np.ones(len(S.q), np.uint8), S.blocks, S.qdesc, S.qlevel, S.qangle, EYE, 1.0, 1.0, 0.0, 0.0, SF, S.r, train_blocked=tb)
    if variant == LOCAL:
        return m.SearchByProjectionLocalMap(S.qxy, np.zeros(len(S.q), np.float32), S.qlevel, np.ones(len(S.q), np.uint8), S.blocks, S.qdesc, SF, S.r / 4.0, tb)
    if variant == INIT:
        m12, _, n = m.SearchForInitialization(S.qkeys, S.qdesc, S.qxy, int(S.r))
        return m12, n
    if variant == BOW:
        return m.SearchByBoW(S.qkeys, S.qdesc, S.qnode, np.zeros(len(S.q), np.uint8), S.keys, S.desc, S.tnode, tb)
    if variant == BOWKF:
        return m.SearchByBoWKeyFrames(S.qkeys, S.qdesc, S.qnode, np.zeros(len(S.q), np.uint8), S.keys, S.desc, S.tnode, S.tblocked)
    p = reloc_points(S)
    tm, n, outside = m.SearchByProjectionReloc(np.eye(3), np.zeros(3), np.zeros(3), p["world_pos"], p["min_distance"], p["max_distance"], p["skip"], S.qangle, p["mp_desc"], 1.0, 1.0, 0.0, 0.0,
                                               LOG_SF, SF, S.r, ORB_DIST, tb)
    assert outside == 0
    return tm, n


def run_judge(variant, S, oracle):
    """The CPU side of the same call: the oracle, or tests/sim3_restatement.py for the relocalisation search."""
    tb = S.tblocked if S.tblocked.any() else None
    if variant == CLAIM:
        from tests import sim3_restatement as R
        p = reloc_points(S)
        tm, n, outside = R.search_by_projection_reloc(oracle, R.make_frame(oracle, S.keys, S.desc, BOUNDS), np.eye(3), np.zeros(3), np.zeros(3), p, S.qangle, (1.0, 1.0, 0.0, 0.0), LOG_SF, SF, S.r,
                                                      ORB_DIST, S.check_ori, tb)
        assert outside == 0
        return tm, n
    F = oracle.make_frame(S.keys, S.desc, BOUNDS)
    if variant == PROJ:
        return oracle.search_by_projection_frame(F, world_points(S), np.ones(len(S.q), np.uint8), S.blocks, S.qdesc, S.qlevel, S.qangle, EYE, 1.0, 1.0, 0.0, 0.0, SF, S.r, S.check_ori, tb)
    if variant == LOCAL:
        return oracle.search_local_map(F, S.qxy, np.zeros(len(S.q), np.float32), S.qlevel, np.ones(len(S.q), np.uint8), S.blocks, S.qdesc, SF, S.r / 4.0, S.nnratio, tb)
    Q = oracle.make_frame(S.qkeys, S.qdesc, BOUNDS)
    if variant == INIT:
        m12, _, n = oracle.search_for_initialization(Q, F, S.qxy, int(S.r), S.nnratio, S.check_ori)
        return m12, n
    if variant == BOW:
        return oracle.search_by_bow(Q, S.qnode, np.zeros(len(S.q), np.uint8), F, S.tnode, tb, S.nnratio, S.check_ori)
    return oracle.search_by_bow_kf(Q, S.qnode, np.zeros(len(S.q), np.uint8), F, S.tnode, S.tblocked, S.nnratio, S.check_ori)


def claim_cases(variant):
    """Every Search that `variant` runs, by name."""
    c = [domino(variant)] + [counted(n) for n in COUNTS] + [rs_nc(), thresholds()] + [train_size(n) for n in train_sizes(variant)]
    if variant != INIT:
        c.append(train_size(65, blocked=True))
    if variant in ORIENTED:
        c += [rotation_bins()] + [rotation_histogram(s) for s in HISTOGRAM_SHAPES]
    if variant == PROJ:
        c.append(proj_overwrite())
    if variant == LOCAL:
        c.append(local_levels())
    if variant == INIT:
        c += [init_displacement(), init_equal(), init_stale_histogram()]
    return c


# ----------------------------------------------------------------------------------------------- 6. small kernels
KNN_SIZES = (255, 256, 257)


def knn_case(nq, nt):
    """Train descriptors bits(3 + j % 50) (so every value repeats: ties everywhere), the last tile's only or first entry the unique minimum bits(1) for half of the queries.
    Queries are bits(0) (even) and bits(60) (odd).  Expected (first index of the minimum, minimum, second)."""
    t = np.stack([bits(3 + j % 50) for j in range(nt)]); t[nt - 1] = bits(1)
    q = np.stack([bits(0) if i % 2 == 0 else bits(60) for i in range(nq)])
    # bits(0): the minimum 1 is the last entry, the second best 3 (index 0).  bits(60): |60 - (3 + j % 50)| is smallest (8) at j % 50 == 49, first at j = 49, and again at j = 99, ...
    bi = np.where(np.arange(nq) % 2 == 0, nt - 1, 49).astype(np.int32)
    bd = np.where(np.arange(nq) % 2 == 0, 1, 8).astype(np.int32)
    sd = np.where(np.arange(nq) % 2 == 0, 3, 8).astype(np.int32)  # the duplicate at j = 99: second == best
    return q, t, (bi, bd, sd)


TRI_F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)  # the epipolar line of (x, y) is the row y


def triangulation_case(n_node, N1=4, zero_F=False):
    """KF1: N1 key points on the row y = 100 in node 3.  KF2: node 3 holds n_node features on that row (n_node around the 64-lane stride), all of them 20 bits from KF1's
    descriptor -- the LARGEST index wins -- except: the last one is 51 bits away (no candidate) and the one before it exactly 50 (a candidate, but not the minimum); feature 1 is
    off the row by 30 px.  Expected: every KF1 key point is matched to feature n_node - 3."""
    k1 = make_keys([(100.0 + 10 * i, 100.0) for i in range(N1)])
    d1 = np.stack([bits(0)] * N1)
    k2 = make_keys([(400.0 + i, 130.0 if i == 1 else 100.0) for i in range(n_node)])
    d2 = np.stack([bits(20)] * n_node); d2[n_node - 1] = bits(51); d2[n_node - 2] = bits(50)
    F12 = np.zeros((3, 3), np.float32) if zero_F else TRI_F12
    exp = np.full(N1, -1 if zero_F else n_node - 3, np.int32)
    return dict(k1=k1, d1=d1, node1=np.full(N1, 3, np.int32), k2=k2, d2=d2, node2=np.full(n_node, 3, np.int32), F12=F12, expected=(exp, 0 if zero_F else N1))


def triangulation_threshold():
    """A single candidate at exactly TH_LOW = 50 bits is matched, one at 51 is not."""
    k1 = make_keys([(100.0, 100.0), (110.0, 100.0)]); k2 = make_keys([(400.0, 100.0), (410.0, 100.0)])
    return dict(k1=k1, d1=np.stack([bits(0)] * 2), node1=np.array([1, 2], np.int32), k2=k2, d2=np.stack([bits(50), bits(51)]), node2=np.array([1, 2], np.int32), F12=TRI_F12,
                expected=(np.array([0, -1], np.int32), 1))


def orientation_cut_case(N1):
    """SearchForTriangulation with N1 independent matches (a node per pair; N1 around the 1 024-thread stride of match_orient_cut): key point i has rotation bin i % 5 with
    bin sizes descending, so bins 0, 1, 2 survive."""
    k1 = make_keys([(100.0, 100.0)] * N1, angle=30.0 * (np.arange(N1) % 5))
    k2 = make_keys([(400.0, 100.0)] * N1)
    d = np.stack([bits(0)] * N1)
    node = np.arange(N1, dtype=np.int32)
    exp = np.where(np.arange(N1) % 5 < 3, np.arange(N1), -1).astype(np.int32)
    return dict(k1=k1, d1=d, node1=node, k2=k2, d2=d, node2=node, F12=TRI_F12, expected=(exp, int((exp >= 0).sum())))


def bow_nodes():
    """SearchByBoW with nodes of 64 and 65 frame features (the 64-lane stride of match_bow_dists), the best in the last place, and key-frame features of node -1 and of a node the
    frame does not have."""
    S = Search("bow_nodes")
    for s, n in ((0, 64), (1, 65)):
        for c in range(n):
            S.train(s, bits(5 if c == n - 1 else 60 + c % 3))
    S.query(0, bits(0)); S.query(1, bits(0)); S.query(2, bits(0)); S.query(3, bits(0))
    S.build()
    S.qnode[2] = -1; S.qnode[3] = 77
    S.closed = {}
    mf = np.full(129, -1, np.int32); mf[63] = 0; mf[128] = 1
    S.closed[BOW] = (mf, 2); S.closed[BOWKF] = (np.array([63, 128, -1, -1], np.int32), 2)
    return S


# ----------------------------------------------------------------------------------------------- 5. the window stream (ORBmatcherStream.search)
STREAM_W, STREAM_H = 320, 240
STREAM_ORB = (500, 1.2, 1, 20, 7)  # ONE pyramid level: an isolated bright pixel is then exactly one key point, at its own position, level 0
STREAM_BOUNDS = (0.0, float(STREAM_W), 0.0, float(STREAM_H))
STREAM_DOTS = ([(60, 60), (100, 60), (140, 60), (180, 100), (220, 100), (260, 140)],
               [(60, 100), (100, 100), (140, 100), (180, 140), (220, 60), (260, 60)],
               [(80, 80), (120, 80), (160, 120), (200, 120), (240, 160), (280, 160)],
               [(160, 120)])


def stream_images():
    """Four frames of isolated bright pixels: three pairs (f, f + 1); the last frame holds ONE key point.  Every key point has the same descriptor (the same neighbourhood)."""
    imgs = np.full((len(STREAM_DOTS), STREAM_H, STREAM_W), 40, np.uint8)
    for f, dots in enumerate(STREAM_DOTS):
        for x, y in dots:
            imgs[f, y, x] = 250
    return imgs


def stream_case(frames, middle_valid):
    """frames: (keys, descriptors) of the four frames as extracted.  The queries of pair p are frame p's key points in the extractor's order; query i is sent onto the train key
    point with a chosen index (its position, through the identity pose with fx = fy = 1, cx = cy = 0), window radius 5, every descriptor equal:
      pair 0   query i -> train i for i = 2, 3, 4; queries 0 and 1 both -> train 1 (the first holds it, the second finds nothing else); the LAST query -> train 0
      pair 1   query i -> train i: its FIRST query and pair 0's last, neighbours in the query array, want the key point of the same index in two different frames; with
               middle_valid = False no query of this pair is valid
      pair 2   every query -> the only train key point, none of them blocking: each claim counts and the last one stays
    Returns the arguments of the search and, per pair, (train_match, nmatches)."""
    n = [len(k) for k, _ in frames]
    assert n == [6, 6, 6, 1]
    target = [[1, 1, 2, 3, 4, 0], [0, 1, 2, 3, 4, 5], [0] * 6]
    wp, valid, blocks = [], [], []
    for p in range(3):
        tk = frames[p + 1][0]
        wp.append(np.stack([tk["x"][target[p]], tk["y"][target[p]], np.ones(6, np.float32)], axis=1).astype(np.float32))
        valid.append(np.full(6, int(p != 1 or middle_valid), np.uint8))
        blocks.append(np.full(6, int(p != 2), np.uint8))
    desc = [frames[p][1] for p in range(3)]
    expected = [(np.array([5, 0, 2, 3, 4, -1], np.int32), 5),
                (np.arange(6, dtype=np.int32), 6) if middle_valid else (np.full(6, -1, np.int32), 0),
                (np.array([5], np.int32), 6)]
    return dict(world_pos=wp, valid=valid, blocks=blocks, mp_desc=desc, Tcw=[EYE] * 3, th=5.0, sf=np.ones(1, np.float32), expected=expected)
