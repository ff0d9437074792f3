"""Designed inputs for the stereo searches (include/cubeslam_hip/stereo_search.h; match_project<true>, match_candidates<true> of cube_slam_amd/csrc/match.hip): each case with
the result it must give.  A helper, not a test module; it imports neither the oracle nor the device library.  tests/test_stereo_search_patterns.py holds the restatement
(tests/stereo_search_restatement.py) to these expectations on the CPU and asserts every case's precondition; tests/test_stereo_search_gpu.py holds the device to the restatement on
the same inputs; tests/test_stereo_search_restatement_pins.py holds the restatement to the reference's text.

Frame bounds, the spots of `Search` and the bits(n) descriptors are those of tests/match_patterns.py, so every border is exact.  The camera is fx = fy = 1, cx = cy = 0 with the
identity pose: a map point (x z, y z, z) with z = 1 or 2 projects onto (x, y) exactly, invzc = 1 / z, and with mbf = BF the predicted right coordinate is x - BF / z, exact as
well.  With Tcw = I the camera centre is -0 and tlc.z is LastFrame's tz itself, so a direction case chooses tlc.z to the ulp; the `general` cases take seeded rotations."""
import numpy as np

from tests import match_patterns as P
from tests import stereo_search_restatement as R
from tests.match_patterns import BOUNDS, CELL, EYE, SF, Search, above, below, bit_range, bits, make_keys

f32 = np.float32
BF, MB = 8.0, 0.5
INTR = (1.0, 1.0, 0.0, 0.0)
TINY = f32(np.nextafter(f32(0), f32(1)))  # the smallest positive float: tested


def pose(tz=0.0, Rm=None, t=None):
    T = np.zeros((3, 4), np.float32)
    T[:, :3] = np.eye(3) if Rm is None else Rm
    T[:, 3] = (0.0, 0.0, tz) if t is None else t
    return T


TLW = {R.NEITHER: pose(0.0), R.FORWARD: pose(1.0), R.BACKWARD: pose(-1.0)}  # against MB = 0.5


class Case:
    """One search.  kind "proj": SearchByProjection(CurrentFrame, LastFrame, th, bMono); the queries are the last frame's key points with their map points (x z, y z, z).
    kind "local": SearchByProjection(F, vpMapPoints, th) over the fields isInFrustum leaves (proj_xy, proj_xr, level; view_cos = 0, so the radius is 4 th scale[level])."""

    def __init__(self, name, kind, keys, desc, u_right, qxy, qdesc, qlevel, blocks, qangle=None, tblocked=None, depth=None, proj_xr=None, th=10.0, sf=SF, nnratio=0.9,
                 check_ori=False, Tlw=None, mb=MB, bf=BF, mono=0, Tcw=EYE, valid=None, closed=None, want_direction=None):
        nq = len(qxy)
        self.name, self.kind, self.keys, self.desc = name, kind, keys, np.asarray(desc, np.uint8).reshape(len(keys), 32)
        self.u_right = np.asarray(u_right, np.float32)
        assert len(self.u_right) == len(keys)
        self.qxy = np.asarray(qxy, np.float32).reshape(nq, 2); self.qdesc = np.asarray(qdesc, np.uint8).reshape(nq, 32); self.qlevel = np.asarray(qlevel, np.int32)
        self.blocks = np.asarray(blocks, np.uint8); self.qangle = np.zeros(nq, np.float32) if qangle is None else np.asarray(qangle, np.float32)
        self.tblocked = None if tblocked is None or not np.any(tblocked) else np.asarray(tblocked, np.uint8)
        self.depth = np.ones(nq, np.float32) if depth is None else np.asarray(depth, np.float32)
        self.proj_xr = (self.qxy[:, 0] - f32(bf)).astype(np.float32) if proj_xr is None else np.asarray(proj_xr, np.float32)
        self.th, self.sf, self.nnratio, self.check_ori = float(th), np.asarray(sf, np.float32), nnratio, check_ori
        self.Tcw, self.Tlw, self.mb, self.bf, self.mono = np.asarray(Tcw, np.float32), TLW[R.NEITHER] if Tlw is None else np.asarray(Tlw, np.float32), float(mb), float(bf), int(mono)
        self.valid = np.ones(nq, np.uint8) if valid is None else np.asarray(valid, np.uint8)
        self.closed, self.want_direction = closed, want_direction

    @property
    def world_pos(self):
        z = self.depth
        return np.stack([self.qxy[:, 0] * z, self.qxy[:, 1] * z, z], axis=1).astype(np.float32)

    # the three ways a case is run: the restatement, the stereo entry, the monocular entry the library had
    def restate(self, stereo_test=True, mono=None):
        mono = self.mono if mono is None else mono
        if self.kind == "proj":
            return R.search_by_projection_frame(self.keys, self.desc, BOUNDS, self.u_right, self.world_pos, self.valid, self.blocks, self.qdesc, self.qlevel, self.qangle, self.Tcw,
                                                self.Tlw, INTR, self.bf, self.mb, mono, self.sf, self.th, self.check_ori, self.tblocked, stereo_test=stereo_test)
        tm, n, nc, _ = R.search_local_map(self.keys, self.desc, BOUNDS, self.u_right, self.qxy, self.proj_xr, np.zeros(len(self.qxy), np.float32), self.qlevel, self.valid, self.blocks,
                                          self.qdesc, self.sf, self.th / 4.0, self.nnratio, self.tblocked, stereo_test=stereo_test)
        return tm, n, R.NEITHER, nc

    def device(self, m, u_right="host", mono=None):
        """-> (train_match, nmatches, direction, candidates); `m`: a cube_slam_amd.matcher.ORBmatcher.  u_right: "host", or a callable that turns the array into a device address."""
        mono = self.mono if mono is None else mono
        m.mfNNratio, m.mbCheckOrientation = self.nnratio, self.check_ori
        m.set_frame(self.keys, self.desc, BOUNDS)
        if not (mono and self.kind == "proj"):
            m.set_u_right(self.u_right if u_right == "host" else u_right(self.u_right), n=len(self.u_right))
        if self.kind == "proj":
            tm, n = m.SearchByProjectionFrameStereo(self.world_pos, self.valid, self.blocks, self.qdesc, self.qlevel, self.qangle, self.Tcw, *INTR, self.sf, self.th, self.Tlw, self.bf,
                                                    self.mb, bool(mono), self.tblocked)
            d = m.last_direction
        else:
            tm, n = m.SearchByProjectionLocalMap(self.qxy, np.zeros(len(self.qxy), np.float32), self.qlevel, self.valid, self.blocks, self.qdesc, self.sf, self.th / 4.0, self.tblocked,
                                                 proj_xr=self.proj_xr)
            d = R.NEITHER
        return tm, n, d, m.last_candidate_stats()["candidates"]

    def device_mono(self, m):
        """The entry the library had: cs_match_by_projection_frame / cs_match_local_map."""
        m.mfNNratio, m.mbCheckOrientation = self.nnratio, self.check_ori
        m.set_frame(self.keys, self.desc, BOUNDS)
        if self.kind == "proj":
            return m.SearchByProjectionFrame(self.world_pos, self.valid, self.blocks, self.qdesc, self.qlevel, self.qangle, self.Tcw, *INTR, self.sf, self.th, self.tblocked)
        return m.SearchByProjectionLocalMap(self.qxy, np.zeros(len(self.qxy), np.float32), self.qlevel, self.valid, self.blocks, self.qdesc, self.sf, self.th / 4.0, self.tblocked)

    # the frustum form of a local case whose queries are all of level 0: map points (x, y, 1) seen from the origin with max_distance = their distance (PredictScale gives level 0)
    def frustum_points(self):
        assert self.kind == "local" and not self.qlevel.any() and len(self.sf) >= 1 and self.sf[0] == 1.0
        wp = np.concatenate([self.qxy, np.ones((len(self.qxy), 1), np.float32)], axis=1).astype(np.float32)
        d = np.sqrt((wp.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
        return {"world_pos": wp, "normal": np.zeros_like(wp), "min_distance": (d * f32(0.5)).astype(np.float32), "max_distance": d, "skip": (1 - self.valid).astype(np.uint8),
                "mp_desc": self.qdesc}

    def device_frustum(self, m, stereo=True):
        """Tracking::SearchLocalPoints in one call: viewing_cos_limit 0 lets the zero normals through with view_cos = 0 (radius 4 th)."""
        p = self.frustum_points()
        m.mfNNratio = self.nnratio
        m.set_frame(self.keys, self.desc, BOUNDS)
        if stereo:
            m.set_u_right(self.u_right)
        return m.SearchLocalPoints(np.eye(3), np.zeros(3), np.zeros(3), p["world_pos"], p["normal"], p["min_distance"], p["max_distance"], p["skip"], self.blocks, p["mp_desc"], *INTR,
                                   self.bf, P.LOG_SF, self.sf, self.th / 4.0, 0.0, self.tblocked, stereo=stereo)


def from_search(name, kind, S, u_right, **kw):
    """A match_patterns.Search (built) as a case; a local case takes the search's nnratio."""
    kw.setdefault("nnratio", S.nnratio); kw.setdefault("check_ori", S.check_ori)
    return Case(name, kind, S.keys, S.desc, u_right, S.qxy, S.qdesc, S.qlevel, S.blocks, qangle=S.qangle, tblocked=S.tblocked, th=S.r, **kw)


def ur_of(S, q, z=1.0):
    """The predicted right coordinate of query q at depth z."""
    return f32(S.qxy[q, 0] - f32(f32(BF) * f32(f32(1.0) / f32(z))))


# ----------------------------------------------------------------------------------------------- direction
def _one_point(name, **kw):
    S = Search(name)
    S.train(0, bits(0)); S.query(0, bits(3))
    S.build()
    kw.setdefault("closed", (np.array([0], np.int32), 1))
    return from_search(name, "proj", S, [-1.0], **kw)


def _rotation(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32)


def direction_cases():
    """tlc.z equal to mb, one ulp above and one below, the same for -tlc.z, mono = 1 with a large motion, and three pairs of general poses whose baseline is put on tlc.z itself
    and one ulp below its magnitude (no query is valid in those: the poses are not the designed camera)."""
    mb = f32(MB)
    c = [_one_point("dir_equal", Tlw=pose(mb), want_direction=R.NEITHER), _one_point("dir_above", Tlw=pose(above(mb)), want_direction=R.FORWARD),
         _one_point("dir_below", Tlw=pose(below(mb)), want_direction=R.NEITHER), _one_point("back_equal", Tlw=pose(-mb), want_direction=R.NEITHER),
         _one_point("back_above", Tlw=pose(-above(mb)), want_direction=R.BACKWARD), _one_point("back_below", Tlw=pose(-below(mb)), want_direction=R.NEITHER),
         _one_point("mono_large", Tlw=pose(5.0), mono=1, want_direction=R.NEITHER)]
    for seed in (1, 2, 3, 4):
        rng = np.random.default_rng(100 + seed)
        Tcw, Tlw = pose(Rm=_rotation(seed), t=rng.uniform(-2, 2, 3)), pose(Rm=_rotation(10 + seed), t=rng.uniform(-2, 2, 3))
        z = R.tlc_z(Tcw, Tlw)
        moving = R.FORWARD if z > 0 else R.BACKWARD
        for tag, b, want in (("on", abs(z), R.NEITHER), ("under", below(abs(z)), moving)):
            c.append(_one_point("general%d_%s" % (seed, tag), Tcw=Tcw, Tlw=Tlw, mb=float(b), valid=[0], closed=(np.array([-1], np.int32), 0), want_direction=want))
    return c


# ----------------------------------------------------------------------------------------------- level ranges
def level_case(o, d):
    """One query of level o over three key points of its spot.  o = 0: levels 7, 1, 0 at 1, 5, 9 bits -- forward (0, -1) checks no level and takes the level-7 key point,
    backward (0, 0) only level 0, neither (-1, 1) the level-1 one.  o = 7: levels 3, 6, 7 -- forward (7, -1) level 7, backward (0, 7) level 3, neither (6, 8) level 6."""
    S = Search("levels_o%d_%d" % (o, d))
    for lev, n in zip((7, 1, 0) if o == 0 else (3, 6, 7), (1, 5, 9)):
        S.train(0, bits(n), level=lev)
    S.query(0, bits(0), level=o)
    S.build()
    winner = {R.FORWARD: 0 if o == 0 else 2, R.BACKWARD: 2 if o == 0 else 0, R.NEITHER: 1}[d]
    m = np.full(3, -1, np.int32); m[winner] = 0
    return from_search(S.name, "proj", S, [-1.0] * 3, Tlw=TLW[d], closed=(m, 1), want_direction=d)


def level_cases():
    return [level_case(o, d) for o in (0, 7) for d in (R.FORWARD, R.BACKWARD, R.NEITHER)]


# ----------------------------------------------------------------------------------------------- the mvuRight test
UR_SPOTS = ("equal_plus", "above_plus", "zero", "minus_one", "tiny", "equal_minus", "below_minus")
UR_KEPT = {"equal_plus": True, "above_plus": False, "zero": True, "minus_one": True, "tiny": False, "equal_minus": True, "below_minus": False}


def u_right_case():
    """One key point per spot at radius 10: mvuRight at er == radius (kept), one ulp outside (dropped), on both sides; exactly 0 and -1 (not tested, although 0 is far outside);
    the smallest positive float (tested, dropped).  Spot 7: the Hamming-best key point fails the test and the second takes the query."""
    S = Search("u_right")
    for s in range(len(UR_SPOTS)):
        S.train(s, bits(0))
    S.train(7, bits(2)); S.train(7, bits(6))
    for s in range(8):
        S.query(s, bits(0) if s == 7 else bits(3))
    S.build()
    r = f32(10.0)
    ur = [ur_of(S, q) for q in range(8)]
    u = [f32(ur[0] + r), above(f32(ur[1] + r)), f32(0.0), f32(-1.0), TINY, f32(ur[5] - r), below(f32(ur[6] - r)), f32(ur[7] + f32(20.0)), f32(ur[7] + f32(1.0))]
    m = np.array([q if UR_KEPT[name] else -1 for q, name in enumerate(UR_SPOTS)] + [-1, 7], np.int32)
    c = from_search("u_right", "proj", S, u, closed=(m, int((m >= 0).sum())))
    c.radius, c.ur = r, ur
    return c


def u_right_ulp_case():
    """The same border to the ulp of the RADIUS: with mbf = 50 the spot at x = 64 predicts ur = 14, and a right coordinate below 16 has ulps finer than 10's.  mvuRight = 4:
    er == 10, kept.  4 - 2^-20: er = 10 + 2^-20, the float above 10, dropped.  The float below 4 (4 - 2^-22): the exact difference 10 + 2^-22 ROUNDS to 10 as a float -- er is a
    float in the reference (:1462) -- and the candidate is kept."""
    S = Search("u_right_ulp")
    for s in (0, 14, 28):  # three spots in the column x = 64
        S.train(s, bits(0)); S.query(s, bits(3))
    S.build()
    assert (S.qxy[:, 0] == 64.0).all()
    u = [f32(4.0), f32(4.0 - 2.0 ** -20), below(f32(4.0))]
    c = from_search("u_right_ulp", "proj", S, u, bf=50.0, closed=(np.array([0, -1, 2], np.int32), 2))
    c.radius, c.ur = f32(10.0), [f32(14.0)] * 3
    return c


def domino_stereo():
    """match_patterns.domino with the test in the chain.  Query 0 (depth 1, ur = x - 8) loses t_0 to the test (mvuRight = x + 6: er = 14 > 10), so it takes t_1 and does NOT
    claim t_0; query 1 (depth 2, ur = x - 4: er = 10, kept; its map point has no observations, blocks = 0) takes the unclaimed t_0; query 2 finds t_1 claimed and moves on, and
    so forth through the whole batch.  Result: t_0 <- query 1, t_1 <- query 0, t_i <- query i."""
    S = P.domino(P.PROJ)
    u = np.full(65, -1.0, np.float32); u[0] = f32(S.qxy[0, 0] + f32(6.0))
    depth = np.ones(64, np.float32); depth[1] = 2.0
    m = np.full(65, -1, np.int32); m[:64] = np.arange(64); m[0], m[1] = 1, 0
    c = from_search("domino_stereo", "proj", S, u, depth=depth, closed=(m, 64))
    c.blocks[1] = 0
    return c


def local_ratio_case():
    """SearchByProjection(F, vpMapPoints): best (10 bits) and second (19) on one level with nnratio 0.5 -- 10 > 9.5, rejected.  Spot 0: the test removes the second and the ratio
    rule accepts; spot 1: the second sits at er == radius, stays, and the query is rejected; spot 2: one ulp further out, removed."""
    S = Search("local_ratio", nnratio=0.5)
    for s in range(3):
        S.train(s, bits(10)); S.train(s, bits(19))
        S.query(s, bits(0))
    S.build()
    r = f32(10.0)
    xr = [ur_of(S, q) for q in range(3)]
    u = [-1.0, f32(xr[0] + f32(11.0)), -1.0, f32(xr[1] + r), -1.0, above(f32(xr[2] + r))]
    c = from_search("local_ratio", "local", S, u, closed=(np.array([0, -1, -1, -1, 2, -1], np.int32), 2))
    c.radius, c.xr = r, xr
    return c


# ----------------------------------------------------------------------------------------------- seams
SEAM_COUNTS = (63, 64, 65, 129)


def counted_stereo(nq, kind):
    """match_patterns.counted at match_resolve's batch seams with the test on the contested pair: u is dropped for every query, so the first of the pair takes w (24 bits away)
    and the second finds nothing; every third other key point carries a right coordinate that passes."""
    S = P.counted(nq)
    u = np.full(nq, -1.0, np.float32)
    for i in range(0, nq - 2, 3):
        u[i] = ur_of(S, i)
    u[nq - 2] = f32(ur_of(S, nq - 2) + f32(30.0))
    m = np.arange(nq, dtype=np.int32); m[nq - 2] = -1; m[nq - 1] = nq - 2
    return from_search("counted%d_%s" % (nq, kind), kind, S, u, closed=(m, nq - 1))


def window_frame_small():
    """A key point at every cell centre of columns 0 .. 20, rows 0 .. 6, and 21 along the last row at y = 758 (what the 17-cell window that comes up from below the grid reaches);
    all of level 0.  Key point i carries mvuRight -1 (i % 3 == 0), x - BF (1: passes in every window that holds it: er = |dx| < r) or x - BF + 1000 (2: dropped)."""
    pts = [(CELL * c, CELL * r) for r in range(7) for c in range(21)] + [(CELL * c, 758.0) for c in range(21)]
    keys = make_keys(pts)
    desc = np.stack([bits(1 + (7 * i) % 97) for i in range(len(keys))])
    i = np.arange(len(keys))
    u = np.where(i % 3 == 0, f32(-1.0), keys["x"] - f32(BF) + np.where(i % 3 == 2, f32(1000.0), f32(0.0))).astype(np.float32)
    return keys, desc, u


WINDOW_SEAMS = ((40.0, 40.0, 17.0, 16), (140.0, 873.0, 120.0, 17))  # (x, y, r, cells): MC_G = 16 lanes walk a window


def window_case(x, y, r, cells):
    keys, desc, u = window_frame_small()
    c = Case("window%d" % cells, "local", keys, desc, u, [(x, y)], [bits(0)], [0], [1], th=4.0, sf=np.array([r / 4.0], np.float32), nnratio=1.0)
    c.cells = cells
    return c


def rs_nc_stereo():
    """8 and 9 surviving candidates (RS_NC = 8 stay in registers) of 12 and 13, dropped ones interleaved among them: every dropped key point is 1 bit from the query and would
    win; the minimum of the survivors (10 bits) is the last of them, the others 60 bits away.  Spot 2: all three candidates are dropped."""
    S = Search("rs_nc_stereo")
    drop = {0: (1, 3, 6, 9), 1: (0, 4, 8, 11)}
    u = []
    for s, n in ((0, 12), (1, 13)):
        last = max(k for k in range(n) if k not in drop[s])
        for k in range(n):
            S.train(s, bits(1) if k in drop[s] else bits(10) if k == last else bits(60))
    for k in range(3):
        S.train(2, bits(1))
    for s in range(3):
        S.query(s, bits(0))
    S.build()
    for s, n in ((0, 12), (1, 13)):
        u += [f32(ur_of(S, s) + f32(50.0)) if k in drop[s] else (ur_of(S, s) if k % 2 else f32(-1.0)) for k in range(n)]
    u += [f32(ur_of(S, 2) + f32(50.0))] * 3
    m = np.full(28, -1, np.int32); m[11] = 0; m[12 + 12] = 1
    c = from_search("rs_nc_stereo", "proj", S, u, closed=(m, 2))
    c.survivors = (8, 9, 0)
    return c


def empty_train(kind):
    """A train frame without key points."""
    return Case("empty_train_" + kind, kind, make_keys([]), np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), [(128.0, 128.0)], [bits(0)], [0], [1],
                closed=(np.zeros(0, np.int32), 0))


def seam_cases():
    return ([counted_stereo(n, k) for n in SEAM_COUNTS for k in ("proj", "local")] + [window_case(*w) for w in WINDOW_SEAMS] + [rs_nc_stereo(), empty_train("proj"), empty_train("local")])


# ----------------------------------------------------------------------------------------------- equivalences
EQUIVALENCE_MAX_TRAIN = 2500


def equivalence_cases(kind):
    """The claim cases of match_patterns (up to EQUIVALENCE_MAX_TRAIN train key points) with right coordinates that are never tested -- -1 and exactly 0, alternating -- and neither
    direction: the stereo entries must give the bytes of the monocular ones."""
    out = []
    for S in P.claim_cases(P.PROJ if kind == "proj" else P.LOCAL):
        if len(S.t) > EQUIVALENCE_MAX_TRAIN:
            continue
        u = np.where(np.arange(len(S.t)) % 2 == 0, f32(-1.0), f32(0.0)).astype(np.float32)
        out.append(from_search("eq_%s_%s" % (kind, S.name), kind, S, u, sf=SF))
    return out


def designed_cases():
    """Every case with a stereo branch in it, by name."""
    return direction_cases() + level_cases() + [u_right_case(), u_right_ulp_case(), domino_stereo(), local_ratio_case()] + seam_cases()


# ----------------------------------------------------------------------------------------------- the window stream
STREAM_TLW = (TLW[R.FORWARD], TLW[R.BACKWARD], TLW[R.NEITHER])
STREAM_DIRECTIONS = (R.FORWARD, R.BACKWARD, R.NEITHER)


def stream_u_right(frames, seed=7):
    """mvuRight of the current frames of match_patterns.stream_images(), packed: the key point's x less a seeded disparity of 0 .. 16 px (the queries predict x - BF = x - 8 and
    the radius is 5), every fourth key point without one."""
    rng = np.random.default_rng(seed)
    out = []
    for k, _ in frames[1:]:
        u = (k["x"] - rng.uniform(0.0, 16.0, len(k)).astype(np.float32)).astype(np.float32)
        u[np.arange(len(k)) % 4 == 3] = -1.0
        out.append(u)
    return out
