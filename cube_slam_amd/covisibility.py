"""Python host-side mirror of the graph work at both ends of ORB_SLAM2::LocalMapping's key-frame cycle (include/cubeslam_hip/covisibility.h): KeyFrame::UpdateConnections
(reference orb_object_slam/src/KeyFrame.cc:345-437) with the AddConnection / UpdateBestCovisibles it causes on the other key frames (:140-180), LocalMapping::KeyFrameCulling
(LocalMapping.cc:833-902) and LocalMapping::MapPointCulling (:249-302).  ctx = None takes the library's host forms (the same predicates, no device)."""
import ctypes as C
import os
import re

import numpy as np

from ._lib import _HERE, CubeSlamError, STATUS, check, lib, ptr

CS_ERR_CAPACITY = -4
MP_BAD, MP_DYNAMIC = 1, 2  # mp_flags
KF_ID0, KF_NOT_ERASE = 1, 2  # kf_flags
KEPT, CULLED, TO_BE_ERASED, SKIPPED = 0, 1, 2, 3  # verdicts of KeyFrameCulling
COUNTER_TILE = 4096  # COVIS_COUNTER_TILE of csrc/covis_math.h: key-frame indices per sweep of the vote kernel (n_kf above it takes several sweeps)


def source_counter_tile():
    """COVIS_COUNTER_TILE as the kernel source states it."""
    m = re.search(r"constexpr\s+int\s+COVIS_COUNTER_TILE\s*=\s*(\d+)", open(os.path.join(_HERE, "csrc", "covis_math.h")).read())
    return int(m.group(1))


class CsObsTable(C.Structure):
    """cs_obs_table of include/cubeslam_hip/covisibility.h."""
    _fields_ = [("n_kf", C.c_int), ("n_points", C.c_int), ("obs_off", C.POINTER(C.c_int)), ("obs_kf", C.POINTER(C.c_int)), ("obs_octave", C.POINTER(C.c_int)),
                ("obs_stereo", C.POINTER(C.c_uint8)), ("mp_nobs", C.POINTER(C.c_int)), ("mp_flags", C.POINTER(C.c_uint8))]


class ObsTable:
    """The observation side of the map as flat arrays: mObservations of every point as runs of ascending key-frame index (obs_off / obs_kf, with obs_octave =
    mvKeysUn[idx].octave and obs_stereo = mvuRight[idx] >= 0 of each observation), MapPoint::nObs (mp_nobs) and mp_flags (bit 0 isBad, bit 1 is_dynamic)."""

    def __init__(self, n_kf, obs_off, obs_kf, obs_octave, obs_stereo, mp_nobs, mp_flags):
        i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
        u8 = lambda a: np.ascontiguousarray(a, np.uint8).reshape(-1)
        self.n_kf = int(n_kf)
        self.obs_off, self.obs_kf, self.obs_octave, self.obs_stereo = i32(obs_off), i32(obs_kf), i32(obs_octave), u8(obs_stereo)
        self.mp_nobs, self.mp_flags = i32(mp_nobs), u8(mp_flags)
        self.n_points = len(self.mp_nobs)
        if len(self.obs_off) != self.n_points + 1 or len(self.mp_flags) != self.n_points:
            raise ValueError("obs_off, mp_nobs and mp_flags disagree on the number of points")
        if not len(self.obs_kf) == len(self.obs_octave) == len(self.obs_stereo) or (self.n_points and len(self.obs_kf) < self.obs_off.max()):
            raise ValueError("obs_kf, obs_octave and obs_stereo must hold obs_off[n_points] entries each")

    @property
    def n_obs(self):
        return len(self.obs_kf)

    def c_struct(self):
        """The struct, typed field by field: an array of another dtype is a TypeError here, before the call.  It points into this object's arrays."""
        return CsObsTable(self.n_kf, self.n_points, ptr(self.obs_off), ptr(self.obs_kf), ptr(self.obs_octave), ptr(self.obs_stereo), ptr(self.mp_nobs), ptr(self.mp_flags))

    def with_state(self, mp_nobs, mp_flags, alive=None):
        """The table a stage leaves: new nObs and flags, and (KeyFrameCulling's alive bytes) only the observation entries that are still alive."""
        if alive is None:
            return ObsTable(self.n_kf, self.obs_off, self.obs_kf, self.obs_octave, self.obs_stereo, mp_nobs, mp_flags)
        keep = np.asarray(alive, bool)
        off = np.concatenate([[0], np.cumsum(keep)])[self.obs_off].astype(np.int32)
        return ObsTable(self.n_kf, off, self.obs_kf[keep], self.obs_octave[keep], self.obs_stereo[keep], mp_nobs, mp_flags)


def _lists(kf_off, kf_mp):
    off, mp = np.ascontiguousarray(kf_off, np.int32).reshape(-1), np.ascontiguousarray(kf_mp, np.int32).reshape(-1)
    return off, mp


def _call(ctx, name, *args):
    """cs_<name> on the context's device, or cs_<name>_host when there is no context."""
    if ctx is None:
        return getattr(lib(), "cs_%s_host" % name)(*args)
    return getattr(lib(), "cs_%s" % name)(ctx.ptr, *args)


def covisibility_update(ctx, table, query_kf, kf_off, kf_mp, skip_dynamic=False, th=15, conn_cap=None):
    """cs_covisibility_update.  conn_cap = None sizes the buffers from the cnt_off a first call with no room returns.  Returns a dict: cnt_off, cnt_kf, cnt_w, kf_max, w_max,
    ord_off, ord_kf, ord_w."""
    q = np.ascontiguousarray(query_kf, np.int32).reshape(-1)
    off, mp = _lists(kf_off, kf_mp)
    n = len(q)
    cnt_off, ord_off, kf_max, w_max = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), np.full(max(n, 1), -1, np.int32), np.zeros(max(n, 1), np.int32)
    t = table.c_struct()

    def run(cap):
        bufs = [np.zeros(max(cap, 1), np.int32) for _ in range(4)]
        r = _call(ctx, "covisibility_update", C.byref(t), n, ptr(q), ptr(off), ptr(mp), int(bool(skip_dynamic)), int(th), int(cap), ptr(cnt_off), ptr(bufs[0]), ptr(bufs[1]),
                  ptr(kf_max), ptr(w_max), ptr(ord_off), ptr(bufs[2]), ptr(bufs[3]))
        return r, bufs

    r, bufs = run(0 if conn_cap is None else conn_cap)
    if r == CS_ERR_CAPACITY and conn_cap is None:
        r, bufs = run(int(cnt_off[n]))
    if r != 0:
        err = CubeSlamError("cs_covisibility_update failed: %s" % STATUS.get(r, r))
        err.status, err.cnt_off = r, cnt_off
        raise err
    nc, no = int(cnt_off[n]), int(ord_off[n])
    return dict(cnt_off=cnt_off, cnt_kf=bufs[0][:nc], cnt_w=bufs[1][:nc], kf_max=kf_max[:n], w_max=w_max[:n], ord_off=ord_off, ord_kf=bufs[2][:no], ord_w=bufs[3][:no])


class Connections:
    """The connection side of the key-frame table, as KeyFrame holds it: mConnectedKeyFrameWeights (weights[k], a dict), mvpOrderedConnectedKeyFrames / mvOrderedWeights
    (ordered_kf[k], ordered_w[k]), mpParent (parent[k], -1 none), mbFirstConnection (first_connection[k]) and mnId (ids[k]; only `== 0` is asked)."""

    def __init__(self, n_kf, ids=None):
        self.weights = [dict() for _ in range(n_kf)]
        self.ordered_kf = [[] for _ in range(n_kf)]
        self.ordered_w = [[] for _ in range(n_kf)]
        self.parent = [-1] * n_kf
        self.children = [[] for _ in range(n_kf)]
        self.first_connection = [True] * n_kf
        self.ids = list(range(n_kf)) if ids is None else list(ids)

    def AddConnection(self, k, other, weight):
        """KeyFrame::AddConnection (:140-156) on key frame k."""
        if self.weights[k].get(other) == weight:
            return
        self.weights[k][other] = weight
        self.UpdateBestCovisibles(k)

    def UpdateBestCovisibles(self, k):
        """:158-178: sort ascending on (weight, pointer), then push_front."""
        pairs = sorted(((w, kf) for kf, w in self.weights[k].items()), reverse=True)
        self.ordered_kf[k], self.ordered_w[k] = [kf for _, kf in pairs], [w for w, _ in pairs]

    def snapshot(self):
        return dict(weights=[sorted(w.items()) for w in self.weights], ordered_kf=[list(v) for v in self.ordered_kf], ordered_w=[list(v) for v in self.ordered_w],
                    parent=list(self.parent), children=[list(v) for v in self.children], first_connection=list(self.first_connection))


def UpdateConnections(ctx, table, queries, kf_off, kf_mp, connections, skip_dynamic=False, th=15):
    """KeyFrame::UpdateConnections for every key frame of `queries`, one library call for the batch; then, in query order, what the reference does with each result: the
    AddConnection(this, w) calls on the other key frames in ascending index (with their UpdateBestCovisibles), the query's own weights and ordered lists, and the parent of its
    first connection (:424-429).  A query with an empty counter leaves everything as it is (:382).  The votes depend on the observation table alone, so the batch equals the
    sequence.  Returns the library's result."""
    r = covisibility_update(ctx, table, queries, kf_off, kf_mp, skip_dynamic, th)
    for q, kf in enumerate(np.asarray(queries).reshape(-1).tolist()):
        c0, c1, o0, o1 = int(r["cnt_off"][q]), int(r["cnt_off"][q + 1]), int(r["ord_off"][q]), int(r["ord_off"][q + 1])
        if c1 == c0:
            continue
        okf, ow = r["ord_kf"][o0:o1].tolist(), r["ord_w"][o0:o1].tolist()
        for w, other in sorted(zip(ow, okf), key=lambda p: p[1]):  # the walk over KFcounter is ascending
            connections.AddConnection(other, kf, w)
        connections.weights[kf] = dict(zip(r["cnt_kf"][c0:c1].tolist(), r["cnt_w"][c0:c1].tolist()))
        connections.ordered_kf[kf], connections.ordered_w[kf] = okf, ow
        if connections.first_connection[kf] and connections.ids[kf] != 0:
            connections.parent[kf] = okf[0]
            connections.children[okf[0]].append(kf)
            connections.first_connection[kf] = False
    return r


def KeyFrameCulling(ctx, table, local_kf, kf_off, kf_mp, slot_octave, slot_depth, kf_th_depth, monocular, kf_flags, th_obs=3):
    """cs_keyframe_culling.  Returns a dict: verdict, n_mps, n_redundant, mp_nobs, mp_flags, alive, n_rounds; the caller's tables are not written.  The new mpRefKF of a point
    (its lowest alive index) and the connection and spanning-tree repair of KeyFrame::SetBadFlag stay with the caller."""
    lk = np.ascontiguousarray(local_kf, np.int32).reshape(-1)
    off, mp = _lists(kf_off, kf_mp)
    n = len(lk)
    octv, depth = np.ascontiguousarray(slot_octave, np.int32).reshape(-1), np.ascontiguousarray(slot_depth, np.float32).reshape(-1)
    thd, kfl = np.ascontiguousarray(kf_th_depth, np.float32).reshape(-1), np.ascontiguousarray(kf_flags, np.uint8).reshape(-1)
    if len(octv) != len(mp) or len(depth) != len(mp) or len(thd) != n or len(kfl) != n or len(off) != n + 1:
        raise ValueError("per-slot and per-key-frame arrays disagree with the lists")
    verdict, n_mps, n_red = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    nobs, flags, alive = np.zeros(max(table.n_points, 1), np.int32), np.zeros(max(table.n_points, 1), np.uint8), np.zeros(max(table.n_obs, 1), np.uint8)
    rounds = C.c_int()
    t = table.c_struct()
    r = _call(ctx, "keyframe_culling", C.byref(t), n, ptr(lk), ptr(off), ptr(mp), ptr(octv), ptr(depth), ptr(thd), int(bool(monocular)), ptr(kfl), int(th_obs), ptr(verdict),
              ptr(n_mps), ptr(n_red), ptr(nobs), ptr(flags), ptr(alive), C.byref(rounds))
    check(ctx.ptr if ctx is not None else None, r, "cs_keyframe_culling")
    return dict(verdict=verdict[:n], n_mps=n_mps[:n], n_redundant=n_red[:n], mp_nobs=nobs[:table.n_points], mp_flags=flags[:table.n_points], alive=alive[:table.n_obs],
                n_rounds=rounds.value)


def MapPointCulling(ctx, table, recent, mp_found, mp_visible, mp_first_kf_id, current_kf_id, th_obs):
    """cs_mappoint_culling: the case of every entry of mlpRecentAddedMapPoints (0 stays; 1 bad or dynamic; 2 found ratio; 3 few observations; 4 old enough).  Cases 2 and 3 are
    the reference's SetBadFlag calls (apply_mappoint_cases); every case but 0 leaves the list."""
    rc = np.ascontiguousarray(recent, np.int32).reshape(-1)
    found, vis, first = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (mp_found, mp_visible, mp_first_kf_id))
    if not len(found) == len(vis) == len(first) == table.n_points:
        raise ValueError("mp_found, mp_visible and mp_first_kf_id hold one entry per point")
    cases = np.zeros(max(len(rc), 1), np.uint8)
    t = table.c_struct()
    r = _call(ctx, "mappoint_culling", C.byref(t), len(rc), ptr(rc), ptr(found), ptr(vis), ptr(first), int(current_kf_id), int(th_obs), ptr(cases))
    check(ctx.ptr if ctx is not None else None, r, "cs_mappoint_culling")
    return cases[:len(rc)]


def apply_mappoint_cases(table, recent, cases):
    """What MapPointCulling's cases do to the map: MapPoint::SetBadFlag for cases 2 and 3 (the point is bad and its observations are gone).  Returns the new table and the recent
    list that remains."""
    rc, cs = np.asarray(recent, np.int32).reshape(-1), np.asarray(cases, np.uint8).reshape(-1)
    flags = table.mp_flags.copy()
    flags[rc[(cs == 2) | (cs == 3)]] |= MP_BAD
    alive = np.repeat((flags & MP_BAD) == 0, np.diff(table.obs_off))
    return table.with_state(table.mp_nobs, flags, alive), rc[cs == 0]
