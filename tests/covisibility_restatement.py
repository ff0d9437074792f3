"""KeyFrame::UpdateConnections (reference orb_object_slam/src/KeyFrame.cc:345-437) with AddConnection / UpdateBestCovisibles (:140-180), LocalMapping::KeyFrameCulling
(LocalMapping.cc:833-902) with KeyFrame::SetBadFlag (KeyFrame.cc:511-529) and MapPoint::EraseObservation / SetBadFlag (MapPoint.cc:178-205, :287-307), and
LocalMapping::MapPointCulling (LocalMapping.cc:249-302), restated as the reference's sequential loops over the tables of include/cubeslam_hip/covisibility.h.  Objects are
dictionaries, std::map<KeyFrame *, ...> is walked in ascending key-frame index (the library's definition of pointer order).  tests/test_covisibility_restatement_pins.py
holds it against the reference's own functions."""
import numpy as np

BAD, DYNAMIC = 1, 2


class Map:
    """Map points with mObservations (dict kf -> entry), nObs, mbBad, is_dynamic, built from the table."""

    def __init__(self, t):
        self.t = t
        self.obs = [dict((int(t["obs_kf"][e]), e) for e in range(t["obs_off"][p], t["obs_off"][p + 1])) if not t["mp_flags"][p] & BAD else {} for p in range(t["n_points"])]
        self.nobs = [int(v) for v in t["mp_nobs"]]
        self.bad = [bool(f & BAD) for f in t["mp_flags"]]
        self.dynamic = [bool(f & DYNAMIC) for f in t["mp_flags"]]

    def SetBadFlag(self, p):
        self.bad[p] = True
        self.obs[p].clear()

    def EraseObservation(self, p, kf):
        bad = False
        if kf in self.obs[p]:
            e = self.obs[p][kf]
            self.nobs[p] -= 2 if self.t["obs_stereo"][e] else 1
            del self.obs[p][kf]
            if self.nobs[p] <= 2:
                bad = True
        if bad:
            self.SetBadFlag(p)

    def state(self):
        alive = np.zeros(len(self.t["obs_kf"]), np.uint8)
        for o in self.obs:
            for e in o.values():
                alive[e] = 1
        flags = np.array([(BAD if b else 0) | (DYNAMIC if d else 0) for b, d in zip(self.bad, self.dynamic)], np.uint8)
        return np.array(self.nobs, np.int32), flags, alive


def update_connections(t, query_kf, kf_off, kf_mp, skip_dynamic, th=15):
    """Per query: KFcounter (ascending pairs), (kf_max, w_max), and the ordered pairs [(kf, w)] = mvpOrderedConnectedKeyFrames / mvOrderedWeights."""
    m = Map(t)
    out = []
    for q, me in enumerate(query_kf):
        counter = {}
        for s in range(kf_off[q], kf_off[q + 1]):
            p = int(kf_mp[s])
            if p < 0:
                continue
            if m.bad[p]:
                continue
            if skip_dynamic and m.dynamic[p]:
                continue
            for kf in sorted(m.obs[p]):
                if kf == me:
                    continue
                counter[kf] = counter.get(kf, 0) + 1
        if not counter:
            out.append(dict(counter=[], kf_max=-1, w_max=0, ordered=[]))
            continue
        nmax, kfmax, pairs = 0, None, []
        for kf in sorted(counter):
            if counter[kf] > nmax:
                nmax, kfmax = counter[kf], kf
            if counter[kf] >= th:
                pairs.append((counter[kf], kf))
        if not pairs:
            pairs.append((nmax, kfmax))
        pairs.sort()
        ordered = []
        for w, kf in pairs:
            ordered.insert(0, (kf, w))
        out.append(dict(counter=sorted(counter.items()), kf_max=kfmax, w_max=nmax, ordered=ordered))
    return out


def apply_connections(n_kf, queries, results, ids=None):
    """The connection state of n_kf fresh key frames after UpdateConnections of `queries` in order: weights, ordered lists, parents (mbFirstConnection, mnId != 0)."""
    ids = list(range(n_kf)) if ids is None else ids
    weights = [dict() for _ in range(n_kf)]
    okf, ow = [[] for _ in range(n_kf)], [[] for _ in range(n_kf)]
    parent, children, first = [-1] * n_kf, [[] for _ in range(n_kf)], [True] * n_kf

    def best_covisibles(k):
        pairs = sorted((w, kf) for kf, w in weights[k].items())
        lk, lw = [], []
        for w, kf in pairs:
            lk.insert(0, kf)
            lw.insert(0, w)
        okf[k], ow[k] = lk, lw

    def add_connection(k, other, w):
        if other not in weights[k]:
            weights[k][other] = w
        elif weights[k][other] != w:
            weights[k][other] = w
        else:
            return
        best_covisibles(k)

    for me, r in zip(queries, results):
        if not r["counter"]:
            continue
        for kf, w in sorted(r["ordered"]):
            add_connection(kf, me, w)
        weights[me] = dict(r["counter"])
        okf[me], ow[me] = [kf for kf, _ in r["ordered"]], [w for _, w in r["ordered"]]
        if first[me] and ids[me] != 0:
            parent[me] = okf[me][0]
            children[parent[me]].append(me)
            first[me] = False
    return dict(weights=[sorted(w.items()) for w in weights], ordered_kf=okf, ordered_w=ow, parent=parent, children=children, first_connection=first)


def keyframe_culling(t, local_kf, kf_off, kf_mp, slot_octave, slot_depth, kf_th_depth, monocular, kf_flags, th_obs=3, frozen=False):
    """The loop as a sequence.  frozen = True evaluates every key frame on the initial state (what a single parallel pass would say): for the patterns that show the difference."""
    m = Map(t)
    verdict, n_mps, n_red = [], [], []
    for i, kf in enumerate(local_kf):
        if kf_flags[i] & 1:  # mnId == 0
            verdict.append(3); n_mps.append(0); n_red.append(0)
            continue
        mps = red = 0
        for s in range(kf_off[i], kf_off[i + 1]):
            p = int(kf_mp[s])
            if p < 0 or m.bad[p]:
                continue
            if not monocular:
                if np.float32(slot_depth[s]) > np.float32(kf_th_depth[i]) or np.float32(slot_depth[s]) < 0:
                    continue
            if m.dynamic[p]:
                continue
            mps += 1
            if m.nobs[p] > th_obs:
                level, n = int(slot_octave[s]), 0
                for kfi in sorted(m.obs[p]):
                    if kfi == kf:
                        continue
                    if int(t["obs_octave"][m.obs[p][kfi]]) <= level + 1:
                        n += 1
                        if n >= th_obs:
                            break
                if n >= th_obs:
                    red += 1
        n_mps.append(mps); n_red.append(red)
        if float(red) > 0.9 * float(mps):
            if kf_flags[i] & 2:  # mbNotErase: mbToBeErased only
                verdict.append(2)
                continue
            verdict.append(1)
            if not frozen:
                for s in range(kf_off[i], kf_off[i + 1]):
                    if kf_mp[s] >= 0:
                        m.EraseObservation(int(kf_mp[s]), int(kf))
        else:
            verdict.append(0)
    nobs, flags, alive = m.state()
    return dict(verdict=np.array(verdict, np.uint8), n_mps=np.array(n_mps, np.int32), n_redundant=np.array(n_red, np.int32), mp_nobs=nobs, mp_flags=flags, alive=alive)


def mappoint_culling(t, recent, mp_found, mp_visible, mp_first_kf_id, current_kf_id, th_obs):
    cases = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in recent:
            f = int(t["mp_flags"][p])
            if f & (BAD | DYNAMIC):
                cases.append(1)
            elif np.float32(mp_found[p]) / np.float32(mp_visible[p]) < np.float32(0.25):
                cases.append(2)
            elif int(current_kf_id) - int(mp_first_kf_id[p]) >= 2 and int(t["mp_nobs"][p]) <= th_obs:
                cases.append(3)
            elif int(current_kf_id) - int(mp_first_kf_id[p]) >= 3:
                cases.append(4)
            else:
                cases.append(0)
    return np.array(cases, np.uint8)
