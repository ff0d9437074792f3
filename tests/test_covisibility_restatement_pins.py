"""The judge of the covisibility tests (tests/covisibility_restatement.py) against the reference's own text, cut out of the reference at test time into tmp_path and compiled
there around our stand-ins (tests/cpp/ref_covisibility_standins.cpp).  Nothing cut or compiled is written inside the repository.

KeyFrame::UpdateConnections, AddConnection, UpdateBestCovisibles and SetBadFlag, MapPoint::EraseObservation and SetBadFlag, LocalMapping::KeyFrameCulling and MapPointCulling
run on the tables of every pattern.  What the reference lets one observe must equal the restatement's: for the vote the counters (mConnectedKeyFrameWeights), the ordered lists,
the connections the other key frames received and the parents; for the key-frame culling which key frames are bad or to be erased, the final nObs, the bad flags and the
observations that are left; for the map-point culling which entries stay and which points turned bad.  nMPs, nRedundantObservations and the delete_case counters are locals of
the reference and are not observable.  The reference hard-codes th = 15 and thObs = 3: patterns built for another value are judged on the same tables at the reference's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import covisibility_patterns as P
from tests import covisibility_restatement as R
from tests.test_sim3_restatement_pins import _cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the restatement is pinned to the reference's text under /root/reference")

WANT = [("orb_object_slam/src/KeyFrame.cc", ["void KeyFrame::AddConnection(KeyFrame *pKF, const int &weight)", "void KeyFrame::UpdateBestCovisibles()", "void KeyFrame::UpdateConnections()",
                                             "void KeyFrame::SetBadFlag()"]),
        ("orb_object_slam/src/MapPoint.cc", ["void MapPoint::EraseObservation(KeyFrame *pKF)", "void MapPoint::SetBadFlag()"]),
        ("orb_object_slam/src/LocalMapping.cc", ["void LocalMapping::MapPointCulling()", "void LocalMapping::KeyFrameCulling()"])]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("ref_covisibility")
    parts = []
    for rel, sigs in WANT:
        text = open(os.path.join(REF, rel)).read()
        parts += [_cut(text, s) for s in sigs]
    (d / "ref_covisibility_extracted.inc").write_text("\n\n".join(parts) + "\n")
    so = str(d / "libref_covisibility.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fPIC", "-shared", "-I" + str(d), "-o", so, os.path.join(ROOT, "tests", "cpp", "ref_covisibility_standins.cpp")])
    lib = C.CDLL(so)
    lib.pin_update_connections.restype = C.c_int
    lib.pin_keyframe_culling.restype = None
    lib.pin_mappoint_culling.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _table_args(t):
    return [C.c_int(t["n_kf"]), C.c_int(t["n_points"]), _p(t["obs_off"]), _p(t["obs_kf"]), _p(t["obs_octave"]), _p(t["obs_stereo"]), _p(t["mp_nobs"]), _p(t["mp_flags"])]


def _connection_words(state):
    out = []
    for k in range(len(state["weights"])):
        if not state["weights"][k] and state["parent"][k] < 0:
            continue
        out += [k, len(state["ordered_kf"][k])] + list(state["ordered_kf"][k]) + list(state["ordered_w"][k]) + [len(state["weights"][k])]
        for kf, w in state["weights"][k]:
            out += [kf, w]
        out += [state["parent"][k], int(state["first_connection"][k]), len(state["children"][k])] + sorted(state["children"][k])
    return out


@pytest.mark.parametrize("name", P.VOTE_NAMES)
def test_update_connections(ref, name):
    c = P.case(name)
    t, queries = c["t"], c["query_kf"]
    ids = np.arange(1, t["n_kf"] + 1, dtype=np.int32)
    ids[queries[-1]] = 0  # one queried key frame is the map's first: it takes no parent
    for sd in c["skip_dynamic"]:
        out = np.zeros(16 + 8 * t["n_kf"] + 6 * len(t["obs_kf"]) * max(1, len(queries)), np.int32)
        n = ref.pin_update_connections(*_table_args(t), C.c_int(len(queries)), _p(queries), _p(c["kf_off"]), _p(c["kf_mp"]), _p(ids), C.c_int(sd), _p(out), C.c_int(len(out)))
        assert n >= 0
        results = R.update_connections(t, queries, c["kf_off"], c["kf_mp"], sd, 15)
        want = _connection_words(R.apply_connections(t["n_kf"], queries.tolist(), results, ids.tolist()))
        assert out[:n].tolist() == want


@pytest.mark.parametrize("name", P.CULL_NAMES)
def test_keyframe_culling(ref, name):
    c = P.case(name)
    t = c["t"]
    nl = len(c["local_kf"])
    state, nobs, flags, alive = np.zeros(max(nl, 1), np.uint8), np.zeros(max(t["n_points"], 1), np.int32), np.zeros(max(t["n_points"], 1), np.uint8), np.zeros(max(len(t["obs_kf"]), 1), np.uint8)
    ref.pin_keyframe_culling(*_table_args(t), C.c_int(nl), _p(c["local_kf"]), _p(c["kf_off"]), _p(c["kf_mp"]), _p(c["slot_octave"]), _p(c["slot_depth"]), _p(c["kf_th_depth"]),
                             C.c_int(c["monocular"]), _p(c["kf_flags"]), _p(state), _p(nobs), _p(flags), _p(alive))
    want = P.expected(name) if c["th_obs"] == 3 else R.keyframe_culling(t, c["local_kf"], c["kf_off"], c["kf_mp"], c["slot_octave"], c["slot_depth"], c["kf_th_depth"], c["monocular"],
                                                                        c["kf_flags"], 3)
    assert np.array_equal(state[:nl] & 1, (want["verdict"] == 1).astype(np.uint8)), "mbBad"
    assert np.array_equal((state[:nl] >> 1) & 1, (want["verdict"] == 2).astype(np.uint8)), "mbToBeErased"
    assert np.array_equal(nobs[:t["n_points"]], want["mp_nobs"]) and np.array_equal(flags[:t["n_points"]], want["mp_flags"]) and np.array_equal(alive[:len(t["obs_kf"])], want["alive"])


@pytest.mark.parametrize("name", P.MPCULL_NAMES)
def test_mappoint_culling(ref, name):
    c = P.case(name)
    t, recent = c["t"], c["recent"]
    assert c["th_obs"] in (1, 2, 3)
    remains, flags = np.zeros(len(recent), np.uint8), np.zeros(t["n_points"], np.uint8)
    ref.pin_mappoint_culling(C.c_int(t["n_points"]), _p(t["mp_nobs"]), _p(t["mp_flags"]), C.c_int(len(recent)), _p(recent), _p(c["mp_found"]), _p(c["mp_visible"]),
                             _p(c["mp_first_kf_id"]), C.c_int(c["current_kf_id"]), C.c_int(c["th_obs"]), _p(remains), _p(flags))
    cases = P.expected(name)
    assert np.array_equal(remains, (cases == 0).astype(np.uint8))
    want_flags = t["mp_flags"].copy()
    want_flags[recent[(cases == 2) | (cases == 3)]] |= 1
    assert np.array_equal(flags, want_flags)
