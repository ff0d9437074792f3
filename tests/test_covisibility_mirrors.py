"""CPU: the host forms (cs_covisibility_update_host, cs_keyframe_culling_host, cs_mappoint_culling_host) against the restatement on every pattern, the Python mirror's
connection bookkeeping against the restatement's, and the host walk as a stand-alone program (tests/cpp/covisibility_driver.cpp over csrc/covis_walk.h and covis_math.h) built
with g++ plainly and under -fsanitize=address,undefined: both runs clean, both equal to the restatement.  No sanitizer goes near code loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import covisibility_patterns as P
from tests import covisibility_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", P.VOTE_NAMES)
def test_vote_host_form(name):
    c = P.case(name)
    for sd in c["skip_dynamic"]:
        P.assert_equal(P.run_vote(None, c, sd), P.expected(name, sd), P.VOTE_KEYS, "%s skip_dynamic=%d" % (name, sd))


@pytest.mark.parametrize("name", P.CULL_NAMES)
def test_cull_host_form(name):
    got = P.run_cull(None, P.case(name))
    P.assert_equal(got, P.expected(name), P.CULL_KEYS, name)
    assert got["n_rounds"] == 1


@pytest.mark.parametrize("name", P.MPCULL_NAMES)
def test_mpcull_host_form(name):
    got = P.run_mpcull(None, P.case(name))
    assert got.dtype == np.uint8 and np.array_equal(got, P.expected(name))


def test_host_capacity_reports_the_sizes():
    from cube_slam_amd._lib import CubeSlamError
    c, want = P.case("random_vote_1"), P.expected("random_vote_1", 1)
    with pytest.raises(CubeSlamError) as e:
        P.run_vote(None, c, 1, conn_cap=int(want["cnt_off"][-1]) - 1)
    assert e.value.status == -4 and np.array_equal(e.value.cnt_off, want["cnt_off"])
    P.assert_equal(P.run_vote(None, c, 1, conn_cap=int(want["cnt_off"][-1])), want, P.VOTE_KEYS, "exact capacity")


@pytest.mark.parametrize("name", ["vote_threshold", "vote_fallback_tie", "vote_empty", "random_vote_1", "random_vote_2"])
def test_update_connections_applies_the_add_connection_calls(name):
    """UpdateConnections of the Python mirror (host form underneath): the other key frames' weights and re-sorted lists, the query's own, the first-connection parent."""
    from cube_slam_amd.covisibility import Connections, UpdateConnections
    c = P.case(name)
    n_kf, queries = c["t"]["n_kf"], c["query_kf"].tolist()
    ids = [5 + k for k in range(n_kf)]
    ids[queries[-1]] = 0  # one queried key frame is the map's first: it takes no parent
    for pick in (list(range(len(queries))), list(range(len(queries)))[::-1]):  # the AddConnection calls land in query order: both ways round
        order = [queries[i] for i in pick]
        off = np.concatenate([[0], np.cumsum([c["kf_off"][i + 1] - c["kf_off"][i] for i in pick])]).astype(np.int32)
        mp = np.concatenate([c["kf_mp"][c["kf_off"][i]:c["kf_off"][i + 1]] for i in pick] + [np.zeros(0, np.int32)]).astype(np.int32)
        conn = Connections(n_kf, ids)
        UpdateConnections(None, P.obs_table(c["t"]), order, off, mp, conn, skip_dynamic=True, th=c["th"])
        want = R.apply_connections(n_kf, order, R.update_connections(c["t"], order, off, mp, 1, c["th"]), ids)
        assert conn.snapshot() == want


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("covisibility_driver")
    src, inc = os.path.join(ROOT, "tests", "cpp", "covisibility_driver.cpp"), os.path.join(ROOT, "cube_slam_amd", "csrc")
    plain, san = str(d / "driver"), str(d / "driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", inc, src, "-o", plain])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc, src, "-o", san])
    return plain, san


@pytest.mark.parametrize("name", P.NAMES)
def test_driver_plain_and_sanitized(drivers, tmp_path, name):
    c = P.case(name)
    for sd in c.get("skip_dynamic", (None,)):
        (tmp_path / "in.bin").write_bytes(P.dump(c, sd))
        outs = []
        for exe in drivers:
            out = tmp_path / ("out_%s.bin" % os.path.basename(exe))
            r = subprocess.run([exe, str(tmp_path / "in.bin"), str(out)], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and r.stderr == "", r.stderr
            outs.append(out.read_bytes())
        want = P.expected(name, sd) if c["kind"] == "vote" else P.expected(name)
        assert outs[0] == outs[1] == P.expected_bytes(c, want)


def test_driver_refuses_a_broken_table(drivers, tmp_path):
    """A run that is not ascending is a bad argument in the walk itself (the sanitized build reads nothing outside its arrays on the way)."""
    c = dict(P.case("vote_threshold"))
    t = dict(c["t"])
    t["obs_kf"] = t["obs_kf"].copy()
    t["obs_kf"][1] = t["obs_kf"][0]
    c["t"] = t
    (tmp_path / "in.bin").write_bytes(P.dump(c, 1))
    for exe in drivers:
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 3 and "returned -2" in r.stderr


@pytest.fixture(scope="module")
def mirror_exe(tmp_path_factory):
    from tests.test_covisibility_host_cpp_gpu import build_mirror
    return build_mirror(tmp_path_factory.mktemp("covisibility_mirror_host"))


@pytest.mark.parametrize("name", P.NAMES)
def test_cpp_mirror_over_the_host_forms(mirror_exe, tmp_path, name):
    """cubeslam::Covisibility (cube_slam_amd/host/covisibility.hpp) without a context: the restatement's results and the Python mirror's connection state."""
    from tests.test_covisibility_host_cpp_gpu import mirror_bytes, want_bytes
    c = P.case(name)
    for sd in c.get("skip_dynamic", (None,)):
        assert mirror_bytes(mirror_exe, "host", tmp_path, c, sd) == want_bytes(None, name, c, sd, 1)
