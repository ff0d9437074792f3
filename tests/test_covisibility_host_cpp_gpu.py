"""GPU: the C++ mirror (cubeslam::Covisibility, cube_slam_amd/host/covisibility.hpp) compiled with g++ against the C-ABI library through tests/cpp/covisibility_mirror.cpp: on
every pattern its results are the restatement's, and the connection state its UpdateConnections leaves is the Python mirror's."""
import os
import subprocess

import numpy as np
import pytest

from tests import covisibility_patterns as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_mirror(directory):
    e = str(directory / "covisibility_mirror")
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "covisibility_mirror.cpp"), "-o", e, "-L", lib_dir, "-lcubeslam_hip",
                           "-Wl,-rpath," + lib_dir])
    return e


def connection_words(conn):
    """The connection state as tests/cpp/covisibility_mirror.cpp writes it."""
    out = []
    for k in range(len(conn.weights)):
        if not conn.weights[k] and conn.parent[k] < 0:
            continue
        out += [k, len(conn.ordered_kf[k])] + conn.ordered_kf[k] + conn.ordered_w[k] + [len(conn.weights[k])]
        for kf, w in sorted(conn.weights[k].items()):
            out += [kf, w]
        out += [conn.parent[k], int(conn.first_connection[k])] + conn.children[k]
    return np.array(out, np.int32).tobytes()


def mirror_bytes(exe, mode, tmp_path, c, sd):
    (tmp_path / "in.bin").write_bytes(P.dump(c, sd))
    r = subprocess.run([exe, mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return (tmp_path / "out.bin").read_bytes()


def want_bytes(ctx, name, c, sd, rounds):
    """The restatement's results; for a vote, followed by the state the Python mirror's UpdateConnections leaves (itself held to the restatement in the mirror tests)."""
    from cube_slam_amd.covisibility import Connections, UpdateConnections
    if c["kind"] != "vote":
        return P.expected_bytes(c, P.expected(name)) + (np.int32(rounds).tobytes() if c["kind"] == "cull" else b"")
    conn = Connections(c["t"]["n_kf"])
    UpdateConnections(ctx, P.obs_table(c["t"]), c["query_kf"], c["kf_off"], c["kf_mp"], conn, skip_dynamic=bool(sd), th=c["th"])
    return P.expected_bytes(c, P.expected(name, sd)) + connection_words(conn)


def cull_rounds(name):
    v = P.expected(name)["verdict"]
    erased = np.flatnonzero(v == 1)
    return len(erased) + (0 if len(erased) and erased[-1] == len(v) - 1 else 1)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_mirror(tmp_path_factory.mktemp("covisibility_mirror"))


@pytest.mark.parametrize("name", P.NAMES)
def test_cpp_mirror_on_the_device(ctx, exe, tmp_path, name):
    c = P.case(name)
    for sd in c.get("skip_dynamic", (None,)):
        assert mirror_bytes(exe, "device", tmp_path, c, sd) == want_bytes(ctx, name, c, sd, cull_rounds(name) if c["kind"] == "cull" else 0)
