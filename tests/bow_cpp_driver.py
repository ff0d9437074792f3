"""The script protocol of tests/cpp/bow_mirror.cpp (the driver of cube_slam_amd/host/bow.hpp), shared by tests/test_bow_mirrors.py and tests/test_bow_host_cpp_gpu.py."""
import os
import subprocess

import numpy as np

from tests import bow_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(directory):
    exe = os.path.join(str(directory), "bow_mirror")
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "bow_mirror.cpp"), "-o", exe, "-L", lib_dir, "-lcubeslam_hip",
                           "-Wl,-rpath," + lib_dir])
    return exe


def run(exe, mode, lines, directory):
    script = os.path.join(str(directory), "script_%s.txt" % mode)
    with open(script, "w") as f:
        f.write("\n".join(lines) + "\n")
    return subprocess.check_output([exe, mode, script], timeout=120).decode().splitlines()


def hex64(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def hex32(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def bow(b):
    return ",".join("%d:%s" % (w, hex64(x)) for w, x in b.items()) or "-"


def cov(c):
    return ";".join("%d=%s" % (k, ".".join(str(i) for i in v)) for k, v in c.items() if v) or "-"


def ids(c):
    return ",".join(str(i) for i in c) or "-"


def cand(line):
    t = line.split()
    assert t[0] == "cand"
    return [] if t[1] == "-" else [int(x) for x in t[1].split(",")]


def min_score(ops, op):
    ms = op[5]
    if isinstance(ms, tuple):
        ms = np.float32(R.score(op[2], [o for o in ops if o[0] == "add" and o[1] == ms[1]][0][2]))
    return np.float32(ms)


def shared_words(ops):
    """Per query op of a scenario, what cs_bow_db_query returns for it, computed with the restatement: [(id, common, minword, add order, score)] in add order."""
    live, seq, out = {}, 0, []
    for op in ops:
        if op[0] == "add":
            live.pop(op[1], None)
            live[op[1]] = (seq, op[2])
            seq += 1
        elif op[0] == "erase":
            live.pop(op[1], None)
        elif op[0] == "clear":
            live.clear()
        else:
            q = op[2]
            out.append([(i, len(set(q) & set(b)), min(set(q) & set(b)), s, R.score(q, b)) for i, (s, b) in live.items() if set(q) & set(b)])
    return out


def fnv(*arrays):
    h = 14695981039346656037
    for a in arrays:
        for byte in np.ascontiguousarray(a).tobytes():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h
