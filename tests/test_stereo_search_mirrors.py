"""CPU: cube_slam_amd/csrc/stereo_search_math.h -- the one text of the direction, the level window and the mvuRight predicate that match.hip, the host mirrors and plain C++
share -- as a stand-alone program (tests/cpp/stereo_search_driver.cpp) built with g++ plainly and under -fsanitize=address,undefined: both runs clean, both equal to the
restatement (tests/stereo_search_restatement.py) on the direction cases of tests/stereo_search_patterns.py, on seeded poses and on the borders of the predicate.  No sanitizer
goes near code loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import match_patterns as mp
from tests import stereo_search_patterns as SP
from tests import stereo_search_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _records():
    """(Tcw, Tlw, mb, mono, probes): the direction cases, 100 seeded pose pairs with the baseline on and around tlc.z, and four probes of the small predicates per record."""
    u = SP.u_right_case(); v = SP.u_right_ulp_case()
    border = [(u.ur[q], u.u_right[q], u.radius) for q in range(7)] + [(v.ur[t], v.u_right[t], v.radius) for t in range(3)] + [(f32(5.0), f32(np.nan), f32(1.0)), (f32(5.0), f32(np.inf), f32(1.0))]
    recs = [(c.Tcw, c.Tlw, f32(c.mb), c.mono) for c in SP.direction_cases()]
    for seed in range(100):
        rng = np.random.default_rng(7000 + seed)
        Tcw, Tlw = SP.pose(Rm=SP._rotation(seed), t=rng.uniform(-3, 3, 3)), SP.pose(Rm=SP._rotation(500 + seed), t=rng.uniform(-3, 3, 3))
        z = abs(R.tlc_z(Tcw, Tlw))
        recs += [(Tcw, Tlw, z, 0), (Tcw, Tlw, mp.below(z), 0), (Tcw, Tlw, mp.above(z), 0), (Tcw, Tlw, mp.below(z), 1)]
    out = []
    for i, (Tcw, Tlw, mb, mono) in enumerate(recs):
        probes = [((i + p) % 3, (0, 7, 3, 1)[p], *border[(4 * i + p) % len(border)]) for p in range(4)]
        out.append((np.asarray(Tcw, f32).reshape(-1)[:12], np.asarray(Tlw, f32).reshape(-1)[:12], f32(mb), int(mono), probes))
    return out


def _pack(recs):
    b = struct.pack("<i", len(recs))
    for Tcw, Tlw, mb, mono, probes in recs:
        b += Tcw.astype("<f4").tobytes() + Tlw.astype("<f4").tobytes() + struct.pack("<fi", float(mb), mono)
        for d, o, urq, ur, rad in probes:
            b += struct.pack("<ii", d, o) + np.array([urq, ur, rad], "<f4").tobytes()
    return b


def _want(recs):
    b = b""
    for Tcw, Tlw, mb, mono, probes in recs:
        b += R.tlc_z(Tcw, Tlw).astype("<f4").tobytes() + struct.pack("<i", R.direction(Tcw, Tlw, mb, mono))
        for d, o, urq, ur, rad in probes:
            lo, hi = R.levels(d, o)
            b += struct.pack("<iii", lo, hi, int(R.drops(urq, ur, rad)))
    return b


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]], ids=["plain", "asan_ubsan"])
def test_math_header_as_a_stand_alone_program(tmp_path, flags):
    exe = str(tmp_path / "stereo_search_driver")
    subprocess.check_call(["g++", "-O1" if flags else "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "cube_slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "stereo_search_driver.cpp")])
    recs = _records()
    assert {R.direction(r[0], r[1], r[2], r[3]) for r in recs} == {R.NEITHER, R.FORWARD, R.BACKWARD} and len(recs) > 400
    (tmp_path / "in.bin").write_bytes(_pack(recs))
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0 and p.stderr == "", p.stderr
    assert (tmp_path / "out.bin").read_bytes() == _want(recs)
    # a truncated input is refused, not read past its end
    (tmp_path / "short.bin").write_bytes(_pack(recs)[:-3])
    p = subprocess.run([exe, str(tmp_path / "short.bin"), str(tmp_path / "out2.bin")], capture_output=True, text=True)
    assert p.returncode == 2 and "short input" in p.stderr
