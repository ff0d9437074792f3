"""The device quadtree (orb_quadtree in orb.hip) rests on a list-free re-expression of ExtractorNode list surgery.  This test
builds the C++ emulation of that formulation and checks it against the sequential host restatement on 3000 random point sets and on
the input families natural textures do not produce (tests/cpp/quadtree_emul.cpp: lattices whose responses all tie, with a cluster, with
close pairs, one quadrant of one root, 0 / 1 / 2 points or quota, one to six root nodes).  The emulation also counts what the kernel
counts against its pools."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAMILIES = ["random", "lattice, all responses equal", "lattice with one cluster", "lattice of close pairs", "one quadrant of one root",
            "0, 1 or 2 points; quota 0, 1 or 2"]


@pytest.fixture(scope="module")
def emul_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("qt") / "qt_emul"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "quadtree_emul.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode()
    print(out)
    return out


def test_list_free_formulation_equals_sequential(emul_output):
    assert "all equal" in emul_output, emul_output
    rows = {m.group(1).strip(): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^(.+?)\s+(\d+) trials\s+(\d+) mismatches", emul_output, re.M)}
    assert sorted(rows) == sorted(FAMILIES), emul_output
    assert rows["random"] == (3000, 0)
    for name in FAMILIES:
        assert rows[name][0] >= 1500 and rows[name][1] == 0, (name, rows[name])


def test_no_family_exceeds_a_pool_of_the_kernel(emul_output):
    """High-water marks of the node pool, the lists and the (size, id) list as fractions of CAPN = 12N+64, CAPL = 4N+16, CAPV = N+8, counted where
    orb_quadtree tests them: no family gets past a cap, so the kernel's status = 1 is a defensive path (DESIGN.md section 7.1 quotes the figures).
    The lists and the (size, id) list touch their caps by construction (a quota of 0 with four roots gives 16 children for CAPL = 16; the second
    phase's next round holds up to N + 4 entries); the node pool is the one without a closed bound and stays below a third."""
    rows = re.findall(r"^(.+?)\s+\d+ trials\s+\d+ mismatches\s+(\d+) over a cap\s+high water: nodes ([\d.]+) of CAPN, lists ([\d.]+) of CAPL, \(size, id\) ([\d.]+) of CAPV", emul_output, re.M)
    assert sorted(r[0].strip() for r in rows) == sorted(FAMILIES), emul_output
    top = 0.0
    for name, over, fn, fl, fv in rows:
        assert int(over) == 0, (name, over)
        assert float(fn) <= 1.0 and float(fl) <= 1.0 and float(fv) <= 1.0, (name, fn, fl, fv)
        top = max(top, float(fn), float(fl), float(fv))
    m = re.search(r"highest fraction of a cap: ([\d.]+) \((\d+) cases over a cap\)", emul_output)
    assert m and int(m.group(2)) == 0 and abs(float(m.group(1)) - top) < 1e-9
    print("highest fraction of a cap: %.3f; node pool: %.3f" % (top, max(float(r[2]) for r in rows)))
