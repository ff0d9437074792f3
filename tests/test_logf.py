"""The logf restatement the matcher's preamble uses on the device (cube_slam_amd/csrc/glibc_logf.h) equals the host's libm: MapPoint::PredictScale is
ceil(log(ratio) / logScaleFactor) on floats, and a level off by one changes the search radius and the level filter.  LOGF_STRIDE=1 walks every positive
normal float (minutes); the default is every 97th plus the level boundaries 1.2^k and quotients that land on them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_logf_restatement_equals_libm(tmp_path):
    exe = str(tmp_path / "logf_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-ffp-contract=off", "-fno-builtin", "-o", exe, "tests/cpp/logf_check.cpp"], cwd=ROOT)
    out = subprocess.run([exe, os.environ.get("LOGF_STRIDE", "97")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert int(out.stdout.split()[-4]) > 20_000_000, out.stdout  # "<n> values, <bad> mismatches"
