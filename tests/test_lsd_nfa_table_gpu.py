"""GPU parity of the device region stage's rectangle kernels: nfa() read from a table of its own results (lsd_rg_improve), the rectangles the table cannot
serve deferred to the evaluating kernel (lsd_rg_improve_deferred), and the device stage against the host stage with LBD descriptors, twice on one detector.

Frames: 8 of 160 x 120, straight dark segments on a light ground, 1-4 px wide and 6 px to the frame's diagonal long, over seeded noise of a few gray levels:
rectangles from under ten to several hundred pixels, on both sides of every bound the tests set.  Every detected line went through rect_improve, so the
oracle's line count per frame is a lower bound of the rectangles there (asserted: at least 20 per frame).

A detector's size is fixed when it is created, so "the table is rebuilt" is reached the way the code reaches it: a larger batch on the same detector
(the stage's buffers, tables included, are built again) and a second detector of another size, whose LOG_NT, and so every entry, differs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, F = 160, 120, 8
NFA_NMAX = 511  # the table's compiled bound (lsd_regions.hip)


def designed_frames(w=W, h=H, n=F, seed=2024):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    diag = float(np.hypot(w, h))
    frames = []
    for f in range(n):
        img = 200.0 + rng.uniform(-3, 3, (h, w))
        # one long segment per frame, up to the diagonal (frame 0), then a ladder of lengths from 6 px up, widths 1-4 in turn, on a jittered grid
        segs = [(w / 2, h / 2, diag * (1.0 - 0.1 * f), np.arctan2(h, w) * (1 if f % 2 == 0 else -1), 1 + f % 4)]
        k = 0
        for gy in range(5):
            for gx in range(7):
                cx, cy = (gx + 0.5) * w / 7 + rng.uniform(-3, 3), (gy + 0.5) * h / 5 + rng.uniform(-3, 3)
                length = 6 + (k * 5 + f * 3) % 34
                segs.append((cx, cy, length, rng.uniform(0, np.pi), 1 + (k + f) % 4))
                k += 1
        for cx, cy, length, th, wd in segs:
            dx, dy = np.cos(th), np.sin(th)
            t = np.clip((xx - cx) * dx + (yy - cy) * dy, -length / 2, length / 2)
            dist = np.hypot(xx - (cx + t * dx), yy - (cy + t * dy))
            img -= 150.0 * np.clip(wd / 2 + 0.5 - dist, 0, 1) * (img > 100)
        frames.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return np.stack(frames)


def run_detector(det, frames, stage):
    """KeyLines and descriptors of every frame through one region stage, with the table kernel's counters of that run."""
    det.set_region_stage(stage)
    det.upload(frames)
    det.run(with_lbd=True)
    st = det.region_stats()
    assert st["device"] == (stage == "wave_per_frame") and not st["host_fallback"]
    out = [det.read(f) for f in range(len(frames))]
    counters = det.nfa_probe(np.zeros((0, 3), np.int32))[2:] if stage == "wave_per_frame" else (0, 0)
    return [k.tobytes() for k, _ in out], [d.tobytes() for _, d in out], counters, st["candidates"]


def child_main(path):
    """A fresh process per value of CUBESLAM_LSD_NFA_NMAX (the caller set it): the designed frames through the device stage, results to `path`."""
    import torch
    torch.cuda.is_available()
    from cube_slam_amd import _lib
    from cube_slam_amd.lsd import line_lbd_detect
    ctx = _lib.Context(0)
    det = line_lbd_detect(W, H, max_frames=F, ctx=ctx)
    kl, desc, counters, cand = run_detector(det, designed_frames(), "wave_per_frame")
    det.close()
    ctx.close()
    with open(path, "w") as fh:
        json.dump({"kl": [k.hex() for k in kl], "desc": [d.hex() for d in desc], "counters": list(counters), "candidates": cand}, fh)


@pytest.fixture(scope="module")
def frames():
    return designed_frames()


@pytest.fixture(scope="module")
def want(frames, oracle):
    """The oracle's KeyLines and descriptors of the designed frames, computed once."""
    kls = [oracle.lsd_detect(g) for g in frames]
    assert min(len(k) for k in kls) >= 20, [len(k) for k in kls]  # at least that many rectangles per frame reached rect_improve
    return [k.tobytes() for k in kls], [np.asarray(oracle.lbd_compute(g, k)).tobytes() for g, k in zip(frames, kls)]


@pytest.fixture(scope="module")
def det(ctx):
    from cube_slam_amd.lsd import line_lbd_detect
    d = line_lbd_detect(W, H, max_frames=F, ctx=ctx)
    yield d
    d.close()


def test_lookup_equals_direct_call_bitwise(det, frames, monkeypatch):
    monkeypatch.delenv("CUBESLAM_LSD_NFA_NMAX", raising=False)
    run_detector(det, frames, "wave_per_frame")  # the table belongs to a detector that has run the device stage
    t = []
    for j in range(11):
        for n in (0, 1, 2, NFA_NMAX - 1, NFA_NMAX):
            for k in sorted({0, min(1, n), max(n - 1, 0), n}):
                t.append((n, k, j))
        t += [(0, 0, j), (17, 0, j), (17, 17, j)]  # the early returns: n == 0, k == 0, n == k
    rng = np.random.default_rng(7)
    n = rng.integers(0, NFA_NMAX + 1, 4096)
    t += list(zip(n, (rng.random(4096) * (n + 1)).astype(np.int64), rng.integers(0, 11, 4096)))
    t = np.asarray(t, np.int32)
    assert (t[:, 1] <= t[:, 0]).all()
    table, direct, _, _ = det.nfa_probe(t)
    assert not np.isnan(direct).any()
    assert table.tobytes() == direct.tobytes(), t[table.view(np.uint64) != direct.view(np.uint64)][:10]
    assert len(np.unique(direct)) > 2000  # (not a table of one value)
    # beyond the bound the table holds nothing: NaN there, the direct call still answers
    table, direct, _, _ = det.nfa_probe(np.asarray([(NFA_NMAX + 1, 3, 0), (4000, 100, 10)], np.int32))
    assert np.isnan(table).all() and not np.isnan(direct).any()
    from cube_slam_amd._lib import lib, ptr
    bad = np.asarray([(3, 4, 0)], np.int32)
    assert hasattr(lib(), "cs_lsd_nfa_probe")  # exported by the library
    assert lib().cs_lsd_nfa_probe(det.ctx.ptr, det._l, 1, ptr(bad), ptr(np.zeros(2)), None) != 0  # k > n is refused


def test_default_bound_equals_oracle(det, frames, want, monkeypatch):
    monkeypatch.delenv("CUBESLAM_LSD_NFA_NMAX", raising=False)
    kl, desc, (finished, deferred), cand = run_detector(det, frames, "wave_per_frame")
    print("default bound: %d candidates, %d finished by the table kernel, %d deferred" % (cand, finished, deferred))
    assert kl == want[0] and desc == want[1]
    assert finished > 0 and finished + deferred == cand and cand >= 20 * F


@pytest.mark.parametrize("nmax", [8, 24, 0])
def test_lowered_bound_equals_oracle(want, tmp_path, nmax):
    out = tmp_path / "out.json"
    env = dict(os.environ, CUBESLAM_LSD_NFA_NMAX=str(nmax))
    env.pop("CUBESLAM_LSD_REGIONS", None)
    subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], check=True, env=env, cwd=ROOT, timeout=300)
    got = json.loads(out.read_text())
    finished, deferred = got["counters"]
    print("bound %d: %d candidates, %d finished by the table kernel, %d deferred" % (nmax, got["candidates"], finished, deferred))
    assert [bytes.fromhex(k) for k in got["kl"]] == want[0] and [bytes.fromhex(d) for d in got["desc"]] == want[1]
    assert finished + deferred == got["candidates"] and deferred > 0
    assert finished == 0 if nmax == 0 else finished > 0  # both paths ran, or (0) the deferred one alone


def test_table_rebuilt_for_a_larger_batch_and_another_size(ctx, frames, want, oracle, monkeypatch):
    from cube_slam_amd.lsd import line_lbd_detect
    monkeypatch.delenv("CUBESLAM_LSD_NFA_NMAX", raising=False)
    d = line_lbd_detect(W, H, max_frames=F, ctx=ctx)
    kl, desc, (finished, _), _ = run_detector(d, frames[:3], "wave_per_frame")
    assert kl == want[0][:3] and desc == want[1][:3] and finished > 0
    kl, desc, (finished, _), _ = run_detector(d, frames, "wave_per_frame")  # more frames than the stage was built for: built again, tables included
    assert kl == want[0] and desc == want[1] and finished > 0
    d.close()
    w2, h2 = 200, 136
    other = designed_frames(w2, h2, 2, seed=5)
    d = line_lbd_detect(w2, h2, max_frames=2, ctx=ctx)
    kl, desc, (finished, _), _ = run_detector(d, other, "wave_per_frame")
    d.close()
    ref = [oracle.lsd_detect(g) for g in other]
    assert kl == [k.tobytes() for k in ref] and min(len(k) for k in ref) >= 20 and finished > 0
    assert desc == [np.asarray(oracle.lbd_compute(g, k)).tobytes() for g, k in zip(other, ref)]


def test_device_stage_equals_host_stage_with_descriptors_and_twice(det, frames, want, monkeypatch):
    """KeyLines and LBD descriptors of the forced device stage against the host stage, then the device stage again on the same detector: the derivative maps'
    buffers and the rectangle kernels' has / line / counter buffers are reused while nothing of the first run is in flight."""
    monkeypatch.delenv("CUBESLAM_LSD_NFA_NMAX", raising=False)
    monkeypatch.delenv("CUBESLAM_LSD_REGIONS", raising=False)
    host = run_detector(det, frames, "host")
    dev1 = run_detector(det, frames, "wave_per_frame")
    dev2 = run_detector(det, frames, "wave_per_frame")  # back to back: the maps' buffers are reused while nothing of the first run is in flight
    assert host[0] == dev1[0] == dev2[0] == want[0]
    assert host[1] == dev1[1] == dev2[1] == want[1]
    assert sum(len(d) for d in want[1]) >= 32 * 20 * F


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child_main(sys.argv[1])
