"""The region walk of a line detector under the front-end runner runs on its context's background stream and the worker's HOST thread waits for it
(cs_ctx::bg_begin / bg_end, lsd_regions.hip): nothing on the device orders the worker's own stream behind the walk, so everything that reads the walk's
outputs must be launched behind that wait.  Four workers with the wave-per-frame stage, as in the benchmark: five high-priority streams, four background ones."""
import numpy as np
import pytest

from cube_slam_amd import _lib, synth
from cube_slam_amd.frontend import Frontend
from cube_slam_amd.lsd import KEYLINE_DTYPE, line_lbd_detect

pytestmark = pytest.mark.gpu

W, H, F, N_SETS, N_WORKERS = 160, 120, 16, 8, 4


def _frame_sets():
    """N_SETS sets of F distinct textured frames: the sixteen 160x120 tiles of one 640x480 scene each."""
    sets = []
    for i in range(N_SETS):
        g = synth.cuboid_scene(4100 + i, n_boxes=3, bg_texture=0.5)["gray"]
        sets.append(np.ascontiguousarray(np.stack([g[y:y + H, x:x + W] for y in range(0, 480, H) for x in range(0, 640, W)])))
    return sets


def _detector(c):
    d = line_lbd_detect(W, H, max_frames=F, ctx=c)
    d.set_region_stage("wave_per_frame")
    return d


@pytest.fixture(scope="module")
def lone(ctx):
    """(frame sets, per set the (KeyLines, descriptors) bytes of every frame from a lone detector: no runner, same stage, the walk on its own stream)."""
    sets = _frame_sets()
    c = _lib.Context(0)
    d = _detector(c)
    ref = []
    for g in sets:
        d.upload(g)
        d.run()
        assert d.region_stats()["device"] and not d.region_stats()["host_fallback"]
        ref.append([tuple(a.tobytes() for a in d.read(f)) for f in range(F)])
    d.close()
    c.close()
    n_lines = [sum(len(kl) // KEYLINE_DTYPE.itemsize for kl, _ in r) for r in ref]
    assert min(n_lines) >= F  # the frames have lines to find, in every set
    assert len({r[0][0] for r in ref}) == N_SETS  # ... and the sets differ
    return sets, ref


class _Runner:
    """The caller's context, four line workers on contexts of their own (all at the caller's high priority, as bench.py creates them) and the runner over them."""

    def __init__(self, phased=False):
        self.ctx = _lib.Context(0, priority=1)
        self.lctx = [_lib.Context(0, priority=1) for _ in range(N_WORKERS)]
        self.lsds = [_detector(c) for c in self.lctx]
        self.fe = Frontend(self.ctx, line_detectors=self.lsds, phased=phased)

    def close(self):
        self.fe.close()
        for d in self.lsds:
            d.close()
        for c in self.lctx + [self.ctx]:
            c.close()


def _set_of(step, worker):
    return (step + 2 * worker) % N_SETS  # differs between the workers of a step and between a worker's consecutive passes


def _passes(r, sets, ref, steps, per_drain, step0=0):
    """`steps` steps, drained every `per_drain`; in front of each group every detector is handed another frame set.  After a drain all workers are free and the
    runner hands passes out in rotation (phased: by step number), so pass k ran on worker k % N_WORKERS.  -> passes per worker"""
    done = [0] * N_WORKERS
    for k0 in range(step0, step0 + steps, per_drain):
        for w, d in enumerate(r.lsds):
            d.upload(sets[_set_of(k0, w)])
        for _ in range(per_drain):
            r.fe.step()
        r.fe.drain()
        for k in range(k0, k0 + per_drain):
            w = k % N_WORKERS
            d = r.lsds[w]
            done[w] += 1
            assert d.region_stats()["device"] and not d.region_stats()["host_fallback"]
            want = ref[_set_of(k0, w)]
            for f in range(F):
                kl, desc = d.read(f)
                assert kl.tobytes() == want[f][0], (k, w, f)
                assert desc.tobytes() == want[f][1], (k, w, f)
    return done


@pytest.mark.parametrize("phased", [False, True])
def test_results_per_pass(lone, phased):
    """Eight drained steps with the detectors' frames changed in front of each one, then eight steps with four passes in flight at a time: KeyLines and LBD
    descriptors of every frame after every pass are a lone detector's bytes.  A rectangle stage (or the LBD blur, which reuses the walk's map) that started
    before its walk had finished would read the pass before's rectangles and counts, which belong to other frames.  Phased: the same through the gate --
    single passes released by the drain, then complete super-steps that the fourth step opens itself."""
    sets, ref = lone
    r = _Runner(phased=phased)
    try:
        assert r.fe.queues()[1] == 1 + 2 * N_WORKERS
        _passes(r, sets, ref, 8, 1)
        _passes(r, sets, ref, 8, N_WORKERS, step0=8)
    finally:
        r.close()


def test_timing_records(lone):
    """The walk and the scan of its counts are launched on the background stream: one record per pass each with the context's timing on (their event pairs
    are that stream's), none with it off."""
    sets, ref = lone
    r = _Runner()
    try:
        _passes(r, sets, ref, N_WORKERS, N_WORKERS)  # first passes: buffers, the log-gamma table
        for c in r.lctx:
            c.timing(True)
            c.timing_reset()
        done = _passes(r, sets, ref, 8, N_WORKERS, step0=4)
        for c, n in zip(r.lctx, done):
            assert n == 2
            for name in ("lsd_rg_seq", "lsd_rg_cand_scan", "lsd_rg_improve", "lsd_gradient"):
                ms, cnt = c.timing_get(name)
                assert cnt == n and ms > 0, (name, cnt, ms)
        for c in r.lctx:
            c.timing(False)
            c.timing_reset()
        _passes(r, sets, ref, N_WORKERS, N_WORKERS, step0=12)
        for c in r.lctx:
            for name in ("lsd_rg_seq", "lsd_rg_cand_scan", "lsd_rg_improve"):
                assert c.timing_get(name) == (0.0, 0), name
    finally:
        r.close()


def test_teardown_without_a_drain(lone):
    """Two steps, then the runner, the detectors and their contexts are closed with no drain in between: the destroy paths wait for the background streams too."""
    sets, _ = lone
    r = _Runner()
    for w, d in enumerate(r.lsds):
        d.upload(sets[w])
    r.fe.step()
    r.fe.step()
    r.close()
    r = _Runner()  # ... and the device is as usable as before
    try:
        _passes(r, sets, lone[1], 1, 1)
    finally:
        r.close()
