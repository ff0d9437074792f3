"""GPU: lsd_maps (one wave per strip of scaled columns and block of scaled rows, its state in LDS), the two-launch scan and lsd_emit (a
workgroup per group of strips and rows) against the oracle, byte for byte: every frame width and height from 16 to 200 through the host stage,
so that every strip and row-block boundary is crossed whatever the strip width is; the device stage at small sizes, behind empty frames, on a
reused handle and at the bench's frame size."""
import ctypes as C

import numpy as np
import pytest

from cube_slam_amd import synth
from cube_slam_amd.lsd import line_lbd_detect

pytestmark = pytest.mark.gpu


def _host_stage_equals_oracle(ctx, oracle, img):
    H, W = img.shape
    det = line_lbd_detect(W, H, ctx=ctx)
    got = det.detect_raw_lines(img)
    assert not det.region_stats()["device"]
    sc, mg, an = det.maps(0)
    det.close()
    rsc, rmg, ran, _ = oracle.lsd_maps(img)
    assert np.count_nonzero(ran != -1024.0) >= 1, (W, H)  # the image has defined pixels
    assert sc.shape == rsc.shape and np.array_equal(sc, rsc), (W, H)
    assert np.array_equal(mg[:-1, :-1], rmg[:-1, :-1]) and np.array_equal(an, ran), (W, H)
    assert got.tobytes() == oracle.lsd_detect(img).tobytes(), (W, H)


def test_width_sweep_host_stage(ctx, oracle, monkeypatch):
    """W = 16 .. 200 at H = 24: a last strip of one column, a frame narrower than a strip, reflection on both sides inside one strip."""
    monkeypatch.delenv("CUBESLAM_LSD_REGIONS", raising=False)
    for W in range(16, 201):
        _host_stage_equals_oracle(ctx, oracle, synth.texture_image(100 + W, W, 24))


def test_height_sweep_host_stage(ctx, oracle, monkeypatch):
    """H = 16 .. 200 at W = 24: row blocks of one row, the bottom clamp, vertical reflection inside a block."""
    monkeypatch.delenv("CUBESLAM_LSD_REGIONS", raising=False)
    for H in range(16, 201):
        _host_stage_equals_oracle(ctx, oracle, synth.texture_image(400 + H, 24, H))


def _modgrad_angles(det, f):
    """cs_lsd_get_maps without the scaled frame (a device-stage batch does not keep it)."""
    from cube_slam_amd._lib import check, lib
    sw, sh = C.c_int(), C.c_int()
    check(det.ctx.ptr, lib().cs_lsd_get_maps(det.ctx.ptr, det._l, f, None, None, None, C.byref(sw), C.byref(sh)), "cs_lsd_get_maps")
    n = sw.value * sh.value
    mg, an = np.zeros(n), np.zeros(n)
    check(det.ctx.ptr, lib().cs_lsd_get_maps(det.ctx.ptr, det._l, f, None, mg.ctypes.data_as(C.POINTER(C.c_double)), an.ctypes.data_as(C.POINTER(C.c_double)),
                                             C.byref(sw), C.byref(sh)), "cs_lsd_get_maps")
    return mg.reshape(sh.value, sw.value), an.reshape(sh.value, sw.value)


def _device_stage_equals_oracle(det, oracle, frames, min_lines):
    """One device-stage batch: KeyLines, LBD bytes and maps equal the oracle's per frame; the host stage of the same detector gives the same bytes."""
    det.upload(frames)
    det.set_region_stage("wave_per_frame")
    det.run(with_lbd=True)
    st = det.region_stats()
    assert st["device"] and not st["host_fallback"]
    dev = [det.read(f) for f in range(len(frames))]
    for f, img in enumerate(frames):
        rkl = oracle.lsd_detect(img)
        assert len(rkl) >= min_lines[f], f
        assert dev[f][0].tobytes() == rkl.tobytes(), f
        assert dev[f][1].tobytes() == oracle.lbd_compute(img, rkl).tobytes(), f
        mg, an = _modgrad_angles(det, f)
        _, rmg, ran, _ = oracle.lsd_maps(img)
        assert np.array_equal(mg[:-1, :-1], rmg[:-1, :-1]) and np.array_equal(an, ran), f
    det.set_region_stage("host")
    det.run(with_lbd=True)
    assert not det.region_stats()["device"]
    for f in range(len(frames)):
        kl, desc = det.read(f)
        assert dev[f][0].tobytes() == kl.tobytes() and dev[f][1].tobytes() == desc.tobytes(), f


def test_device_stage_small_size_and_handle_reuse(ctx, oracle, monkeypatch):
    """161 x 81 (scaled 129 x 65), six frames with flat ones in front of and between the textured ones: emit<true> (device) and emit<false> (host),
    frame bases behind an empty frame, the alone flags through the walk.  Then the same handle with two frames, then with an all-flat batch (total == 0)."""
    monkeypatch.delenv("CUBESLAM_LSD_REGIONS", raising=False)
    W, H = 161, 81
    flat = np.full((H, W), 90, np.uint8)
    tex = {s: synth.texture_image(s, W, H) for s in (3, 4, 5, 6, 7, 8)}
    det = line_lbd_detect(W, H, max_frames=6, ctx=ctx)
    _device_stage_equals_oracle(det, oracle, np.stack([flat, tex[3], tex[4], tex[5], flat, tex[6]]), (0, 5, 5, 5, 0, 5))
    _device_stage_equals_oracle(det, oracle, np.stack([tex[7], tex[8]]), (5, 5))
    det.upload(np.stack([flat, flat, flat]))
    det.set_region_stage("wave_per_frame")
    det.run(with_lbd=True)
    assert all(len(det.read(f)[0]) == 0 for f in range(3))
    det.close()


def test_device_stage_bench_size(ctx, oracle, monkeypatch):
    """320 x 240, a cuboid scene with textured background: four row blocks of lsd_maps, several strips, bench-like content, through the device stage."""
    monkeypatch.delenv("CUBESLAM_LSD_REGIONS", raising=False)
    img = synth.cuboid_scene(2000, W=320, H=240, n_boxes=3, bg_texture=0.5)["gray"]
    det = line_lbd_detect(320, 240, max_frames=1, ctx=ctx)
    _device_stage_equals_oracle(det, oracle, img[None], (50,))
    det.close()
