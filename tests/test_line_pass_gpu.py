"""GPU: the line pass outside the region walk -- lsd_maps (blur + resize + gradient in one kernel), lsd_rg_improve (variants per lane group), the
pinned hand-overs -- against the host region stage and the oracle, byte for byte."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cube_slam_amd import synth
from cube_slam_amd.lsd import line_lbd_detect

pytestmark = pytest.mark.gpu
F = 512


@pytest.fixture(scope="module")
def batch():
    """511 distinct textured scenes (bg_texture 0 .. 0.5) and one flat frame."""
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        scenes = list(ex.map(lambda i: synth.cuboid_scene(2000 + i, n_boxes=3, bg_texture=0.5 * i / (F - 2))["gray"], range(F - 1)))
    return np.stack(scenes + [np.full((480, 640), 90, np.uint8)])


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


def test_large_batch_device_stage_equals_host_stage(ctx, oracle, batch, monkeypatch):
    """512 distinct frames with LBD: the device region stage (lsd_rg_seq + lsd_rg_improve) gives every frame the KeyLines and descriptors the same
    detector's host stage gives it; eight of them are the oracle's.  Then the maps of the device-stage batch: no scaled frame, modgrad and angles
    the oracle's."""
    monkeypatch.delenv("CUBESLAM_LSD_REGIONS", raising=False)
    det = line_lbd_detect(640, 480, max_frames=F, ctx=ctx)
    det.upload(batch)
    det.set_region_stage("auto")
    det.run(with_lbd=True)
    st = det.region_stats()
    assert st["device"] and not st["host_fallback"] and st["candidates"] > 10000
    dev = [det.read(f) for f in range(F)]
    sample = (0, 1, 97, 200, 255, 384, 510, 511)
    for f in sample:
        mg, an = _modgrad_angles(det, f)
        _, rmg, ran, _ = oracle.lsd_maps(batch[f])
        assert np.array_equal(mg[:-1, :-1], rmg[:-1, :-1]) and np.array_equal(an, ran), f
    with pytest.raises(Exception):
        det.maps(0)  # the device stage took the scaled frames' buffer over
    det.set_region_stage("host")
    det.run(with_lbd=True)
    assert not det.region_stats()["device"]
    n_lines = 0
    for f in range(F):
        kl, desc = det.read(f)
        assert dev[f][0].tobytes() == kl.tobytes(), f
        assert dev[f][1].tobytes() == desc.tobytes(), f
        n_lines += len(kl)
    assert len(dev[F - 1][0]) == 0 and n_lines > 50 * F
    for f in sample:
        assert dev[f][0].tobytes() == oracle.lsd_detect(batch[f]).tobytes(), f
    det.close()


@pytest.mark.parametrize("W,H", [(97, 61), (641, 479), (1241, 376)])
def test_odd_sizes_host_stage_maps(ctx, oracle, monkeypatch, W, H):
    """Odd frame sizes through the host stage: the last strip of lsd_maps is partly outside the frame, the last row block short, the resize taps
    clamped at the right and bottom edges -- scaled frame, modgrad and angles equal the oracle's, and so do the KeyLines."""
    monkeypatch.delenv("CUBESLAM_LSD_REGIONS", raising=False)
    imgs = [synth.texture_image(11, W, H), synth.texture_image(12, W, H, shift=5)]
    if W >= 640:
        imgs.append(synth.cuboid_scene(13, W=W, H=H, n_boxes=3, bg_texture=0.25)["gray"])
    det = line_lbd_detect(W, H, max_frames=len(imgs), ctx=ctx)
    got = det.detect_raw_lines(np.stack(imgs))
    assert not det.region_stats()["device"]
    for f, img in enumerate(imgs):
        sc, mg, an = det.maps(f)
        rsc, rmg, ran, _ = oracle.lsd_maps(img)
        assert sc.shape == rsc.shape and np.array_equal(sc, rsc), f
        assert np.array_equal(mg[:-1, :-1], rmg[:-1, :-1]) and np.array_equal(an, ran), f
        assert got[f].tobytes() == oracle.lsd_detect(img).tobytes(), f
    det.close()
