"""GPU parity of the LBD path (lbd_blur5, lbd_sobel, lbd_line_desc, the batched entry points under cs_lsd_run and the line matcher) off the sizes and lines the
other files use: frames that cross the 256-column strip and the 64-row block of the map kernels by a few pixels, lines whose support region is clamped or lies
outside the frame, walks around the unroll of eight, sample coordinates on .5, a resident batch whose maps live in the region stage's arena, line buffers that
grow on a reused handle, and the matcher at its tile seam.  Every comparison is exact; the inputs come from tests/lbd_patterns.py, and tests/test_lbd_patterns.py
proves on the oracle alone that they are what they claim."""
import ctypes as C

import numpy as np
import pytest

from cube_slam_amd import matcher
from cube_slam_amd._lib import lib
from cube_slam_amd.lsd import line_lbd_detect
from tests import lbd_patterns as lp

pytestmark = pytest.mark.gpu
CS_ERR_BAD_ARG = -2


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _maps(ctx, buf, W, H, stride):
    """cs_lbd_maps on rows of `stride` bytes."""
    b = np.zeros((H, W), np.uint8); dx = np.zeros((H, W), np.int16); dy = np.zeros((H, W), np.int16)
    r = lib().cs_lbd_maps(ctx.ptr, _p(buf, C.c_uint8), W, H, stride, _p(b, C.c_uint8), _p(dx, C.c_int16), _p(dy, C.c_int16))
    assert r == 0, (W, H, r)
    return b, dx, dy


@pytest.fixture(scope="module")
def det(ctx):
    d = line_lbd_detect(64, 64, ctx=ctx)  # cs_lbd_maps / cs_lbd_compute / cs_lbd_match take the frame from their arguments, not from the handle
    yield d
    d.close()


# ----------------------------------------------------------------------------------------------- 1. maps at the seams
@pytest.mark.parametrize("kind", lp.MAP_KINDS)
def test_maps_at_strip_and_block_seams(ctx, oracle, kind):
    """W in {8 .. 13, 31, 252 .. 261, 511 .. 516} at H = 67 and 9, H in {8, 9, 11, 61 .. 70, 127 .. 130} at W = 257 and 13."""
    for W, H in lp.MAP_SIZES:
        img = lp.map_image(kind, W, H)
        for name, a, b in zip(("blur", "dx", "dy"), _maps(ctx, img, W, H, W), oracle.lbd_maps(img)):
            assert np.array_equal(a, b), (kind, W, H, name, np.argwhere(a != b)[:4].tolist())


@pytest.mark.parametrize("kind", lp.MAP_KINDS)
def test_maps_from_padded_rows(ctx, oracle, kind):
    W, H, pad = lp.STRIDE_CASE
    img = lp.map_image(kind, W, H)
    buf, stride = lp.padded(img, pad)
    for a, b in zip(_maps(ctx, buf, W, H, stride), oracle.lbd_maps(img)):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------------------------- 2. descriptors of lines LSD never produces
def _same_descriptors(det, oracle, img, kl):
    desc, fd = det.get_line_descriptors(img, kl, want_float=True)
    rdesc, rfd = oracle.lbd_compute(img, kl, want_float=True)
    bad = np.nonzero((desc != rdesc).any(1))[0]
    assert np.array_equal(desc, rdesc), bad[:8].tolist()
    assert lp.same_vectors(fd, rfd)
    assert np.array_equal(det.get_line_descriptors(img, kl), rdesc), "without the float output"
    return rdesc, rfd


@pytest.mark.parametrize("W,H", lp.DESC_FRAMES)
def test_named_lines(det, oracle, W, H):
    img = lp.texture(lp.DESC_SEED[(W, H)], W, H)
    names, kl = lp.battery(W, H)
    desc, fd = _same_descriptors(det, oracle, img, kl)
    assert sorted(names[i] for i in np.nonzero(np.isnan(fd).any(1))[0]) == ["outside", "walk_0"]
    for i in range(len(kl)):  # one line per launch: the same answer whatever shares the grid
        assert np.array_equal(det.get_line_descriptors(img, kl[i:i + 1]), desc[i:i + 1]), names[i]


@pytest.mark.parametrize("W,H", lp.DESC_FRAMES)
def test_random_lines(det, oracle, W, H):
    _, fd = _same_descriptors(det, oracle, lp.texture(lp.DESC_SEED[(W, H)], W, H), lp.random_lines(W, H))
    assert not np.isnan(fd).any()


@pytest.mark.parametrize("W,H", lp.DESC_FRAMES)
def test_flat_frame(det, oracle, W, H):
    _, kl = lp.battery(W, H)
    img = lp.flat(W, H)
    _same_descriptors(det, oracle, img, kl)
    desc, fd = det.get_line_descriptors(img, kl, want_float=True)
    assert np.isnan(fd).all() and not desc.any()


def test_argument_checks(ctx):
    """Refused before anything is launched: numOfPixels outside [0, 32767] (the reference keeps it in a short), a frame wider than a short holds; n = 0 is accepted."""
    img = lp.flat(64, 16)
    desc = np.full((2, 32), 7, np.uint8)

    def compute(kl, n, W=64, H=16, stride=64):
        return lib().cs_lbd_compute(ctx.ptr, _p(img, C.c_uint8), W, H, stride, kl.ctypes.data_as(C.c_void_p), n, _p(desc, C.c_uint8), None)
    for bad in (-1, 32768):
        assert compute(lp.keylines([(5, 5, 30, 8, None), (5, 5, 30, 8, bad)]), 2) == CS_ERR_BAD_ARG, bad
    ok = lp.keylines([(5, 5, 30, 8, None)])
    assert compute(ok, 1, W=32768, stride=32768) == CS_ERR_BAD_ARG  # (refused by the width alone: the image is never read)
    assert compute(ok, 0) == 0
    assert np.all(desc == 7), "nothing was written"


# ----------------------------------------------------------------------------------------------- 3. the resident batch with LBD in the arena
def _batch_equals_oracle(det, oracle, frames):
    got = [det.read(f) for f in range(len(frames))]
    for f, img in enumerate(frames):
        rkl = oracle.lsd_detect(img)
        assert got[f][0].tobytes() == rkl.tobytes(), f
        assert np.array_equal(got[f][1], oracle.lbd_compute(img, rkl)), f
    return got


def test_partial_batch_with_maps_in_the_arena(ctx, oracle, monkeypatch):
    """261 x 97 (two strips, two row blocks, W * H odd), five frames of max_frames = 8, flat ones first and last, through the device region stage: both LBD maps in its arena."""
    monkeypatch.delenv("CUBESLAM_LSD_REGIONS", raising=False)
    frames = lp.batch_frames()
    det = line_lbd_detect(lp.BATCH_W, lp.BATCH_H, max_frames=lp.BATCH_MAX, ctx=ctx)
    det.upload(frames)
    det.set_region_stage("wave_per_frame")
    det.run(with_lbd=True)
    st = det.region_stats()
    assert st["device"] and not st["host_fallback"]
    dev = _batch_equals_oracle(det, oracle, frames)
    assert [len(kl) for kl, _ in dev] == [0] + list(lp.BATCH_LINES_3_TO_6[:3]) + [0]
    det.set_region_stage("host")
    det.run(with_lbd=True)
    assert not det.region_stats()["device"]
    for f in range(len(frames)):
        kl, desc = det.read(f)
        assert kl.tobytes() == dev[f][0].tobytes() and desc.tobytes() == dev[f][1].tobytes(), f
    det.close()


def test_line_buffers_grow_on_a_reused_handle(ctx, oracle, monkeypatch):
    """One frame, then eight on the same handle: the second batch's lines outgrow the buffers sized for the first (nl > line_cap in lsd_run)."""
    monkeypatch.delenv("CUBESLAM_LSD_REGIONS", raising=False)
    one, eight = lp.growth_batches()
    det = line_lbd_detect(lp.BATCH_W, lp.BATCH_H, max_frames=lp.BATCH_MAX, ctx=ctx)
    det.set_region_stage("host")
    det.upload(one); det.run(with_lbd=True)
    n1 = len(_batch_equals_oracle(det, oracle, one)[0][0])
    det.upload(eight); det.run(with_lbd=True)
    n8 = sum(len(kl) for kl, _ in _batch_equals_oracle(det, oracle, eight))
    assert n8 > n1 + n1 // 4 + 256
    det.close()


# ----------------------------------------------------------------------------------------------- 4. line matcher
def _match_equals_brute_force(det, ctx, oracle, q, t, thres):
    bi, bd, dist = lp.brute_knn(q, t)
    sd = lp.brute_second(dist)
    for got in (matcher.hamming_knn2(ctx, q, t), oracle.hamming_knn2(q, t)):
        assert np.array_equal(got[0], bi) and np.array_equal(got[1], bd) and np.array_equal(got[2], sd)
    for th in thres:
        keep = bd.astype(np.float32) < np.float32(th)
        qi, ti, d = det.match_line_descrip(q, t, th)
        assert np.array_equal(qi, np.nonzero(keep)[0]) and np.array_equal(ti, bi[keep]) and np.array_equal(d, bd[keep]), th
    return bi, bd, sd


def test_matcher_sizes_around_the_tile(det, ctx, oracle):
    for nq in lp.MATCH_NQ:
        for nt in lp.MATCH_NT:
            q, t = lp.descriptors(nq, 100 + nq), lp.descriptors(nt, 200 + nt)
            bi, bd, sd = _match_equals_brute_force(det, ctx, oracle, q, t, (25.0, 110.0, 300.0))
            if nt == 1:
                assert np.all(bi == 0) and np.all(sd == lp.INT_MAX)
    assert len(det.match_line_descrip(lp.descriptors(4, 1), lp.descriptors(513, 2), 300.0)[0]) == 4


def test_matcher_ties_across_tiles(det, ctx, oracle):
    q, t, j = lp.duplicate_case()
    bi, bd, sd = _match_equals_brute_force(det, ctx, oracle, q, t, (25.0,))
    assert (bi[2], bd[2], sd[2]) == (j, 0, 0)
    qi, ti, d = det.match_line_descrip(q, t, 25.0)
    assert list(qi) == [2] and list(ti) == [j] and list(d) == [0]
    q, t, j, nbits = lp.tie_case()
    bi, bd, sd = _match_equals_brute_force(det, ctx, oracle, q, t, (25.0,))
    assert (bi[1], bd[1], sd[1]) == (j, nbits, nbits)


def test_matcher_threshold_is_strict(det, ctx, oracle):
    q, t = lp.descriptors(257, 41), lp.descriptors(513, 42)
    _, bd, _ = lp.brute_knn(q, t)
    at = int(np.sort(bd)[len(bd) // 4])  # a best distance that occurs, with matches below it
    on, above = np.float32(at), np.nextafter(np.float32(at), np.float32(np.inf))
    assert 0 < np.count_nonzero(bd < at) < np.count_nonzero(bd <= at)
    _match_equals_brute_force(det, ctx, oracle, q, t, (on, above, 0.0))
    assert np.array_equal(det.match_line_descrip(q, t, on)[0], np.nonzero(bd < at)[0]), "a match at the threshold is dropped"
    assert np.array_equal(det.match_line_descrip(q, t, above)[0], np.nonzero(bd <= at)[0]), "the next float keeps it"
    assert len(det.match_line_descrip(q, t, 0.0)[0]) == 0
    q, t, j = lp.duplicate_case()
    assert len(det.match_line_descrip(q, t, 0.0)[0]) == 0, "not even a distance of 0 is below 0"
