"""The inputs of tests/test_lbd_edges_gpu.py are what that file says they are: every maker of tests/lbd_patterns.py against the CPU oracle alone.  No device is
needed, so the GPU cases' preconditions can be checked anywhere."""
import numpy as np
import pytest

from tests import lbd_patterns as lp


def test_map_sizes_cross_every_seam():
    ws, hs = {w for w, h in lp.MAP_SIZES}, {h for w, h in lp.MAP_SIZES}
    assert len(lp.MAP_SIZES) == 2 * len(lp.MAP_WIDTHS) + 2 * len(lp.MAP_HEIGHTS) - 4 == 76  # (257, 67), (13, 9), (257, 9) and (13, 67) are in both sweeps
    for n in (1, 2):
        assert {n * lp.STRIP + k for k in range(-1, 5)} <= ws, "a full last strip, and one of 1 .. 4 columns"
    assert lp.STRIP + 5 in ws and {lp.ROWS + k for k in range(-1, 5)} <= hs and {2 * lp.ROWS + k for k in range(-1, 3)} <= hs, "a last block of 1 .. 3 rows"
    assert {w % 4 for w in ws} == {0, 1, 2, 3} and min(ws) == 8 and min(hs) == 8 and any(h < lp.ROWS for h in hs)
    assert any(w * h % 4 for w, h in lp.MAP_SIZES)
    buf, stride = lp.padded(lp.byte_pattern(5, 3), 2)
    assert stride == 7 and buf.shape == (3, 7) and np.all(buf[:, 5:] == 0xFF) and np.array_equal(buf[:, :5], lp.byte_pattern(5, 3))


def test_map_images_reach_the_clamp_and_the_high_byte(oracle):
    on_clamp = 0
    for W, H in lp.MAP_SIZES:
        b = oracle.lbd_maps(lp.saturated(W, H))[0]
        assert np.count_nonzero(b == 255) > 0 and np.count_nonzero(b < 255) > 0, (W, H)
        on_clamp += np.count_nonzero(b == 255)
        _, dx, dy = oracle.lbd_maps(lp.byte_pattern(W, H))
        if W >= 31:  # (7 x + 13 y never wraps inside a frame of 13 columns and 9 rows)
            assert max(np.abs(dx.astype(np.int32)).max(), np.abs(dy.astype(np.int32)).max()) > 255, (W, H)
            assert np.count_nonzero(dx < 0) and np.count_nonzero(dx > 0) and np.count_nonzero(dy < 0) and np.count_nonzero(dy > 0), (W, H)
    W, H, _ = lp.STRIDE_CASE
    assert np.count_nonzero(oracle.lbd_maps(lp.saturated(W, H))[0] == 255) > 5000 and on_clamp > 100000
    img = lp.byte_pattern(40, 20)
    assert np.all(img[:, 1:] != img[:, :-1]) and np.all(img[1:] != img[:-1])


def test_keylines_maker():
    kl = lp.keylines([(1.5, 2, 4.5, 6, None), (10, 3, 2, 3, 5)])
    assert kl.dtype == lp.KEYLINE_DTYPE and list(kl["class_id"]) == [0, 1] and list(kl["numOfPixels"]) == [5, 5] and list(kl["octave"]) == [0, 0]
    assert kl["lineLength"][0] == np.float32(5) and kl["angle"][0] == np.float32(np.arctan2(np.float32(4), np.float32(3))) and kl["angle"][1] == np.float32(np.pi)
    for a, b in (("startPointX", "sPointInOctaveX"), ("startPointY", "sPointInOctaveY"), ("endPointX", "ePointInOctaveX"), ("endPointY", "ePointInOctaveY")):
        assert np.array_equal(kl[a], kl[b])
    assert list(kl["sPointInOctaveX"]) == [1.5, 10] and list(kl["ePointInOctaveY"]) == [6, 3]


@pytest.mark.parametrize("W,H", lp.DESC_FRAMES)
def test_battery(oracle, W, H):
    img = lp.texture(lp.DESC_SEED[(W, H)], W, H)
    names, kl = lp.battery(W, H)
    assert len(set(names)) == len(names) == len(kl) == 6 + len(lp.WALK_COUNTS) + 4 + len(lp.ANGLES)
    assert lp.sample_extent(kl) < 32000
    assert [int(kl["numOfPixels"][names.index("walk_%d" % n)]) for n in lp.WALK_COUNTS] == list(lp.WALK_COUNTS)
    desc, fd = oracle.lbd_compute(img, kl, want_float=True)
    for i, name in enumerate(names):
        if name in ("outside", "walk_0"):
            assert np.isnan(fd[i]).all() and not desc[i].any(), name
        else:
            assert not np.isnan(fd[i]).any() and desc[i].any(), name
    # what hangs over really leaves the frame, on the sides it names
    k = {n: kl[names.index(n)] for n in names}
    assert k["over_left_top"]["sPointInOctaveX"] < 0 and k["over_left_top"]["sPointInOctaveY"] < 0
    assert k["over_right_bottom"]["ePointInOctaveX"] > W - 1 and k["over_right_bottom"]["ePointInOctaveY"] > H - 1
    assert k["over_top_and_bottom"]["sPointInOctaveY"] == -30 and k["over_top_and_bottom"]["ePointInOctaveY"] == H + 30
    assert min(k["outside"]["sPointInOctaveX"] - 31 - W, k["outside"]["sPointInOctaveY"] - 31 - H) > 0, "the whole support region is beyond the corner"
    assert not np.array_equal(desc[names.index("forward")], desc[names.index("backward")])
    # the half-integer lines: every support-region row samples on .5 in the across-line coordinate, and the walk along the line leaves it there
    x0, y0, dL0, dL1 = lp.support_start(oracle, k["half_horizontal"])
    assert (dL0, dL1) == (1, 0) and y0 % 1 == 0.5
    x0, y0, dL0, dL1 = lp.support_start(oracle, k["half_vertical"])
    assert dL1 == 1 and x0 % 1 == 0.5 and abs(dL0) < 1e-7
    xs = x0 - np.arange(63, dtype=np.float32)
    assert np.array_equal((xs + dL0).astype(np.float32), xs) and np.all(xs % 1 == 0.5)
    # the overwritten angles are the float32 values named, outside [-pi, pi] included
    got = [float(kl["angle"][i]) for i, n in enumerate(names) if n.startswith("angle_")]
    assert got == [float(np.float32(a)) for a in lp.ANGLES] and max(got) > 4 * 3.14 and min(got) < -3.15


@pytest.mark.parametrize("W,H", lp.DESC_FRAMES)
def test_random_lines(oracle, W, H):
    kl = lp.random_lines(W, H)
    assert len(kl) == lp.RANDOM_LINES == 400 and lp.sample_extent(kl) < 32000
    xs = np.concatenate([kl["sPointInOctaveX"], kl["ePointInOctaveX"]]); ys = np.concatenate([kl["sPointInOctaveY"], kl["ePointInOctaveY"]])
    assert -W / 4 <= xs.min() < 0 and W <= xs.max() <= 5 * W / 4 and -H / 4 <= ys.min() < 0 and H <= ys.max() <= 5 * H / 4
    desc, fd = oracle.lbd_compute(lp.texture(lp.DESC_SEED[(W, H)], W, H), kl, want_float=True)
    assert not np.isnan(fd).any()
    assert len(np.unique(desc, axis=0)) == len(kl)


@pytest.mark.parametrize("W,H", lp.DESC_FRAMES)
def test_flat_frame_has_no_descriptor(oracle, W, H):
    _, kl = lp.battery(W, H)
    desc, fd = oracle.lbd_compute(lp.flat(W, H), kl, want_float=True)
    assert np.isnan(fd).all() and not desc.any()


def test_batch_frames_and_growth(oracle):
    assert (lp.BATCH_W * lp.BATCH_H) % 4 != 0 and lp.STRIP < lp.BATCH_W < 2 * lp.STRIP and lp.ROWS < lp.BATCH_H < 2 * lp.ROWS
    counts = [len(oracle.lsd_detect(lp.texture(s, lp.BATCH_W, lp.BATCH_H))) for s in lp.BATCH_SEEDS]
    assert tuple(counts[:4]) == lp.BATCH_LINES_3_TO_6
    frames = lp.batch_frames()
    assert len(frames) == 5 < lp.BATCH_MAX and [len(oracle.lsd_detect(f)) for f in frames] == [0] + counts[:3] + [0]
    one, eight = lp.growth_batches()
    assert len(one) == 1 and len(eight) == lp.BATCH_MAX and np.array_equal(one[0], eight[0])
    n1, n8 = counts[0], sum(counts)
    assert n8 > n1 + n1 // 4 + 256, "the second batch does not fit the buffers sized for the first"


def test_matcher_cases(oracle):
    q, t, j = lp.duplicate_case()
    assert np.array_equal(t[j], t[j + 256]) and np.array_equal(q[2], t[j])
    bi, bd, dist = lp.brute_knn(q, t)
    assert bi[2] == j and bd[2] == 0 and np.count_nonzero(dist[2] == 0) == 2 and lp.brute_second(dist)[2] == 0
    q, t, j, nbits = lp.tie_case()
    bi, bd, dist = lp.brute_knn(q, t)
    at = np.nonzero(dist[1] == nbits)[0]
    assert bi[1] == j and bd[1] == nbits > 0 and len(at) == 2 and at[0] // 256 != at[1] // 256 and lp.brute_second(dist)[1] == nbits
    # the numpy brute force and the oracle agree on the whole grid of sizes
    for nq in lp.MATCH_NQ:
        for nt in lp.MATCH_NT:
            q, t = lp.descriptors(nq, 100 + nq), lp.descriptors(nt, 200 + nt)
            bi, bd, dist = lp.brute_knn(q, t)
            obi, obd, osd = oracle.hamming_knn2(q, t)
            assert np.array_equal(obi, bi) and np.array_equal(obd, bd) and np.array_equal(osd, lp.brute_second(dist)), (nq, nt)
