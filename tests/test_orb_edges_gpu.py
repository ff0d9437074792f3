"""GPU parity of the HIP ORBextractor with the CPU oracle, bit for bit, where tests/test_orb_gpu.py does not go: frame sizes off the three it uses, the device
quadtree's hand-over to the host (more than four root nodes, quotas the kernel does not take, frame sizes whose child counts could leave 16 bits), inputs whose
responses and node sizes all tie, the per-cell threshold fallback deciding the result, quotas of 0 / 1 and of thousands, one handle over runs of different
sizes, the sizes cs_orb_create refuses, and a row stride other than the width.

Every test takes its preconditions from the ORACLE (or from the level sizes / quotas the extractor reports), never from the device's result, and asserts
them, so that a test cannot stop stressing what it names without failing.  No tolerance anywhere: key points are compared as bytes, descriptors with array_equal.

Out of scope, because the reference itself is undefined there: a frame one of whose levels has no cell (fewer than 30 pixels between the borders) and a level
with nIni = round(width / height of the candidate frame) = 0, i.e. portrait narrower than 1 : 2 (DistributeOctTree divides by nIni, ORBextractor.cc:547-549)."""
import ctypes as C
import math

import numpy as np
import pytest

from cube_slam_amd import synth
from cube_slam_amd._lib import check, lib
from cube_slam_amd.orb import KEYPOINT_DTYPE, ORBextractor
from tests import orb_patterns as pat
from tests.test_orb_gpu import _check_frame

pytestmark = pytest.mark.gpu

f32 = np.float32
CS_ERR_BAD_ARG, CS_ERR_CAPACITY = -2, -4
INI_TH, MIN_TH = 20, 7
BG = 100


def _nini(w, h):
    """Root nodes of a level of w x h pixels: round((maxBorderX - minBorderX) / (maxBorderY - minBorderY)) in float (ORBextractor.cc:547)."""
    return int(math.floor(float(f32(w - 32) / f32(h - 32)) + 0.5))


def _level_dims(ext):
    out = []
    for l in range(ext.nlevels):
        w, h = C.c_int(), C.c_int()
        check(ext.ctx.ptr, lib().cs_orb_get_level(ext.ctx.ptr, ext._e, 0, l, 0, None, C.byref(w), C.byref(h)), "cs_orb_get_level")
        out.append((w.value, h.value))
    return out


def _qt_lds(quotas):
    """Dynamic LDS of orb_quadtree for the extractor's largest level quota (cs_orb_create): four lists of CAPL shorts, three arrays of CAPV
    64-bit words, two prefix arrays of CAPV + 1 ints, CAPN deletion bits in 32-bit words, CAPV shorts, 64 bytes of slack."""
    n = max(int(max(quotas)), 1)
    capl, capv, capn = 4 * n + 16, n + 8, 12 * n + 64
    return 8 * capl + 8 * capv * 3 + 4 * (capv + 1) * 2 + 4 * ((capn + 31) // 32) + 2 * capv + 64, capn


def _device_quadtree_expected(quotas):
    lds, capn = _qt_lds(quotas)
    return capn < 32768 and lds <= 150 * 1024


def _counted(ctx, fn):
    """fn() with the context's timing on -> (its result, launches of orb_quadtree, host quadtree sections)."""
    ctx.timing(True); ctx.timing_reset()
    try:
        r = fn()
        return r, ctx.timing_get("orb_quadtree")[1], ctx.timing_get("host_orb_quadtree")[1]
    finally:
        ctx.timing(False)


def _assert_equal(got, ref, what=""):
    (gk, gd), (rk, rd) = got, ref
    assert len(gk) == len(rk), "%s: %d key points, the oracle has %d" % (what, len(gk), len(rk))
    assert gk.tobytes() == rk.tobytes(), what + ": keypoints (x, y, size, angle, response, octave) bit-exact"
    assert np.array_equal(gd, rd), what + ": descriptors bit-exact"


def _texture(seed, W, H, shift=0):
    return synth.texture_image(seed, W, H, shift=shift)


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("W,H,sf,nl,frames", [(641, 479, 1.2, 8, 2), (333, 251, 1.2, 8, 2), (255, 255, 1.2, 8, 2), (480, 640, 1.2, 8, 2), (1920, 1080, 1.2, 8, 1),
                                              (641, 479, 1.1, 12, 2), (480, 640, 1.5, 4, 2)])
def test_sizes_off_the_tile_and_block_grids(ctx, oracle, W, H, sf, nl, frames):
    """Odd widths and heights, a portrait frame, a small square one whose top levels are a single cell, the largest common frame, and two other pyramids: every
    pyramid level, blurred level and candidate list, the key points and the descriptors equal the oracle's.  Precondition (oracle): every level yields a key point.
    (1920 x 1080 runs DistributeOctTree on the host: test_child_count_bound_hands_large_frames_to_the_host.)"""
    imgs = [_texture(70 + i, W, H, shift=3 * i) for i in range(frames)]
    ext = ORBextractor(1000, sf, nl, INI_TH, MIN_TH, W, H, max_frames=2, ctx=ctx)
    ora = oracle.ORBextractor(1000, sf, nl, INI_TH, MIN_TH)
    assert np.array_equal(ext.features_per_level(), ora.features_per_level())
    got = ext.extract_batch(np.stack(imgs))
    for f, img in enumerate(imgs):
        rk, rd = _check_frame(oracle, ext, ora, img, f)
        assert sorted(set(rk["octave"].tolist())) == list(range(nl)), "precondition: a key point on every level"
        _assert_equal(got[f], (rk, rd), "%dx%d frame %d" % (W, H, f))
    ext.close()


# ------------------------------------------------------------------------------------------------ the quadtree's way out
@pytest.mark.parametrize("W,H", [(1241, 340), (1280, 300)])
def test_more_than_four_roots_redo_the_batch_on_the_host(ctx, oracle, W, H):
    """A level with nIni >= 5 makes orb_quadtree raise its status and cs_orb_run redo the whole batch with the host quadtree, reusing the blur of the device attempt.
    Preconditions (level sizes the extractor reports): some level has nIni >= 5 and, for 1241 x 340, some level nIni <= 4 (so the kernel did real work on part of the
    batch before the redo).  Evidence that the path ran: orb_quadtree launched once AND host_orb_quadtree counted once in the same run."""
    imgs = [_texture(80 + i, W, H, shift=4 * i) for i in range(3)]
    ext = ORBextractor(2000, 1.2, 8, INI_TH, MIN_TH, W, H, max_frames=3, ctx=ctx)
    ora = oracle.ORBextractor(2000, 1.2, 8, INI_TH, MIN_TH)
    ext.upload(np.stack(imgs))
    ninis = [_nini(w, h) for w, h in _level_dims(ext)]
    assert max(ninis) >= 5, ninis
    if (W, H) == (1241, 340):
        assert min(ninis) <= 4, ninis
    assert _device_quadtree_expected(ext.features_per_level())
    _, n_dev, n_host = _counted(ctx, ext.run)
    assert n_dev == 1 and n_host == 1, "device attempt, then the host redo: orb_quadtree %d, host_orb_quadtree %d" % (n_dev, n_host)
    got = ext.read()
    kps, desc, first = ext.read_packed()
    assert first[0] == 0 and first[-1] == len(kps) == sum(len(k) for k, _ in got)
    for f, img in enumerate(imgs):
        ref = _check_frame(oracle, ext, ora, img, f)
        assert len(ref[0]) > 500
        _assert_equal(got[f], ref, "frame %d" % f)
        _assert_equal((kps[first[f]:first[f + 1]], desc[first[f]:first[f + 1]]), ref, "packed frame %d" % f)
    # a second run of the same handle takes the same way; an extractor without a panorama level on the same context stays on the device
    _, n_dev, n_host = _counted(ctx, ext.run)
    assert (n_dev, n_host) == (1, 1)
    for f, img in enumerate(imgs):
        _assert_equal(ext.read()[f], ora(img), "second run, frame %d" % f)
    vga = [_texture(90 + i, 640, 480) for i in range(2)]
    ext2 = ORBextractor(1000, 1.2, 8, INI_TH, MIN_TH, 640, 480, max_frames=2, ctx=ctx)
    ora2 = oracle.ORBextractor(1000, 1.2, 8, INI_TH, MIN_TH)
    got2, n_dev, n_host = _counted(ctx, lambda: ext2.extract_batch(np.stack(vga)))
    assert (n_dev, n_host) == (1, 0)
    for f, img in enumerate(vga):
        _assert_equal(got2[f], ora2(img), "640x480 frame %d" % f)
    ext2.close(); ext.close()


def test_three_roots_stay_on_the_device(ctx, oracle):
    """nIni = 3 (1000 x 340: three roots on levels 0 - 4, four above).  Preconditions: every level has nIni <= 4, some level exactly 3.  The host quadtree is not counted."""
    W, H = 1000, 340
    imgs = [_texture(85 + i, W, H, shift=2 * i) for i in range(2)]
    ext = ORBextractor(1500, 1.2, 8, INI_TH, MIN_TH, W, H, max_frames=2, ctx=ctx)
    ora = oracle.ORBextractor(1500, 1.2, 8, INI_TH, MIN_TH)
    ext.upload(np.stack(imgs))
    ninis = [_nini(w, h) for w, h in _level_dims(ext)]
    assert max(ninis) <= 4 and 3 in ninis, ninis
    _, n_dev, n_host = _counted(ctx, ext.run)
    assert (n_dev, n_host) == (1, 0)
    got = ext.read()
    for f, img in enumerate(imgs):
        ref = _check_frame(oracle, ext, ora, img, f)
        assert len(ref[0]) > 500
        _assert_equal(got[f], ref, "frame %d" % f)
    ext.close()


# ------------------------------------------------------------------------------------------------ ties
def _pattern(name, W, H):
    """(points, fg per point or one value, the points the oracle must report as level-0 candidates, response values)."""
    sp = 16 if W == 640 else 20
    if name == "lattice":
        p = pat.lattice(W, H, sp)
    elif name == "jittered":
        p = pat.jittered_lattice(W, H, sp, 3, seed=5)
    elif name == "cluster":
        p = pat.cluster_and_sparse(W, H, seed=6)
    elif name == "quadrant":
        p = pat.one_quadrant(W, H, seed=7, spacing=8)
    elif name == "two_classes":
        p, strong = pat.two_classes(W, H, seed=8, spacing=14 if W == 640 else 18)
        fg = pat.two_class_values(strong, BG, INI_TH, MIN_TH)
        cell = pat.level0_cell(W, H, p)
        reported = strong | ~np.isin(cell, cell[strong])  # a weak dot is found only where its cell holds no strong one
        return p, fg, p[reported], sorted({int(v) - BG - 1 for v in fg[reported]})
    pat.check_isolated(p)
    return p, BG + 3 * INI_TH, p, [3 * INI_TH - 1]


def _assert_level0_candidates(ora, expect_points, responses):
    c = ora.candidates(0)
    got = sorted((int(x) + pat.MINB, int(y) + pat.MINB) for x, y, _ in c)
    assert got == sorted((int(x), int(y)) for x, y in expect_points), "precondition: the oracle's level-0 candidates are exactly the drawn dots (%d against %d)" % (len(got), len(expect_points))
    assert sorted(set(c[:, 2].astype(int).tolist())) == responses, "precondition: the responses take the values %s" % responses
    return len(c)


def _nfeatures_for_level0_quota(q):
    """nfeatures whose level-0 quota (1.2 / 8 levels, ORBextractor.cc:431-441) is q or q + 1."""
    factor = 1.0 / 1.2
    return int(math.ceil(q * (1 - factor ** 8) / (1 - factor)))


@pytest.mark.parametrize("W,H", [(640, 480), (1241, 376)])
@pytest.mark.parametrize("name", ["lattice", "jittered", "cluster", "quadrant", "two_classes"])
def test_tied_responses_and_node_sizes(ctx, oracle, monkeypatch, name, W, H):
    """Dots of one brightness (two for two_classes): every level-0 response ties and, on the lattices, node sizes tie -- the best-response rule (first point wins), the
    (size, creation id) order of the largest-first phase and the stable partitions decide which key points come out.  Quotas well below, about equal to and above the
    number of level-0 candidates; device and host quadtree.  Preconditions (oracle): the level-0 candidates are exactly the dots the pattern says, their responses take
    one value (two for two_classes), and the candidate count stands to the level-0 quota as the case names.  The device runs are on the device by the counters."""
    p, fg, expect, responses = _pattern(name, W, H)
    img = pat.dots(W, H, p, BG, fg)
    n = len(expect)
    assert 200 <= n <= 1400, n
    for relation, nfeat in (("above", _nfeatures_for_level0_quota(n // 5)), ("equal", _nfeatures_for_level0_quota(n)), ("below", _nfeatures_for_level0_quota(n * 8 // 5))):
        ora = oracle.ORBextractor(nfeat, 1.2, 8, INI_TH, MIN_TH)
        ref = ora(img)
        assert _assert_level0_candidates(ora, expect, responses) == n
        q0 = int(ora.features_per_level()[0])
        if relation == "above":
            assert n >= 4 * q0, (n, q0)
        elif relation == "equal":
            assert q0 - 1 <= n <= q0, (n, q0)
        else:
            assert q0 >= n * 3 // 2, (n, q0)
        assert _device_quadtree_expected(ora.features_per_level())
        # (dots in one quadrant of one root: the root's only child ends the reference's loop after one pass, "size == prevSize": one key point on level 0)
        assert (ref[0]["octave"] == 0).sum() >= (1 if name == "quadrant" else min(n, q0) * 3 // 4)
        for mode in ("device", "host"):
            if mode == "host":
                monkeypatch.setenv("CUBESLAM_ORB_QUADTREE", "host")
            else:
                monkeypatch.delenv("CUBESLAM_ORB_QUADTREE", raising=False)
            ext = ORBextractor(nfeat, 1.2, 8, INI_TH, MIN_TH, W, H, ctx=ctx)
            got, n_dev, n_host = _counted(ctx, lambda: ext(img))
            assert (n_dev, n_host) == ((1, 0) if mode == "device" else (0, 1)), (mode, n_dev, n_host)
            _assert_equal(got, ref, "%s quadtree, candidates %s the quota (%d features)" % (mode, relation, nfeat))
            ext.close()
    monkeypatch.delenv("CUBESLAM_ORB_QUADTREE", raising=False)


def test_quadtree_compactions_at_wave_and_pass_seams(ctx, oracle):
    """orb_quadtree's two ordered compactions (block_rank, passes of 256 threads) run over the node list of every pass of the first phase: the expandable nodes, and
    behind the children the others.  pat.quadtree_seam_dots brings one pass to each length and pattern of tests/compaction_seams.py (a list of no nodes does not
    occur: a level without candidates ends the kernel ahead of them), so the first compaction sees the pattern and the second its complement.  Preconditions: the
    oracle's level-0 candidates are the dots; the quota stays above every pass's length + 3 x its expandable nodes, so the first phase is the restated one and the
    second never starts; the device quadtree ran."""
    from tests import compaction_seams as cs
    W, H, nfeat = 640, 480, 10000
    ora = oracle.ORBextractor(nfeat, 1.2, 8, INI_TH, MIN_TH)
    ext = ORBextractor(nfeat, 1.2, 8, INI_TH, MIN_TH, W, H, ctx=ctx)
    for n, pattern, fl in cs.cases(cs.SIZES[1:]):
        p, passes, k = pat.quadtree_seam_dots(W, H, fl)
        assert [len(q) > 1 for _, q in passes[k]] == fl.tolist()
        ref = ora(pat.dots(W, H, p, BG, BG + 3 * INI_TH))
        assert _assert_level0_candidates(ora, p, [3 * INI_TH - 1]) == len(p)
        q0 = int(ora.features_per_level()[0])
        assert max(len(s) + 3 * sum(len(q) > 1 for _, q in s) for s in passes) < q0 and _device_quadtree_expected(ora.features_per_level())
        assert (ref[0]["octave"] == 0).sum() == len(passes[-1])
        got, n_dev, n_host = _counted(ctx, lambda: ext(pat.dots(W, H, p, BG, BG + 3 * INI_TH)))
        assert (n_dev, n_host) == (1, 0)
        _assert_equal(got, ref, "%d nodes, %s" % (n, pattern))
    ext.close()


# ------------------------------------------------------------------------------------------------ per-cell threshold fallback
def test_threshold_fallback_is_decided_cell_by_cell(ctx, oracle):
    """Strong and weak dots, sometimes in one cell.  Preconditions from ora.candidates(0): some weak dots are candidates, all of them in cells without a strong dot;
    some weak dots are not, all of them in cells with a strong one; every strong dot is a candidate."""
    W, H = 640, 480
    p, strong = pat.two_classes(W, H, seed=21, spacing=10)
    img = pat.dots(W, H, p, BG, pat.two_class_values(strong, BG, INI_TH, MIN_TH))
    ext = ORBextractor(2000, 1.2, 8, INI_TH, MIN_TH, W, H, ctx=ctx)
    ora = oracle.ORBextractor(2000, 1.2, 8, INI_TH, MIN_TH)
    got = ext(img)
    ref = _check_frame(oracle, ext, ora, img, 0)  # candidates of every level included
    cand = {(int(x) + pat.MINB, int(y) + pat.MINB) for x, y, _ in ora.candidates(0)}
    is_cand = np.array([(int(x), int(y)) in cand for x, y in p])
    cell = pat.level0_cell(W, H, p)
    with_strong = np.isin(cell, cell[strong])
    assert is_cand[strong].all() and len(cand) == is_cand.sum()
    weak_in, weak_out = ~strong & is_cand, ~strong & ~is_cand
    assert weak_in.sum() > 100 and not with_strong[weak_in].any()
    assert weak_out.sum() > 100 and with_strong[weak_out].all()
    _assert_equal(got, ref, "two contrast classes")
    ext.close()


# ------------------------------------------------------------------------------------------------ quotas
@pytest.mark.parametrize("nfeat", [1, 5, 8])
def test_quotas_of_zero_and_one(ctx, oracle, nfeat):
    """Eight levels share 1, 5 or 8 features: quotas of 0 and 1, and the reference still does one split pass per level (up to four key points per root).
    Precondition: some level's quota is 0 or 1."""
    W, H = 640, 480
    imgs = [_texture(100 + i, W, H) for i in range(2)]
    ext = ORBextractor(nfeat, 1.2, 8, INI_TH, MIN_TH, W, H, max_frames=2, ctx=ctx)
    ora = oracle.ORBextractor(nfeat, 1.2, 8, INI_TH, MIN_TH)
    q = ora.features_per_level()
    assert np.array_equal(ext.features_per_level(), q) and q.min() <= 1 and q.sum() == nfeat
    got, n_dev, n_host = _counted(ctx, lambda: ext.extract_batch(np.stack(imgs)))
    assert (n_dev, n_host) == (1, 0)
    for f, img in enumerate(imgs):
        ref = ora(img)
        assert len(ref[0]) >= 8
        _assert_equal(got[f], ref, "frame %d" % f)
    ext.close()


@pytest.mark.parametrize("nfeat", [5000, 10000])
def test_quotas_beyond_64_kb_of_lds(ctx, oracle, nfeat):
    """Level quotas above about 1000 need more than 64 KB of dynamic LDS (hipFuncSetAttribute).  Preconditions: the oracle's level-0 candidates exceed the level-0 quota
    (uniform noise), the LDS recomputed from the documented formula is above 64 KB and within the kernel's 150 KB.  Evidence: orb_quadtree launched, no host quadtree."""
    W, H = 640, 480
    imgs = [pat.noise(W, H, 30 + i) for i in range(2)]
    ext = ORBextractor(nfeat, 1.2, 8, INI_TH, MIN_TH, W, H, max_frames=2, ctx=ctx)
    ora = oracle.ORBextractor(nfeat, 1.2, 8, INI_TH, MIN_TH)
    q = ora.features_per_level()
    lds, capn = _qt_lds(q)
    assert np.array_equal(ext.features_per_level(), q) and 64 * 1024 < lds <= 150 * 1024 and capn < 32768, (lds, capn)
    got, n_dev, n_host = _counted(ctx, lambda: ext.extract_batch(np.stack(imgs)))
    assert (n_dev, n_host) == (1, 0)
    for f, img in enumerate(imgs):
        ref = ora(img)
        assert len(ora.candidates(0)) > q[0], "precondition: more level-0 candidates than the quota"
        assert len(ref[0]) > nfeat // 2
        _assert_equal(got[f], ref, "frame %d" % f)
    ext.close()


def test_quota_the_kernel_does_not_take_goes_to_the_host(ctx, oracle):
    """nfeatures = 20000 on one level: CAPN = 12 N + 64 does not fit the kernel's 16-bit node ids, cs_orb_create plans the host quadtree.  Evidence: the host
    quadtree is counted, orb_quadtree is not launched."""
    W, H = 640, 480
    img = pat.noise(W, H, 40)
    ext = ORBextractor(20000, 1.2, 1, INI_TH, MIN_TH, W, H, ctx=ctx)
    ora = oracle.ORBextractor(20000, 1.2, 1, INI_TH, MIN_TH)
    assert ora.features_per_level().tolist() == [20000] and not _device_quadtree_expected([20000])
    got, n_dev, n_host = _counted(ctx, lambda: ext(img))
    assert (n_dev, n_host) == (0, 1)
    ref = ora(img)
    assert len(ref[0]) > 5000
    _assert_equal(got, ref, "20000 features, one level")
    ext.close()


# ------------------------------------------------------------------------------------------------ one handle, runs of different sizes
def test_handle_reuse_regrows_and_forgets(ctx, oracle):
    """One extractor: three sparse frames, three dense ones (the candidate arrays are freed and regrown), ONE sparse frame (fewer frames than the run before: nothing
    of the dense run's per-level counts and offsets may be read), the three sparse frames again.  Precondition (oracle): the dense batch has more candidates than
    1.25 x the sparse batch + 4096, the room the first allocation left.  Every run equals a fresh extractor and the oracle."""
    W, H = 640, 480
    sparse = np.stack([pat.dots(W, H, pat.lattice(W, H, 40, offset=(7 * i, 5 * i)), BG, BG + 3 * INI_TH) for i in range(3)])
    dense = np.stack([pat.noise(W, H, 50 + i) for i in range(3)])
    ora = oracle.ORBextractor(1000, 1.2, 8, INI_TH, MIN_TH)

    def oracle_batch(imgs):
        out, total = [], 0
        for img in imgs:
            out.append(ora(img))
            total += sum(len(ora.candidates(l)) for l in range(8))
        return out, total

    ref_sparse, n_sparse = oracle_batch(sparse)
    ref_dense, n_dense = oracle_batch(dense)
    assert n_sparse > 0 and n_dense > n_sparse + n_sparse // 4 + 4096, (n_sparse, n_dense)
    ext = ORBextractor(1000, 1.2, 8, INI_TH, MIN_TH, W, H, max_frames=3, ctx=ctx)
    for what, imgs, ref in (("sparse", sparse, ref_sparse), ("dense", dense, ref_dense), ("one sparse frame", sparse[1:2], ref_sparse[1:2]), ("sparse again", sparse, ref_sparse)):
        got = ext.extract_batch(imgs)
        kps, desc, first = ext.read_packed()
        fresh = ORBextractor(1000, 1.2, 8, INI_TH, MIN_TH, W, H, max_frames=3, ctx=ctx)
        got_fresh = fresh.extract_batch(imgs)
        fresh.close()
        assert len(got) == len(imgs) == len(first) - 1
        for f in range(len(imgs)):
            assert len(ref[f][0]) > 50
            _assert_equal(got[f], ref[f], "%s, frame %d" % (what, f))
            _assert_equal(got_fresh[f], ref[f], "%s, fresh extractor, frame %d" % (what, f))
            _assert_equal((kps[first[f]:first[f + 1]], desc[first[f]:first[f + 1]]), ref[f], "%s, packed frame %d" % (what, f))
    ext.close()


# ------------------------------------------------------------------------------------------------ refusal
def test_create_refuses_a_cell_wider_than_the_kernel_holds(ctx, oracle):
    """327 x 240 at 1.2 / 8 levels: level 7 is 91 pixels wide, one cell of 59 columns; orb_cells holds windows of up to 58 + 6.  cs_orb_create returns
    CS_ERR_CAPACITY and leaves *out NULL (DESIGN.md section 8 records the limit); the context goes on to serve a 333 x 251 extractor."""
    out = C.c_void_p(0xdead0)
    r = lib().cs_orb_create(ctx.ptr, 1000, C.c_float(1.2), 8, INI_TH, MIN_TH, 327, 240, 1, C.byref(out))
    assert r == CS_ERR_CAPACITY and not out.value
    W, H = 333, 251
    img = _texture(110, W, H)
    ext = ORBextractor(1000, 1.2, 8, INI_TH, MIN_TH, W, H, ctx=ctx)
    ref = oracle.ORBextractor(1000, 1.2, 8, INI_TH, MIN_TH)(img)
    assert len(ref[0]) > 100
    _assert_equal(ext(img), ref, "333x251 after the refusal")
    ext.close()


# ------------------------------------------------------------------------------------------------ child counts and their 16 bits
def test_child_count_bound_hands_large_frames_to_the_host(ctx, oracle):
    """orb_quadtree packs the four child sizes of a split into 16 bits each.  cs_orb_create bounds the candidates a first-split child can hold (non-maximum suppression
    leaves none 8-adjacent inside a cell; seams between cells counted) and plans the host quadtree where the bound reaches 65536: 1200 x 900 (one root, children of
    584 x 434: bound 66900) is just past it, 1152 x 864 (61 thousand) just below.  Evidence: host quadtree counted and orb_quadtree not launched for the first, the
    reverse for the second; both equal the oracle on a lattice frame."""
    for (W, H), want in (((1200, 900), (0, 1)), ((1152, 864), (1, 0))):
        p = pat.lattice(W, H, 16)
        img = pat.dots(W, H, p, BG, BG + 3 * INI_TH)
        ext = ORBextractor(2000, 1.2, 8, INI_TH, MIN_TH, W, H, ctx=ctx)
        ora = oracle.ORBextractor(2000, 1.2, 8, INI_TH, MIN_TH)
        assert _device_quadtree_expected(ora.features_per_level()) and _nini(W, H) == 1
        got, n_dev, n_host = _counted(ctx, lambda: ext(img))
        assert (n_dev, n_host) == want, (W, H, n_dev, n_host)
        ref = ora(img)
        assert _assert_level0_candidates(ora, p, [3 * INI_TH - 1]) > 3000 and len(ref[0]) > 1000
        _assert_equal(got, ref, "%dx%d lattice" % (W, H))
        ext.close()


# ------------------------------------------------------------------------------------------------ stride
def test_row_stride_other_than_the_width(ctx):
    """cs_orb_extract, cs_lsd_detect and cs_lbd_compute on frames embedded in a buffer of W + 13 bytes per row, the padding filled with 0xFF: byte-equal to the
    contiguous call.  stride = W - 1 is CS_ERR_BAD_ARG."""
    from cube_slam_amd.lsd import KEYLINE_DTYPE, line_lbd_detect
    W, H, S = 640, 480, 640 + 13
    imgs = np.stack([_texture(120 + i, W, H, shift=3 * i) for i in range(2)])
    wide = np.full((2, H, S), 0xFF, np.uint8)
    wide[:, :, :W] = imgs
    u8 = C.POINTER(C.c_uint8)
    # ORB
    ext = ORBextractor(1000, 1.2, 8, INI_TH, MIN_TH, W, H, max_frames=2, ctx=ctx)

    def orb(buf, stride):
        kps = np.zeros((2, ext.cap), KEYPOINT_DTYPE); desc = np.zeros((2, ext.cap, 32), np.uint8); counts = np.zeros(2, np.int32)
        r = lib().cs_orb_extract(ctx.ptr, ext._e, buf.ctypes.data_as(u8), 2, stride, kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(u8), ext.cap, counts.ctypes.data_as(C.POINTER(C.c_int)))
        return r, [(kps[f, :counts[f]].copy(), desc[f, :counts[f]].copy()) for f in range(2)]

    r0, want = orb(imgs, W)
    r1, got = orb(wide, S)
    assert r0 == 0 and r1 == 0
    for f in range(2):
        assert len(want[f][0]) > 500
        _assert_equal(got[f], want[f], "ORB, stride %d, frame %d" % (S, f))
    assert orb(imgs, W - 1)[0] == CS_ERR_BAD_ARG
    ext.close()
    # LSD
    det = line_lbd_detect(W, H, max_frames=2, ctx=ctx)

    def lsd(buf, stride):
        out = np.zeros((2, det.cap), KEYLINE_DTYPE); counts = np.zeros(2, np.int32)
        r = lib().cs_lsd_detect(ctx.ptr, det._l, buf.ctypes.data_as(u8), 2, stride, out.ctypes.data_as(C.c_void_p), det.cap, counts.ctypes.data_as(C.POINTER(C.c_int)))
        return r, [out[f, :counts[f]].copy() for f in range(2)]

    r0, want_l = lsd(imgs, W)
    r1, got_l = lsd(wide, S)
    assert r0 == 0 and r1 == 0
    for f in range(2):
        assert len(want_l[f]) > 50 and got_l[f].tobytes() == want_l[f].tobytes(), "LSD, stride %d, frame %d" % (S, f)
    assert lsd(imgs, W - 1)[0] == CS_ERR_BAD_ARG

    # LBD
    def lbd(buf, stride, kl):
        desc = np.zeros((len(kl), 32), np.uint8); fd = np.zeros((len(kl), 72), np.float32)
        r = lib().cs_lbd_compute(ctx.ptr, buf.ctypes.data_as(u8), W, H, stride, kl.ctypes.data_as(C.c_void_p), len(kl), desc.ctypes.data_as(u8), fd.ctypes.data_as(C.POINTER(C.c_float)))
        return r, desc, fd

    kl = np.ascontiguousarray(want_l[1])
    r0, d0, f0 = lbd(np.ascontiguousarray(imgs[1]), W, kl)
    r1, d1, f1 = lbd(np.ascontiguousarray(wide[1]), S, kl)
    assert r0 == 0 and r1 == 0 and d0.any()
    assert np.array_equal(d0, d1) and f0.tobytes() == f1.tobytes(), "LBD, stride %d" % S
    assert lbd(np.ascontiguousarray(imgs[1]), W - 1, kl)[0] == CS_ERR_BAD_ARG
    det.close()
