"""CPU tests of the designed stereo inputs (tests/stereo_patterns.py): the restatement of Frame::ComputeStereoMatches reaches every seam a group was built for, with
the exact counts of the design.  These are the conditions that keep tests/test_stereo_edges_gpu.py from passing on all -1.  No device and no oracle: level 0 is the
designed image itself, the upper levels are stand-in arrays of the level sizes (only level 0 is designed)."""
import numpy as np
import pytest

from tests import stereo_patterns as sp
from tests import stereo_restatement as sr

f32 = np.float32


@pytest.fixture(scope="module")
def runs():
    out = {}
    for group, pairs in sp.groups().items():
        for p in pairs:
            st = {}
            uR, dep, kept = sr.compute_stereo_matches(p.kl, p.dl, p.kr, p.dr, sp.stand_in_levels(p.left), sp.stand_in_levels(p.right), sp.SF, sp.ISF, p.bf, p.b, stats=st)
            print(group, p.name, "nl %d nr %d" % (len(p.kl), len(p.kr)), {k: v for k, v in st.items() if k not in ("best", "sad")})
            out[p.name] = (p, st, uR, dep, kept)
    return out


def test_level_sizes_are_the_extractors():
    """cvRound(256 * inv_scale) x cvRound(128 * inv_scale): level 7 still holds the 11 x 21 strip."""
    assert list(zip(sp.LEVEL_W, sp.LEVEL_H)) == [(256, 128), (213, 107), (178, 89), (148, 74), (123, 62), (103, 51), (86, 43), (71, 36)]


def test_right_frames_are_level_major():
    for p in sp.batch():
        assert np.all(np.diff(p.kr["octave"]) >= 0), p.name


@pytest.mark.parametrize("name", [p.name for ps in sp.groups().values() for p in ps])
def test_every_pair_reaches_its_design(runs, name):
    sp.assert_reached(*runs[name])


@pytest.mark.parametrize("name", list(sp.CUT_SETS))
def test_cut_multisets(runs, name):
    p, st, uR, dep, kept = runs[name]
    sads, median = sp.CUT_SETS[name]
    assert [s for _, s in st["sad"]] == sads and st["median"] == median == sorted(sads)[len(sads) // 2]
    assert kept == sum(f32(s) < f32(f32(f32(1.5) * f32(1.4)) * f32(median)) for s in sads)


def test_cut_seams(runs):
    k = {n: runs[n][4] for n in sp.CUT_SETS}
    assert k == {"cut_first_of_bin": 8, "cut_256_last_of_bin": 5, "cut_bin0_exact": 7, "cut_512": 10, "cut_255": 4, "cut_n1": 1, "cut_n2": 2, "cut_zero": 0}
    # (float)s == thDist exactly: 1.5f * 1.4f * 10 is 21.0 in float, and 21 is dropped by the strict `<` (a product rounded up instead would keep it)
    p, st, uR, dep, kept = runs["cut_bin0_exact"]
    i21 = [i for i, s in st["sad"] if s == 21]
    assert len(i21) == 1 and f32(21) == sp.th_dist(10) and uR[i21[0]] == -1
    assert uR[[i for i, s in st["sad"] if s == 20][0]] >= 0
    # 537 < 537.6 <= 538 and 1075 < 1075.2 <= 1076
    p, st, uR, dep, kept = runs["cut_256_last_of_bin"]
    assert [s for i, s in st["sad"] if uR[i] < 0] == [538, 700]
    p, st, uR, dep, kept = runs["cut_512"]
    assert [s for i, s in st["sad"] if uR[i] < 0] == [1076]
    # the rank at the last / first element of its bin, in the loops that stride by 256
    assert [(len(runs[n][0].kl), runs[n][1]["median"], runs[n][4]) for n in ("cut_nl255", "cut_nl256", "cut_nl257")] == [(255, 1248, 255), (256, 1256, 256), (257, 1248, 257)]
    for n, k in (("cut_nl255", 127), ("cut_nl256", 128), ("cut_nl257", 128)):
        v = sorted(s for _, s in runs[n][1]["sad"])
        assert v[k] == runs[n][1]["median"]
    v = sorted(s for _, s in runs["cut_nl255"][1]["sad"])
    assert v[127] != v[128]  # the last of its value
    v = sorted(s for _, s in runs["cut_nl256"][1]["sad"])
    assert v[127] != v[128]  # the first of its value
    p, st, uR, dep, kept = runs["cut_all_rejected"]
    assert st["empty"] == 1 and st["edge_shift"] == 6 and st["accepted"] == 0 and kept == 0


def test_shift_and_disparity_exits(runs):
    p, st, uR, dep, kept = runs["shift"]
    assert st["edge_shift"] == 3 and st["accepted"] == 9  # e = -5, e = +5 and the all-equal row; e = -4 .. 4 accepted
    assert [i for i in range(12) if uR[i] < 0] == [0, 10, 11]
    p, st, uR, dep, kept = runs["disparity"]
    assert st["clamp"] == 3 and st["disparity"] == 3 and st["accepted"] == 7 and kept == 7
    i9 = p.tags.index("accept", 6)  # the symmetric pattern at disparity 9: deltaR == 0
    assert uR[i9] == p.kl["x"][i9] - f32(9) and dep[i9] == f32(f32(p.bf) / f32(9))


def test_window_rows_and_octaves(runs):
    p, st, uR, dep, kept = runs["window"]
    assert st["cand"] == 8 and kept == 8 and p.count("no_cand") == 6
    assert f32(80.0) in p.kr["x"] and np.nextafter(f32(80), f32(-np.inf)) in p.kr["x"] and f32(103.0) in p.kr["x"] and np.nextafter(f32(103), f32(np.inf)) in p.kr["x"]
    p, st, uR, dep, kept = runs["octave"]
    assert st["right_octave"] == 2 and st["cand"] == 4 and sorted(set(p.kr["octave"].tolist())) == [-1, 0, 1, 2, 5, 6, 7, 8]


def test_level_tables(runs):
    assert sorted(set(runs["levels_only7"][0].kr["octave"].tolist())) == [7]
    assert sorted(set(runs["levels_025"][0].kr["octave"].tolist())) == [0, 2, 5]
    p = runs["levels_seam"][0]
    assert np.all(p.kr["octave"][:256] == 1) and np.all(p.kr["octave"][256:] == 2) and len(p.kr) > 256
    assert sorted(b[1] for b in runs["levels_seam"][1]["best"])[-2:] == [256, 257]  # octave 3 starts its walk at the block seam
    p = runs["levels_ends"][0]
    assert p.kr["octave"][0] == -1 and p.kr["octave"][-1] == 8


def test_descriptor_seams(runs):
    for nl in (15, 16, 17):
        p, st, uR, dep, kept = runs["descriptor_nl%d" % nl]
        assert len(p.kl) == nl
        assert sorted(b[3] for b in st["best"]) == [1, 15, 15, 16, 17, 33] and sorted(p.fail_cand.values()) == [1, 16]
        assert sorted(b[2] for b in st["best"]) == [40, 40, 40, 99, 99, 99]  # TH_HIGH - 1 passes ...
        for iL, n in p.fail_cand.items():  # ... TH_HIGH does not
            assert min(sp.hamming(p.dl[iL], p.dr[r]) for r in range(len(p.kr)) if p.kr["y"][r] == p.kl["y"][iL]) == sr.TH_HIGH
        assert sorted(how for _, _, how in p.ties) == ["lanes", "lanes", "lanes", "lanes", "stride"]


def test_batch_holds_empty_sides():
    b = sp.batch()
    sizes = [(len(p.kl), len(p.kr)) for p in b]
    assert (3, 0) in sizes and (0, 3) in sizes and (0, 0) in sizes and len(b) == sum(len(v) for v in sp.groups().values()) + 3
    assert sizes[0][1] > 0 and sizes[-1][1] > 0
