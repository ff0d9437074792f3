"""CPU: tests/klt_restatement.py itself.  The definition it restates is recalled, not checked against an OpenCV build, so one check rests on nothing but geometry: a
smooth texture shifted by a known sub-pixel vector must be tracked to that vector.  The pyramid's stop rule at its seam, and Scharr / pyrDown rows worked out by hand."""
import numpy as np

from tests import klt_patterns as kp
from tests import klt_restatement as kr

f32 = np.float32


def test_translation_is_recovered():
    """An untracked or sign-flipped point is off by at least 2 pixels, a tracked one by the 8-bit rounding of the texture: well under 0.5."""
    w, h, shift = 120, 100, np.array([2.3, -2.6])
    a, b = kp.texture(1, w, h), kp.texture(1, w, h, *shift)
    pts = np.array([[x, y] for y in range(30, h - 29, 10) for x in range(30, w - 29, 12)], f32)
    nxt, status, err = kr.track(a, b, pts)
    off = np.abs(nxt - pts - shift).max()
    print("translation: %d points, all tracked %s, worst error %.4f px, worst err %.3f" % (len(pts), bool(status.all()), off, err.max()))
    assert len(pts) >= 20 and status.all() and off < 0.5
    back = kr.track(b, a, pts)  # and the other way round
    assert back[1].all() and np.abs(back[0] - pts + shift).max() < 0.5


def test_level_stop_rule_at_its_seam():
    for w, h, want in ((169, 169, 4), (168, 168, 3), (169, 60, 2), (42, 64, 1), (64, 42, 1), (42, 42, 1), (43, 43, 2), (640, 480, 4)):
        levels = kr.build_pyramid(np.zeros((h, w), np.uint8))
        assert len(levels) == want == kr.n_levels(w, h), (w, h)
    assert [l.shape[1] for l in kr.build_pyramid(np.zeros((169, 169), np.uint8))] == [169, 85, 43, 22]
    assert [l.shape[1] for l in kr.build_pyramid(np.zeros((168, 168), np.uint8))] == [168, 84, 42]  # the next one would be 21 wide


def test_scharr_and_pyrdown_rows_by_hand():
    """I(x, y) = x^2 + 3 y on 5 x 5.  Scharr: the vertical pass gives t0 = 16 x^2 + c(y) and t1 = 6 (0 on the edge rows, where row -1 is row 1), so
    Ix = 16 ((x + 1)^2 - (x - 1)^2) inside and 0 in the edge columns (column -1 is column 1), Iy = (6 + 6) 3 + 60 = 96 inside and 0 on the edge rows.
    pyrDown: the kernel is separable and I is a sum, so a pixel is (16 (F + G) + 128) >> 8 with F = [16, 80, 176] (the taps over x^2 with columns -2, -1 -> 2, 1 and
    5, 6 -> 3, 2) and G = [36, 96, 156]."""
    y, x = np.mgrid[0:5, 0:5]
    img = (x * x + 3 * y).astype(np.uint8)
    d = kr.scharr_deriv(img)
    for row in range(5):
        assert d[row, :, 0].tolist() == [0, 64, 128, 192, 0], row
        assert d[row, :, 1].tolist() == ([0] * 5 if row in (0, 4) else [96] * 5), row
    assert kr.pyr_down(img).tolist() == [[3, 7, 13], [7, 11, 17], [11, 15, 21]]
    assert kr.pad_zero(d)[20, 21:26, 0].tolist() == [0] * 5 and kr.pad_zero(d)[21, 21:26, 0].tolist() == [0, 64, 128, 192, 0]
    p = kr.pad_reflect101(img)
    assert p[21, 17:30].tolist() == [16, 9, 4, 1, 0, 1, 4, 9, 16, 9, 4, 1, 0]  # REFLECT_101 repeats with period 2 (n - 1)


def test_weights_round_half_even():
    assert kr.weights(f32(0), f32(0)) == (16384, 0, 0, 0)
    assert kr.weights(f32(0), f32(1 - 5 / 32768)) == (2, 0, 16382, 0)   # (1 - b) 2^14 = 2.5 -> 2
    assert kr.weights(f32(0), f32(1 - 7 / 32768)) == (4, 0, 16380, 0)   # 3.5 -> 4
    assert kr.cv_round(2.5) == 2 and kr.cv_round(3.5) == 4 and kr.cv_round(-0.5) == 0
