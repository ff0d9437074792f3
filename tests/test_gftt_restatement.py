"""CPU: what can be checked about tests/gftt_restatement.py without resting on the recalled OpenCV text: corners of known squares, the distance and mask rules, the
order of quality, the grid against the walk without a grid, the disc against the table, and hand-computed derivatives and eigenvalues on a 5 x 5 image."""
import numpy as np

from tests import gftt_patterns as gp
from tests import gftt_restatement as gr

f32 = np.float32


def _squares():
    img = np.full((80, 100), 200, np.uint8)
    true = []
    for x0, y0 in [(10, 10), (50, 12), (20, 45), (65, 50)]:
        img[y0:y0 + 20, x0:x0 + 20] = 30
        true += [(x0, y0), (x0 + 19, y0), (x0, y0 + 19), (x0 + 19, y0 + 19)]
    return img, np.array(true)


def test_corners_of_dark_squares():
    img, true = _squares()
    r = gr.good_features(img, None, 200, 0.1, 10.0)
    assert len(r["corners"]) == 16
    for x, y in r["corners"]:
        assert np.abs(true - [x, y]).max(axis=1).min() <= 1  # within 1 px of a true corner
    d = np.linalg.norm(r["corners"][:, None] - r["corners"][None], axis=2) + 1e9 * np.eye(16)
    assert d.min() >= 10.0
    assert (np.diff(r["quality"]) <= 0).all()


def test_distance_mask_and_order_on_textures():
    for w, h in gp.SIZES[2:]:
        c = gp.size_case(w, h)
        p, q = c["want"]["corners"], c["want"]["quality"]
        d = np.linalg.norm(p[:, None] - p[None], axis=2) + 1e9 * np.eye(len(p))
        assert d.min() >= c["min_distance"] and (np.diff(q) <= 0).all()
        assert all(c["mask"][int(y), int(x)] for x, y in p)


def test_grid_walk_equals_walk_without_a_grid():
    for c in list(gp.designed_cases().values()) + [gp.size_case(w, h) for w, h in gp.SIZES[2:]]:
        h, w = c["img"].shape
        for md in (1.0, 2.5, 3.5, 10.0, 10.4):
            for mc in (5, 200):
                assert gr.select_grid(c["want"]["sorted"], w, h, mc, md) == gr.select_all_pairs(c["want"]["sorted"], w, mc, md), (w, h, md, mc)


def test_disc_walk_equals_table():
    assert gr.disc_half_widths() == gr.DISC_TABLE
    good, _ = gr.build_mask(np.ones((41, 41), np.uint8), [[20.0, 20.0]], [1])
    for off in range(-10, 11):
        row = np.flatnonzero(good[20 + off] == 0)
        assert row.min() == 20 - gr.DISC_TABLE[abs(off)] and row.max() == 20 + gr.DISC_TABLE[abs(off)] and len(row) == 2 * gr.DISC_TABLE[abs(off)] + 1
    assert good[9].all() and good[31].all() and (good == 0).sum() == sum(2 * k + 1 for k in gr.DISC_TABLE) * 2 - 21


def test_hand_computed_5x5():
    """A vertical step edge and one with a corner, by hand.  img columns 0-1 are 0, columns 2-4 are 255: at (2, 2) the row pass gives r = 255 on every row, so
    Dx = (255 + 255) s + 255 (2 s) with s = 1 / 3060: 1/6 + 1/6 = 1/3 up to float rounding, and Dy = 0; one eigenvalue of the box sum is 0."""
    img = np.zeros((5, 5), np.uint8)
    img[:, 2:] = 255
    dx, dy = gr.derivatives(img)
    s = f32(1.0 / 3060)
    want = f32(f32(f32(510) * s) + f32(f32(255) * f32(s * f32(2))))
    assert dx[2, 2] == want and abs(float(want) - 1 / 3) < 1e-6 and (dy == 0).all()
    assert dx[2, 0] == 0 and dx[2, 1] == want and dx[2, 3] == 0                               # column 0 reflects: p(1) - p(1) = 0
    assert (gr.min_eigen(img) == 0).all()                                                     # an edge has no second direction: a + c - sqrt((a - c)^2) = 0
    img[:2, :] = 0                                                                            # rows 0-1 dark: a corner at (2, 2)
    dx, dy = gr.derivatives(img)
    # at (2, 2): rows 1, 2, 3 have r = 0, 255, 255 -> Dx = (0 + 255) s + 255 (2 s); Dy = q(3) - q(1) with q(3) = 255 (2 s) + (0 + 255) s, q(1) = 0
    wx = f32(f32(f32(255) * s) + f32(f32(255) * f32(s * f32(2))))
    wy = f32(f32(f32(255) * f32(s * f32(2))) + f32(f32(255) * s))
    assert dx[2, 2] == wx and dy[2, 2] == wy and abs(float(wx) - 0.25) < 1e-6
    eig = gr.min_eigen(img)
    cov = np.stack([dx * dx, dx * dy, dy * dy]).astype(np.float64)
    box = [f32(((cov[c, 1, 1:4].sum() if False else (cov[c, 1, 1] + cov[c, 1, 2]) + cov[c, 1, 3]) + ((cov[c, 2, 1] + cov[c, 2, 2]) + cov[c, 2, 3])) + ((cov[c, 3, 1] + cov[c, 3, 2]) + cov[c, 3, 3]))
           for c in range(3)]
    a, b, c = box[0] * f32(0.5), box[1], box[2] * f32(0.5)
    assert eig[2, 2] == (a + c) - np.sqrt((a - c) * (a - c) + b * b) and eig[2, 2] > 0 and np.argmax(eig) in (2 * 5 + 2, 2 * 5 + 1, 1 * 5 + 2, 1 * 5 + 1)
