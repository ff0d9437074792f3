"""GPU: one cs_cuboid_batch taken through a fixed sequence of set_lines / set_scene calls that grows its size classes one group at a time; after every call its cuboids
equal, byte for byte, those of a fresh batch created on that scene.

Two synth.cuboid_scene frames (seeds 700 and 701, three boxes and 76 edge rows each, 640 x 480).  `first` is each frame's box 0, `big` the bounding box of its boxes 0 and 1
(345 / 349 px wide: more top samples, a wider distance transform), `all` its three boxes, `other` its box 1; `half` is the first 38 edge rows of a frame, `full` all 76.

Plan sizes per class by the arithmetic of plan_build / plan_derived (yaw_cap 18, no roll / pitch or height samples; ROIs w x h with n top samples), and the capacities
batch_reserve leaves: create takes the exact sizes, a class that has to grow takes need + need / 4 (+ 64 for lines_in and line_rows).

  call                       ROIs (w x h, tops)                                pix     hyp   vp units boxes lines_in line_rows wgmap   dttmp   exceeds its capacity
  create(first, half)        216x227,10  253x258,11                         114368     832   36     2     2       76        76   158  124160   (all: exact)
  1 set_lines(full)          unchanged                                      114368     832   36     2     2      152       152   158  124160   lines_in, line_rows
      capacities                                                            114368     832   36     2     2      254       254   158  124160
  2 set_scene(big, full)     385x238,17  389x268,17                         195904    1280   36     2     2      152       152   275  259072   pix, hyp, wgmap, dttmp
      capacities                                                            244880    1600   36     2     2      254       254   343  323840
  3 set_scene(all, full)     216x227 188x237 234x266 253x258 204x227 232x238 322816   2368  108     6     6      152       456   448  371968   boxes, units, vp, line_rows
      capacities                                                            403520    2960  135     7     7      254       634   560  464960     (and pix, hyp, wgmap, dttmp again)
  4 set_scene(first, half)   216x227,10  253x258,11                         114368     832   36     2     2       76        76   158  124160   nothing: the slices lie where
      capacities                                                            unchanged                                                              other units' pixels were
  5 set_scene(other, NULL)   188x237,10  204x227,10                          90944     768   36     2     2   (stay)        76   130  118784   nothing; the edge lists stay
"""
import numpy as np
import pytest

from cube_slam_amd import synth
from cube_slam_amd.cuboid import CuboidBatch, detect_3d_cuboid

gpu = pytest.mark.gpu


def bounding(a, b):
    x0, y0 = min(a[0], b[0]), min(a[1], b[1])
    x1, y1 = max(a[0] + a[2], b[0] + b[2]), max(a[1] + a[3], b[1] + b[3])
    return np.array([[x0, y0, x1 - x0, y1 - y0, 0.9]])


@gpu
def test_every_class_grows_and_the_cuboids_equal_a_fresh_batch(ctx):
    S = [synth.cuboid_scene(700 + i, n_boxes=3) for i in range(2)]
    assert [len(s["boxes"]) for s in S] == [3, 3] and [len(s["lines"]) for s in S] == [76, 76]  # what the table above is worked out for
    K, T, gray = S[0]["K"], np.stack([s["Twc"] for s in S]), np.ascontiguousarray(np.stack([s["gray"] for s in S]))
    opts = detect_3d_cuboid(ctx).opts()
    first, other, every = [s["boxes"][:1] for s in S], [s["boxes"][1:2] for s in S], [s["boxes"] for s in S]
    big = [bounding(s["boxes"][0], s["boxes"][1]) for s in S]
    full, half = [s["lines"] for s in S], [s["lines"][:38] for s in S]

    def cuboids(b):
        b.run()
        return b.read()

    def fresh(boxes, lines):
        b = CuboidBatch(ctx, gray, K, T, boxes, lines, opts)
        try:
            return cuboids(b)
        finally:
            b.close()

    batch = CuboidBatch(ctx, gray, K, T, first, half, opts)
    try:
        steps = [("create", None, first, half),
                 ("1 more lines only", lambda: batch.set_lines(full), first, full),
                 ("2 a larger box at the same count", lambda: batch.set_scene(T, big, full), big, full),
                 ("3 more boxes", lambda: batch.set_scene(T, every, full), every, full),
                 ("4 back to the first scene", lambda: batch.set_scene(T, first, half), first, half),
                 ("5 line_offsets NULL", lambda: batch.set_scene(T, other, None), other, half)]
        found = 0
        for name, call, boxes, lines in steps:
            if call:
                call()
            got, want = cuboids(batch), fresh(boxes, lines)
            assert len(got) == len(want) == sum(len(b) for b in boxes), name
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), name
            found += sum(len(c) for c in want)
        assert found >= 1  # (the comparison is not one of empty lists)
    finally:
        batch.close()
