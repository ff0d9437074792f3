"""Element counts and flag patterns that cross the seams of the workgroup-wide ordered compaction and scan of csrc/common.h (block_rank, block_excl_scan): a partial
last wave, exactly one wave, one element more than a wave, a second pass of 256 threads, nothing flagged and everything flagged.  The order of every compaction is
the order of the reference's push_back loop; the GPU tests of the kernels that call the helpers drive them over these cases against their own restatements."""
import numpy as np

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 513]
PATTERNS = ["none", "all", "alternating", "last_lane_of_a_wave", "first_lane_of_the_second_wave"]


def flags(pattern, n, wave=64):
    """-> bool [n]: which of n elements in index order are flagged"""
    i = np.arange(n)
    return {"none": i < 0, "all": i >= 0, "alternating": i % 2 == 0, "last_lane_of_a_wave": i == wave - 1, "first_lane_of_the_second_wave": i == wave}[pattern]


def cases(sizes=SIZES):
    """-> [(n, pattern, flags)] over sizes x PATTERNS"""
    return [(n, p, flags(p, n)) for n in sizes for p in PATTERNS]
