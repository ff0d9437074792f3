#!/usr/bin/env python3
"""Share of the rect_improve candidates that lsd_rg_improve defers to lsd_rg_improve_deferred (nfa() not in the table) on the bench batch: the counters of
cs_lsd_nfa_probe after one line pass.  CUBESLAM_LSD_NFA_NMAX lowers the table's bound for the run.  python tools/nfa_share.py [frames]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from cube_slam_amd import _lib  # noqa: E402
from cube_slam_amd.lsd import line_lbd_detect  # noqa: E402

F = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
ctx = _lib.Context(0)
gray = np.stack([s["gray"] for s in bench.make_frames(F, 3, seed0=1000)])
det = line_lbd_detect(640, 480, max_frames=F, ctx=ctx)
det.upload(gray)
det.run(with_lbd=True)
st = det.region_stats()
_, _, finished, deferred = det.nfa_probe(np.zeros((0, 3), np.int32))
print(json.dumps({"frames": F, "CUBESLAM_LSD_NFA_NMAX": os.environ.get("CUBESLAM_LSD_NFA_NMAX"), "candidates": st["candidates"], "finished_by_table": finished, "deferred": deferred,
                  "share_deferred": deferred / max(1, st["candidates"])}))
