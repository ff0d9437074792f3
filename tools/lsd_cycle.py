#!/usr/bin/env python3
"""From a rocprofv3 kernel-trace database of the headline command: per queue the median interval between consecutive lsd_rg_seq starts,
and the in-run durations of the line pass's other kernels.  usage: tools/lsd_cycle.py results.db"""
import collections
import sqlite3
import statistics
import sys

c = sqlite3.connect(sys.argv[1])
cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
name = "name" if "name" in cols else [x for x in cols if "name" in x][0]
q = "queue_id" if "queue_id" in cols else ("stream_id" if "stream_id" in cols else None)
rows = c.execute("select %s, %s, start, end from kernels order by start" % (q, name)).fetchall()
clean = lambda n: n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]
seq = collections.defaultdict(list)
dur = collections.defaultdict(list)
for qq, n, s, e in rows:
    k = clean(n)
    if k == "lsd_rg_seq":
        seq[qq].append(s)
    dur[k].append((e - s) / 1e6)
allint = []
for qq, st in sorted(seq.items()):
    iv = [(b - a) / 1e6 for a, b in zip(st, st[1:])]
    allint += iv
    if iv:
        print("queue %s: %d lsd_rg_seq, interval median %.1f ms (min %.1f, max %.1f)" % (qq, len(st), statistics.median(iv), min(iv), max(iv)))
if allint:
    print("all queues: interval median %.1f ms over %d intervals" % (statistics.median(allint), len(allint)))
for k in sorted(dur, key=lambda k: -sum(dur[k])):
    if k.startswith("lsd_") or k.startswith("lbd_") or "copyBuffer" in k or k.startswith("cuboid_sweep_score"):
        d = dur[k]
        print("%-28s calls %6d  avg %8.3f ms  median %8.3f ms  total %9.1f ms" % (k, len(d), sum(d) / len(d), statistics.median(d), sum(d)))
