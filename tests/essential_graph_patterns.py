"""Seeded maps for the pose-graph tests (tests/test_essential_graph_*.py): pointer-style maps as tests/essential_graph_restatement.py takes them, the smallest shapes that
reach each place cs_essential_graph_* can go wrong, and a Python statement of the library's symbolic analysis (minimum degree with ties to the lower index, elimination tree,
level sets) so that the preconditions on the tree can be asserted without a device.  A helper, not a test module.

A map is a camera going round a circle: true poses, a drifted copy of them (per step a small rotation, a translation error and a scale factor that accumulates), a spanning
tree, covisibility within `reach` steps, and a loop closed between the last key frame (pCurKF) and kfs[loop_idx] (pLoopKF) the way LoopClosing::CorrectLoop prepares it:
CorrectedSim3 / NonCorrectedSim3 for pCurKF and the key frames before it, LoopConnections from those to the neighbourhood of pLoopKF."""
import math

import numpy as np

from tests import essential_graph_restatement as R
from tests import sim3_opt_restatement as S3


def _rot(axis, deg):
    return S3._rot(axis, deg)


def _qmat(q):
    return np.array([[float(x) for x in row] for row in R.quat_to_matrix(tuple(float(v) for v in q))])


def make_map(seed, n, loop_idx=0, reach=2, n_corrected=3, rot_deg=0.4, trans=0.01, scale_step=0.03, n_points=0, extras=False, loop_twist_deg=0.0, loop_scale=None, turns=0.9, id_step=3, spurs=0, near_reach=2):
    rng = np.random.RandomState(seed)
    n_all, n = n, n - spurs  # the last `spurs` key frames hang off the ring by a tree edge alone: leaves of the elimination tree
    # true camera poses Tcw_k on a circle of radius 5, and the drifted chain
    true = []
    for k in range(n):
        a = 2 * math.pi * turns * k / max(n - 1, 1)
        Rwc = _qmat(_rot((0, 0, 1), math.degrees(a))) @ _qmat(_rot(rng.normal(size=3), rng.uniform(0, 3)))
        p = np.array([5 * math.cos(a), 5 * math.sin(a), 0.2 * rng.normal()])
        true.append((Rwc.T, -Rwc.T @ p))
    drift = [true[0]]
    s_acc = [1.0]
    for k in range(1, n):
        Rrel = true[k][0] @ true[k - 1][0].T
        trel = true[k][1] - Rrel @ true[k - 1][1]
        s_acc.append(s_acc[-1] * (1.0 + scale_step))
        Rrel = _qmat(_rot(rng.normal(size=3), rot_deg * rng.uniform(0.5, 1.5))) @ Rrel
        trel = s_acc[-1] * trel + trans * rng.normal(size=3)
        drift.append((Rrel @ drift[-1][0], Rrel @ drift[-1][1] + trel))
    kfs = [R.KF(id_step * k + 1, drift[k][0], drift[k][1]) for k in range(n)]
    for k in range(1, n):  # spanning tree: the key frame before, now and then the one before that
        par = kfs[k - 2] if (k >= 2 and k != n - 1 and rng.rand() < 0.2) else kfs[k - 1]
        kfs[k].parent = par
        par.children.add(kfs[k])
    for k in range(n):  # covisibility, symmetric weights, GetCovisiblesByWeight(100) by falling weight
        for j in range(k + 1, min(n, k + reach + 1)):
            w = int(260 - (170.0 / max(reach, 1)) * (j - k) + rng.randint(-25, 26))
            kfs[k].weights[kfs[j]] = w
            kfs[j].weights[kfs[k]] = w
    for kf in kfs:
        kf.covisibles = [o for o, w in sorted(kf.weights.items(), key=lambda ow: (-ow[1], ow[0].mnId)) if w >= R.MIN_FEAT]
    loop_kf, cur_kf = kfs[loop_idx], kfs[n - 1]
    # CorrectLoop: g2oScw of pCurKF from the loop's Sim3, carried to the key frames before it
    Slw = loop_kf.pose_sim3()
    Rcl = true[n - 1][0] @ true[loop_idx][0].T
    tcl = true[n - 1][1] - Rcl @ true[loop_idx][1]
    if loop_twist_deg:
        Rcl = _qmat(_rot(rng.normal(size=3), loop_twist_deg)) @ Rcl
    s_cl = (s_acc[loop_idx] / s_acc[n - 1]) if loop_scale is None else loop_scale
    Scl = (S3.quat_from_matrix([[float(x) for x in row] for row in Rcl]), tuple(float(x) for x in s_acc[loop_idx] * tcl), float(s_cl))
    g2oScw = S3.sim3_mul(Scl, Slw)
    corrected, non_corrected = {}, {}
    Swc_old = S3.sim3_inverse(cur_kf.pose_sim3())
    for k in range(n - n_corrected, n):
        if k == loop_idx or k < 0:
            continue
        old = kfs[k].pose_sim3()
        corrected[kfs[k]] = g2oScw if kfs[k] is cur_kf else S3.sim3_mul(S3.sim3_mul(old, Swc_old), g2oScw)
        non_corrected[kfs[k]] = old
    connections = {}
    if n > 2 or extras:
        for kf in corrected:
            near = [kfs[j] for j in range(max(0, loop_idx - near_reach), min(n, loop_idx + near_reach + 1)) if kfs[j] not in corrected and kfs[j] is not kf]
            for o in near:
                w = 60 if (kf is cur_kf and o is loop_kf) else int(rng.choice([40, 80, 120, 160, 200]))
                kf.weights[o] = w  # GetWeight of a loop connection; not a GetCovisiblesByWeight member of the old graph
                connections.setdefault(kf, set()).add(o)
        connections.setdefault(cur_kf, set()).add(loop_kf)
        cur_kf.weights[loop_kf] = 60
    if extras:
        connections[cur_kf].add(kfs[n - 2])  # its parent: the pair carries a tree edge and a loop connection
        connections[cur_kf].add(kfs[n - 3])  # a strong covisible that is no parent, child or loop edge: suppressed by sInsertedEdges
        assert cur_kf.parent is kfs[n - 2] and cur_kf.weights[kfs[n - 2]] >= 100 and cur_kf.weights[kfs[n - 3]] >= 100 and kfs[n - 3] in cur_kf.covisibles
        for a, b in ((n // 2, 2), (n // 2 + 5, 4), (n - 6, 1)):  # loop edges stored by earlier loops
            if 0 <= b < a < n and kfs[a] is not kfs[b]:
                kfs[a].loop_edges.add(kfs[b])
                kfs[b].loop_edges.add(kfs[a])
        ghost = R.KF(id_step * n + 50, np.eye(3), np.zeros(3))  # a bad key frame that two covisibility lists still name
        ghost.bad = True
        kfs[n // 3].covisibles.insert(1, ghost)
        kfs[n // 3 + 1].covisibles.append(ghost)
    for k in range(n, n_all):
        h = int(rng.randint(0, n - n_corrected))
        kf = R.KF(id_step * k + 1, drift[h][0], drift[h][1] + 0.3 * rng.normal(size=3))
        kf.parent = kfs[h]
        kfs[h].children.add(kf)
        kf.weights[kfs[h]] = kfs[h].weights[kf] = 150
        kf.covisibles = [kfs[h]]
        kfs[h].covisibles.append(kf)
        kfs.append(kf)
    points = []
    cor_list = sorted(corrected, key=lambda kf: kf.mnId)
    for p in range(n_points):
        ref = kfs[rng.randint(0, n_all)]
        Rm, t = ref.Rcw.astype(np.float64), ref.tcw.astype(np.float64)
        pc = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(2, 12)])
        pw = Rm.T @ (pc - t)
        if p % 7 == 3 and cor_list:
            points.append(R.MP(pw, ref, corrected_by=cur_kf.mnId, corrected_reference=cor_list[p % len(cor_list)].mnId))
        else:
            points.append(R.MP(pw, ref, corrected_by=(kfs[0].mnId if p % 5 == 0 else -1), corrected_reference=kfs[0].mnId))
    return R.Map(kfs, points, loop_kf, cur_kf, corrected, non_corrected, connections)


# name -> (make_map arguments, fix_scale)
CASES = {
    "two": (dict(seed=1, n=2, loop_idx=0, reach=1, n_corrected=1), True),
    "chain5": (dict(seed=2, n=5, loop_idx=2, reach=1, n_corrected=2, turns=0.3), False),
    "ring12": (dict(seed=30, n=12, loop_idx=0, reach=2, n_corrected=1, near_reach=0, rot_deg=1.0, trans=0.02, scale_step=0.03), False),
    "ring12_fix": (dict(seed=30, n=12, loop_idx=0, reach=2, n_corrected=1, near_reach=0, rot_deg=1.0, trans=0.02, scale_step=0.03), True),
    "kf40": (dict(seed=4, n=40, loop_idx=1, reach=3, n_corrected=13, n_points=1000, extras=True), False),
    "kf300": (dict(seed=5, n=300, spurs=90, loop_idx=3, reach=7, n_corrected=20, scale_step=0.002, rot_deg=0.1, trans=0.005, extras=True), False),
    "twist": (dict(seed=6, n=24, loop_idx=0, reach=2, n_corrected=4, loop_twist_deg=172.0), False),
    "efolds": (dict(seed=7, n=24, loop_idx=0, reach=2, n_corrected=4, loop_scale=math.exp(3.0)), False),
}
_made, _judged = {}, {}


def case(name):
    if name not in _made:
        _made[name] = make_map(**CASES[name][0])
    return _made[name]


def judged(name):
    """The restatement's result for a case, computed once and left unchanged."""
    if name not in _judged:
        _judged[name] = R.run_map(case(name), CASES[name][1])
    return _judged[name]


def graph_2000():
    """The 2 000-vertex / ~12 000-edge map of the bench tool."""
    return make_map(seed=8, n=2000, spurs=300, loop_idx=5, reach=8, n_corrected=30, scale_step=0.0003, rot_deg=0.03, trans=0.002, extras=True, turns=3.7), False


# ---------------------------------------------------------------------------------------------------------------------------------- graph-level cases
# Cases given as a graph (what cube_slam_amd.optimizer.build_essential_graph returns) rather than as a map: R.optimize and O.EssentialGraph take them as they are.
def _fan(n_free, seed):
    """A hub-anchored ring: n_free free vertices on a ring, each with an edge to the fixed hub (the last vertex), so the system is well conditioned; 2 * n_free edges in both
    orientations.  Every edge is a "normal" one measured from NonCorrectedSim3 = the true poses, and the estimates start a small Sim3 step away from them."""
    rng = np.random.RandomState(seed)
    n = n_free + 1
    true = np.zeros((n, 8))
    for v in range(n_free):
        a = 2 * math.pi * v / n_free
        q = S3.quat_mul(_rot((0, 0, 1), math.degrees(a)), _rot(rng.normal(size=3), rng.uniform(0, 5)))
        true[v] = [5 * math.cos(a), 5 * math.sin(a), 0.2 * rng.normal(), q[0], q[1], q[2], q[3], 1.0 + 0.1 * rng.uniform(-1, 1)]
    true[n_free] = [0, 0, 0, 0, 0, 0, 1, 1]
    U = 0.02 * rng.normal(size=(n, 7))
    U[n_free] = 0.0
    Scw = R._to8(S3.sim3_mul(R.sim3_exp_rows(U), R._arr(true)), n)
    ei = [v if v % 2 else (v + 1) % n_free for v in range(n_free)] + [v if v % 3 else n_free for v in range(n_free)]
    ej = [(v + 1) % n_free if v % 2 else v for v in range(n_free)] + [n_free if v % 3 else v for v in range(n_free)]
    return {"edge_i": np.array(ei, np.int32), "edge_j": np.array(ej, np.int32), "edge_kind": np.ones(2 * n_free, np.uint8), "fixed_vertex": n_free, "Scw": Scw, "Snc": true,
            "has_nc": np.ones(n, np.uint8)}


def _nan_vertex():
    """chain5 with one NaN in a free vertex's translation: every error and Jacobian of its edges is NaN, the solve fails on every trial and nothing is ever accepted."""
    _, ei, ej, kind, fixed, Scw, Snc = R.build_edges(case("chain5"))
    n = len(Scw)
    Scw8 = np.stack([S3.sim3_to8(S) for S in Scw])
    Snc8, has = np.zeros((n, 8)), np.zeros(n, np.uint8)
    for v, S in Snc.items():
        Snc8[v], has[v] = S3.sim3_to8(S), 1
    v = [u for u in range(n) if u != fixed][1]
    Scw8[v, 1] = np.nan
    return {"edge_i": np.asarray(ei, np.int32), "edge_j": np.asarray(ej, np.int32), "edge_kind": np.asarray(kind, np.uint8), "fixed_vertex": int(fixed), "Scw": Scw8, "Snc": Snc8,
            "has_nc": has}


# name -> (builder, iterations).  fan256: n = 257 and exactly m = 512 edges, full last blocks of the per-edge kernels (256 threads), where the `>= m` guard excludes nobody;
# fan255 is its twin one below (n = 256: a full last block of the per-vertex kernel).  The seeds are chosen so that no trial of the restatement is near a tie
# (tests/test_essential_graph_gpu.py asserts stats["margins"] > 1e-6 on the CPU).
GRAPH_CASES = {
    "fan256": (lambda: _fan(256, 41), 2),
    "fan255": (lambda: _fan(255, 42), 2),
    "nan_vertex": (_nan_vertex, 20),
}
_graphs, _graph_judged = {}, {}


def graph_case(name):
    if name not in _graphs:
        _graphs[name] = GRAPH_CASES[name][0]()
    return _graphs[name]


def graph_judged(name):
    """R.optimize on a graph-level case -> (sim3, Tiw, stats), computed once and left unchanged."""
    if name not in _graph_judged:
        g = graph_case(name)
        _graph_judged[name] = R.optimize(g["edge_i"], g["edge_j"], g["edge_kind"], g["fixed_vertex"], False, g["Scw"], g["Snc"], g["has_nc"], GRAPH_CASES[name][1])
    return _graph_judged[name]


# ---------------------------------------------------------------------------------------------------------------------------------- the symbolic analysis, restated
def symbolic(n, ei, ej, fixed):
    """-> {levels, widths (columns per level), l_blocks, h_blocks, fill (blocks of L absent from H)} of the free vertices' graph: minimum degree, ties to the lower index;
    and, as cs_essential_graph_create decides them, launches (the launch list, ("par", columns) / ("seq", columns) in order), longest_column (most sub-diagonal blocks in a
    column of L), longest_row (most blocks in a row structure), roots (columns without a parent); and the order itself for tests/essential_graph_solve_patterns.py: free (the
    free vertices ascending), pos (by rank in `free`: the position in the elimination order), columns (by position: the rows of the column's sub-diagonal blocks, ascending)."""
    fv = {}
    for v in range(n):
        if v != fixed:
            fv[v] = len(fv)
    nf = len(fv)
    adj = [set() for _ in range(nf)]
    for a, b in zip(ei, ej):
        if int(a) != fixed and int(b) != fixed:
            adj[fv[int(a)]].add(fv[int(b)])
            adj[fv[int(b)]].add(fv[int(a)])
    h_blocks = nf + sum(len(s) for s in adj) // 2
    pos, nb_at, gone = [-1] * nf, [], [False] * nf
    for k in range(nf):
        best = -1
        for a in range(nf):
            if not gone[a] and (best < 0 or len(adj[a]) < len(adj[best])):
                best = a
        gone[best], pos[best] = True, k
        nb = sorted(adj[best])
        nb_at.append(nb)
        for a in nb:
            adj[a].discard(best)
        for s in range(len(nb)):
            for t in range(s + 1, len(nb)):
                adj[nb[s]].add(nb[t])
                adj[nb[t]].add(nb[s])
    level, parent, row_len, col_len = [0] * nf, [-1] * nf, [0] * nf, [0] * nf
    l_blocks = 0
    for k in range(nf):
        rows = sorted(pos[a] for a in nb_at[k])
        l_blocks += 1 + len(rows)
        col_len[k] = len(rows)
        for r in rows:
            row_len[r] += 1
        if rows:
            parent[k] = rows[0]
            level[rows[0]] = max(level[rows[0]], level[k] + 1)
    levels = max(level) + 1
    widths = [level.count(l) for l in range(levels)]
    # the launch list as cs_essential_graph_create decides it: one parallel launch per level, except that a level of one column is a sequential launch, and joins the
    # sequential launch before it when its column is the parent of that launch's last
    launches, last = [], -1
    for l in range(levels):
        cols = [k for k in range(nf) if level[k] == l]
        if len(cols) == 1 and launches and launches[-1][0] == "seq" and parent[last] == cols[0]:
            launches[-1] = ("seq", launches[-1][1] + 1)
        else:
            launches.append(("seq" if len(cols) == 1 else "par", len(cols)))
        last = cols[-1]
    return {"levels": levels, "widths": widths, "l_blocks": l_blocks, "h_blocks": h_blocks, "fill": l_blocks - h_blocks,
            "launches": launches, "longest_column": max(col_len), "longest_row": max(row_len), "roots": parent.count(-1),
            "pos": pos, "free": sorted(fv), "columns": [sorted(pos[a] for a in nb) for nb in nb_at]}
