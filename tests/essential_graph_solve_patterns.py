"""Designed linear systems for the pose graph's sparse block Cholesky (eg_assemble / eg_factor / eg_back of cube_slam_amd/csrc/posegraph.hip through cs_essential_graph_solve,
include/cubeslam_hip/essential_graph_solve.h), and the dense float64 / long-double judge of a solution.  A helper, not a test module.

A case is a graph (n, fixed vertex, edge list), a seeded J (m, 2, 7, 7) in eg_linearize's layout and err (m, 7), and the lambdas it is solved at.  J holds integers of [-2, 2] and err
integers of [-3, 3] -- on the fixed vertex's side of an edge too, which nothing may read -- so every entry of H = sum J^T J and b = -sum J^T err is an integer far below 2^53 and
exact in float64 whatever the order of the sums.  A = H + lambda on the diagonal, one float64 addition per entry as eg_factor forms it; from there on A is the problem, exactly.
make() asserts that the dense Cholesky of A succeeds and that cond_2(A) <= COND_CAP at every lambda of the case.

What each graph reaches (the figures are asserted by tests/test_essential_graph_solve_patterns.py from the symbolic analysis of tests/essential_graph_patterns.py):
  clique40       40 free vertices all adjacent: one sequential launch of 40 columns, the first with 39 sub-diagonal blocks -- (nb - 1) * 7 = 273 > 256 rows to scale (a second
                 pass of eg_factor's row loop) and nb * 49 = 1960 items (8 passes of its gather loop); a row structure of 39
  two_cliques39  two cliques of 39 joined only through the fixed vertex (index 39, in the middle): 39 parallel levels of width 2, two roots, columns of 38 blocks
                 (266 > 256) inside a parallel level
  path30         a path with the fixed vertex at its end (the last index): one sequential launch of 30 one-block columns.  `anchor`: see below
  star300        a free hub (vertex 0) with 300 free leaves, the fixed vertex on the hub: a level 299 wide, then a sequential launch of 2; the hub's row structure and its
                 diagonal update list have 299 terms, its incidence list in eg_assemble 301 edges.  `anchor`
  grid6x6        a 6 x 6 grid, the fixed vertex on two opposite corners: fill, and a sequential chain that starts below parallel levels
  forest         the fixed vertex is an articulation point: a single vertex (a column of one block), a path of 2, a triangle and a path of 6 hang off it -- 4 roots at
                 different levels, and a sequential launch that begins where the shorter trees have ended
  multi          6 vertices with up to three edges over one pair, in both orientations: slot lists longer than one with both `side` values
  kf300_real     graph, J and err of the map "kf300" at its initial estimates (R.linearize, R.edge_errors), lambda 1e-16: real scaling, 101-wide levels, 1 069 fill blocks.
                 Not integers, and no condition cap: its cond_2(A) is what the map has, and the test's tolerance on x carries it
`anchor`: with integer J a free vertex that has a single edge leaves A singular or nearly so at lambda = 1e-16 (a leaf's 7 x 7 block is J^T J of one random integer matrix, and a
path multiplies thirty of them); path30 and star300 therefore give every free vertex one more edge, to the fixed vertex.  That edge adds J^T J to the vertex's diagonal block and
nothing to the free vertices' graph, so the structure in the table is unchanged.  Both lambdas are kept for every designed case."""
import numpy as np
import scipy.linalg

from tests import essential_graph_patterns as P
from tests import essential_graph_restatement as R

U = 2.0 ** -53
COND_CAP = 1e8
LAMBDAS = (1e-16, 1.0)


def _clique(vs):
    return [(vs[a], vs[b]) for a in range(len(vs)) for b in range(a + 1, len(vs))]


def _path(vs):
    return [(vs[a], vs[a + 1]) for a in range(len(vs) - 1)]


def _graph(name):
    """-> (n, fixed, edges, anchor)"""
    if name == "clique40":
        return 41, 40, _clique(list(range(40))) + [(40, 7)], False
    if name == "two_cliques39":
        return 79, 39, _clique(list(range(39))) + _clique(list(range(40, 79))) + [(3, 39), (39, 60)], False
    if name == "path30":
        return 31, 30, _path(list(range(31))), True
    if name == "star300":
        return 302, 301, [(0, l) if l % 2 else (l, 0) for l in range(1, 301)] + [(301, 0)], True
    if name == "grid6x6":
        e = [(r * 6 + c, r * 6 + c + 1) for r in range(6) for c in range(5)] + [(r * 6 + c, r * 6 + c + 6) for r in range(5) for c in range(6)]
        return 37, 36, e + [(36, 0), (35, 36)], False
    if name == "forest":
        # fixed 0; a single vertex {1}; a path of two {2, 3}; a triangle {4, 5, 6}; a path of six {7 .. 12}
        return 13, 0, [(0, 1), (2, 0), (2, 3), (0, 4), (4, 5), (5, 6), (6, 4), (7, 0)] + _path(list(range(7, 13))), False
    if name == "multi":
        return 6, 2, [(0, 1), (1, 0), (0, 1), (1, 2), (3, 4), (4, 3), (2, 3), (4, 5), (5, 0), (0, 5), (5, 2), (3, 1)], False
    raise KeyError(name)


DESIGNED = ("clique40", "two_cliques39", "path30", "star300", "grid6x6", "forest", "multi")
SEEDS = {"clique40": 11, "two_cliques39": 12, "path30": 13, "star300": 14, "grid6x6": 15, "forest": 16, "multi": 17}
NAMES = DESIGNED + ("kf300_real",)
_made = {}


def dense(n, fixed, ei, ej, J, err):
    """-> (H, b) of the free vertices in vertex order: constructQuadraticForm of every edge (R.build_system)."""
    H, b = R.build_system(np.asarray(J, np.float64).reshape(-1, 2, 7, 7), np.asarray(err, np.float64).reshape(-1, 7), ei, ej, fixed, n)
    idx = np.concatenate([np.arange(7 * v, 7 * v + 7) for v in range(n) if v != fixed])
    return H[np.ix_(idx, idx)], b[idx]


def with_lambda(H, lam):
    A = H.copy()
    i = np.arange(len(A))
    A[i, i] = A[i, i] + lam  # one float64 addition per entry
    return A


def make(name):
    """-> {name, n, fixed, ei, ej, J, err, lambdas, sym, H, b, designed}, computed once and left unchanged."""
    if name in _made:
        return _made[name]
    if name == "kf300_real":
        _, ei, ej, kind, fixed, Scw, Snc = R.build_edges(P.case("kf300"))
        n = len(Scw)
        Scw8 = np.stack([R.S3.sim3_to8(S) for S in Scw])
        Snc8, has = np.zeros((n, 8)), np.zeros(n, np.uint8)
        for v, S in Snc.items():
            Snc8[v], has[v] = R.S3.sim3_to8(S), 1
        ei, ej = np.asarray(ei, np.int32), np.asarray(ej, np.int32)
        Cm, X = R.measurements(ei, ej, np.asarray(kind), Scw8, Snc8, has), R._arr(Scw8)
        err = R.edge_errors(Cm, R._take(X, ei), R._take(X, ej))
        J = R.linearize(Cm, X, ei, ej, fixed, False)
        lambdas, designed = (1e-16,), False
    else:
        n, fixed, edges, anchor = _graph(name)
        if anchor:
            edges = edges + [((v, fixed) if v % 2 else (fixed, v)) for v in range(n) if v != fixed]
        rng = np.random.RandomState(SEEDS[name])
        ei, ej = np.array([e[0] for e in edges], np.int32), np.array([e[1] for e in edges], np.int32)
        J = rng.randint(-2, 3, size=(len(edges), 2, 7, 7)).astype(np.float64)
        err = rng.randint(-3, 4, size=(len(edges), 7)).astype(np.float64)
        lambdas, designed = LAMBDAS, True
    if designed:  # estimates for a run of the optimiser on the same handle: every vertex at the identity
        Scw8 = np.tile(np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float64), (n, 1))
        Snc8, has = Scw8.copy(), np.zeros(n, np.uint8)
    H, b = dense(n, fixed, ei, ej, J, err)
    c = {"name": name, "Scw": Scw8, "Snc": Snc8, "has_nc": has, "n": n, "fixed": int(fixed), "ei": ei, "ej": ej, "J": np.ascontiguousarray(J), "err": np.ascontiguousarray(err), "lambdas": lambdas,
         "sym": P.symbolic(n, ei, ej, fixed), "H": H, "b": b, "designed": designed, "systems": {}}
    for lam in lambdas:
        s = system(c, lam)
        if designed:
            assert s["cond"] <= COND_CAP, (name, lam, s["cond"])
    _made[name] = c
    return c


def graph_dict(c):
    """What cube_slam_amd.optimizer.EssentialGraph takes."""
    return {"Scw": c["Scw"], "edge_i": c["ei"], "edge_j": c["ej"], "edge_kind": np.zeros(len(c["ei"]), np.uint8), "fixed_vertex": c["fixed"]}


def tolerance_k(c):
    """k = 7 * (longest row structure + 2): the longest inner product the factor and the substitutions form in this case."""
    return 7 * (c["sym"]["longest_row"] + 2)


def higham_ceiling(c):
    N = 7 * (c["n"] - 1)
    return N * (3 * N + 1) * U


def refine(A, b):
    """The reference solution: a float64 Cholesky refined with long-double residuals until the correction stops shrinking."""
    cf = scipy.linalg.cho_factor(A, lower=True, check_finite=False)  # raises LinAlgError where A is not positive definite
    AL, bL = A.astype(np.longdouble), b.astype(np.longdouble)
    x = scipy.linalg.cho_solve(cf, b, check_finite=False).astype(np.longdouble)
    x0, last = x.astype(np.float64), np.inf
    for _ in range(40):
        d = scipy.linalg.cho_solve(cf, (bL - AL @ x).astype(np.float64), check_finite=False)
        size = float(np.max(np.abs(d)))
        if not size < last:
            break
        x, last = x + d, size
    return x, x0


def system(c, lam):
    """-> {A, b, norm (|A|_2), cond, x_ref (long double, refined), x_lapack (float64, unrefined), row_norms (|A_p,:|_2 per free vertex)} for one lambda, computed once."""
    if lam not in c["systems"]:
        A = with_lambda(c["H"], lam)
        sv = np.linalg.svd(A, compute_uv=False)
        x_ref, x0 = refine(A, c["b"])
        rows = np.array([np.linalg.norm(A[7 * p:7 * p + 7], 2) for p in range(len(A) // 7)])
        c["systems"][lam] = {"A": A, "b": c["b"], "norm": float(sv[0]), "cond": float(sv[0] / sv[-1]), "x_ref": x_ref, "x_lapack": x0, "row_norms": rows}
    return c["systems"][lam]


def backward_errors(s, x):
    """x (nf * 7,) of the free vertices in vertex order -> (eta, the largest per-block-row eta, its block row): r = b - A x in long double,
    eta = |r|_2 / (|A|_2 |x|_2 + |b|_2) and per block row |r_p|_2 / (|A_p,:|_2 |x|_2 + |b_p|_2)."""
    xL = np.asarray(x, np.float64).reshape(-1).astype(np.longdouble)
    r = s["b"].astype(np.longdouble) - s["A"].astype(np.longdouble) @ xL
    nx = float(np.sqrt(np.sum(xL * xL)))
    eta = float(np.sqrt(np.sum(r * r))) / (s["norm"] * nx + float(np.linalg.norm(s["b"])))
    rp = np.sqrt(np.sum((r * r).reshape(-1, 7), axis=1)).astype(np.float64)
    bp = np.linalg.norm(s["b"].reshape(-1, 7), axis=1)
    per = rp / (s["row_norms"] * nx + bp)
    return eta, float(np.max(per)), int(np.argmax(per))


def free_rows(c, x):
    """(n, 7) by vertex -> (nf * 7,) of the free vertices in vertex order."""
    return np.asarray(x, np.float64).reshape(c["n"], 7)[[v for v in range(c["n"]) if v != c["fixed"]]].reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------------- the mutant
def fill_blocks(c):
    """The blocks (row, column) of L, by position in the elimination order, that H does not have."""
    sym = c["sym"]
    pos_of_vertex = {v: sym["pos"][k] for k, v in enumerate(sym["free"])}
    have = set()
    for a, b in zip(c["ei"], c["ej"]):
        if int(a) != c["fixed"] and int(b) != c["fixed"]:
            pa, pb = pos_of_vertex[int(a)], pos_of_vertex[int(b)]
            have.add((max(pa, pb), min(pa, pb)))
    return [(r, k) for k, rows in enumerate(sym["columns"]) for r in rows if (r, k) not in have]


def block_cholesky_solve(c, lam, drop=None):
    """A dense-storage block-7 Cholesky of the case in the solver's elimination order, over the solver's structure, and the two substitutions -> x (nf * 7,) in vertex order.
    drop = (row, column): the last update L_ik L_jk^T into that block is left out -- what a lost entry of an update list does."""
    sym = c["sym"]
    nf = len(sym["free"])
    perm = np.empty(nf, int)  # position -> free-vertex rank
    for k, p in enumerate(sym["pos"]):
        perm[p] = k
    idx = np.concatenate([np.arange(7 * k, 7 * k + 7) for k in perm])
    A = with_lambda(c["H"], lam)[np.ix_(idx, idx)]
    b = c["b"][idx].copy()
    blk = lambda M, i, j: M[7 * i:7 * i + 7, 7 * j:7 * j + 7]
    last_k = None
    if drop is not None:
        last_k = max(k for k, rows in enumerate(sym["columns"]) if drop[0] in rows and drop[1] in rows)
    L = np.zeros_like(A)
    for k in range(nf):  # right-looking
        D = np.linalg.cholesky(blk(A, k, k))
        blk(L, k, k)[:] = D
        rows = sym["columns"][k]
        for i in rows:
            blk(L, i, k)[:] = scipy.linalg.solve_triangular(D, blk(A, i, k).T, lower=True).T
        for a, j in enumerate(rows):
            for i in rows[a:]:
                if drop == (i, j) and k == last_k:
                    continue
                blk(A, i, j)[:] -= blk(L, i, k) @ blk(L, j, k).T
    y = scipy.linalg.solve_triangular(L, b, lower=True)
    xp = scipy.linalg.solve_triangular(L.T, y, lower=False)
    x = np.empty_like(xp)
    x[idx] = xp
    return x
