"""Seeded patterns of the project's own data for the place-recognition tests: vocabularies, frames and key-frame database scenarios, the smallest shapes at which each
piece can go wrong.  tests/test_bow_patterns.py asserts on the CPU, through the restatement, that every pattern contains what it is named for."""
import functools

import numpy as np

from tests import bow_restatement as R

SEED = 20240611


def _flip(rng, d, nbits):
    d = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _tree(rng, k, L, n_children, leaf_at, flips=40, ties=False, stop=0.2):
    """Nodes in the order a depth-first writer leaves them (parent < id).  n_children(depth, rng) children for a node that is not a leaf; leaf_at(depth, rng) says whether a
    node at depth < L stops there.  A child's descriptor is its parent's with `flips` bits flipped; with `ties`, siblings repeat or lie at equal distances of one another."""
    parent, leaf, desc, weight = [0], [0], [np.zeros(32, np.uint8)], [0.0]

    def grow(node, depth):
        nc = n_children(depth, rng)
        base = desc[node] if node else rng.integers(0, 256, 32).astype(np.uint8)
        kids = []
        for c in range(nc):
            if ties and c % 3 == 1:
                d = kids[-1].copy()                      # equal to the sibling before it
            elif ties and c % 3 == 2:
                d = _flip(rng, kids[-1], 2)              # two bits off a sibling: equidistant pairs for the midpoint features
            else:
                d = _flip(rng, base, flips)
            kids.append(d)
        for d in kids:
            i = len(parent)
            is_leaf = depth + 1 == L or leaf_at(depth + 1, rng)
            parent.append(node); leaf.append(1 if is_leaf else 0); desc.append(d)
            weight.append(0.0 if (is_leaf and rng.random() < stop) else float(rng.random() * 9.0 + 0.25) if is_leaf else 0.0)
            if not is_leaf:
                grow(i, depth + 1)

    grow(0, 0)
    return R.Vocabulary(k, L, parent, leaf, np.stack(desc), weight)


@functools.lru_cache(maxsize=None)
def vocabularies():
    """{name: (Vocabulary, levelsup)}"""
    rng = np.random.default_rng(SEED)
    full = lambda k: (lambda depth, r: k)
    never = lambda depth, r: False
    out = {}
    out["k10_L3_full"] = (_tree(rng, 10, 3, full(10), never), 4)            # 1 111 nodes, the node level is the root (L - levelsup < 0)
    out["k10_L3_up1"] = (_tree(rng, 10, 3, full(10), never), 1)             # ... and with the node level 2
    out["k20_L2"] = (_tree(rng, 20, 2, full(20), never), 1)                 # the 32-lane group
    out["k3_L5_up4"] = (_tree(rng, 3, 5, full(3), never), 4)                # the node level is 1
    out["k5_L2_root"] = (_tree(rng, 5, 2, full(5), never), 4)               # every node is the root
    out["unbalanced"] = (_tree(rng, 10, 5, lambda depth, r: int(r.integers(2, 8)) if depth else 10, lambda depth, r: depth >= 2 and r.random() < 0.4), 3)  # leaves at depth 2..5
    out["ties"] = (_tree(rng, 6, 3, full(6), never, ties=True), 1)
    return out


def malformed():
    """{name: (k, L, parent, is_leaf, levelsup, scoring, weighting)}: the inputs cs_bow_vocab_create refuses."""
    v, _ = vocabularies()["k5_L2_root"]
    p, l = v.parent.copy(), v.is_leaf.copy()
    out = {}
    a = l.copy(); a[1] = 1                                   # an inner node flagged as a leaf
    out["leaf flag on an inner node"] = (5, 2, p, a, 4, 0, 0)
    a = l.copy(); a[len(a) - 1] = 0                          # a childless node not flagged
    out["childless node without the flag"] = (5, 2, p, a, 4, 0, 0)
    u, _ = vocabularies()["unbalanced"]
    out["leaf above level L - levelsup"] = (10, 5, u.parent, u.is_leaf, 1, 0, 0)  # leaves at depth 2 and 3, node level 4
    out["k = 1"] = (1, 2, p, l, 4, 0, 0)
    out["k = 21"] = (21, 2, p, l, 4, 0, 0)
    out["L = 0"] = (5, 0, p, l, 4, 0, 0)
    out["L = 11"] = (5, 11, p, l, 4, 0, 0)
    a = p.copy(); a[3] = 3
    out["parent equal to the node"] = (5, 2, a, l, 4, 0, 0)
    a = p.copy(); a[2] = 7
    out["parent behind the node"] = (5, 2, a, l, 4, 0, 0)
    out["TF weighting"] = (5, 2, p, l, 4, 0, 1)
    out["L2 scoring"] = (5, 2, p, l, 4, 1, 0)
    return out


def _near_leaves(rng, v, n, noise=12):
    leaves = np.flatnonzero(v.is_leaf > 0)
    return np.stack([_flip(rng, v.desc[rng.choice(leaves)], int(rng.integers(0, noise + 1))) for _ in range(n)]) if n else np.zeros((0, 32), np.uint8)


def _filtered(rng, v, levelsup, n, want_stopped):
    out = []
    while len(out) < n:
        for d in _near_leaves(rng, v, 4 * n, noise=4):
            if (R.transform_feature(v, d, levelsup)[1] > 0) != want_stopped and len(out) < n:
                out.append(d)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def frames(voc_name):
    """{name: (n, 32) uint8} for one vocabulary."""
    v, levelsup = vocabularies()[voc_name]
    rng = np.random.default_rng([SEED, sorted(vocabularies()).index(voc_name)])
    out = {}
    for n in (0, 1, 63, 64, 65, 2000):
        near = _near_leaves(rng, v, n - n // 4)
        out["n%d" % n] = np.concatenate([near, rng.integers(0, 256, (n // 4, 32)).astype(np.uint8)])
    out["one_word"] = np.repeat(_filtered(rng, v, levelsup, 1, want_stopped=False), 70, axis=0)
    out["all_stopped"] = _filtered(rng, v, levelsup, 66, want_stopped=True)
    inner = rng.choice(len(v.parent) - 1, 40) + 1
    mids = []
    for _ in range(40):  # bitwise midpoints of two siblings: half of the bits in which they differ taken from each
        kids = v.children[int(rng.choice([i for i in range(len(v.parent)) if len(v.children[i]) >= 2]))]
        a, b = v.desc[kids[0]], v.desc[kids[1]] if not np.array_equal(v.desc[kids[0]], v.desc[kids[1]]) else v.desc[kids[-1]]
        diff = [i for i in range(256) if (a[i >> 3] ^ b[i >> 3]) >> (i & 7) & 1]
        d = a.copy()
        for i in diff[: len(diff) // 2]:
            d[i >> 3] ^= np.uint8(1 << (i & 7))
        mids.append(d)
    out["node_equal_and_midpoints"] = np.concatenate([v.desc[inner], np.stack(mids)])
    return out


BATCH_ORDER = ("n0", "n1", "n63", "one_word", "n0", "all_stopped", "node_equal_and_midpoints", "n64", "n65", "n2000", "n0")


def batch(voc_name):
    f = frames(voc_name)
    return [f[n] for n in BATCH_ORDER]


# ---------------------------------------------------------------------------------------------------------------- key-frame database scenarios
def _bow(rng, words):
    """A BowVector over `words` with the L1 norm 1, summed as BowVector::normalize does."""
    words = sorted(int(w) for w in words)
    raw = [float(rng.random() + 0.05) for _ in words]
    norm = 0.0
    for x in raw:
        norm += abs(x)
    return {w: x / norm for w, x in zip(words, raw)}


def _sharing(rng, q, c, private, extra=6):
    """A key frame that has the first c words of q (in q's order) and `extra` words of its own from `private` on."""
    return _bow(rng, list(q)[:c] + list(range(private, private + extra)))


@functools.lru_cache(maxsize=None)
def scenarios():
    """{name: [op, ...]} with op = ("add", id, bow) | ("erase", id) | ("clear",) | ("loop", query id, bow, connected ids, best_covisibles, minScore | ("at", kf id)) |
    ("reloc", query id, bow, best_covisibles).  minScore ("at", kf) = the float score of that key frame against the query, for the `>=` at equality."""
    rng = np.random.default_rng(SEED + 1)
    S = {}
    q = _bow(rng, range(100, 140))
    S["empty"] = [("loop", 3, q, [], {}, 0.01), ("reloc", 3, q, {})]
    S["one_key_frame"] = [("add", 1, _sharing(rng, q, 12, 1000)), ("loop", 9, q, [], {1: []}, 0.0), ("reloc", 9, q, {1: []})]
    # 65 key frames over a small word range: every mechanism at once, with connected key frames and random covisibility lists
    ops, ids = [], list(range(1, 66))
    for i in ids:
        ops.append(("add", i, _bow(rng, rng.choice(np.arange(90, 200), int(rng.integers(15, 45)), replace=False))))
    cov = {i: [int(x) for x in rng.choice(ids, 10, replace=False) if x != i] for i in ids}
    ops += [("loop", 70, q, [2, 3, 5, 8], cov, 0.02), ("reloc", 70, q, cov), ("loop", 71, _bow(rng, range(120, 170)), [], cov, 0.05), ("loop", 71, q, [1], cov, 0.0)]
    S["k65"] = ops
    # erased and added again: 11 and 12 first meet the query at the same word; after erase + add of 11 the order is 12, 11
    a, b = _sharing(rng, q, 20, 1000), _sharing(rng, q, 20, 1100)
    S["erase_and_add_again"] = [("add", 11, a), ("add", 12, b), ("loop", 20, q, [], {}, 0.0), ("erase", 11), ("loop", 21, q, [], {}, 0.0), ("add", 11, a), ("loop", 22, q, [], {}, 0.0),
                                ("clear",), ("loop", 23, q, [], {}, 0.0), ("add", 12, b), ("reloc", 24, q, {})]
    S["no_common_word"] = [("add", 1, _bow(rng, range(500, 530))), ("add", 2, _bow(rng, range(10, 30))), ("loop", 4, q, [], {1: [2]}, 0.0), ("reloc", 4, q, {1: [2]})]
    # query id 0: mnLoopQuery / mnRelocQuery start at 0, so nothing is reset and nothing is listed; the words counted meanwhile are reset by the next query
    S["query_id_0"] = [("add", 1, _sharing(rng, q, 30, 1000)), ("add", 2, _sharing(rng, q, 25, 1100)), ("loop", 0, q, [], {1: [2], 2: [1]}, 0.0), ("reloc", 0, q, {1: [2], 2: [1]}),
                       ("loop", 6, q, [], {1: [2], 2: [1]}, 0.0), ("reloc", 6, q, {1: [2], 2: [1]}), ("loop", 6, q, [], {1: [2], 2: [1]}, 0.0)]
    S["score_at_minScore"] = [("add", 1, _sharing(rng, q, 30, 1000)), ("add", 2, _sharing(rng, q, 28, 1100)), ("add", 3, _sharing(rng, q, 29, 1200)),
                              ("loop", 5, q, [], {}, ("at", 2)), ("loop", 6, q, [], {1: [2, 3]}, ("at", 3))]
    # maxCommonWords * 0.8f: multiples of 5, where the product is a whole number and `>` decides by one word (5 -> 4, 10 -> 8, 15 -> 12, 35 -> 28), and their neighbours
    ops = []
    for n, m in enumerate((5, 10, 15, 35, 34, 36)):
        ops.append(("clear",))
        for j, c in enumerate((m, int(m * 0.8), int(m * 0.8) + 1, max(int(m * 0.8) - 1, 1))):
            ops.append(("add", 100 * n + j, _sharing(rng, q, c, 1000 + 50 * j)))
        cov = {100 * n + j: [100 * n + jj for jj in range(4) if jj != j] for j in range(4)}
        ops += [("loop", 1000 + n, q, [], cov, 0.0), ("reloc", 1000 + n, q, cov)]
    S["min_common_words"] = ops
    # two relocalisation queries in a row: key frame 3 is scored by the first (it shares most of q1) and shares too few words with q2 to be scored again, but is a
    # neighbour of 1, which is: the second query adds the mRelocScore the first left
    q2 = _bow(rng, list(range(100, 118)) + list(range(300, 320)))
    S["reloc_twice"] = [("add", 1, _bow(rng, list(range(100, 116)) + list(range(300, 318)))), ("add", 2, _bow(rng, list(range(104, 140)))),
                        ("add", 3, _bow(rng, list(range(110, 140)) + [700, 701])), ("reloc", 50, q, {1: [3], 2: [3, 1], 3: [2]}), ("reloc", 51, q2, {1: [3], 2: [3, 1], 3: [2]})]
    # covisibility groups that return the same best key frame: 1 and 2 are both scored, both have 3 as their neighbour, and 3 scores highest
    c3 = dict(q)
    S["same_best_twice"] = [("add", 1, _sharing(rng, q, 36, 1000)), ("add", 2, _sharing(rng, q, 35, 1100)), ("add", 3, c3), ("add", 4, _sharing(rng, q, 34, 1200)),
                            ("loop", 8, q, [], {1: [3], 2: [3], 3: [], 4: []}, 0.0), ("reloc", 8, q, {1: [3], 2: [3], 3: [], 4: []})]
    return S


def replay(ops, db, make_kf=None):
    """Runs a scenario on a database (the restatement's, with make_kf = R.KF, or a mirror taking ids) -> the candidate list of every query op, in order."""
    out, kfs = [], {}
    for op in ops:
        if op[0] == "add":
            if make_kf:
                kfs.setdefault(op[1], make_kf(op[1], op[2]))
                db.add(kfs[op[1]])
            else:
                db.add(op[1], op[2])
        elif op[0] == "erase":
            db.erase(kfs[op[1]] if make_kf else op[1])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "loop":
            ms = op[5]
            if isinstance(ms, tuple):
                ms = float(np.float32(R.score(op[2], [o for o in ops if o[0] == "add" and o[1] == ms[1]][0][2])))
            out.append(list(db.DetectLoopCandidates(op[1], op[2], op[3], op[4], ms)))
        else:
            out.append(list(db.DetectRelocalizationCandidates(op[1], op[2], op[3])))
    return out
