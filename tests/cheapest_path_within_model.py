"""The Python model of cheapest_path_within (a helper of test_cheapest_path_within_cpu.py / test_cheapest_path_within_gpu.py).

The contract (include/pgq_hip.h, pgq_cheapest_path_within).  D_0 .. D_K = the labels cheapest_path_length_within defines for the
row's source and K = max_hops (cheapest_within_model.hop_rounds), INF = max / 2 of the weight type, every sum in the weight
type's own arithmetic.  The row is None when D_K[dst] == INF or an endpoint is NULL, [src] when src == dst.  Otherwise h = the
smallest k with D_k[dst] == D_K[dst] as bit patterns, x_h = dst and, for i = h .. 1, x_{i-1} = the smallest u with
D_{i-1}[u] < INF and a slot (u, x_i) with D_{i-1}[u] + w[s] == D_i[x_i], e_i = edge_ids[the first such slot of u's out-list into
x_i]; the list is [x_0, e_1, x_1, ..., e_h, x_h].

`bounded_paths` is that, on the labels of hop_rounds.  `brute_force` enumerates every walk of at most K edges of a tiny graph
instead: the smallest left-to-right fold, then the fewest edges, then — reading from the dst side — the smallest predecessor
and its first slot.  MUTANTS are the ways an implementation can go wrong that the fixtures must notice; the fixtures of the
GPU tests that are new here are built here too, so that the CPU tests can show that they do."""
import numpy as np

import cheapest_path_model as P
from cheapest_path_model import _fixture, fold, slot_sources  # noqa: F401  (fold: for the tests)
from cheapest_within_model import bits, hop_rounds, inf_of

# final: parents tested against D_K instead of D_{i-1} (the labels left in place read instead of the round log)
# late: h = the last round, K, instead of the first that shows the value
# max_parent: the largest tight parent instead of the smallest
# first_slot: the first slot of u into x, tight or not
# filter: cheapest_path's list, None where it has more than K hops
MUTANTS = ("final", "late", "max_parent", "first_slot", "filter")


def hop_history(V, off, adj, w, src, K):
    """[D_0, D_1, ...] for one source, up to D_K or to the last round that changed a label: D_k = hist[min(k, len - 1)]."""
    hist = []
    for D, moving in hop_rounds(V, off, adj, w, src, int(min(K, V))):
        if hist and not moving:
            break
        hist.append(D.copy())
    return hist


def walk_back(V, off, adj, eid, w, hist, K, src, dst, mutant=None):
    """The list of one row, or None.  A mutant that loses its way returns ("lost",)."""
    if src == dst:
        return [int(src)]
    inf = inf_of(w)
    last = min(int(K), len(hist) - 1)
    DK = hist[last]
    if not DK[dst] < inf:
        return None
    want = bits(DK[dst:dst + 1])[0]
    h = int(min(K, V - 1)) if mutant == "late" else next(k for k in range(last + 1) if bits(hist[k][dst:dst + 1])[0] == want)
    u_of = slot_sources(V, off)
    x, target = int(dst), DK[dst]
    rev = [x]
    for i in range(h, 0, -1):
        Dp = DK if mutant == "final" else hist[min(i - 1, last)]
        into = adj == x
        with np.errstate(over="ignore", invalid="ignore"):
            cand = Dp[u_of] + w
        tight = into & (Dp[u_of] < inf) & (bits(cand) == bits(np.full(1, target, dtype=w.dtype))[0])
        if not tight.any():
            return ("lost",)
        us = u_of[tight]
        u = int(us.max() if mutant == "max_parent" else us.min())
        slots = np.flatnonzero(into & (u_of == u) & (tight if mutant != "first_slot" else True))
        rev += [int(eid[slots[0]]), u]
        x, target = u, Dp[u]
    if x != src:
        return ("lost",)
    return rev[::-1]


def bounded_paths(V, off, adj, eid, w, rs, rd, K, mutant=None):
    """The lists of the rows (rs, rd) under K = max_hops; rs < 0 or rd < 0 is a NULL row."""
    rs, rd = np.asarray(rs, dtype=np.int64), np.asarray(rd, dtype=np.int64)
    eid = np.asarray(eid, dtype=np.int64)
    if mutant == "filter":
        return [p if p is None or len(p) // 2 <= K else None for p in P.cheapest_paths(V, off, adj, eid, w, rs, rd)]
    out = [None] * len(rs)
    hists = {}
    for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
        if s < 0 or d < 0:
            continue
        if s not in hists:
            hists[s] = hop_history(V, off, adj, w, s, K)
        out[i] = walk_back(V, off, adj, eid, w, hists[s], K, s, d, mutant)
    return out


def brute_force(V, off, adj, eid, w, src, dst, K):
    """Over ALL walks src -> dst of at most K edges of a tiny graph: the smallest fold, then the fewest edges, then — comparing
    from the dst side — the smallest predecessor and, for it, the first slot.  None when no walk's fold gets under INF."""
    if src == dst:
        return [int(src)]
    inf = inf_of(w)
    best = []  # (fold, walk as [(u, slot), ...])

    def walk(v, acc, steps):
        if v == dst and steps:
            best.append((acc, list(steps)))
        if len(steps) == K:
            return
        for s in range(int(off[v]), int(off[v + 1])):
            with np.errstate(over="ignore", invalid="ignore"):
                nxt = acc + w[s]
            if not nxt < inf:
                continue
            steps.append((v, s))
            walk(int(adj[s]), nxt, steps)
            steps.pop()

    walk(int(src), w.dtype.type(0), [])
    if not best:
        return None
    low = min(f for f, _ in best)
    cands = [p for f, p in best if f == low]
    k = min(len(p) for p in cands)
    cands = [p for p in cands if len(p) == k]
    chosen = min(cands, key=lambda p: [x for step in reversed(p) for x in step])
    out = []
    for u, s in chosen:
        out += [u, int(eid[s])]
    return out + [int(dst)]


# ---- the fixtures that are new here: (V, off, adj, eid, w, rs, rd), edge ids are not the slot numbers ---------------------

def shortcut_path(double):
    """cheapest_within_model.shortcut_path with edge ids and rows: 0 -> 1 -> ... -> 6 with weights 1, shortcuts 0 -> j of weight
    10 j.  The cheapest walk 0 -> 6 of at most K edges takes the shortcut to 6 - (K - 1) and walks on, so the list changes with
    every K = 1 .. 6, and the vertices 2 .. 6 improve in several rounds."""
    es = list(range(6)) + [0] * 5
    ed = list(range(1, 7)) + list(range(2, 7))
    ew = [1] * 6 + [10 * j for j in range(2, 7)]
    return _fixture(7, es, ed, ew, [(0, 6), (0, 5), (0, 3), (1, 6), (6, 0), (0, 0)], double)


def absorbed_shortcut():
    """0 -> 2 (1.0), 0 -> 1 (0.25), 1 -> 2 (0.25), 2 -> 3 (2^53).  1.0 + 2^53 == 0.5 + 2^53: round 2 labels vertex 3 and round 3
    does not improve it, so the bounded list of (0, 3) is 0, 2, 3 for every K >= 2, where cheapest_path follows the final label
    0.5 of vertex 2 through vertex 1.  Both fold to 2^53."""
    return _fixture(4, [0, 0, 1, 2], [2, 1, 2, 3], [1.0, 0.25, 0.25, 2.0 ** 53], [(0, 3), (0, 2)], True)


def long_out_list(n, double):
    """0 -> 1 -> 2 -> 3, and the tight parent 2 of dst 3 has n slots into it: all but the LAST of a heavier weight."""
    es = [0, 1] + [2] * n
    ed = [1, 2] + [3] * n
    ew = [1, 1] + [9] * (n - 1) + [1]
    return _fixture(4, es, ed, ew, [(0, 3), (1, 3), (2, 3)], double)


def many_sources(m, double):
    """m distinct sources 0 .. m - 1, each with one edge (weight 1 + i % 3) into m, then the shared tail m -> m + 1 -> m + 2."""
    es = list(range(m)) + [m, m + 1]
    ed = [m] * m + [m + 1, m + 2]
    ew = [1 + i % 3 for i in range(m)] + [2, 3]
    rows = [(i, m + 2) for i in range(m)] + [(i, m + 1) for i in range(0, m, 5)]
    return _fixture(m + 3, es, ed, ew, rows, double)


def directed_path(n, double):
    """0 -> 1 -> ... -> n - 1, weights 1 .. 3 in turn; the rows (0, j) for every j and a few from the middle."""
    s = np.arange(n - 1)
    rows = [(0, j) for j in range(n)] + [(3, n - 1), (n - 1, 0), (5, 12)]
    return _fixture(n, s, s + 1, (s % 3) + 1, rows, double)
