"""The Python model of cheapest_path (a helper of test_cheapest_path_cpu.py / test_cheapest_path_gpu.py).

The contract (include/pgq_hip.h, pgq_cheapest_path).  D[v] = the labels cheapest_path_length defines: the least fixpoint of
dist[n] = min(dist[n], dist[v] + w) from dist[src] = 0 under INF = max / 2 of the weight type, in the weight type's own
arithmetic.  A slot s of u's out-list with adj[s] = x is TIGHT when D[u] < INF and D[u] + w[s] == D[x].  H[src] = 0 and
H[x] = 1 + min H[u] over the tight slots (u, x): the BFS levels of the tight subgraph.  For a row with D[dst] < INF and
k = H[dst] the path is x_k = dst and, for i = k .. 1, x_{i-1} = the smallest u with H[u] = i - 1 that has a tight slot into x_i,
e_i = edge_ids[the first tight slot of that u into x_i]; the list is [x_0, e_1, x_1, ..., e_k, x_k].  src == dst gives [src];
a NULL endpoint or an unreachable dst gives None.

`settle` runs Bellman-Ford sweeps with numpy in the element type, `levels` the BFS over the tight slots, `walk_back` the
walk.  `brute_force` enumerates the simple paths of a tiny graph instead: the smallest left-to-right fold, then the fewest
edges, then the tie-break from the dst side.  MUTANTS are the ways an implementation can go wrong that the fixtures must
notice; the fixtures of the GPU tests are built here too, so that the CPU tests can show that they do."""
import numpy as np

from cheapest_within_model import csr_of, inf_of

# greedy: the smallest u with a tight slot into x, whatever its H (loops on zero-weight and absorbed cycles: cut after V steps)
# first_slot: the first slot of u into x, tight or not
# max_parent: the largest u of the level instead of the smallest
# le: "tight" read as D[x] <= D[u] + w — true of every edge out of a labelled vertex, so the path is the hop-shortest one
MUTANTS = ("greedy", "first_slot", "max_parent", "le")


def slot_sources(V, off):
    """The vertex every slot belongs to."""
    return np.repeat(np.arange(V, dtype=np.int64), np.diff(off))


def settle(V, off, adj, w, src):
    """D for one source: sweeps over every slot until nothing changes."""
    inf = inf_of(w)
    D = np.full(V, inf, dtype=w.dtype)
    D[src] = 0
    u = slot_sources(V, off)
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(V + 1):
            cand = D[u] + w
            good = cand < D[adj]  # false for NaN, +inf and every sum that does not get under INF
            if not good.any():
                break
            np.minimum.at(D, adj[good], cand[good])
    return D


def tight_slots(V, off, adj, w, D, mutant=None):
    inf = inf_of(w)
    u = slot_sources(V, off)
    with np.errstate(over="ignore", invalid="ignore"):
        cand = D[u] + w
        if mutant == "le":
            return (D[u] < inf) & (D[adj] <= cand)
        return (D[u] < inf) & (cand == D[adj])


def levels(V, off, adj, tight, src):
    """H: -1 where the tight subgraph does not reach."""
    u = slot_sources(V, off)
    H = np.full(V, -1, dtype=np.int64)
    H[src] = 0
    front = np.zeros(V, dtype=bool)
    front[src] = True
    k = 0
    while front.any():
        k += 1
        hit = tight & front[u] & (H[adj] < 0)
        front = np.zeros(V, dtype=bool)
        front[adj[hit]] = True
        H[front] = k
    return H


def walk_back(V, off, adj, eid, w, D, H, tight, src, dst, mutant=None):
    """The list of one row, or None.  A mutant that loses its way returns what it has after V steps, or ("lost",)."""
    if src == dst:
        return [int(src)]
    if not D[dst] < inf_of(w):
        return None
    u_of = slot_sources(V, off)
    x = int(dst)
    rev = [x]
    for _ in range(V):
        if x == src:
            break
        into = adj == x
        cands = into & tight
        if mutant != "greedy":
            cands &= H[u_of] == H[x] - 1
        if not cands.any():
            return ("lost",)
        us = u_of[cands]
        u = int(us.max() if mutant == "max_parent" else us.min())
        slots = np.flatnonzero(into & (u_of == u) & (tight if mutant != "first_slot" else True))
        rev += [int(eid[slots[0]]), u]
        x = u
    if x != src:
        return ("lost",)
    return rev[::-1]


def cheapest_paths(V, off, adj, eid, w, rs, rd, mutant=None):
    """The lists of the rows (rs, rd); rs < 0 or rd < 0 is a NULL row."""
    rs, rd = np.asarray(rs, dtype=np.int64), np.asarray(rd, dtype=np.int64)
    eid = np.asarray(eid, dtype=np.int64)
    out = [None] * len(rs)
    state = {}
    for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
        if s < 0 or d < 0:
            continue
        if s not in state:
            D = settle(V, off, adj, w, s)
            tight = tight_slots(V, off, adj, w, D, mutant)
            state[s] = (D, tight, levels(V, off, adj, tight, s))
        D, tight, H = state[s]
        out[i] = walk_back(V, off, adj, eid, w, D, H, tight, s, d, mutant)
    return out


def fold(w, eid, path):
    """The left-to-right fold of the weights of a list's edges in the element type (edge id -> slot through eid)."""
    slot_of = {int(e): k for k, e in enumerate(np.asarray(eid).tolist())}
    acc = w.dtype.type(0)
    with np.errstate(over="ignore", invalid="ignore"):
        for e in path[1::2]:
            acc = acc + w[slot_of[int(e)]]
    return acc


def brute_force(V, off, adj, eid, w, src, dst):
    """Over the SIMPLE paths src -> dst of a tiny graph: the smallest fold, then the fewest edges, then — comparing from the dst
    side — the smallest predecessor and, for it, the first slot.  None when no path's fold gets under INF."""
    if src == dst:
        return [int(src)]
    inf = inf_of(w)
    best = []  # (fold, path as [(u, slot), ...])

    def walk(v, acc, seen, steps):
        if v == dst:
            best.append((acc, list(steps)))
            return
        for s in range(int(off[v]), int(off[v + 1])):
            n = int(adj[s])
            if n in seen:
                continue
            with np.errstate(over="ignore", invalid="ignore"):
                nxt = acc + w[s]
            if not nxt < inf:
                continue
            seen.add(n)
            steps.append((v, s))
            walk(n, nxt, seen, steps)
            steps.pop()
            seen.remove(n)

    walk(int(src), w.dtype.type(0), {int(src)}, [])
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


# ---- the fixtures of the GPU tests -----------------------------------------------------------------------------------
# every fixture: (V, off, adj, eid, w, rs, rd); edge ids are NOT the slot numbers, so a slot returned for an id shows

def _fixture(V, es, ed, ew, rows, double):
    es = np.asarray(es, dtype=np.int64)
    ew = np.asarray(ew, dtype=np.float64 if double else np.int64)
    off, adj, w = csr_of(V, es, ed, ew)
    eid = 1000 + np.argsort(es, kind="stable").astype(np.int64)  # 1000 + the edge's position in the lists above
    rs, rd = np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.int64)
    return V, off, adj, eid, w, rs, rd


def diamond(double):
    """0 -> 3 over two routes of cost 6: 0 -> 1 -> 2 -> 3 (three hops, through the smaller ids) and 0 -> 4 -> 3 (two)."""
    return _fixture(5, [0, 1, 2, 0, 4], [1, 2, 3, 4, 3], [2, 2, 2, 3, 3], [(0, 3), (0, 2), (1, 3), (3, 0)], double)


def tied_parents(double):
    """0 -> 5 and 0 -> 2, both -> 6, all of one cost: two parents of one level and one cost.  The edge rows name 5 first and 0's
    out-list reaches 5 first; the in-list of 6 cannot (a CSR's slots ascend by source, and the reverse CSR is a stable sort of
    them by destination, so every in-list ascends by source) — what tells the smaller parent from the other is the max_parent
    mutant, and long_in_list puts the one tight parent behind smaller ones."""
    return _fixture(7, [0, 0, 5, 2], [5, 2, 6, 6], [1, 1, 4, 4], [(0, 6), (0, 5), (2, 6)], double)


def parallel_edges(double):
    """0 -> 1 three times (weights 5, 3, 3: the tight slot is not the first, and of the two tight ones the first wins), then
    1 -> 2 twice with one weight."""
    return _fixture(3, [0, 0, 0, 1, 1], [1, 1, 1, 2, 2], [5, 3, 3, 7, 7], [(0, 1), (0, 2), (1, 2)], double)


def zero_ring(double):
    """src 5 -> 1 (weight 2) and a zero-weight ring of five, 1 -> 2 -> 3 -> 4 -> 0 -> 1: dst on the ring, reached over zero
    edges only.  The smallest tight predecessor of 1 is 0, on the ring: a walk back that takes it goes round for ever."""
    es = [5, 1, 2, 3, 4, 0]
    ed = [1, 2, 3, 4, 0, 1]
    return _fixture(6, es, ed, [2, 0, 0, 0, 0, 0], [(5, 3), (5, 0), (5, 1), (2, 1), (4, 3)], double)


def absorption():
    """3 -> 0 of weight 2^53, then the cycle 0 -> 2 -> 1 -> 0 of weights 1.0: 2^53 + 1.0 == 2^53, so every edge of the cycle
    is tight, and the smallest tight predecessor of 0 is 1, on the cycle."""
    es = [3, 0, 2, 1]
    ed = [0, 2, 1, 0]
    return _fixture(4, es, ed, [2.0 ** 53, 1.0, 1.0, 1.0], [(3, 1), (3, 2), (3, 0), (0, 1)], True)


def long_in_list(n, double):
    """dst = n + 2 has n in-edges, from 1 .. n in that order.  All of them sit two hops from src 0 at cost 2 (0 -> n + 1 -> j),
    so all pass the level test; the decoys 1 .. n - 1 reach dst over a weight of 9, and only n, in the LAST slot of the in-list
    and with the largest id, over the tight weight of 1."""
    dst = n + 2
    es = [0] + [n + 1] * n + list(range(1, n + 1))
    ed = [n + 1] + list(range(1, n + 1)) + [dst] * n
    ew = [1] + [1] * n + [9] * (n - 1) + [1]
    return _fixture(n + 3, es, ed, ew, [(0, dst), (n + 1, dst), (1, dst)], double)


def long_chain(n, double):
    """0 -> 1 -> ... -> n - 1, one out-edge each: the chain the length call answers in its pre-pass."""
    s = np.arange(n - 1)
    w = (s % 7) + 1
    return _fixture(n, s, s + 1, w * 0.25 if double else w, [(0, n - 1), (5, n - 2), (n - 1, 0), (17, 17)], double)


def random_weighted(V, E, double, seed=5, unit=False, rows=300):
    """A random graph with weights from {0, 1, 2, 3} (ties everywhere) or all ones, parallel edges and self-loops as they fall.
    No random edge enters the last five vertices; the last edge, V - 1 -> V - 2, gives V - 2 an in-edge nobody else reaches.
    Every 41st row has src == dst, every 23rd from the 8th on asks for V - 2 (searched, not found), from the 12th on for V - 3
    (no in-edge at all)."""
    rng = np.random.default_rng(seed)
    es, ed = rng.integers(0, V, E), rng.integers(0, V - 5, E)
    es[-1], ed[-1] = V - 1, V - 2
    ew = np.ones(E, dtype=np.int64) if unit else rng.integers(0, 4, E)
    rs, rd = rng.integers(0, V - 5, rows), rng.integers(0, V, rows)
    rd[7::23] = V - 2
    rd[11::23] = V - 3
    rd[::41] = rs[::41]
    return _fixture(V, es, ed, ew, list(zip(rs.tolist(), rd.tolist())), double)


def small_fixtures(double):
    """The fixtures a mutant must fail on at least once."""
    fx = {"diamond": diamond(double), "tied_parents": tied_parents(double), "parallel_edges": parallel_edges(double),
          "zero_ring": zero_ring(double), "long_in_list_65": long_in_list(65, double)}
    if double:
        fx["absorption"] = absorption()
    return fx
