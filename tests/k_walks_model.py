"""The Python model of walk_count and k_shortest_walks (a helper of test_k_walks_cpu.py / test_k_walks_gpu.py).

The contract (include/pgq_hip.h).  For a row (src, dst), lo = min_hops, K = max_hops, over the forward CSR's slots (parallel edges
are separate slots):
    W_0[v] = 1 if v == src else 0
    W_t[x] = min(INT64_MAX, sum of W_{t-1}[u] over ALL in-slots (u, x))      t = 1 .. K
    count  = min(INT64_MAX, sum of W_t[dst] for t = lo .. K)
src == dst is not special: the empty walk counts when lo == 0, and every closed walk of lo..K edges.  A NULL endpoint gives -1.
The lists are the first min(count, k) walks, each [x_0, e_1, x_1, ..., e_t, x_t] ([src] for the empty walk), shorter walks first;
walk number r: the smallest t >= lo with r < W_t[dst] after subtracting the shorter lengths' W_t[dst]; then x_t = dst and for
i = t .. 1 the in-list of x_i is scanned in its stored order — by (parent id, forward slot) — and for every in-slot (u, x_i):
r < W_{i-1}[u] takes the slot, else r -= W_{i-1}[u].  A row without a walk (and a NULL row) has no list: None.
The list form reports, beside the lists, the hops of the first walk (-1: none) and `count_k`: the walks of lo..T edges, T the length
of the row's last emitted walk (a row that has its k walks adds no more): count when count <= k, else between k and count.

Plain Python integers, so that nothing here can wrap.  `brute_force` enumerates every walk of at most K edges instead.  MUTANTS are
the ways an implementation can go wrong that the fixtures must notice; the fixtures of the GPU tests are built here too, so that
the CPU tests can show that they do."""
import numpy as np

import all_shortest_model as A

INT64_MAX = A.INT64_MAX
K_ALL = (1 << 31) - 1
MAX_HOPS = 64  # PGQ_WALK_MAX_HOPS

# wrap                the sum wraps as a signed 64-bit add instead of saturating
# bfs_only            no revisits: a vertex only gets the W of the round that reaches it first (degenerates to ALL SHORTEST)
# lower_ignored       min_hops taken as 0
# empty_walk_always   [src] counted for src == dst also when min_hops > 0
# trivial_src_eq_dst  src == dst answered with [[src]] and nothing else, as the other calls do
# length_order        walks of the larger lengths emitted first
# collapse            parallel edges counted once
# slot_order          candidates ordered by (which of the parent's parallel slots, parent) instead of (parent, slot)
# k_plus_1            one walk more than k
# m_mod_64            which of the parent's slots into x_i the taken in-slot is, counted modulo 64
# slot_first_64       the parent's m-th slot into x_i searched in the first 64 entries of its out-list only
MUTANTS = ("wrap", "bfs_only", "lower_ignored", "empty_walk_always", "trivial_src_eq_dst", "length_order", "collapse", "slot_order", "k_plus_1",
           "m_mod_64", "slot_first_64")


def _add(a, b, mutant):
    s = a + b
    if mutant == "wrap":
        return (s + (1 << 63)) % (1 << 64) - (1 << 63)
    return min(s, INT64_MAX)


def _in_slots(rin, x, mutant):
    """The in-slots of x as (parent, slot, m) in scan order; m = which of the parent's slots into x this is."""
    out, seen = [], {}
    for u, slot in rin[x]:
        m = seen.get(u, 0)
        seen[u] = m + 1
        if mutant == "collapse" and m > 0:
            continue
        out.append((u, slot, m))
    if mutant == "slot_order":
        out.sort(key=lambda c: (c[2], c[0]))
    return out


def tables(V, rin, src, K, mutant=None, have=None):
    """[W_0, ..., W_K] of the source, each a dict vertex -> W > 0 (wrap: != 0); `have`: the rounds computed so far, extended in place."""
    Ws = [{src: 1}] if not have else have
    reached = set()
    if mutant == "bfs_only":
        for W in Ws:
            reached |= set(W)
    while len(Ws) <= K:
        prev, cur = Ws[-1], {}
        if prev:
            for x in range(V):
                if mutant == "bfs_only" and x in reached:
                    continue
                acc, any_parent = 0, False
                for u, _, _ in _in_slots(rin, x, mutant):
                    if u in prev:
                        acc, any_parent = _add(acc, prev[u], mutant), True
                if any_parent:
                    cur[x] = acc
        reached |= set(cur)
        Ws.append(cur)
    return Ws


def unrank(off, adj, eid, rin, Ws, src, dst, t, r, mutant=None):
    """Walk number r among the walks of t edges, or ("lost",) when a (mutant) walk finds no slot or does not come home."""
    x = dst
    rev = [int(x)]
    for i in range(t, 0, -1):
        taken = None
        for u, slot, m in _in_slots(rin, x, mutant):
            w = Ws[i - 1].get(u, 0)
            if r < w:
                taken = (u, slot, m)
                break
            r -= max(w, 0)
        if taken is None:
            return ("lost",)
        u, slot, m = taken
        if mutant in ("m_mod_64", "slot_first_64"):
            slot = A.mth_slot(off, adj, u, x, m, mutant)
            if slot is None:
                return ("lost",)
        rev += [int(eid[slot]), int(u)]
        x = u
    return rev[::-1] if x == src else ("lost",)


def solve(V, off, adj, eid, rs, rd, min_hops, max_hops, k, mutant=None, state=None):
    """(counts, hops, lists, counts_k) of the rows.  counts: -1 = NULL; hops -1 and lists None where the row has no list.  `state`:
    a dict that keeps the tables of every source between calls on ONE graph and ONE mutant."""
    state = {} if state is None else state
    if "rin" not in state:
        state["rin"] = A.in_lists(V, off, adj)
    rin = state["rin"]
    lo = 0 if mutant == "lower_ignored" else min_hops
    take_max = k + (1 if mutant == "k_plus_1" else 0)
    counts, hops, lists, counts_k = [], [], [], []
    for s, d in zip(np.asarray(rs).tolist(), np.asarray(rd).tolist()):
        if s < 0 or d < 0:
            counts.append(-1), hops.append(-1), lists.append(None), counts_k.append(-1)
            continue
        if mutant == "trivial_src_eq_dst" and s == d:
            counts.append(1), hops.append(0), lists.append([[int(s)]]), counts_k.append(1)
            continue
        Ws = state[s] = tables(V, rin, s, max_hops, mutant, state.get(s))
        per_len = [(t, Ws[t].get(d, 0)) for t in range(lo, max_hops + 1)]
        if mutant == "empty_walk_always" and s == d and lo > 0:
            per_len = [(0, 1)] + per_len
        count = 0
        for _, w in per_len:
            count = _add(count, w, mutant)
        counts.append(count)
        if mutant == "length_order":
            per_len = per_len[::-1]
        walks, first, ck = [], -1, 0
        for t, w in per_len:
            if len(walks) >= take_max or ck >= take_max:
                break
            if w > 0:
                first = t if first < 0 else first
                ck = _add(ck, w, mutant)
                walks += [unrank(off, adj, eid, rin, Ws, s, d, t, r, mutant) for r in range(min(w, take_max - len(walks)))]
        hops.append(first), lists.append(walks or None), counts_k.append(ck)
    return counts, hops, lists, counts_k


def brute_force(V, off, adj, eid, src, K):
    """Every walk of at most K edges from src, per destination, as (slots, list) in the contract's order: by length, then from
    the destination end by (x_{t-1}, slot of e_t), (x_{t-2}, slot of e_{t-1}), ...  Sorted independently of the unranking."""
    u_of = A.slot_sources(V, off)
    per_dst = [[] for _ in range(V)]
    stack = [(src, [])]
    while stack:
        v, slots = stack.pop()
        per_dst[v].append(slots)
        if len(slots) < K:
            for s in range(off[v], off[v + 1]):
                stack.append((int(adj[s]), slots + [s]))
    out = []
    for walks in per_dst:
        walks.sort(key=lambda sl: (len(sl), [(int(u_of[s]), s) for s in reversed(sl)]))
        lists = []
        for sl in walks:
            p = [int(src)]
            for s in sl:
                p += [int(eid[s]), int(adj[s])]
            lists.append(p)
        out.append(lists)
    return out


# ---- fixtures: (V, off, adj, eid, rs, rd) -------------------------------------------------------------------------------------
def with_edges(fx, es, ed, rows):
    """The fixture's graph with more edges (they come behind the existing slots of their sources) and other rows."""
    V, off, adj = fx[:3]
    return A._fx(V, A.slot_sources(V, off).tolist() + list(es), adj.tolist() + list(ed), rows)


def in_list_gadget(deg):
    """all_shortest_model.in_list_gadget with a back edge x -> s: the row (s, x) has walks of 3 and of 7 edges, (s, s) and (x, x)
    closed walks of 4.  The in-list of x and the out-list of s2 have `deg` entries."""
    fx = A.in_list_gadget(deg)
    rs, rd = fx[4], fx[5]
    s, x = int(rs[0]), int(rd[0])
    return with_edges(fx, [x], [s], [(s, x), (int(rs[1]), int(rd[1])), (s, int(rd[2])), (s, s), (x, x), (x, s)])


def ring(n=5):
    """0 -> 1 -> ... -> n-1 -> 0: the closed walks have n, 2 n, ... edges."""
    return A._fx(n, list(range(n)), [(i + 1) % n for i in range(n)], [(0, 0), (0, 2), (2, 0), (3, 3), (4, 0)])


def self_loop():
    """Vertex 0 with a self-loop and 0 -> 1 -> 2; 2 has no out-edge."""
    return A._fx(3, [0, 0, 1], [0, 1, 2], [(0, 0), (0, 1), (0, 2), (1, 1), (1, 0), (2, 2)])


def chain8(n=22):
    """A chain 0 -> 1 -> ... -> n with 8 parallel edges per hop: W_t[t] = 8^t, 2^60 at t = 20 (exact), saturated at t = 21."""
    es = [i for i in range(n) for _ in range(8)]
    return A._fx(n + 1, es, [i + 1 for i in es], [(0, 20), (0, 21), (0, 22), (0, 5), (1, 21)])


def two_loops():
    """One vertex with two self-loops: W_t = 2^t; lo = 0, K = 62 gives 2^63 - 1 unsaturated, K = 63 saturates."""
    return A._fx(1, [0, 0], [0, 0], [(0, 0)])


def loops_and_fan():
    """a with two self-loops and three edges a -> b: W_t[b] = 3 * 2^(t-1) stays below 2^63 up to t = 62, the sum over 1..62 does not."""
    return A._fx(2, [0, 0, 0, 0, 0], [0, 0, 1, 1, 1], [(0, 1), (0, 0), (1, 1), (1, 0)])


BOUNDS = ((0, 0), (0, 3), (1, 3), (2, 4), (3, 3))
KS = (1, 3, K_ALL)


def gpu_fixtures():
    """name -> (fixture, ((min_hops, max_hops, the k values), ...)) the GPU file runs; the CPU file shows that they catch MUTANTS."""
    general = tuple(b + (KS,) for b in BOUNDS)
    fx = {"tiny0": (A.tiny_multigraph(0), general), "random": (A.random_fixture(), general),
          "parallel": (A.parallel_edges(), ((0, 3, (1, 9, 10, 11)), (1, 2, (1, K_ALL)), (2, 2, (2, 9, 10)))),
          "ring5": (ring(5), ((0, 10, (1, 2, 3)), (1, 10, (1, 2, 3)), (1, 4, (1,)), (5, 5, (1, 2)), (6, 12, (1, 2)))),
          "self_loop": (self_loop(), ((0, 3, KS), (1, 3, KS), (2, 5, (1, 4, K_ALL)))),
          "dead_ends": (A.dead_ends(), ((0, 2, (1, 3)), (1, 2, (1, 3)))),
          "chain8": (chain8(), ((0, MAX_HOPS, (3,)), (1, 30, (1, 3)), (21, 21, (3,)))),
          "two_loops": (two_loops(), ((0, 62, (3,)), (0, 63, (3,)), (1, MAX_HOPS, (3,)))),
          "loops_and_fan": (loops_and_fan(), ((1, 62, (3,)), (1, 61, (3,)), (0, 3, (K_ALL,))))}
    for deg in (63, 64, 65, 127, 128, 129):
        fx["in_list_%d" % deg] = (in_list_gadget(deg), ((0, 3, (1, K_ALL)), (3, 7, (1, 200)), (4, 4, (K_ALL,))))
    for n in (63, 64, 65, 128, 129):
        fx["sources_%d" % n] = (A.many_sources(n), ((1, 3, (2,)),))
    for P in (63, 64, 65, 129):
        fx["parallel_run_%d" % P] = (A.parallel_run(P), ((2, 2, (1, K_ALL)), (1, 2, (1, K_ALL))))
    return fx
