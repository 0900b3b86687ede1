"""The Python model of cheapest_walk_length / cheapest_walk (a helper of test_cheapest_walk_cpu.py / test_cheapest_walk_gpu.py).

The contract (include/pgq_hip.h, pgq_cheapest_walk_length).  For a row (src, dst), lo = min_hops, K = max_hops, INF = max / 2 of the
weight type, every sum in the weight type's own arithmetic and counting only where it is below INF (never as NaN):
    E_0[src] = 0, E_0[v] = INF otherwise
    E_t[x]   = min over the in-slots (u, x) with E_{t-1}[u] < INF of E_{t-1}[u] + w      t = 1 .. lo   (INF if none: no carry-over)
    L_lo     = E_lo
    L_t[x]   = min(L_{t-1}[x], min over the in-slots (u, x) of L_{t-1}[u] + w)           t = lo + 1 .. K
The value is L_K[dst], NULL when that is INF or an endpoint is NULL.  With Λ_i = E_i (i <= lo), L_i (i > lo): h = the smallest t in
[lo, K] with Λ_t[dst] == L_K[dst] as bit patterns, x_h = dst and, for i = h .. 1, x_{i-1} = the smallest u with Λ_{i-1}[u] < INF and
a slot (u, x_i) with Λ_{i-1}[u] + w[s] == Λ_i[x_i], e_i = edge_ids[the first such slot of u's out-list into x_i].  src == dst is no
special row.

`history` is the recurrence, written down as it stands (every round offers from EVERY labelled vertex; no queue), plus the rounds
a lane batch of this one source runs: round t runs while t <= K and the queue behind round t - 1 is not empty — the source before
round 1, every vertex with a finite label behind an exact round, every vertex that improved behind a later one.  `solve` answers
rows.  `brute_force` enumerates every walk of lo..K edges of a tiny graph instead.  MUTANTS are the ways an implementation can go
wrong that the GPU tests' fixtures (gpu_fixtures) must notice."""
import numpy as np

import cheapest_path_model as P
import cheapest_path_within_model as CPW
from cheapest_path_model import _fixture, slot_sources
from cheapest_within_model import bits, inf_of

INT64_MAX = int(np.iinfo(np.int64).max)
MAX_HOPS = 64  # PGQ_WALK_MAX_HOPS: the largest lower bound

# no_reset:        the exact rounds keep E_{t-1}[x] (k_hop_snapshot without the take)
# filter:          cheapest_path_(length_)within(K)'s answer if its h >= lo, else NULL
# exact_to_K:      exact rounds all the way to K
# seed_D:          the rounds behind lo start from D_lo (the _within labels) instead of E_lo
# lo_minus_1 / lo_plus_1:  one exact round too few / too many
# src_eq_dst_zero: a src == dst row answered 0 / [src] although lo >= 1
# trivial_zero:    only the src == dst rows without an out-edge or without an in-edge answered 0 / [src] at lo >= 1
# stale_lookup:    the walk-back reads a vertex's latest log entry of round <= j, whatever its round (list only)
# h_unchecked:     h = the round of dst's latest entry even where it lies below lo (list only)
# max_parent:      the largest tight parent instead of the smallest (list only)
# last_slot:       the last tight slot instead of the first (list only)
MUTANTS = ("no_reset", "filter", "exact_to_K", "seed_D", "lo_minus_1", "lo_plus_1", "src_eq_dst_zero", "trivial_zero", "stale_lookup",
           "h_unchecked", "max_parent", "last_slot")
LIST_ONLY = ("stale_lookup", "h_unchecked", "max_parent", "last_slot")


def _round(P_, u_of, adj, w, inf, carry):
    """One round from the labels P_: (the new labels, the vertices whose label is new)."""
    with np.errstate(over="ignore", invalid="ignore"):
        cand = P_[u_of] + w
    good = (P_[u_of] < inf) & (cand < inf)  # false for NaN, for +inf and for every sum that does not get under INF
    new = P_.copy() if carry else np.full(len(P_), inf, dtype=P_.dtype)
    np.minimum.at(new, adj[good], cand[good])
    changed = np.flatnonzero(new < P_) if carry else np.flatnonzero(new < inf)
    return new, changed


def history(V, off, adj, w, src, lo, K, mutant=None):
    """(hist, rounds, entries): hist[t] = Λ_t for t = 0 .. len - 1, Λ_t = hist[-1] behind it (the labels stand still, or K is
    reached); rounds = the rounds a batch of this source runs; entries[t] = the vertices the log holds an entry of round t for."""
    inf = inf_of(w)
    u_of = slot_sources(V, off)
    exact = {"no_reset": lo, "exact_to_K": min(K, max(lo, MAX_HOPS)), "seed_D": lo, "lo_minus_1": max(lo - 1, 0), "lo_plus_1": min(lo + 1, K)}.get(mutant, lo)
    lab = np.full(V, inf, dtype=w.dtype)
    lab[src] = 0
    hist, entries = [lab], [np.array([src], dtype=np.int64)]
    shadow = lab  # seed_D: the _within labels beside the exact ones
    rounds, queued = 0, 1
    t = 0
    while t < K and (queued or t < exact):
        t += 1
        rounds += 1 if queued else 0
        carry = t > exact or mutant == "no_reset"
        lab, changed = _round(lab, u_of, adj, w, inf, carry)
        if mutant == "seed_D":
            shadow, _ = _round(shadow, u_of, adj, w, inf, True)
            if t == exact:
                changed = np.flatnonzero(shadow < inf)
                lab = shadow
        hist.append(lab)
        entries.append(changed)
        queued = len(changed)
    return hist, rounds, entries


def _walk_back(V, off, adj, eid, w, hist, entries, lo, h, src, dst, mutant):
    inf = inf_of(w)
    u_of = slot_sources(V, off)
    last = len(hist) - 1

    def labels_at(j):
        if mutant != "stale_lookup":
            return hist[min(j, last)]
        out = np.full(V, inf, dtype=w.dtype)  # every vertex's latest entry of round <= j, whatever its round
        for r in range(min(j, last) + 1):
            out[entries[r]] = hist[r][entries[r]]
        return out

    x, target = int(dst), hist[min(h, last)][dst]
    rev = [x]
    for i in range(h, 0, -1):
        Dp = labels_at(i - 1)
        into = adj == x
        with np.errstate(over="ignore", invalid="ignore"):
            cand = Dp[u_of] + w
        tight = into & (Dp[u_of] < inf) & (bits(cand) == bits(np.full(1, target, dtype=w.dtype))[0])
        if not tight.any():
            return ("lost",)
        us = u_of[tight]
        u = int(us.max() if mutant == "max_parent" else us.min())
        slots = np.flatnonzero(tight & (u_of == u))
        rev += [int(eid[slots[-1] if mutant == "last_slot" else slots[0]]), u]
        x, target = u, Dp[u]
    return rev[::-1] if x == src else ("lost",)


def solve(V, off, adj, eid, w, rs, rd, lo, K, mutant=None, state=None):
    """(out, ok, hops, lists, rounds) of the rows: out / ok as cheapest_walk_length (0 / False for NULL), hops = h (-1 for NULL),
    lists as cheapest_walk (None for NULL; a mutant that loses its way: ("lost",)), rounds = {source: the rounds its batch runs}.
    rs < 0 or rd < 0 is a NULL row.  state: a dict that keeps the histories between calls on ONE graph, bounds and mutant."""
    rs, rd = np.asarray(rs, dtype=np.int64), np.asarray(rd, dtype=np.int64)
    eid = np.asarray(eid, dtype=np.int64)
    lo, K = int(lo), int(K)
    inf = inf_of(w)
    n = len(rs)
    out, ok, hops, lists, rounds = np.zeros(n, dtype=w.dtype), np.zeros(n, dtype=bool), [-1] * n, [None] * n, {}
    state = {} if state is None else state
    roff = np.bincount(adj, minlength=V)
    model_lo = 0 if mutant == "filter" else lo
    for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
        if s < 0 or d < 0:
            continue
        trivial = s == d and (off[s + 1] == off[s] or roff[s] == 0)
        if lo >= 1 and s == d and (mutant == "src_eq_dst_zero" or (mutant == "trivial_zero" and trivial)):
            ok[i], hops[i], lists[i] = True, 0, [int(s)]
            continue
        if lo >= 1 and trivial:
            continue  # no lane: NULL
        if s not in state:
            state[s] = history(V, off, adj, w, s, model_lo, K, mutant)
        hist, rounds[s], entries = state[s]
        final = hist[-1]
        if not final[d] < inf:
            if mutant == "h_unchecked":  # dst's latest entry, of a round below lo: its label was taken
                r = max((t for t in range(len(hist)) if d in entries[t].tolist()), default=-1)
                if r >= 0:
                    out[i], ok[i], hops[i] = hist[r][d], True, r
                    lists[i] = _walk_back(V, off, adj, eid, w, hist, entries, lo, r, s, d, mutant)
            continue
        want = bits(final[d:d + 1])[0]
        h = next(t for t in range(min(model_lo, len(hist) - 1), len(hist)) if bits(hist[t][d:d + 1])[0] == want)
        if mutant == "filter" and h < lo:
            continue
        out[i], ok[i], hops[i] = final[d], True, h
        lists[i] = _walk_back(V, off, adj, eid, w, hist, entries, model_lo, h, s, d, mutant)
    return out, ok, hops, lists, rounds


def brute_force(V, off, adj, eid, w, src, dst, lo, K):
    """Over ALL walks src -> dst of lo..K edges of a tiny graph (every prefix's fold below INF): (value, h, list) — the smallest
    left-to-right fold, the fewest edges among the walks with that fold, and among those, reading from the dst side, the smallest
    predecessor and its first slot.  None when there is no such walk."""
    inf = inf_of(w)
    found = []  # (fold, walk as [(u, slot), ...])

    def walk(v, acc, steps):
        if v == dst and len(steps) >= lo:
            found.append((acc, list(steps)))
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
    if not found:
        return None
    low = min(f for f, _ in found)
    cands = [p for f, p in found if bits(np.array([f], dtype=w.dtype))[0] == bits(np.array([low], dtype=w.dtype))[0]]
    h = min(len(p) for p in cands)
    cands = [p for p in cands if len(p) == h]
    chosen = min(cands, key=lambda p: [x for step in reversed(p) for x in step])
    lst = []
    for u, s in chosen:
        lst += [u, int(eid[s])]
    return low, h, lst + [int(dst)]


# ---- the fixtures of the GPU tests: name -> ((V, off, adj, eid, w, rs, rd), bounds); edge ids are not the slot numbers ---------

def bound_binds(double):
    """0 -> 3 directly (1), over 1 in two edges (2 + 3 = 5), over 4 and 5 in three (1 + 1 + 2 = 4): {1,3} -> 1, {2,2} -> 5,
    {2,3} -> 4 with the three-edge list, {3,3} -> 4."""
    return _fixture(6, [0, 0, 1, 0, 4, 5], [3, 1, 3, 4, 5, 3], [1, 2, 3, 1, 1, 2], [(0, 3), (0, 5), (1, 3), (0, 0)], double)


BOUND_BINDS_EXPECTED = {(1, 3): (1, 1), (2, 2): (5, 2), (2, 3): (4, 3), (3, 3): (4, 3)}  # bounds -> (value, h) of row (0, 3)


def path4(double):
    """0 -> 1 -> 2 -> 3: row (0, 1) has ONE walk, of one edge — NULL at {2,3}, which only a reset shows."""
    return _fixture(4, [0, 1, 2], [1, 2, 3], [1, 2, 3], [(0, 1), (0, 2), (0, 3), (1, 3), (0, 0), (3, 3)], double)


def odd_walks(double):
    """0 -> 1 <-> 2: the walks 0 -> 1 have 1, 3, 5, ... edges, the walks 0 -> 2 have 2, 4, ...: {2,2} is NULL for (0, 1), {2,3} its
    three-edge walk."""
    return _fixture(3, [0, 1, 2], [1, 2, 1], [1, 2, 4], [(0, 1), (0, 2), (1, 1), (2, 2), (1, 2)], double)


def loops(double, shared):
    """A self-loop (0), a ring of two (1, 2), a ring of three (3, 4, 5), and 0 -> 1, 2 -> 3 between them: src == dst rows, alone on
    their lane or (shared) with other rows of the same source."""
    es, ed = [0, 0, 1, 2, 2, 3, 4, 5], [0, 1, 2, 1, 3, 4, 5, 3]
    ew = [2, 1, 3, 4, 1, 5, 6, 7]
    rows = [(v, v) for v in range(6)]
    if shared:
        rows += [(0, 1), (0, 2), (1, 2), (1, 5), (3, 5), (4, 3), (2, 0)]
    return _fixture(6, es, ed, ew, rows, double)


def dead_ends(double):
    """2 has no out-edge, 3 no in-edge, 4 neither: their src == dst rows take no lane and are NULL for lo >= 1."""
    return _fixture(5, [0, 1, 1, 3], [1, 0, 2, 0], [1, 1, 1, 1], [(2, 2), (3, 3), (4, 4), (0, 0), (3, 2), (1, 1)], double)


def many_sources(m, double):
    """m distinct sources 0 .. m - 1, each with one edge (weight 1 + i % 3) into m, the tail m -> m + 1 -> m + 2 and m + 2 -> 0
    back: every source but 0 has no in-edge, 0 has a closed walk of four edges.  The common destination is m + 2; the distinct
    sources are exactly 0 .. m - 1."""
    es = list(range(m)) + [m, m + 1, m + 2, m]
    ed = [m] * m + [m + 1, m + 2, 0, m + 2]
    ew = [1 + i % 3 for i in range(m)] + [2, 3, 1, 9]
    rows = [(i, m + 2) for i in range(m)] + [(i, i) for i in (0, 1, m - 1)] + [(i, m + 1) for i in range(0, m, 5)]
    return _fixture(m + 3, es, ed, ew, rows, double)


def stale_gadget(double):
    """0 -> 9 directly (2) and over 5 (1 + 1): at {2,2} the list is [0, ., 5, ., 9].  The source's entry of round 0 (label 0) makes
    the direct slot look tight against the label 2 of round 2 for a look-up that does not ask for round 1 exactly — and 0 < 5."""
    return _fixture(10, [0, 0, 5, 9], [9, 5, 9, 0], [2, 1, 1, 1], [(0, 9), (0, 0), (5, 5)], double)


def chain(n, double):
    """0 -> 1 -> ... -> n: n edges, weights 1 .. 3 in turn."""
    s = np.arange(n)
    return _fixture(n + 1, s, s + 1, (s % 3) + 1, [(0, n), (0, 2), (0, 3), (0, 8), (0, 9), (0, 10)], double)


def ring(n, double):
    """A ring of n vertices, weights 1 .. 3 in turn: the queue never runs dry, only K stops a batch."""
    s = np.arange(n)
    return _fixture(n, s, (s + 1) % n, (s % 3) + 1, [(0, 0), (0, 2), (0, n - 1)], double)


def near_inf():
    """int64 sums that reach INF = 2^62 - 1: 0 -> 1 -> 2 of 2^61 each sums to 2^62 (no label), 0 -> 3 -> 2 to INF - 1 (a label)."""
    inf = int(inf_of(np.zeros(1, dtype=np.int64)))
    return _fixture(4, [0, 1, 0, 3, 2], [1, 2, 3, 2, 0], [1 << 61, 1 << 61, inf - 2, 1, 1], [(0, 2), (0, 1), (0, 0), (3, 3), (1, 1)], False)


RING_BOUNDS = ((2, 4), (3, 3), (0, 4), (5, 12))  # the first three stop at K with the queue still full
CHAIN_BOUNDS = ((3, INT64_MAX), (9, INT64_MAX), (8, 8), (9, 9), (1, 20))
SMALL_BOUNDS = ((0, 0), (0, 3), (1, 1), (1, 3), (2, 2), (2, 3), (3, 3), (2, 4), (3, INT64_MAX))
OUT_LIST = (7, 8, 9, 64, 65, 128, 129)
IN_LIST = (63, 64, 65, 128, 129)
SOURCES = (63, 64, 65, 129)


def gpu_fixtures(double):
    """name -> (fixture, the bounds it is run under)."""
    fx = {"bound_binds": (bound_binds(double), tuple(BOUND_BINDS_EXPECTED) + ((0, 3), (1, 1))),
          "path4": (path4(double), SMALL_BOUNDS), "odd_walks": (odd_walks(double), SMALL_BOUNDS),
          "loops_alone": (loops(double, False), SMALL_BOUNDS), "loops_shared": (loops(double, True), SMALL_BOUNDS),
          "dead_ends": (dead_ends(double), SMALL_BOUNDS), "stale_gadget": (stale_gadget(double), SMALL_BOUNDS),
          "tied_parents": (P.tied_parents(double), SMALL_BOUNDS), "parallel_edges": (P.parallel_edges(double), SMALL_BOUNDS),
          "zero_ring": (P.zero_ring(double), SMALL_BOUNDS + ((5, 9),)),
          "chain20": (chain(20, double), CHAIN_BOUNDS), "ring5": (ring(5, double), RING_BOUNDS)}
    for m in SOURCES:
        fx["sources_%d" % m] = (many_sources(m, double), ((2, 3), (3, 4), (1, INT64_MAX)))
    for n in OUT_LIST:
        fx["out_list_%d" % n] = (CPW.long_out_list(n, double), ((2, 3), (3, 3), (1, 2)))
    for n in IN_LIST:
        fx["in_list_%d" % n] = (P.long_in_list(n, double), ((2, 3), (3, 3), (1, 2)))
    if double:
        fx["absorbed_shortcut"] = (CPW.absorbed_shortcut(), ((2, 2), (2, 3), (2, INT64_MAX), (3, 3), (1, 3)))
    else:
        fx["near_inf"] = (near_inf(), SMALL_BOUNDS)
    return fx
