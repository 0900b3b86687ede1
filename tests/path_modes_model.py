"""The Python model of k_shortest_walks_mode and walk_count_mode (a helper of test_path_modes_cpu.py / test_path_modes_gpu.py).

The contract (include/pgq_hip.h).  For a row (src, dst), lo = min_hops, K = max_hops, S = every walk of lo..K edges in
k_shortest_walks' order (k_walks_model.py: by length, then by in-list positions read from the destination end).  A walk
[x_0, e_1, x_1, ..., e_t, x_t] is admitted by
    ACYCLIC  when no two of x_0 .. x_t are equal,
    SIMPLE   when no two are equal except that x_0 == x_t is allowed,
    TRAIL    when no two of e_1 .. e_t (the list's elements: edge ids) are equal,
    NONE / WALK  always.
The row's list is the first min(a, k) admitted walks of S, a their number; the count form gives min(a, limit); a NULL endpoint gives
-1 / None.  Edge ids are shared by an edge's two directions at most (the binder's undirected CTE); then every walk of
dist(src, dst) edges is admitted by every mode.

Two independent restatements:
    filter_model   k_walks_model.brute_force's lists (every walk of at most K edges, sorted on its own) filtered by `admitted`.
    search_model   the depth-first search as the kernel does it: for t = lo .. K with W_t[dst] > 0, from x_t = dst, at depth i the
                   in-list of x_i from the depth's cursor in trips of 64 positions; a position is live when W_{i-1}[u] > 0 and the mode
                   admits u; the first live one is taken and the cursor left behind it.  Vertex modes: u is not among x_i .. x_t (SIMPLE
                   leaves x_t out when i - 1 == 0) and is not the source unless i - 1 == 0.  TRAIL: the taken in-slot is the m-th from u
                   into x_i, its edge the m-th slot of u's out-list into x_i; an id already among e_{i+1} .. e_t rejects it and the
                   cursor has moved on by one.  A STEP is one trip or one descent.  The model returns the steps of the counting pass
                   (the search until min(a, k) walks are found or the lengths are used up) and of the emitting pass (the same search
                   until the last of those walks is found; nothing when there is none).
The rounds: the walks of d = dist(src, dst) edges are admitted by every mode, so a row with lo <= d is settled at round d when
W_d[dst] >= k; every other row needs round K (or the empty queue).  `rounds_needed` says which.

MUTANTS are the ways an implementation can go wrong that the GPU fixtures must notice, in the lists, the counts or the steps."""
import numpy as np

import all_shortest_model as A
import k_walks_model as W

NONE, WALK, SIMPLE, TRAIL, ACYCLIC = range(5)  # PGQ_MODE_*
MODES = (SIMPLE, TRAIL, ACYCLIC)
MODE_NAMES = {NONE: "none", WALK: "walk", SIMPLE: "simple", TRAIL: "trail", ACYCLIC: "acyclic"}
K_ALL = W.K_ALL
MAX_HOPS = W.MAX_HOPS
OVER = ("over the step cap",)
MUTANT_STEP_CAP = 50000  # a mutant is cut here, well above what the fixtures take, and differs by that ...
ENDLESS_STEP_CAP = 5000  # ... the two that may never end (or enumerate 2^64 walks) sooner

# filter_first_k     the filter applied to the first k walks of S only
# top_off_stack      x_t is not on the stack
# source_midwalk     ACYCLIC lets the source be passed mid-walk (same lists, more steps: the walk is refused at its last step)
# simple_as_acyclic  SIMPLE treated as ACYCLIC
# acyclic_as_simple  ACYCLIC treated as SIMPLE
# trail_by_slot      TRAIL compares forward slots, not edge ids
# trail_by_vertex    TRAIL compares vertices (as SIMPLE does)
# stack_63           the stack test covers the last 63 depths only
# cursor_reset       the cursor of a depth starts at 0 again on backtrack
# no_pop             a vertex stays on the stack after backtracking over it
# prune_w_i          the prune reads W_i in place of W_{i-1}
# k_plus_1           one walk more than k
# length_order       the longer lengths first
# m_mod_64           which of the parent's slots the taken in-slot is, counted modulo 64
# stop_below_lo      the stop rule closes a row whose distance is below lo
MUTANTS = ("filter_first_k", "top_off_stack", "source_midwalk", "simple_as_acyclic", "acyclic_as_simple", "trail_by_slot", "trail_by_vertex",
           "stack_63", "cursor_reset", "no_pop", "prune_w_i", "k_plus_1", "length_order", "m_mod_64", "stop_below_lo")


def admitted(p, mode):
    """The contract's test, on the list itself."""
    xs, es = p[0::2], p[1::2]
    if mode == ACYCLIC:
        return len(set(xs)) == len(xs)
    if mode == SIMPLE:
        return len(set(xs[1:])) == len(xs[1:]) and len(set(xs[:-1])) == len(xs[:-1])
    if mode == TRAIL:
        return len(set(es)) == len(es)
    return True


def filter_model(V, off, adj, eid, rs, rd, min_hops, max_hops, k, mode, brute=None):
    """(counts, hops, lists): counts = min(a, k), -1 for a NULL row; hops of the first list (-1: none); lists None where there is none.
    `brute`: a dict source -> k_walks_model.brute_force(..., source, max_hops), filled here."""
    brute = {} if brute is None else brute
    counts, hops, lists = [], [], []
    for s, d in zip(np.asarray(rs).tolist(), np.asarray(rd).tolist()):
        if s < 0 or d < 0:
            counts.append(-1), hops.append(-1), lists.append(None)
            continue
        if s not in brute:
            brute[s] = W.brute_force(V, off, adj, eid, s, max_hops)
        got = [p for p in brute[s][d] if len(p) // 2 >= min_hops and admitted(p, mode)][:k]
        counts.append(len(got)), hops.append(len(got[0]) // 2 if got else -1), lists.append(got or None)
    return counts, hops, lists


def rounds_needed(Ws, dst, min_hops, max_hops, k, mutant=None):
    """The round after which the row asks for no more: its distance d when min_hops <= d and W_d[dst] >= k, else max_hops."""
    for t in range(max_hops + 1):
        w = Ws[t].get(dst, 0)
        if w > 0:
            return t if (t >= min_hops or mutant == "stop_below_lo") and w >= k else max_hops
    return max_hops


def _search_row(off, adj, eid, rin, Ws, src, dst, lo, R, k, mode, mutant, cap):
    """(lists, steps of the counting pass, steps of the emitting pass) of one row over the tables W_0 .. W_R; OVER past the cap."""
    if mutant == "simple_as_acyclic" and mode == SIMPLE:
        mode = ACYCLIC
    elif mutant == "acyclic_as_simple" and mode == ACYCLIC:
        mode = SIMPLE
    elif mutant == "trail_by_vertex" and mode == TRAIL:
        mode = SIMPLE
    vertex_mode = mode in (SIMPLE, ACYCLIC)
    want = k + (1 if mutant == "k_plus_1" else 0)
    found, steps, steps_at_last = [], 0, 0
    lengths = range(lo, R + 1)
    for t in (reversed(lengths) if mutant == "length_order" else lengths):
        if len(found) >= want:
            break
        if Ws[t].get(dst, 0) <= 0:
            continue
        x, e, cur, stale = [None] * (t + 1), [None] * (t + 1), [0] * (t + 1), [dst]
        i = t
        x[t] = dst
        while i <= t and len(found) < want:
            if i == 0:
                if t > 0 and x[0] != src:
                    return ("lost",), steps, steps
                p = [int(x[0])]
                for j in range(1, t + 1):
                    p += [int(e[j][1]), int(x[j])]
                found.append(p)
                steps_at_last = steps
                i = 1
                continue
            inl = rin[x[i]]
            Wp = Ws[i] if mutant == "prune_w_i" and i < len(Ws) else Ws[i - 1]
            top = t - 1 if (mode == SIMPLE and i == 1) or mutant == "top_off_stack" else t
            if mutant == "stack_63":
                top = min(top, i + 62)
            stack = stale if mutant == "no_pop" else x[i:top + 1]
            pos, c = -1, cur[i]
            while c < len(inl) and pos < 0:
                steps += 1
                if steps > cap:
                    return OVER, steps, steps
                for q in range(c, min(c + 64, len(inl))):
                    u = inl[q][0]
                    if Wp.get(u, 0) <= 0:
                        continue
                    if vertex_mode and ((i > 1 and u == src and not (mutant == "source_midwalk" and mode == ACYCLIC)) or u in stack):
                        continue
                    pos = q
                    break
                c += 64
            if pos < 0:
                i += 1
                if mutant == "cursor_reset" and i <= t:
                    cur[i] = 0
                continue
            cur[i] = pos + 1
            u, slot = inl[pos]
            if mutant == "m_mod_64":
                slot = A.mth_slot(off, adj, u, x[i], sum(1 for q in range(pos) if inl[q][0] == u), mutant)
                if slot is None:
                    return ("lost",), steps, steps
            key = slot if mutant == "trail_by_slot" else int(eid[slot])
            if mode == TRAIL and any(e[j][0] == key for j in range(i + 1, t + 1)):
                continue
            steps += 1
            if steps > cap:
                return OVER, steps, steps
            e[i] = (key, int(eid[slot]))
            x[i - 1] = u
            stale.append(u)
            i -= 1
            if i > 0:
                cur[i] = 0
    return found, steps, (steps_at_last if found else 0)


def search_model(V, off, adj, eid, rs, rd, min_hops, max_hops, k, mode, mutant=None, state=None, cap=None):
    """(counts, hops, lists, steps of the counting pass per row, steps of the emitting pass per row, rounds needed per row).  counts =
    min(a, k), -1 for a NULL row; a row without a lane takes no step.  `state` keeps every source's tables between calls on ONE graph."""
    state = {} if state is None else state
    if "rin" not in state:
        state["rin"] = A.in_lists(V, off, adj)
    rin = state["rin"]
    cap = cap if cap is not None else (ENDLESS_STEP_CAP if mutant in ("cursor_reset", "filter_first_k") else MUTANT_STEP_CAP if mutant else 1 << 24)
    counts, hops, lists, steps1, steps2, rounds = [], [], [], [], [], []
    for s, d in zip(np.asarray(rs).tolist(), np.asarray(rd).tolist()):
        if s < 0 or d < 0:
            counts.append(-1), hops.append(-1), lists.append(None), steps1.append(0), steps2.append(0), rounds.append(0)
            continue
        if s == d and off[s] == off[s + 1]:  # no lane: the empty walk or nothing
            one = min_hops == 0
            counts.append(1 if one else 0), hops.append(0 if one else -1), lists.append([[int(s)]] if one else None)
            steps1.append(0), steps2.append(0), rounds.append(0)
            continue
        Ws = state[s] = W.tables(V, rin, s, max_hops, None, state.get(s))
        R = rounds_needed(Ws, d, min_hops, max_hops, k, mutant)
        if mutant == "filter_first_k":
            got, a, b = _search_row(off, adj, eid, rin, Ws, s, d, min_hops, R, k, WALK, None, cap)
            got = got if got == OVER else [p for p in got if admitted(p, mode)]
        else:
            got, a, b = _search_row(off, adj, eid, rin, Ws, s, d, min_hops, R, k, mode, mutant, cap)
        if got == OVER or got == ("lost",):
            counts.append(got), hops.append(got), lists.append(got)
        else:
            counts.append(len(got)), hops.append(len(got[0]) // 2 if got else -1), lists.append(got or None)
        steps1.append(a), steps2.append(b), rounds.append(R)
    return counts, hops, lists, steps1, steps2, rounds


# ---- fixtures: (V, off, adj, eid, rs, rd) -------------------------------------------------------------------------------------
def with_shared_ids(fx, pairs):
    """The fixture with the edge ids of the slot pairs (a, b) made equal (an undirected edge's two directions)."""
    V, off, adj, eid, rs, rd = fx
    eid = eid.copy()
    for a, b in pairs:
        eid[b] = eid[a]
    return V, off, adj, eid, rs, rd


def undirected(V, edges, rows):
    """Every edge {u, v} as the slots u -> v and v -> u with ONE id, as the binder's undirected CTE gives them."""
    es = [u for u, v in edges] + [v for u, v in edges]
    ed = [v for u, v in edges] + [u for u, v in edges]
    V, off, adj, eid, rs, rd = A._fx(V, es, ed, rows)
    n = len(edges)
    eid = np.where(eid >= 1000 + n, eid - n, eid)  # (A.graph numbers an edge 1000 + its position in the edge list)
    return V, off, adj, eid, rs, rd


def in_list_positions(deg):
    """Four destinations whose in-lists have `deg` entries each, parents in id order, of which only some can be reached from the
    source s = 0 (walks of 2 edges): the last position; position 64 — the first of the second trip — where there is one, else 0;
    positions 3 and 40 (two in one trip); positions 62 and 66, or the last two (neighbouring trips, or the cursor's resume).
    The fifth row asks for a destination nobody reaches."""
    sets = [[deg - 1], [64 if deg > 64 else 0], [3, 40], [62, 66] if deg > 66 else [deg - 2, deg - 1]]
    es, ed, rows = [], [], []
    v = 1
    for live in sets:
        parents = list(range(v, v + deg))
        x = v + deg
        v = x + 1
        for j, p in enumerate(parents):
            es.append(p), ed.append(x)
            if j in live:
                es.append(0), ed.append(p)
        rows.append((0, x))
    rows.append((0, v))
    return A._fx(v + 1, es, ed, rows)


def chain_with_chord(n=64):
    """0 -> 1 -> ... -> n with the chord 30 -> 32: (0, n) has a walk of n - 1 and one of n edges, the stack is full at n = 64."""
    return A._fx(n + 1, list(range(n)) + [30], list(range(1, n + 1)) + [32], [(0, n), (1, n), (0, n - 1), (n, 0)])


def ring(n):
    """0 -> 1 -> ... -> n-1 -> 0: the one closed walk of n edges is simple and not acyclic; at n = 64 its test runs over 64 depths."""
    return A._fx(n, list(range(n)), [(i + 1) % n for i in range(n)], [(0, 0), (0, n - 1), (1, 0), (n // 2, n // 2)])


def parallel_run_back(P):
    """all_shortest_model.parallel_run(P) with the back edge x -> u: (u, x) has P^2 walks of 3 edges, P (P - 1) of them trails, and
    none of them is simple; the m-th of the P slots lies past position 64 of the in-list and of the out-list."""
    return W.with_edges(A.parallel_run(P), [3], [2], [(0, 3), (2, 3), (2, 2), (3, 3)])


def pair_and_triangle():
    """An undirected pair 0 - 1 and an undirected triangle 2 - 3 - 4: going back over an edge is no trail, though the slots differ."""
    return undirected(5, [(0, 1), (2, 3), (3, 4), (4, 2)], [(0, 0), (0, 1), (1, 1), (2, 2), (2, 3), (3, 2), (4, 4), (2, 4)])


def detour():
    """s = 0 -> d = 1 directly, a self-loop on d, and 0 -> 2 -> 3 -> 1: under {2,3} the shortest walk (0, 1, 1) repeats a vertex, the
    shortest simple one has 3 edges — and the row's distance, 1, is below lo.  Also 0 -> 4 -> 0 for closed rows."""
    return A._fx(5, [0, 1, 0, 2, 3, 0, 4], [1, 1, 2, 3, 1, 4, 0], [(0, 1), (0, 0), (2, 1), (1, 1), (4, 4), (0, 3)])


def random_shared(seed):
    """A random multigraph of at most 7 vertices and 12 slots; every second one gets the ids of its antiparallel slot pairs shared."""
    rng = np.random.default_rng(7000 + seed)
    V = int(rng.integers(3, 8))
    E = int(rng.integers(1, 13))
    es, ed = rng.integers(0, V, E), rng.integers(0, V, E)
    fx = A._fx(V, es, ed, [(s, d) for s in range(V) for d in range(V)])
    if seed % 2 == 0:
        return fx
    V, off, adj = fx[:3]
    u_of = A.slot_sources(V, off).tolist()
    pairs, used = [], set()
    for a in range(len(adj)):
        for b in range(a + 1, len(adj)):
            if a not in used and b not in used and u_of[a] == adj[b] and u_of[b] == adj[a] and u_of[a] != u_of[b]:
                pairs.append((a, b))
                used |= {a, b}
    return with_shared_ids(fx, pairs)


def gpu_fixtures():
    """name -> (fixture, ((min_hops, max_hops, the k values, the modes), ...)) the GPU file runs; the CPU file shows that they catch
    MUTANTS."""
    fx = {"tiny0": (A.tiny_multigraph(0), ((0, 3, (1, 3, K_ALL), MODES), (2, 4, (1, 3), MODES))),
          "chain64": (chain_with_chord(), ((0, MAX_HOPS, (1, 2, 3), MODES), (MAX_HOPS, MAX_HOPS, (1,), MODES))),
          "ring64": (ring(64), ((1, MAX_HOPS, (1, 2), MODES), (0, MAX_HOPS, (2,), MODES))),
          "ring5": (W.ring(5), ((0, 10, (1, 2, 3), MODES), (1, 10, (1, 3), MODES), (5, 5, (1,), MODES))),
          "self_loop": (W.self_loop(), ((0, 3, (1, K_ALL), MODES), (1, 3, (1, K_ALL), MODES), (2, 5, (4,), MODES))),
          "two_loops": (W.two_loops(), ((0, MAX_HOPS, (3, K_ALL), MODES), (1, 5, (K_ALL,), MODES), (2, 2, (1, 2, 3), MODES))),
          "pair_and_triangle": (pair_and_triangle(), ((0, 6, (1, K_ALL), MODES), (2, 4, (1, 2, K_ALL), MODES), (3, 3, (K_ALL,), MODES))),
          "detour": (detour(), ((2, 3, (1, 2, K_ALL), MODES), (0, 4, (1, K_ALL), MODES), (1, 2, (1,), MODES))),
          "parallel": (A.parallel_edges(), ((0, 3, (1, 9, 10, 11), MODES), (2, 2, (2, 9, 10), (TRAIL,))))}
    for deg in (63, 64, 65, 128, 129):
        fx["in_list_%d" % deg] = (in_list_positions(deg), ((0, 2, (1, 2, K_ALL), MODES), (2, 3, (1, 3), (ACYCLIC,))))
    for n in (63, 64, 65, 128, 129):
        fx["sources_%d" % n] = (A.many_sources(n), ((1, 3, (2,), MODES),))
    for P in (63, 64, 65, 129):
        fx["parallel_run_%d" % P] = (parallel_run_back(P), ((3, 3, (1, P, K_ALL), (TRAIL,)), (1, 3, (K_ALL,), (SIMPLE, ACYCLIC))))
    return fx
