"""The Python model of k_shortest_groups, SQL/PGQ's SHORTEST k GROUP (a helper of test_k_groups_cpu.py / test_k_groups_gpu.py).

The contract (include/pgq_hip.h).  For a row (src, dst), lo = min_hops, K = max_hops, g = groups, P = max_paths and a path mode:
    S            the sequence k_shortest_walks_mode defines for the mode with unlimited k (k_walks_model / path_modes_model): every
                 admitted walk of lo..K edges, shortest first, equal lengths by in-list positions read from the destination end.
    the lengths  t_1 < t_2 < ...: the lengths in [lo, K] with at least one admitted walk.  A length whose W_t[dst] is 0, a length all
                 of whose walks the mode refuses and a length below lo are no groups.
    A            the admitted walks of lengths t_1 .. t_min(g, number of lengths).
    the list     the first min(|A|, P) walks of A; P may cut inside a group, which is emitted as far as P goes.
    npaths = min(|A|, P); ngroups = the distinct lengths among the emitted walks; count = min(|A|, P + 1); len = the hops of the first
    walk, -1 without one.  No admitted walk: None, count 0, ngroups 0; a NULL endpoint: None, count -1.
The model is k_walks_model's tables and unranking (NONE / WALK) and path_modes_model's depth-first search (TRAIL / ACYCLIC / SIMPLE)
with their unlimited sequence cut as above.  Under a mode it also returns the steps of both passes the way search_model does: the
counting pass looks for P + 1 walks and ends behind the length that completed group g; the emitting pass repeats the search up to
the last walk it keeps.
The rounds: under NONE / WALK a row is open while it has seen fewer than g non-empty lengths and their walks' (saturating) sum is
<= P; under a mode a row closes at its distance d when lo <= d and either g == 1 or W_d[dst] > P, every other row stays open.  A
batch — 64 distinct sources that take a lane, in id order — runs rounds until round K, an empty queue, or no open row.

MUTANTS are the ways an implementation can go wrong that the GPU fixtures must notice."""
import numpy as np

import all_shortest_model as A
import k_walks_model as W
import path_modes_model as M

NONE, WALK, SIMPLE, TRAIL, ACYCLIC = M.NONE, M.WALK, M.SIMPLE, M.TRAIL, M.ACYCLIC
MODES = M.MODES
ALL_MODES = (NONE, WALK) + MODES
MODE_NAMES = M.MODE_NAMES
P_ALL = W.K_ALL
MAX_HOPS = W.MAX_HOPS
INT64_MAX = W.INT64_MAX
OVER = M.OVER

# mode_group_by_w         under a mode a length is a group when W_t[dst] > 0, although the mode refuses all its walks
# empty_length_group      a length without a walk uses up a group
# below_lo_group          a non-empty length below lo uses up a group
# groups_as_k             groups taken for k: the first g walks (a cut inside a group)
# cut_group_dropped       the group that max_paths cuts is left out whole
# ngroups_planned         ngroups counts the lengths of A, not the lengths among the emitted walks
# close_at_ge             a row is closed at cum >= P instead of cum > P: on a boundary the count stays P
# mode_close_at_distance  under a mode with g >= 2 a row is closed at its distance
# count_uncapped          count = |A| instead of min(|A|, P + 1)
MUTANTS = ("mode_group_by_w", "empty_length_group", "below_lo_group", "groups_as_k", "cut_group_dropped", "ngroups_planned", "close_at_ge",
           "mode_close_at_distance", "count_uncapped")


def _is_walk(mode):
    return mode in (NONE, WALK)


def _distance(Ws, d, K):
    return next((t for t in range(K + 1) if Ws[t].get(d, 0) > 0), None)


def _cut(per_len, g, P, mutant):
    """per_len: [(t, the admitted walks of t edges, or their number)] of the candidate lengths in order; an entry without a walk is
    no group.  -> (number kept per length [(t, take)], |A|, ngroups)."""
    size = lambda w: w if isinstance(w, int) else len(w)  # noqa: E731
    planned, total, seen = [], 0, 0
    for t, w in per_len:
        if seen >= g or (mutant == "close_at_ge" and total >= P):
            break
        if size(w) == 0 and mutant != "empty_length_group":
            continue
        seen += 1
        if size(w):
            planned.append((t, size(w)))
            total = min(total + size(w), INT64_MAX)
    if mutant == "groups_as_k":
        P = min(P, g)
    kept, left = [], P
    for t, w in planned:
        take = min(w, left)
        if take < w and mutant == "cut_group_dropped":
            take = 0
        if take > 0:
            kept.append((t, take))
        left -= take
    ngroups = len(planned) if mutant == "ngroups_planned" else len(kept)
    return kept, total, ngroups


def _walk_row(off, adj, eid, rin, Ws, s, d, lo, K, g, P, mutant):
    if mutant == "below_lo_group":  # (a non-empty length below lo: a group that yields nothing)
        g = max(g - sum(1 for t in range(lo) if Ws[t].get(d, 0) > 0), 0)
    kept, total, ngroups = _cut([(t, Ws[t].get(d, 0)) for t in range(lo, K + 1)], g, P, mutant)
    lists = [W.unrank(off, adj, eid, rin, Ws, s, d, t, r) for t, take in kept for r in range(take)]
    return lists, total, ngroups


def _search_row(off, adj, eid, rin, Ws, src, dst, lo, K, g, P, mode, mutant, cap):
    """path_modes_model._search_row with the group rule: (the walks found — P + 1 at most —, the lengths that counted as groups,
    steps of the counting pass, steps when walk number i was found)."""
    vertex_mode = mode in (SIMPLE, ACYCLIC)
    want = P + 1
    found, at, steps, seen = [], [], 0, 0
    d0 = _distance(Ws, dst, K)
    first = 0 if mutant == "below_lo_group" else lo
    for t in range(first, K + 1):
        if len(found) >= want or seen >= g:
            break
        if mutant == "mode_close_at_distance" and d0 is not None and lo <= d0 < t:
            break
        if Ws[t].get(dst, 0) <= 0:
            seen += 1 if mutant == "empty_length_group" else 0
            continue
        if t < lo:
            seen += 1
            continue
        fresh = True
        if mutant == "mode_group_by_w":
            fresh, seen = False, seen + 1
        x, e, cur = [None] * (t + 1), [None] * (t + 1), [0] * (t + 1)
        i = t
        x[t] = dst
        while i <= t and len(found) < want:
            if i == 0:
                if t > 0 and x[0] != src:
                    return ("lost",), 0, steps, []
                p = [int(x[0])]
                for j in range(1, t + 1):
                    p += [int(e[j]), int(x[j])]
                found.append(p)
                at.append(steps)
                if fresh:
                    fresh, seen = False, seen + 1
                i = 1
                continue
            inl = rin[x[i]]
            Wp = Ws[i - 1]
            top = t - 1 if mode == SIMPLE and i == 1 else t
            stack = x[i:top + 1]
            pos, c = -1, cur[i]
            while c < len(inl) and pos < 0:
                steps += 1
                if steps > cap:
                    return OVER, 0, steps, []
                for q in range(c, min(c + 64, len(inl))):
                    u = inl[q][0]
                    if Wp.get(u, 0) <= 0:
                        continue
                    if vertex_mode and ((i > 1 and u == src) or u in stack):
                        continue
                    pos = q
                    break
                c += 64
            if pos < 0:
                i += 1
                continue
            cur[i] = pos + 1
            u, slot = inl[pos]
            key = int(eid[slot])
            if mode == TRAIL and any(e[j] == key for j in range(i + 1, t + 1)):
                continue
            steps += 1
            if steps > cap:
                return OVER, 0, steps, []
            e[i] = key
            x[i - 1] = u
            i -= 1
            if i > 0:
                cur[i] = 0
    return found, seen, steps, at


def _mode_row(off, adj, eid, rin, Ws, s, d, lo, K, g, P, mode, mutant, cap):
    """-> (lists, count, ngroups, steps of the counting pass, steps of the emitting pass)"""
    if mutant == "count_uncapped":
        full = _search_row(off, adj, eid, rin, Ws, s, d, lo, K, g, P_ALL, mode, None, cap)[0]
    found, seen, steps, at = _search_row(off, adj, eid, rin, Ws, s, d, lo, K, g, P, mode, mutant, cap)
    if found in (OVER, ("lost",)):
        return found, found, found, steps, steps
    per_len = []
    for p in found:
        if per_len and per_len[-1][0] == len(p) // 2:
            per_len[-1][1].append(p)
        else:
            per_len.append((len(p) // 2, [p]))
    kept, total, ngroups = _cut(per_len, g, P, mutant if mutant in ("groups_as_k", "cut_group_dropped", "ngroups_planned") else None)
    lists = [p for t, take in kept for p in dict(per_len)[t][:take]]
    count = len(full) if mutant == "count_uncapped" else len(found)
    return lists, count, ngroups, steps, (at[len(lists) - 1] if lists else 0)


def _open_after(Ws, d, lo, t, g, P, mode, mutant):
    """Is the row still open behind round t?"""
    if _is_walk(mode):
        seen = cum = 0
        for tt in range(lo, t + 1):
            if seen >= g or (cum >= P if mutant == "close_at_ge" else cum > P):
                break
            w = Ws[tt].get(d, 0)
            if w > 0:
                seen, cum = seen + 1, min(cum + w, INT64_MAX)
        return seen < g and not (cum >= P if mutant == "close_at_ge" else cum > P)
    d0 = _distance(Ws, d, t)
    if d0 is None or d0 < lo:
        return True
    return not (g == 1 or Ws[d0].get(d, 0) > P or mutant == "mode_close_at_distance")


def batch_rounds(V, off, adj, rs, rd, lo, K, g, P, mode, mutant=None, state=None):
    """The rounds the call runs, summed over its batches (pgq_stats_t.levels)."""
    state = {} if state is None else state
    rin = state.setdefault("rin", A.in_lists(V, off, adj))
    rows = [(s, d) for s, d in zip(np.asarray(rs).tolist(), np.asarray(rd).tolist())
            if s >= 0 and d >= 0 and off[s] < off[s + 1] and len(rin[d]) > 0]
    sources = sorted({s for s, _ in rows})
    total = 0
    for b in range(0, len(sources), 64):
        batch = set(sources[b:b + 64])
        mine = [(s, d) for s, d in rows if s in batch]
        Wb = {}
        for s in batch:
            Wb[s] = state[s] = W.tables(V, rin, s, K, None, state.get(s))
        t = 0
        while t < K and any(Wb[s][t] for s in batch) and any(_open_after(Wb[s], d, lo, t, g, P, mode, mutant) for s, d in mine):
            t += 1
        total += t
    return total


def groups_model(V, off, adj, eid, rs, rd, lo, K, groups, max_paths, mode, mutant=None, state=None, cap=None):
    """A dict: lists (None where there is none), npaths, ngroups, count (-1: a NULL row), len (-1: none) per row; rounds (of the
    whole call); under a mode steps1 / steps2 per row (the counting and the emitting pass), zeros otherwise.  `state` keeps every
    source's tables between calls on ONE graph."""
    state = {} if state is None else state
    rin = state.setdefault("rin", A.in_lists(V, off, adj))
    cap = cap if cap is not None else 1 << 24
    out = {k: [] for k in ("lists", "npaths", "ngroups", "count", "len", "steps1", "steps2")}

    def row(lists, count, ngroups, s1=0, s2=0):
        if lists in (OVER, ("lost",)):
            for k in ("lists", "npaths", "ngroups", "count", "len"):
                out[k].append(lists)
        else:
            out["lists"].append(lists or None), out["npaths"].append(len(lists)), out["ngroups"].append(ngroups)
            out["count"].append(count), out["len"].append(len(lists[0]) // 2 if lists else -1)
        out["steps1"].append(s1), out["steps2"].append(s2)

    for s, d in zip(np.asarray(rs).tolist(), np.asarray(rd).tolist()):
        if s < 0 or d < 0:
            row([], -1, 0)
        elif s == d and off[s] == off[s + 1]:  # no lane: the empty walk or nothing
            row([[int(s)]] if lo == 0 else [], 1 if lo == 0 else 0, 1 if lo == 0 else 0)
        else:
            Ws = state[s] = W.tables(V, rin, s, K, None, state.get(s))
            if _is_walk(mode):
                lists, total, ngroups = _walk_row(off, adj, eid, rin, Ws, s, d, lo, K, groups, max_paths, mutant)
                row(lists, total if mutant == "count_uncapped" else min(total, max_paths + 1), ngroups)
            else:
                row(*_mode_row(off, adj, eid, rin, Ws, s, d, lo, K, groups, max_paths, mode, mutant, cap))
    out["rounds"] = batch_rounds(V, off, adj, rs, rd, lo, K, groups, max_paths, mode, mutant, state)
    return out


def brute_groups(V, off, adj, eid, rs, rd, lo, K, groups, max_paths, mode, brute=None):
    """The contract from an enumeration of every walk of at most K edges (k_walks_model.brute_force), filtered by the mode
    (path_modes_model.admitted) and grouped by length: lists, npaths, ngroups, count, len per row."""
    brute = {} if brute is None else brute
    out = {k: [] for k in ("lists", "npaths", "ngroups", "count", "len")}
    for s, d in zip(np.asarray(rs).tolist(), np.asarray(rd).tolist()):
        if s not in brute:
            brute[s] = W.brute_force(V, off, adj, eid, s, K)
        walks = [p for p in brute[s][d] if len(p) // 2 >= lo and M.admitted(p, mode)]
        lengths = sorted({len(p) for p in walks})[:groups]
        a = [p for p in walks if len(p) in lengths]
        got = a[:max_paths]
        out["lists"].append(got or None), out["npaths"].append(len(got)), out["ngroups"].append(len({len(p) for p in got}))
        out["count"].append(min(len(a), max_paths + 1)), out["len"].append(len(got[0]) // 2 if got else -1)
    return out


# ---- fixtures: (V, off, adj, eid, rs, rd) -------------------------------------------------------------------------------------
def second_group_positions(deg):
    """Two destinations whose in-lists have `deg` entries, parents in id order.  The source 0 reaches parent 3 of each directly (one
    walk of 2 edges: group 1) and, over the middle vertex 1, ONE other parent (a walk of 3 edges: group 2's only parent): the last
    slot for the first destination; position 64 — the head of the second trip — where there is one, else position 0, for the second."""
    es, ed, rows = [0], [1], []
    v = 2
    for late in (deg - 1, 64 if deg > 64 else 0):
        parents = list(range(v, v + deg))
        x = v + deg
        v = x + 1
        for p in parents:
            es.append(p), ed.append(x)
        es.append(0), ed.append(parents[3])
        es.append(1), ed.append(parents[late])
        rows.append((0, x))
    rows.append((0, v))  # nobody reaches it
    return A._fx(v + 1, es, ed, rows)


def bipartite():
    """0 -> {1, 3} -> 2 and back 2 -> 1: (0, 2) has walks of 2, 4, 6, ... edges and none of an odd length; (0, 1) of 1, 3, 5, ..."""
    return A._fx(4, [0, 0, 1, 3, 2], [1, 3, 2, 2, 1], [(0, 2), (0, 1), (1, 1), (2, 2), (3, 1), (2, 0)])


def boundary():
    """0 =3 parallel edges=> 1 -> 2 with a self-loop on 2: (0, 2) has exactly 3 walks of every length >= 2.  TRAIL admits the lengths
    2 and 3, the vertex modes the length 2 alone."""
    return A._fx(3, [0, 0, 0, 1, 2], [1, 1, 1, 2, 2], [(0, 2), (0, 1), (2, 2), (1, 2)])


def gap():
    """0 -> 1 with a self-loop on 1, and 0 -> 2 -> 3 -> 4 -> 1.  (0, 1): the walk of 3 edges takes the loop twice — no trail — between
    the trails of 1, 2 and 4 edges; the vertex modes admit 1 and 4 edges and refuse 2 and 3 between them."""
    return A._fx(5, [0, 1, 0, 2, 3, 4], [1, 1, 2, 3, 4, 1], [(0, 1), (0, 4), (1, 1), (2, 1), (4, 0)])


G_ALL = MAX_HOPS + 1  # more groups than a row can have


def gpu_fixtures():
    """name -> (fixture, ((min_hops, max_hops, the groups, the max_paths values, the modes), ...)) the GPU file runs; the CPU file
    shows that they catch MUTANTS."""
    walk = (WALK,)
    fx = {"tiny0": (A.tiny_multigraph(0), ((0, 3, (1, 2, G_ALL), (1, 3, P_ALL), ALL_MODES), (2, 4, (1, 2), (2, P_ALL), ALL_MODES))),
          "bipartite": (bipartite(), ((0, 6, (1, 2, 3, 4), (1, P_ALL), ALL_MODES), (3, 7, (1, 2), (2, P_ALL), (NONE, TRAIL)), (1, 1, (2,), (4,), walk))),
          "ring5": (W.ring(5), ((0, 12, (1, 2, 3), (1, P_ALL), ALL_MODES), (1, 12, (1, 2, G_ALL), (2, P_ALL), ALL_MODES), (3, 6, (1,), (1,), walk))),
          "ring64": (M.ring(64), ((1, MAX_HOPS, (1, 2), (3,), (WALK, SIMPLE, ACYCLIC)), (0, MAX_HOPS, (2,), (P_ALL,), (WALK, SIMPLE, TRAIL)))),
          "self_loop": (W.self_loop(), ((0, 4, (1, 2, 4, G_ALL), (1, 3, P_ALL), ALL_MODES), (1, 3, (1, 2), (P_ALL,), ALL_MODES), (2, 5, (2,), (1, 2, 3), walk))),
          # |A| = 6 at g = 2, a group boundary at 3: one below, at, one above each; K = 2: no later length behind the boundary
          "boundary": (boundary(), ((0, 5, (1, 2, 3), (2, 3, 4, 5, 6, 7), ALL_MODES), (2, 2, (1, 2), (2, 3, 4), ALL_MODES), (2, 3, (2,), (3, 6), walk),
                                    (4, 5, (1, 2), (3,), (WALK, TRAIL)))),
          "gap": (gap(), ((0, 5, (1, 2, 3, 4), (1, 2, P_ALL), ALL_MODES), (1, 4, (2, 3), (2, P_ALL), MODES), (2, 5, (1, 2), (P_ALL,), ALL_MODES))),
          "detour": (M.detour(), ((2, 3, (1, 2), (1, P_ALL), ALL_MODES), (0, 4, (1, 2, 3), (2, P_ALL), ALL_MODES))),
          "pair_and_triangle": (M.pair_and_triangle(), ((0, 6, (1, 2, 3), (1, P_ALL), MODES), (2, 4, (1, 2), (2, P_ALL), ALL_MODES))),
          "chain64": (M.chain_with_chord(), ((0, MAX_HOPS, (1, 2, 3), (1, P_ALL), ALL_MODES), (MAX_HOPS, MAX_HOPS, (1,), (1,), ALL_MODES)))}
    for deg in (63, 64, 65, 128, 129):
        fx["in_list_%d" % deg] = (second_group_positions(deg), ((0, 3, (1, 2, 3), (1, 2, P_ALL), ALL_MODES), (3, 3, (1,), (P_ALL,), (WALK, ACYCLIC))))
    for n in (63, 64, 65, 128, 129):
        fx["sources_%d" % n] = (A.many_sources(n), ((1, 3, (1, 2), (2, P_ALL), (WALK, SIMPLE)),))
    for P in (63, 64, 65, 129):
        fx["parallel_run_%d" % P] = (M.parallel_run_back(P), ((3, 3, (1,), (P - 1, P), (WALK, TRAIL)), (1, 3, (1, 2), (P + 1,), (TRAIL, SIMPLE))))
    return fx
