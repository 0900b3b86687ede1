"""The Python model of walk_length (a helper of test_walk_length_cpu.py / test_walk_length_gpu.py).

The contract (include/pgq_hip.h).  With W_t as walk_count defines it (k_walks_model.py), the result of a row (src, dst) is the
smallest t in [lower, upper] with W_t[dst] > 0, and -1 (NULL) when there is none or an endpoint is NULL.  src == dst is not special.

The model follows the call's two stages, so that it can also say what the call's statistics must be:
  stage 1   the distance d within `upper`: rows with lower <= d answer d, rows farther apart than upper or unreachable answer -1,
            rows with 0 <= d < lower are left (`rest`);
  stage 2   the rows left, lane-assigned by source (a source takes a lane when it has an out-edge and its row's destination an
            in-edge; lanes in vertex order), in batches of 64 lanes.  Round t: M_t[x] = OR over in-slots (u, x) of M_{t-1}[u], with
            NO visited set.  `push` expands the queue of round t - 1; `pull` walks every vertex's in-list by the upload's work
            partition (`partition`: parts of ordinary vertices, hubs slice by slice), 128 slots per trip, and leaves a list once its
            word holds every lane of the batch.  A row takes t when t >= lower and M_t[dst] has its lane's bit.  The rounds stop
            behind round `upper`, when no row of the batch is open, or when nothing is active.
`solve` returns (answers, stats): stats = rest, batches, levels, push_levels, pull_levels, edges (adjacency entries the rounds
walked; under `pull` exact for graphs without hubs — a hub's slices see each other's words in no fixed order).

MUTANTS are the ways an implementation can go wrong that the GPU fixtures must notice, in the answers or in the statistics."""
import numpy as np

import all_shortest_model as A
import k_walks_model as KW

LC = 64
MAX_HOPS = KW.MAX_HOPS
DEFAULT_LAYOUT = (1024, 4096)  # part_weight, hub_chunk as the library ships them
SMALL_LAYOUT = (64, 64)        # the smallest values the upload accepts: in-degrees above 64 are hubs, their slices 64 entries
PULL_DIV = 16                  # walk_length_pull_div as shipped

# visited            a visited set: M_t[x] loses the lanes that reached x before (a BFS level)
# lower_ignored      the distance returned whatever `lower`
# t_gt_lower         a row takes t only when t > lower
# src_eq_dst_zero    src == dst answered 0 also when lower >= 1
# trip_last_slot     pull: the last slot of every 64-slot trip dropped
# hub_last_slice     pull: a hub's last slice dropped
# exit_all_ones      pull: the early exit tests ~0 instead of the batch's lanes (a partial batch walks every list to its end)
# far_rows_answered  stage 1 not held to `upper`: a row farther apart answers its distance
# stop_early         the stop at "nothing active" taken one round early: from the queue's out-edges, before the round that finds it
# masks_not_zeroed   the two mask arrays not zeroed between batches
MUTANTS = ("visited", "lower_ignored", "t_gt_lower", "src_eq_dst_zero", "trip_last_slot", "hub_last_slice", "exit_all_ones",
           "far_rows_answered", "stop_early", "masks_not_zeroed")


def partition(roff, part_weight, hub_chunk):
    """pgq_csr_pull_layout's description restated: (parts [(begin, end)], hubs [vertex], slices [(vertex, begin, end)]).  Hubs are
    the vertices with more than C = max(64, hub_chunk) in-edges; a part is a contiguous vertex range without a hub, of at most 16
    vertices and at most max(64, part_weight) of (in-degree + 8 per vertex), packed greedily inside runs of 256 vertices; a hub's
    in-list is cut into slices of max(64, C / 4) entries."""
    W, C = max(64, part_weight), max(64, hub_chunk)
    S = max(64, C // 4)
    V = len(roff) - 1
    parts, hubs = [], []
    for v0 in range(0, V, 256):
        v1 = min(V, v0 + 256)
        begin, acc = v0, 0
        for v in range(v0, v1):
            d = int(roff[v + 1] - roff[v])
            if d > C:
                hubs.append(v)
                if v > begin:
                    parts.append((begin, v))
                begin, acc = v + 1, 0
                continue
            if v > begin and (acc + d + 8 > W or v - begin >= 16):
                parts.append((begin, v))
                begin, acc = v, 0
            acc += d + 8
        if v1 > begin:
            parts.append((begin, v1))
    slices = [(v, b, min(b + S, int(roff[v + 1]))) for v in hubs for b in range(int(roff[v]), int(roff[v + 1]), S)]
    return parts, hubs, slices


class Graph:
    def __init__(self, V, off, adj):
        self.V, self.E = V, len(adj)
        self.out = [np.asarray(adj[off[v]:off[v + 1]]).tolist() for v in range(V)]
        rin = A.in_lists(V, off, adj)
        self.radj = [u for x in range(V) for u, _ in rin[x]]
        self.roff = np.cumsum([0] + [len(rin[x]) for x in range(V)]).tolist()
        self._dist, self._parts = {}, {}

    def dist(self, s):
        """Every distance from s (unbounded)."""
        if s not in self._dist:
            d, frontier = {s: 0}, [s]
            while frontier:
                nxt = []
                for v in frontier:
                    for x in self.out[v]:
                        if x not in d:
                            d[x] = d[v] + 1
                            nxt.append(x)
                frontier = nxt
            self._dist[s] = d
        return self._dist[s]

    def parts(self, layout):
        if layout not in self._parts:
            self._parts[layout] = partition(self.roff, *layout)
        return self._parts[layout]


def _or_list(g, prev, b, e, exit_mask, mutant, stats):
    acc = 0
    for j0 in range(b, e, 128):
        for k in range(j0, min(j0 + 128, e)):
            if mutant == "trip_last_slot" and (k - b) % 64 == 63:
                continue
            acc |= prev.get(g.radj[k], 0)
        stats["edges"] += min(128, e - j0)
        if j0 + 128 < e and (acc & exit_mask) == exit_mask:
            break
    return acc


def _pull(g, prev, cur, exit_mask, layout, mutant, stats):
    parts, hubs, slices = g.parts(layout)
    for begin, end in parts:
        for x in range(begin, end):
            cur[x] = _or_list(g, prev, g.roff[x], g.roff[x + 1], exit_mask, mutant, stats) if g.roff[x + 1] > g.roff[x] else 0
    for x in hubs:
        cur[x] = 0
    for x, b, e in slices:
        if mutant == "hub_last_slice" and e == g.roff[x + 1]:
            continue
        cur[x] |= _or_list(g, prev, b, e, exit_mask, mutant, stats)


def _batch(g, lanes, rows, ans, lo, hi, direction, layout, mutant, marr, stats):
    """rows: (row, lane, dst) of the batch; marr: the two mask arrays (dicts vertex -> word) as the batch before left them."""
    full = (1 << len(lanes)) - 1
    exit_mask = (1 << 64) - 1 if mutant == "exit_all_ones" else full
    stats["batches"] += 1
    if mutant != "masks_not_zeroed":
        marr[0].clear(), marr[1].clear()
    for l, v in enumerate(lanes):
        marr[0][v] = 1 << l
    seen = dict(marr[0])
    queue = list(lanes)
    steps = sum(len(g.out[v]) for v in queue)
    active, dense = len(queue), direction == "pull"
    is_open = [True] * len(rows)
    t = 1
    while t <= hi and active > 0 and any(is_open):
        prev, cur = marr[(t - 1) & 1], marr[t & 1]
        if mutant == "stop_early" and sum(len(g.out[v]) for v, m in prev.items() if m) == 0:
            break
        if direction == "auto" and steps > g.E / PULL_DIV:
            dense = True
        if dense:
            _pull(g, prev, cur, exit_mask, layout, mutant, stats)
            stats["pull_levels"] += 1
        else:
            cur.clear()
            for v in queue:
                for x in g.out[v]:
                    cur[x] = cur.get(x, 0) | prev[v]
                stats["edges"] += len(g.out[v])
            stats["push_levels"] += 1
        if mutant == "visited":
            for x in list(cur):
                cur[x] &= ~seen.get(x, 0)
                seen[x] = seen.get(x, 0) | cur[x]
        queue = [x for x, m in cur.items() if m]
        active = len(queue)
        steps = 0 if dense else sum(len(g.out[v]) for v in queue)
        for k, (row, lane, dst) in enumerate(rows):
            if is_open[k] and (t > lo if mutant == "t_gt_lower" else t >= lo) and (cur.get(dst, 0) >> lane) & 1:
                ans[row], is_open[k] = t, False
        stats["levels"] += 1
        t += 1


def solve(V, off, adj, rs, rd, lo, hi, direction="push", layout=DEFAULT_LAYOUT, mutant=None, graph=None):
    """(answers, stats).  direction: "push", "pull" or "auto" (walk_length_pull = 0, 1, 2); layout: (part_weight, hub_chunk) of the
    upload; graph: a Graph of (V, off, adj) to reuse."""
    g = graph or Graph(V, off, adj)
    stats = dict(rest=0, batches=0, levels=0, push_levels=0, pull_levels=0, edges=0)
    ans, rest = [], []
    for i, (s, d) in enumerate(zip(np.asarray(rs).tolist(), np.asarray(rd).tolist())):
        ans.append(-1)
        if s < 0 or d < 0:
            continue
        dd = g.dist(s).get(d, -1)
        if mutant == "src_eq_dst_zero" and s == d:
            ans[i] = 0
        elif dd < 0 or (dd > hi and mutant != "far_rows_answered"):
            pass
        elif dd >= lo or mutant == "lower_ignored":
            ans[i] = dd
        else:
            rest.append((i, s, d))
    stats["rest"] = len(rest)
    laned = [(i, s, d) for i, s, d in rest if g.out[s] and g.roff[d + 1] > g.roff[d]]
    sources = sorted({s for _, s, _ in laned})
    lane_of = {s: k for k, s in enumerate(sources)}
    marr = ({}, {})
    for base in range(0, len(sources), LC):
        lanes = sources[base:base + LC]
        rows = [(i, lane_of[s] - base, d) for i, s, d in laned if base <= lane_of[s] < base + LC]
        _batch(g, lanes, rows, ans, lo, hi, direction, layout, mutant, marr, stats)
    return ans, stats


def reference(V, off, adj, rs, rd, lo, hi, tables=None):
    """The contract itself, from walk_count's tables: the smallest t in [lo, hi] with W_t[dst] > 0."""
    rin = A.in_lists(V, off, adj)
    tables = {} if tables is None else tables
    out = []
    for s, d in zip(np.asarray(rs).tolist(), np.asarray(rd).tolist()):
        if s < 0 or d < 0:
            out.append(-1)
            continue
        Ws = tables[s] = KW.tables(V, rin, s, hi, None, tables.get(s))
        out.append(next((t for t in range(lo, hi + 1) if Ws[t].get(d, 0) > 0), -1))
    return out


# ---- fixtures: (V, off, adj, eid, rs, rd) -------------------------------------------------------------------------------------
def pair():
    """0 <-> 1: (0, 1) has walks of 1, 3, 5, ... edges, (0, 0) of 0, 2, 4, ..."""
    return A._fx(2, [0, 1], [1, 0], [(0, 1), (1, 0), (0, 0), (1, 1)])


def chain3():
    """0 -> 1 -> 2: the rounds of (0, 2) under {3,5} end when nothing is active, behind round 3."""
    return A._fx(3, [0, 1], [1, 2], [(0, 2)])


def last_slot_gadget(deg):
    """x with `deg` in-slots: s (the first, d = 1) and deg - 1 parents p_j, of which only the LAST is reachable (s -> a -> p_last):
    at round 3 the one live parent of x sits in its in-list's last slot.  Rows: (s, x) — {2,2} none, {2,3} 3 — and (a, x)."""
    s, a, x, p0 = 0, 1, 2, 3
    ps = list(range(p0, p0 + deg - 1))
    es = [s, s, a] + ps
    ed = [x, a, ps[-1]] + [x] * len(ps)
    return A._fx(p0 + deg - 1, es, ed, [(s, x), (a, x), (s, ps[-1])])


def wide_exit(deg=300):
    """Two sources that both reach every one of y's `deg` in-neighbours, and y -> s0: under a pull the batch's two lanes are
    complete after y's first trip; a walk to the list's end shows in the edge count alone."""
    s0, s1, q0 = 0, 1, 2
    y = q0 + deg
    qs = list(range(q0, y))
    es = [s0] * deg + [s1] * deg + qs + [y]
    ed = qs + qs + [y] * deg + [s0]
    return A._fx(y + 1, es, ed, [(s0, y), (s1, y), (s0, s0)])


def many_sources(n, V=150):
    """A.many_sources' graph with a ring through every vertex (each has an out-edge and an in-edge: every source takes a lane) and
    a closed row per source in front of its rows: n distinct sources among the rows left under lower >= 1."""
    fx = A.many_sources(n, V)
    rows = [(s, s) for s in range(n)] + list(zip(fx[4].tolist(), fx[5].tolist()))
    return KW.with_edges(fx, list(range(V)), [(v + 1) % V for v in range(V)], rows)


def random_rows(V=300, E=2000, rows=2000, seed=21):
    """A random multigraph; every tenth row closed (src == dst)."""
    rng = np.random.default_rng(seed)
    es, ed = rng.integers(0, V, E), rng.integers(0, V, E)
    rs, rd = rng.integers(0, V, rows), rng.integers(0, V, rows)
    rd[::10] = rs[::10]
    return A._fx(V, es, ed, list(zip(rs.tolist(), rd.tolist())))


RANDOM_BOUNDS = ((0, 3), (1, 3), (2, 4), (3, 3), (5, MAX_HOPS))
LIST_DEGREES = (63, 64, 65, 127, 128, 129)
SOURCE_COUNTS = (1, 63, 64, 65, 128, 129)


def gpu_fixtures():
    """name -> (fixture, the (lower, upper) bounds, the upload layouts) the GPU file runs, each under push, pull and auto; the CPU
    file shows that they catch MUTANTS."""
    both = (DEFAULT_LAYOUT, SMALL_LAYOUT)
    fx = {"ring5": (KW.ring(5), ((1, 4), (1, 5), (6, 10), (0, 3)), (DEFAULT_LAYOUT,)),
          "self_loop": (KW.self_loop(), ((1, 1), (0, 3), (2, 5)), (DEFAULT_LAYOUT,)),
          "pair": (pair(), ((2, 2), (2, 3), (0, 1)), (DEFAULT_LAYOUT,)),
          "chain3": (chain3(), ((3, 5), (2, 5)), (DEFAULT_LAYOUT,)),
          "two_loops": (KW.two_loops(), ((1, MAX_HOPS), (0, 62), (5, MAX_HOPS)), (DEFAULT_LAYOUT,)),
          "loops_and_fan": (KW.loops_and_fan(), ((1, 62), (2, MAX_HOPS), (0, 3)), (DEFAULT_LAYOUT,)),
          "wide_exit": (wide_exit(), ((3, 5),), (DEFAULT_LAYOUT,)),
          "random": (random_rows(), RANDOM_BOUNDS, both)}
    for deg in LIST_DEGREES:
        fx["last_slot_%d" % deg] = (last_slot_gadget(deg), ((2, 2), (2, 3)), both)
    for n in SOURCE_COUNTS:
        fx["sources_%d" % n] = (many_sources(n), ((1, 3), (2, 4)), (DEFAULT_LAYOUT,))
    return fx
