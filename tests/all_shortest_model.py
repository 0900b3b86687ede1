"""The Python model of shortestpath_count and all_shortestpaths (a helper of test_all_shortest_cpu.py / test_all_shortest_gpu.py).

The contract (include/pgq_hip.h).  For a row (src, dst): L[v] = the BFS level of v from src, d = L[dst];
    sigma[src] = 1,  sigma[x] = min(INT64_MAX, sum of sigma[u] over the in-slots (u, x) with L[u] = L[x] - 1)
Parallel edges are separate slots and count separately.  count = sigma[dst]: 1 for src == dst, 0 when dst is unreachable or
d > max_hops, -1 (NULL) for a NULL endpoint.  The lists are the first min(sigma[dst], max_paths) shortest paths, each
[x_0, e_1, x_1, ..., e_d, x_d]; path number r is found by unranking: x_d = dst, and at step t the in-list of x_t is scanned in its
stored order — by (parent id, forward slot) — and for every in-slot (u, x_t) with L[u] = t - 1: r < sigma[u] takes the slot, else
r -= sigma[u].  src == dst gives [[src]]; NULL endpoints, unreachable rows and rows beyond the bound give None.

Plain Python integers, so that nothing here can wrap.  `brute_force` enumerates every walk of d edges instead.  MUTANTS are the
ways an implementation can go wrong that the fixtures must notice; the fixtures of the GPU tests are built here too, so that
the CPU tests can show that they do."""
import numpy as np

INT64_MAX = (1 << 63) - 1
MAX_PATHS_ALL = (1 << 31) - 1

# wrap          the sum wraps as a signed 64-bit add instead of saturating
# any_level     the level test on a parent is dropped: any in-neighbour that has been reached counts.  (Literally "from any EARLIER
#               level" cannot differ: an edge (u, x) gives L[x] <= L[u] + 1, so no in-neighbour lies below level L[x] - 1.  What an
#               implementation can get wrong is to admit a parent that is NOT on an earlier level; sigma is evaluated in (level,
#               vertex id) order, so a same-level parent with a smaller id brings its sigma along.)
# slot_order    candidates ordered by (which of the parent's parallel slots, parent) instead of (parent, slot)
# collapse      parallel edges counted once
# first_slot    the edge of the taken in-slot is the parent's FIRST slot into x_t, not its m-th
# no_bound      max_hops ignored
# paths_plus_1  one path more than max_paths
# m_mod_64      which of the parent's slots into x_t the taken in-slot is, counted modulo 64
# slot_first_64 the parent's m-th slot into x_t searched in the first 64 entries of its out-list only
MUTANTS = ("wrap", "any_level", "slot_order", "collapse", "first_slot", "no_bound", "paths_plus_1", "m_mod_64", "slot_first_64")


def graph(V, es, ed, eid_base=1000):
    """(off, adj, eid) in slot order: a stable sort by source; edge ids are eid_base + the edge's position in (es, ed), so that an
    id is never its slot number."""
    es, ed = np.asarray(es, dtype=np.int64), np.asarray(ed, dtype=np.int64)
    order = np.argsort(es, kind="stable")
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(es, minlength=V), out=off[1:])
    return off, ed[order].copy(), (eid_base + order).astype(np.int64)


def slot_sources(V, off):
    return np.repeat(np.arange(V, dtype=np.int64), np.diff(off))


def in_lists(V, off, adj):
    """Per vertex its in-slots (parent, forward slot) in the reverse CSR's order: the forward slots stably sorted by target."""
    u_of = slot_sources(V, off).tolist()
    rin = [[] for _ in range(V)]
    for slot, x in enumerate(adj.tolist()):
        rin[x].append((u_of[slot], slot))
    return rin


def bfs_levels(V, off, adj, src):
    L = [-1] * V
    L[src] = 0
    front = [src]
    while front:
        nxt = []
        for v in front:
            for n in adj[off[v]:off[v + 1]].tolist():
                if L[n] < 0:
                    L[n] = L[v] + 1
                    nxt.append(n)
        front = nxt
    return L


def _add(a, b, mutant):
    s = a + b
    if mutant == "wrap":
        return (s + (1 << 63)) % (1 << 64) - (1 << 63)
    return min(s, INT64_MAX)


def _parents(rin, L, x, mutant):
    """The in-slots of x that count, as (parent, slot, m) in scan order; m = which of the parent's slots into x this is."""
    out, seen = [], {}
    for u, slot in rin[x]:
        m = seen.get(u, 0)
        seen[u] = m + 1
        on_level = L[u] >= 0 if mutant == "any_level" else L[u] == L[x] - 1
        if not on_level or (mutant == "collapse" and m > 0):
            continue
        out.append((u, slot, m))
    if mutant == "slot_order":
        out.sort(key=lambda c: (c[2], c[0]))
    return out


def sigmas(V, rin, L, src, mutant=None):
    sigma = [0] * V
    sigma[src] = 1
    for x in sorted((v for v in range(V) if L[v] > 0), key=lambda v: (L[v], v)):
        acc = 0
        for u, _, _ in _parents(rin, L, x, mutant):
            acc = _add(acc, sigma[u], mutant)
        sigma[x] = acc
    return sigma


def mth_slot(off, adj, u, x, m, mutant=None):
    """The m-th slot of u's out-list into x, as an implementation finds it that walks the out-list; None when it finds none."""
    if mutant == "m_mod_64":
        m %= 64
    end = min(off[u + 1], off[u] + 64) if mutant == "slot_first_64" else off[u + 1]
    into = [s for s in range(off[u], end) if adj[s] == x]
    return into[m] if m < len(into) else None


def unrank(V, off, adj, eid, rin, L, sigma, src, dst, r, mutant=None):
    """Path number r of the row, or ("lost",) when a (mutant) walk finds no slot or does not come home."""
    x = dst
    rev = [int(x)]
    for _ in range(V):
        if x == src:
            break
        taken = None
        for u, slot, m in _parents(rin, L, x, mutant):
            if r < sigma[u]:
                taken = (u, slot, m)
                break
            r -= sigma[u]
        if taken is None:
            return ("lost",)
        u, slot, m = taken
        if mutant == "first_slot":
            slot = next(s for s in range(off[u], off[u + 1]) if adj[s] == x)
        if mutant in ("m_mod_64", "slot_first_64"):
            slot = mth_slot(off, adj, u, x, m, mutant)
            if slot is None:
                return ("lost",)
        rev += [int(eid[slot]), int(u)]
        x = u
    return rev[::-1] if x == src else ("lost",)


def solve(V, off, adj, eid, rs, rd, max_hops, max_paths, mutant=None, state=None):
    """(counts, hops, lists) of the rows: count -1 = NULL; hops -1 and lists None where the row has no list.  `state`: a dict
    that keeps the levels and sigma of every source between calls on ONE graph and ONE mutant (they do not depend on the bounds)."""
    state = {} if state is None else state
    if "rin" not in state:
        state["rin"] = in_lists(V, off, adj)
    rin = state["rin"]
    counts, hops, lists = [], [], []
    for s, d in zip(np.asarray(rs).tolist(), np.asarray(rd).tolist()):
        if s < 0 or d < 0:
            counts.append(-1), hops.append(-1), lists.append(None)
            continue
        if s == d:
            counts.append(1), hops.append(0), lists.append([[int(s)]])
            continue
        if s not in state:
            L = bfs_levels(V, off, adj, s)
            state[s] = (L, sigmas(V, rin, L, s, mutant))
        L, sigma = state[s]
        if L[d] < 0 or (L[d] > max_hops and mutant != "no_bound"):
            counts.append(0), hops.append(-1), lists.append(None)
            continue
        take = min(sigma[d], max_paths + (1 if mutant == "paths_plus_1" else 0))
        counts.append(sigma[d]), hops.append(L[d])
        lists.append([unrank(V, off, adj, eid, rin, L, sigma, s, d, r, mutant) for r in range(max(take, 0))])
    return counts, hops, lists


def brute_force(V, off, adj, eid, src, dst):
    """Every walk of d = dist(src, dst) edges from src to dst, as lists, in the contract's order; None when there is none."""
    if src == dst:
        return [[int(src)]]
    d = bfs_levels(V, off, adj, src)[dst]
    if d < 0:
        return None
    walks, stack = [], [(src, [])]
    while stack:
        v, slots = stack.pop()
        if len(slots) == d:
            if v == dst:
                walks.append(slots)
            continue
        for s in range(off[v], off[v + 1]):
            stack.append((int(adj[s]), slots + [s]))
    u_of = slot_sources(V, off)
    # from the destination end: (x_{d-1}, slot of e_d), then (x_{d-2}, slot of e_{d-1}), ...
    walks.sort(key=lambda sl: [(int(u_of[s]), s) for s in reversed(sl)])
    out = []
    for sl in walks:
        p = [int(src)]
        for s in sl:
            p += [int(eid[s]), int(adj[s])]
        out.append(p)
    return out


# ---- fixtures: (V, off, adj, eid, rs, rd) -------------------------------------------------------------------------------------
def _fx(V, es, ed, rows):
    rs = np.array([r[0] for r in rows], dtype=np.int64)
    rd = np.array([r[1] for r in rows], dtype=np.int64)
    return (V,) + graph(V, es, ed) + (rs, rd)


def tiny_multigraph(seed):
    """V <= 9, up to 30 edges, parallel edges and self-loops as they fall; every (src, dst)."""
    rng = np.random.default_rng(1000 + seed)
    V = int(rng.integers(3, 10))
    E = int(rng.integers(V, 31))
    es, ed = rng.integers(0, V, E), rng.integers(0, V, E)
    return _fx(V, es, ed, [(s, d) for s in range(V) for d in range(V)])


def random_fixture(V=200, E=1200, rows=320, seed=5):
    rng = np.random.default_rng(seed)
    es, ed = rng.integers(0, V, E), rng.integers(0, V, E)
    return _fx(V, es, ed, list(zip(rng.integers(0, V, rows).tolist(), rng.integers(0, V, rows).tolist())))


def diamond_chain(k):
    """k diamonds a -> b, a -> c, b -> d, c -> d, d being the next a: 2^k paths of 2 k hops from vertex 0 to vertex 3 k.
    Rows: the whole chain, and the chain up to its middle."""
    es, ed = [], []
    for i in range(k):
        a, b, c, d = 3 * i, 3 * i + 1, 3 * i + 2, 3 * i + 3
        es += [a, a, b, c]
        ed += [b, c, d, d]
    return _fx(3 * k + 1, es, ed, [(0, 3 * k), (0, 3 * (k // 2)), (3, 3 * k)])


def in_list_gadget(deg):
    """A destination x on level 3 whose in-list has `deg` entries p_0 < ... < p_{deg-1}: every third one, the first and the last are
    on level 2, reached from the source through 1 + j % 4 middle vertices (so their sigma values differ); of the others one half
    is unreachable, the other half sits on level 3.  With every path emitted the ranks fall into the first, the middle and the
    last position of the in-list, across its 64-wide chunks.  Second row: a source whose OUT-list has `deg` entries, of which the
    first and the last lead on to the destination."""
    s, mids = 0, [1, 2, 3, 4]
    p0 = 5
    x = p0 + deg
    deep = x + 1               # level 3 by another route: s -> 1 -> far -> deep-level parents
    far = x + 2
    s2 = x + 3
    y0 = s2 + 1
    z = y0 + deg
    es, ed = [], []
    for m in mids:
        es.append(s), ed.append(m)
    es.append(1), ed.append(far)
    for j in range(deg):
        p = p0 + j
        es.append(p), ed.append(x)
        if j % 3 == 0 or j == deg - 1:
            for m in mids[:1 + j % 4]:
                es.append(m), ed.append(p)
        elif j % 2 == 0:
            es.append(far), ed.append(p)  # level 3: not a parent of x
    es.append(far), ed.append(deep)
    for j in range(deg):
        es.append(s2), ed.append(y0 + j)
    for y in (y0, y0 + deg - 1):
        es.append(y), ed.append(z)
    return _fx(z + 1, es, ed, [(s, x), (s2, z), (s, deep)])


def parallel_edges():
    """0 -> 2 three times and 2 -> 3 three times: 9 paths with distinct edge ids; plus the single-edge route 0 -> 1 -> 3 through the
    smaller parent, which comes first.  sigma(0, 3) = 10."""
    es = [0, 0, 0, 2, 2, 0, 2, 1]
    ed = [2, 1, 2, 3, 3, 2, 3, 3]
    return _fx(4, es, ed, [(0, 3), (0, 2), (1, 3), (3, 0)])


def parallel_run(P):
    """s = 0, middle vertices u0 = 1 < u = 2, destination x = 3, decoy y = 4.  One slot u0 -> x; P parallel slots u -> x, each behind a
    decoy slot u -> y in u's out-list: the k-th slot into x stands at out-position 2 k + 1 and at in-position 1 + k of x's in-list,
    behind u0's.  Rows (s, x): 1 + P paths, and (u, x): P.  For P >= 64 the run of u's in-slots crosses position 64 of the in-list;
    from P = 33 on the m-th slot into x lies behind the out-list's first 64 entries, from P = 65 on m itself reaches 64."""
    es, ed = [0, 0, 1], [1, 2, 3]
    for _ in range(P):
        es += [2, 2]
        ed += [4, 3]
    return _fx(5, es, ed, [(0, 3), (2, 3)])


def many_sources(k, V=150, seed=9):
    """k distinct sources with two destinations each over one graph: the lane batches of 64 walk vertices earlier ones touched."""
    rng = np.random.default_rng(seed)
    es, ed = rng.integers(0, V, 5 * V), rng.integers(0, V, 5 * V)
    rows = [(s, (7 * s + 3) % V) for s in range(k)] + [(s, (11 * s + 5) % V) for s in range(k)]
    return _fx(V, es, ed, rows)


def dead_ends():
    """Vertex 3 has no out-edge, vertex 0 no in-edge; 4 is isolated."""
    return _fx(5, [0, 0, 1, 2], [1, 2, 3, 3], [(3, 0), (1, 0), (0, 3), (4, 4), (0, 4), (4, 0), (3, 3), (0, 0)])


HOPS = (0, 1, 2, 3, INT64_MAX)
PATHS = (1, 2, 7, MAX_PATHS_ALL)


def gpu_fixtures():
    """name -> (fixture, the max_hops values, the max_paths values) the GPU file runs; the CPU file shows that they catch MUTANTS."""
    fx = {"random": (random_fixture(), HOPS, PATHS), "parallel": (parallel_edges(), (1, 2, INT64_MAX), (1, 9, 10, 11)),
          "dead_ends": (dead_ends(), (0, 5), (1, 3))}
    for seed in range(6):
        fx["tiny%d" % seed] = (tiny_multigraph(seed), HOPS, PATHS)
    for deg in (63, 64, 65, 127, 128, 129):
        fx["in_list_%d" % deg] = (in_list_gadget(deg), (2, 3, INT64_MAX), (1, MAX_PATHS_ALL))
    for k in (62, 63, 64):
        fx["diamonds_%d" % k] = (diamond_chain(k), (2 * k - 1, INT64_MAX), (3,))
    for k in (63, 64, 65, 129):
        fx["sources_%d" % k] = (many_sources(k), (3, INT64_MAX), (2,))
    for P in (63, 64, 65, 129):
        fx["parallel_run_%d" % P] = (parallel_run(P), (2, INT64_MAX), (1, MAX_PATHS_ALL))
    return fx
