"""Plain Python / numpy models of csrc/pgq_analytics.hip (k_pr_*, k_wcc_min_edge / k_wcc_hook, k_lcc*) and the fixtures the
analytics tests share.  No GPU, no oracle: test_analytics_cpu.py holds the models against the oracle, the reference's goldens
and a run in extended precision; test_analytics_gpu.py holds the kernels against the models, bit for bit.

PageRank.  The reference (pagerank.cpp:11-111) iterates over v_size = V + 2 entries; the two trailing entries have no slots and
count as dangling.  Per iteration: every entry with slots adds rank / degree to its neighbours, slot by slot in CSR order;
the others add their rank to one total; then rank' = (1 - 0.85) / vs + 0.85 * (sum + total / vs), and the iteration stops
when the largest |rank' - rank| is below 1e-6.  Every double operation below is one numpy or Python operation, so nothing is
contracted by accident; the last update is ONE rounding of 0.85 * x + c (the reference's build contracts it, and its goldens
hold those bits): computed exactly in integers and rounded once by Python's integer division.
mode="reference" adds the dangling ranks in one ordered chain; mode="device" adds them as k_pr_dangling does: 1024 ordered
slices of ceil(vs / 1024) entries, then the ordered sum of the 1024 partial sums (a slice without a dangling entry adds +0.0).
"""
import numpy as np

DAMPING, EPS, SLICES = 0.85, 1e-6, 1024
PR_SIZES = (0, 1, 62, 63, 1022, 1023, 2046, 2047)  # vs = V + 2 = 2, 3, 64, 65, 1024, 1025, 2048, 2049

# One switch per way in which a PageRank kernel could be subtly wrong.  test_analytics_cpu.py: each of PR_MUTANTS changes a bit
# or the iteration count on a fixture of the GPU test; the two of PR_EQUIVALENT cannot, at any size these fixtures have, and the
# test checks the reason instead.
PR_MUTANTS = (
    "unfused",            # 0.85 * x rounded before c is added
    "no_trailing",        # the two trailing entries left out of the dangling total
    "drop_last_slice",    # the last non-empty slice of k_pr_dangling dropped
    "per_floor",          # per = vs // 1024
    "reverse_in_list",    # an in-list summed from its last entry to its first
)
PR_EQUIVALENT = (
    "dangling_contrib",   # a dangling vertex's contribution not zeroed: rank / 1.  No in-list names a vertex without slots, so
                          # the value is never read (k_pr_contrib's zero keeps x / 0 out of the buffer, nothing more)
    "stop_le",            # stop at max delta <= 1e-6.  Ranks are >= RN(0.15 / vs) > 2^-14 for vs <= 2049, so every delta is a
                          # multiple of 2^-66, and the double 1e-6 (0x3EB0C6F7A0B5ED8D, odd in units of 2^-72) is not
)


def csr(V, src, dst):
    """(off[V + 1], adj[E]) of an edge table: slot order = table order per source, as the reference's single thread fills it."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    off = np.zeros(V + 1, dtype=np.int64)
    if len(src):
        np.cumsum(np.bincount(src, minlength=V), out=off[1:])
    return off, dst[np.argsort(src, kind="stable")].copy()


def in_lists(V, off, adj):
    """roff[V + 1], psrc[E]: the in-list of v holds the sources of the slots that name v, in slot order — the order in which
    the reference's `temp_rank[neighbor] += contrib` reaches v, and (source, slot) order of the device's reverse CSR."""
    E = int(off[V])
    slot_src = np.repeat(np.arange(V, dtype=np.int64), np.diff(off[:V + 1]))
    order = np.argsort(adj[:E], kind="stable")
    roff = np.zeros(V + 1, dtype=np.int64)
    if E:
        np.cumsum(np.bincount(adj[:E], minlength=V), out=roff[1:])
    return roff, slot_src[order]


def _pull_plan(V, roff, reverse=False):
    """Per position k of the in-lists: (the vertices with more than k in-slots, the index of their k-th in-slot)."""
    indeg = np.diff(roff)
    plan = []
    for k in range(int(indeg.max()) if V else 0):
        v = np.flatnonzero(indeg > k)
        plan.append((v, roff[v + 1] - 1 - k if reverse else roff[v] + k))
    return plan


def fma_exact(a, xs, c):
    """[RN(a * x + c) for x in xs]: one rounding.  Doubles are dyadic rationals; Python's int / int is correctly rounded."""
    an, ad = float(a).as_integer_ratio()
    cn, cd = float(c).as_integer_ratio()
    out = []
    for x in xs:
        xn, xd = x.as_integer_ratio()
        out.append((an * xn * cd + cn * ad * xd) / (ad * xd * cd))
    return out


def dangling_total(rank, dangling, vs, mode, mutant=None):
    idx = np.flatnonzero(dangling).tolist()
    r = rank.tolist()
    if mode == "reference":
        s = 0.0
        for i in idx:
            s += r[i]
        return s
    assert mode == "device"
    per = vs // SLICES if mutant == "per_floor" else (vs + SLICES - 1) // SLICES
    part = [0.0] * SLICES
    last = -1
    for tid in range(SLICES):
        lo, hi = tid * per, min(tid * per + per, vs)
        if hi > lo:
            last = tid
        s = 0.0
        for i in range(lo, hi):
            if dangling[i]:
                s += r[i]
        part[tid] = s
    if mutant == "drop_last_slice" and last >= 0:
        part[last] = 0.0
    t = 0.0
    for p in part:
        t += p
    return t


def pagerank(V, off, adj, mode="reference", mutant=None, deltas=None):
    """(rank[V + 2], iterations).  `mutant`: one of PR_MUTANTS or PR_EQUIVALENT; `deltas`: a list that receives every
    iteration's max delta."""
    assert mutant is None or mutant in PR_MUTANTS + PR_EQUIVALENT
    vs = V + 2
    deg = np.zeros(vs, dtype=np.int64)
    deg[:V] = np.diff(off[:V + 1])
    dangling = deg == 0
    has = np.flatnonzero(~dangling)
    counted = dangling.copy()
    if mutant == "no_trailing":
        counted[V:] = False
    roff, psrc = in_lists(V, off, adj)
    plan = _pull_plan(V, roff, reverse=mutant == "reverse_in_list")
    rank = np.full(vs, 1.0 / float(vs))
    c = (1 - DAMPING) / float(vs)
    it = 0
    while True:
        contrib = rank.copy() if mutant == "dangling_contrib" else np.zeros(vs)
        contrib[has] = rank[has] / deg[has].astype(np.float64)
        t = np.zeros(vs)
        for v, at in plan:
            t[v] = t[v] + contrib[psrc[at]]
        corr = dangling_total(rank, counted, vs, mode, mutant) / float(vs)
        x = t + corr
        if mutant == "unfused":
            new = c + DAMPING * x
        else:
            new = np.array(fma_exact(DAMPING, x.tolist(), c))
        max_delta = float(np.max(np.abs(new - rank)))
        if deltas is not None:
            deltas.append(max_delta)
        rank = new
        it += 1
        if (max_delta <= EPS if mutant == "stop_le" else max_delta < EPS) or it >= 10000:
            return rank, it


def pagerank_extended(V, off, adj, iterations, dtype=np.longdouble):
    """The same recurrence for a given number of iterations in a wider format, every constant formed in that format (0.85
    and 1e-6 excepted: 0.85 is the double the reference multiplies by).  Sums in the same order; plain a * x + c."""
    vs = V + 2
    deg = np.zeros(vs, dtype=np.int64)
    deg[:V] = np.diff(off[:V + 1])
    has, dang = np.flatnonzero(deg > 0), np.flatnonzero(deg == 0)
    roff, psrc = in_lists(V, off, adj)
    plan = _pull_plan(V, roff)
    one, n = dtype(1), dtype(vs)
    a = dtype(DAMPING)
    rank = np.full(vs, one / n, dtype=dtype)
    for _ in range(iterations):
        contrib = np.zeros(vs, dtype=dtype)
        contrib[has] = rank[has] / deg[has].astype(dtype)
        t = np.zeros(vs, dtype=dtype)
        for v, at in plan:
            t[v] = t[v] + contrib[psrc[at]]
        total = dtype(0)
        for r in rank[dang]:
            total = total + r
        rank = (one - a) / n + a * (t + total / n)
    return rank


# ---- weakly connected components: the Boruvka rounds ----------------------------------------------------------------------
def boruvka(V, off, adj):
    """(rounds that hooked something, longest hook chain of any round, number of chosen slots) of k_wcc_min_edge / k_wcc_hook:
    every component takes the smallest slot that leaves it (from either end), hooks onto the component on the other side; of
    two components that chose the same slot the larger root hooks and the smaller stays.  A chosen slot is flagged even where
    its component stays a root."""
    E = int(off[V]) if V else 0
    slot_src = np.repeat(np.arange(V, dtype=np.int64), np.diff(off[:V + 1]))
    adj = np.asarray(adj[:E], dtype=np.int64)
    comp = np.arange(V, dtype=np.int64)
    msf = np.zeros(E, dtype=bool)
    none = np.iinfo(np.int64).max
    rounds = longest = 0
    for _ in range(64):
        cu, cv = comp[slot_src], comp[adj]
        k = np.flatnonzero(cu != cv)
        best = np.full(V, none, dtype=np.int64)
        np.minimum.at(best, cu[k], k)
        np.minimum.at(best, cv[k], k)
        roots = np.flatnonzero((comp == np.arange(V)) & (best != none))
        kb = best[roots]
        ra, rb = comp[slot_src[kb]], comp[adj[kb]]
        other = np.where(ra == roots, rb, ra)
        msf[kb] = True
        stays = (best[other] == kb) & (roots < other)  # the mutual choice: the smaller root stays
        hook = np.arange(V, dtype=np.int64)
        hook[roots[~stays]] = other[~stays]
        if stays.all():
            break
        rounds += 1
        x, depth = np.arange(V, dtype=np.int64), 0
        while True:
            nx = hook[x]
            if (nx == x).all():
                break
            x, depth = nx, depth + 1
        longest = max(longest, depth)
        comp = x[comp]
    return rounds, longest, int(msf.sum())


# ---- local clustering coefficient -----------------------------------------------------------------------------------------
def lcc_count(V, off, adj, s):
    """Sum over the SLOTS of s of the slots of that neighbour whose vertex is a neighbour of s; in Python integers."""
    nb = adj[off[s]:off[s + 1]]
    member = np.zeros(V, dtype=bool)
    member[nb] = True
    uniq, mult = np.unique(nb, return_counts=True)
    return sum(int(m) * int(member[adj[off[u]:off[u + 1]]].sum()) for u, m in zip(uniq.tolist(), mult.tolist()))


def lcc_value(count, deg, truncate=False):
    """float(count) / (deg_f * (deg_f - 1)): three float32 operations.  truncate: the conversion chops instead of rounding."""
    if truncate and count.bit_length() > 24:
        sh = count.bit_length() - 24
        count = count >> sh << sh
    df = np.float32(deg)
    return np.float32(float(count)) / (df * (df - np.float32(1.0)))  # count < 2^53: float() is exact, float32() rounds once


def lcc(V, off, adj, rows):
    out = np.zeros(len(rows), dtype=np.float32)
    for i, s in enumerate(np.asarray(rows).tolist()):
        deg = int(off[s + 1] - off[s]) if s >= 0 else 0  # a NULL row's payload is 0
        if deg >= 2:
            out[i] = lcc_value(lcc_count(V, off, adj, s), deg)
    return out


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
def _slice_edges(V):
    """Vertices at k * per - 1 and k * per for the first, a middle and the last non-empty slice of k_pr_dangling, and V - 1."""
    vs = V + 2
    per = (vs + SLICES - 1) // SLICES
    n = (vs + per - 1) // per
    idx = {V - 1}
    for k in (0, 1, n // 2, n - 1):
        idx |= {k * per - 1, k * per}
    return sorted(i for i in idx if 0 <= i < V)


def _random_rows(rng, V, sources, lo=1, hi=5):
    """Every source gets lo .. hi - 1 slots to random vertices; then 1 in 8 rows twice and a self loop at 1 source in 8."""
    d = rng.integers(lo, hi, len(sources))
    s = np.repeat(sources, d)
    t = rng.integers(0, V, len(s))
    twice = rng.random(len(s)) < 0.125
    loops = sources[rng.random(len(sources)) < 0.125]
    s, t = np.concatenate([s, s[twice], loops]), np.concatenate([t, t[twice], loops])
    p = rng.permutation(len(s))
    return s[p], t[p]


_cache = {}


def pagerank_fixtures():
    """[(name, V, off, adj)]: multigraphs with parallel edges and self loops at the sizes around k_pr_dangling's slicing.
      empty   no slots: every entry dangles, one iteration, max delta exactly 0
      cycle   a cycle with chords: only the two trailing entries dangle
      edges   dangling vertices exactly on the edges of the first, a middle and the last slice, and at V - 1
      skew    one vertex of in-degree >= 1000 fed by sources of out-degree 1 .. 500: the in-list's order shows in the last bits"""
    if "pr" in _cache:
        return _cache["pr"]
    out = []
    for V in PR_SIZES:
        rng = np.random.default_rng(1000 + V)
        out.append(("empty_V%d" % V, V) + csr(V, [], []))
        if V == 0:
            continue
        ring = np.arange(V, dtype=np.int64)
        cs, ct = _random_rows(rng, V, ring, 0, 3)
        s, t = np.concatenate([ring, cs]), np.concatenate([(ring + 1) % V, ct])
        p = rng.permutation(len(s))
        out.append(("cycle_V%d" % V, V) + csr(V, s[p], t[p]))
        if V >= 62:
            sources = np.setdiff1d(ring, _slice_edges(V))
            out.append(("edges_V%d" % V, V) + csr(V, *_random_rows(rng, V, sources)))
    for V in (1022, 2047):
        rng = np.random.default_rng(2000 + V)
        hub = V // 3
        feed = np.setdiff1d(np.arange(V, dtype=np.int64), [hub, 5, V - 1])[:1010]  # 5 and V - 1 dangle
        d = 1 + (np.arange(len(feed)) * 7) % 500
        s = np.repeat(feed, d)
        t = rng.integers(0, V, len(s))
        first = np.concatenate([[0], np.cumsum(d)[:-1]])
        at = first + rng.integers(0, d)  # the slot that names the hub: anywhere in the source's list
        t[at] = hub
        t[first[d > 3] + 1] = hub  # ... and a second one: parallel edges into the hub
        s, t = np.concatenate([s, [hub, hub, hub]]), np.concatenate([t, [hub, 0, 0]])
        out.append(("skew_V%d" % V, V) + csr(V, s, t))
    _cache["pr"] = out
    return out


WCC_PATH_V, WCC_CHAIN_V = 3000, 5000


def wcc_fixtures():
    """[(name, V, src, dst)]: directed edge tables for weakly_connected_component."""
    if "wcc" in _cache:
        return _cache["wcc"]
    rng = np.random.default_rng(31)
    out = []
    p = rng.permutation(WCC_PATH_V).astype(np.int64)
    flip = rng.random(WCC_PATH_V - 1) < 0.5
    out.append(("shuffled_path", WCC_PATH_V, np.where(flip, p[1:], p[:-1]), np.where(flip, p[:-1], p[1:])))
    out.append(("chain", WCC_CHAIN_V, np.arange(WCC_CHAIN_V - 1, dtype=np.int64), np.arange(1, WCC_CHAIN_V, dtype=np.int64)))
    leaves = np.arange(1, 301, dtype=np.int64)
    flip = rng.random(300) < 0.5
    out.append(("star_centre_lowest", 301, np.where(flip, leaves, 0), np.where(flip, 0, leaves)))
    out.append(("star_centre_highest", 301, np.where(flip, leaves - 1, 300), np.where(flip, 300, leaves - 1)))
    for V in (255, 256, 257):
        out.append(("empty_V%d" % V, V, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)))
    loops = np.repeat(np.arange(10, dtype=np.int64), [1, 0, 3, 1, 0, 0, 65, 2, 1, 1])
    out.append(("self_loops_only", 10, loops, loops.copy()))
    out.append(("two_vertices_parallel", 2, np.array([0, 1, 1, 0, 1, 0, 0], dtype=np.int64), np.array([1, 0, 0, 1, 0, 1, 1], dtype=np.int64)))
    for n in (62, 63, 64, 128):  # vertex 1: n self loops, then its one leaving slot; 0 -> 2 precedes it in slot order
        s = np.concatenate([[0], np.full(n + 1, 1)]).astype(np.int64)
        d = np.concatenate([[2], np.full(n, 1), [3]]).astype(np.int64)
        out.append(("loops_%d_then_leave" % n, 5, s, d))
    _cache["wcc"] = out
    return out


# p, q of the two-vertex gadget: vertex 0 has one self loop and p slots to vertex 1, vertex 1 has q slots to vertex 0; row 0 has
# deg = p + 1 and count = 1 + p + p * q.  deg 512 is k_lcc's longest list, above it k_lcc_big takes the row; both counts are odd
# and above 2^24, where a float32 holds even integers only.  test_analytics_cpu.py: a chopping conversion changes both RESULTS
# (with p = 512, deg 513, it changes the count and the quotient rounds the difference away: hence 513)
LCC_GADGETS = {"k_lcc": (511, 40001), "k_lcc_big": (513, 40001)}
LCC_ROWS = np.array([0, 1, 2, 3, 4, -1], dtype=np.int64)  # -1: a NULL row


def lcc_gadget(p, q):
    """(V, off, adj) of the gadget plus vertex 2 (degree exactly 2: slots to 0 and 1), vertex 3 (one slot) and vertex 4 (none)."""
    s = np.concatenate([np.zeros(p + 1), np.ones(q), [2, 2, 3]]).astype(np.int64)
    d = np.concatenate([[0], np.ones(p), np.zeros(q), [0, 1, 0]]).astype(np.int64)
    return (5,) + csr(5, s, d)


def pagerank_of(name, mode):
    """pagerank() of a fixture by name, computed once per process: (rank, iterations, max delta of every iteration)."""
    key = ("pr", name, mode)
    if key not in _cache:
        _, V, off, adj = next(f for f in pagerank_fixtures() if f[0] == name)
        deltas = []
        rank, it = pagerank(V, off, adj, mode, deltas=deltas)
        rank.setflags(write=False)
        _cache[key] = (rank, it, deltas)
    return _cache[key]
