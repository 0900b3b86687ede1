"""The Python model of cheapest_path_length_within (a helper of test_cheapest_within_cpu.py / test_cheapest_within_gpu.py).

For a row (src, dst) and K = max_hops the answer is D_K[dst] of
    D_0[src] = 0, D_0[v] = INF otherwise;   D_k[n] = min(D_{k-1}[n], min over edges (u, n) of D_{k-1}[u] + w(u, n))
with INF = max / 2 of the weight type, a sum counting only where it is < D_{k-1}[n] (so never at or above INF, and never as
NaN), and NULL when D_K[dst] == INF.  `hop_rounds` runs exactly these rounds with numpy, frontier-wise: round k expands the
vertices whose label changed in round k - 1, every candidate is computed from the labels as they stood BEFORE the round.
`brute_force` enumerates every walk of at most K edges of a tiny graph and folds its weights left to right.  The CPU oracle
has no bounded form, so every bounded expectation of the tests comes from here.  The mutants (MUTANTS) are the ways a round
can go wrong that the fixtures must notice; the fixtures of the GPU tests are built here too, so that the CPU tests can show
that they do."""
import numpy as np

INT64_MAX = np.iinfo(np.int64).max
MUTANTS = ("live", "short", "long", "filter")


def inf_of(w):
    """The reference's sentinel for the weight array's type (cheapest_path_length.cpp:15)."""
    return np.finfo(np.float64).max / 2 if np.asarray(w).dtype.kind == "f" else INT64_MAX // 2


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def differing(out, ok, want_out, want_ok):
    """Rows whose validity differs, or whose value does where both are valid (int64 values, doubles as bit patterns)."""
    return np.flatnonzero((ok != want_ok) | (ok & want_ok & (bits(out) != bits(want_out))))


def _edges_of(off, vs):
    """Slots of the out-lists of the vertices vs, list by list, and each slot's vertex."""
    deg = off[vs + 1] - off[vs]
    total = int(deg.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    start = np.repeat(off[vs] - np.concatenate([[0], np.cumsum(deg)[:-1]]), deg)
    return start + np.arange(total, dtype=np.int64), np.repeat(vs, deg)


def hop_rounds(V, off, adj, w, src, rounds, live=False):
    """Yields (D_k, whether a label changed in round k) for k = 0, 1, ..., rounds and one source (the same array, updated:
    copy what you keep); once nothing changes the remaining rounds repeat the last labels.  live = True is the mutant that reads a source label from
    the live array: the frontier's vertices are expanded one after the other, in queue order, each with the label it has
    by then."""
    inf = inf_of(w)
    D = np.full(V, inf, dtype=w.dtype)
    D[src] = 0
    front = np.array([src], dtype=np.int64)
    yield D, True
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(rounds):
            if len(front):
                if live:
                    changed = []
                    for v in front:
                        sl = np.arange(off[v], off[v + 1])
                        cand = D[v] + w[sl]
                        for n, c in zip(adj[sl], cand):
                            if c < D[n]:
                                D[n] = c
                                changed.append(n)
                    front = np.unique(np.array(changed, dtype=np.int64))
                else:
                    slots, u = _edges_of(off, front)
                    cand = D[u] + w[slots]  # all from D_{k-1}: nothing is written before every candidate exists
                    tgt = adj[slots]
                    good = cand < D[tgt]    # false for NaN, for +inf and for every sum that does not get under INF
                    tgt, cand = tgt[good], cand[good]
                    if len(tgt):
                        order = np.argsort(tgt, kind="stable")
                        tgt, cand = tgt[order], cand[order]
                        first = np.flatnonzero(np.concatenate([[True], tgt[1:] != tgt[:-1]]))
                        D[tgt[first]] = np.minimum.reduceat(cand, first)
                        front = tgt[first]
                    else:
                        front = tgt
            yield D, len(front) > 0


def bounded_cheapest(V, off, adj, w, rs, rd, Ks, mutant=None):
    """{K: (out, ok)} for the rows (rs, rd) and every K of Ks; rs < 0 or rd < 0 is a NULL row.  mutant: None, or one of
    MUTANTS — live (hop_rounds), short / long (one round fewer / more), filter (the unbounded value, NULL where the
    unbounded cheapest walk with the fewest edges has more than K)."""
    rs, rd = np.asarray(rs, dtype=np.int64), np.asarray(rd, dtype=np.int64)
    Ks = [int(k) for k in Ks]
    inf = inf_of(w)
    res = {K: (np.zeros(len(rs), dtype=w.dtype), np.zeros(len(rs), dtype=bool)) for K in Ks}
    shift = {"short": -1, "long": 1}.get(mutant, 0)
    want = {K: max(0, min(K + shift, V)) for K in Ks}  # (D_k stands still from k = V - 1 on)
    top = V if mutant == "filter" else max(want.values())
    rows_of = {}
    for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
        if s >= 0 and d >= 0:
            rows_of.setdefault(s, []).append(i)
    for s, rows in rows_of.items():
        rows = np.array(rows, dtype=np.int64)
        dst = rd[rows]
        hist = []  # D_k[dst] for k = 0, 1, ... until the labels stand still
        for D, moving in hop_rounds(V, off, adj, w, s, top, live=mutant == "live"):
            hist.append(D[dst].copy())
            if not moving:
                break
        if mutant == "filter":  # the first round that shows the final label = the fewest edges of a cheapest walk
            same = np.array([bits(h) == bits(hist[-1]) for h in hist])
            hops = same.argmax(axis=0)
        for K in Ks:
            val = hist[-1] if mutant == "filter" else hist[min(want[K], len(hist) - 1)]
            ok = val < inf
            if mutant == "filter":
                ok &= hops <= K
            res[K][0][rows] = np.where(ok, val, 0)
            res[K][1][rows] = ok
    return res


def brute_force(V, es, ed, ew, src, K, stats=None):
    """Per vertex: the smallest left-to-right fold over ALL walks src -> vertex of at most K edges (Python numbers: exact
    integers, IEEE doubles), None where no walk's fold gets under INF.  stats (a dict) counts what the folds met: `absorbed`,
    a weight that left the sum unchanged although it is not zero; `nonassoc`, a walk whose fold from the right differs."""
    is_float = np.asarray(ew).dtype.kind == "f"
    inf = float(inf_of(ew)) if is_float else int(inf_of(ew))
    out = [[] for _ in range(V)]
    for s, d, x in zip(es.tolist(), ed.tolist(), ew.tolist()):
        out[s].append((d, x))
    best = [inf] * V

    def walk(v, acc, ws):
        if acc < best[v]:
            best[v] = acc
        if len(ws) == K:
            return
        for n, x in out[v]:
            nxt = acc + x
            if stats is not None and is_float and x != 0 and nxt == acc and acc == acc and abs(acc) != float("inf"):
                stats["absorbed"] = stats.get("absorbed", 0) + 1
            ws.append(x)
            if stats is not None and is_float and nxt == nxt:
                right = 0.0
                for y in reversed(ws):
                    right = y + right
                if right != nxt:
                    stats["nonassoc"] = stats.get("nonassoc", 0) + 1
            walk(n, nxt, ws)
            ws.pop()

    walk(src, 0.0 if is_float else 0, [])
    return [None if not b < inf else b for b in best]


# ---- the fixtures of the GPU tests -----------------------------------------------------------------------------------

def csr_of(V, es, ed, ew):
    """(off, adj, w) in slot order: a stable sort by source, the reference's single-thread order."""
    es, ed = np.asarray(es, dtype=np.int64), np.asarray(ed, dtype=np.int64)
    order = np.argsort(es, kind="stable")
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(es, minlength=V), out=off[1:])
    return off, ed[order].copy(), np.asarray(ew)[order].copy()


def shortcut_path(double):
    """0 -> 1 -> ... -> 6 with weights 1, plus shortcuts 0 -> j of weight 10 j, j = 2 .. 6: the cheapest walk 0 -> 6 of at most
    K edges takes the shortcut to 6 - (K - 1) and walks on: NULL, 60, 51, 42, 33, 24, 6 for K = 0 .. 6."""
    es = list(range(6)) + [0] * 5
    ed = list(range(1, 7)) + list(range(2, 7))
    ew = [1] * 6 + [10 * j for j in range(2, 7)]
    return (7,) + csr_of(7, es, ed, np.array(ew, dtype=np.float64 if double else np.int64))


SHORTCUT_EXPECTED = (None, 60, 51, 42, 33, 24, 6)


def path_graph(n, double):
    """A directed path of n vertices, weights 1 (int64) or 0.1 (double); the rows (i, j) for every i < j <= i + 5."""
    s = np.arange(n - 1, dtype=np.int64)
    w = np.full(n - 1, 0.1) if double else np.ones(n - 1, dtype=np.int64)
    i = np.repeat(np.arange(n, dtype=np.int64), 5)
    j = i + np.tile(np.arange(1, 6, dtype=np.int64), n)
    keep = j < n
    return (n,) + csr_of(n, s, s + 1, w) + (i[keep], j[keep])


def zero_ring(n, double):
    """A ring of n vertices, every weight 0; the rows (i, (i + t) % n) for t = 1 .. 5 and every i."""
    s = np.arange(n, dtype=np.int64)
    w = np.zeros(n, dtype=np.float64 if double else np.int64)
    i = np.repeat(s, 5)
    t = np.tile(np.arange(1, 6, dtype=np.int64), n)
    return (n,) + csr_of(n, s, (s + 1) % n, w) + (i, (i + t) % n, t)


RANDOM_WEIGHTS = ("int_small", "int_wide", "double_special", "int_ones", "double_ones")


def random_graph(V, E, kind, seed=7):
    """A skewed random graph (a quarter of the edges leave one of 16 hubs), parallel edges and self-loops as they fall.
    kind: int_small = int64 1 .. 999; int_wide = int64 over 40 binary orders; double_special = doubles with -0.0, 0.0, inf,
    NaN, a NaN with the sign bit set and 1e308 among them; int_ones / double_ones = all 1 / 1.0."""
    rng = np.random.default_rng(seed)
    es = rng.integers(0, V, E)
    hubs = rng.choice(V, 16, replace=False)
    hot = rng.random(E) < 0.25
    es[hot] = hubs[rng.integers(0, 16, int(hot.sum()))]
    ed = rng.integers(0, V, E)
    if kind == "int_small":
        ew = rng.integers(1, 1000, E).astype(np.int64)
    elif kind == "int_wide":
        ew = (np.int64(1) << rng.integers(0, 40, E)) + rng.integers(0, 1000, E)
    elif kind == "double_special":
        ew = rng.random(E) * 10.0
        special = np.array([-0.0, 0.0, np.inf, np.nan, -np.nan, 1e308])
        pick = rng.random(E) < 0.08
        ew[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
        neg_nan = np.flatnonzero(np.isnan(ew))[::2]
        ew.view(np.uint64)[neg_nan] |= np.uint64(1) << np.uint64(63)  # a NaN with the sign bit set, whatever -nan parsed to
    elif kind == "int_ones":
        ew = np.ones(E, dtype=np.int64)
    elif kind == "double_ones":
        ew = np.ones(E, dtype=np.float64)
    else:
        raise ValueError(kind)
    return (V,) + csr_of(V, es, ed, ew)


def random_rows(V, seed=11, scattered=300, group=40):
    """`scattered` random pairs, every 97th of them with src == dst, and a group x group product grouped by source."""
    rng = np.random.default_rng(seed)
    rs = rng.integers(0, V, scattered)
    rd = rng.integers(0, V, scattered)
    rd[::97] = rs[::97]
    gs = rng.choice(V, group, replace=False)
    gd = rng.choice(V, group, replace=False)
    return (np.concatenate([rs, np.repeat(gs, group)]).astype(np.int64),
            np.concatenate([rd, np.tile(gd, group)]).astype(np.int64))
