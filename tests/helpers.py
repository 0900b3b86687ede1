"""Shared helpers for the parity tests (graph feeds shaped like the reference's SQL)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def directed_rows(edges):
    """Row feed of CreateDirectedCSRCTE (compressed_sparse_row.cpp:234-251): one row per edge-table row, in table
    order, edge id = edge rowid."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return e[:, 0].copy(), e[:, 1].copy(), np.arange(len(e), dtype=np.int64)


def undirected_rows(edges):
    """Row feed of CreateUndirectedCSRCTE (compressed_sparse_row.cpp:208-223): one row per distinct ordered pair in
    forward U reverse (GROUP BY src,dst), edge id = any_value -> we take the smallest contributing edge rowid, and
    emit rows sorted by (src,dst) (the reference's order is hash-aggregate order, i.e. unspecified)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    best = {}
    for rid, (s, d) in enumerate(e.tolist()):
        for a, b in ((s, d), (d, s)):
            if (a, b) not in best:
                best[(a, b)] = rid
    keys = sorted(best)
    src = np.array([k[0] for k in keys], dtype=np.int64)
    dst = np.array([k[1] for k in keys], dtype=np.int64)
    eid = np.array([best[k] for k in keys], dtype=np.int64)
    return src, dst, eid


def all_pairs(V):
    s, d = np.meshgrid(np.arange(V, dtype=np.int64), np.arange(V, dtype=np.int64), indexing="ij")
    return s.ravel().copy(), d.ravel().copy()


def csr_arrays_from_rows(V, src, dst):
    """offsets[V+1], adj[E], slot permutation (stable counting sort on src == reference single-thread slot order)."""
    order = np.argsort(src, kind="stable")
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=V), out=off[1:])
    return off, dst[order].astype(np.int64), order


def sparse_ids_graph(rng, V, n_active, E, hubs=4, chains=0, chain_len=10):
    """A graph on about n_active vertices spread over [0, V), for kernels whose per-vertex bit maps are sized by V.  Among
    the active ids: 0, V // 2, V - 2, V - 1, and ids of the last 32-vertex word and of the last 128-vertex block of such a
    map.  Random edges between them, a few hubs whose out- and in-lists span a good part of the active set, and 50
    duplicated edges.  `chains` directed paths of `chain_len` edges over ids of their own, which no other edge touches:
    pairs along a chain are at distances 1 .. chain_len, pairs against its direction are unreachable.
    Returns (active ids, src, dst, hub ids, chains as a list of id arrays)."""
    top = V - 1
    tail = [0, V - 1, V - 2, V // 2, top // 32 * 32, top // 128 * 128]
    tail += list(rng.integers(top // 32 * 32, V, 3)) + list(rng.integers(top // 128 * 128, V, 3))
    act = np.unique(np.concatenate([rng.integers(0, V, n_active), tail]))
    act = act[(act >= 0) & (act < V)]
    n = len(act)
    s = rng.integers(0, n, E)
    d = rng.integers(0, n, E)
    hub = rng.choice(n, hubs, replace=False)
    hs = np.repeat(hub, n // 3)
    hd = rng.integers(0, n, len(hs))
    s = np.concatenate([s, hs, hd, s[:50]])  # hub out- and in-lists, 50 duplicated edges
    d = np.concatenate([d, hd, hs, d[:50]])
    s, d = act[s].astype(np.int64), act[d].astype(np.int64)
    paths = []
    if chains:
        free = np.setdiff1d(np.unique(rng.integers(0, V, 4 * chains * (chain_len + 1))), act)
        rng.shuffle(free)
        assert len(free) >= chains * (chain_len + 1), "V too small for the chains"
        for k in range(chains):
            c = free[k * (chain_len + 1):(k + 1) * (chain_len + 1)].astype(np.int64)
            paths.append(c)
            s, d = np.concatenate([s, c[:-1]]), np.concatenate([d, c[1:]])
    return act, s, d, act[hub], paths


# The largest V at which each bit-map kernel keeps its map in LDS (or, for k_src_ball, runs two workgroups per CU).  One vertex
# more and the host picks the global-memory variant (or one workgroup per CU).  test_lds_limits_gpu.py runs both sides of
# every entry; test_lds_budget_cpu.py recomputes every entry from the host rules and the static LDS of the built kernels.
LDS_LIMITS = {
    "ball_2_per_cu": 466_944,    # k_src_ball, two workgroups per CU (above: one, its map still in LDS)
    "ball_1_per_cu": 1_122_304,  # k_src_ball, one workgroup per CU with 137 KB of dynamic LDS (above: global maps)
    "meet4": 1_212_416,          # k_meet4d, k_meet4<paths>
    "bibfs": 606_080,            # k_bibfs, both visited maps
    # k_pull_lanes<WD, *, true> (lanes = 1) and k_pull_sparse<WD, *, 16, *> (lanes = 0), by lane words WD
    "pull_lanes": {1: 974_272, 2: 961_792, 4: 836_992, 8: 787_008, 16: 687_168, 32: 487_424},
    "pull_sparse": {1: 803_392, 2: 792_448, 4: 770_624, 8: 726_912, 16: 639_552, 32: 464_768},
    # k_lcc_big's vertex bit map (pgq_analytics.hip:161, lcc_device: bm_words * 4 + 256 <= 150 KiB with bm_words = ceil(V / 32));
    # above: a per-workgroup slice of global memory.  No kernel class counts its launches, so test_degree_edges_gpu.py checks
    # results on both sides and nothing else
    "lcc_big": 1_226_752,
}


# The limits of the lane batches' destination probes (pgq_msbfs.hip: k_probe, k_probe2; pgq_internal.h: the options' defaults).
# helpers.probe_gadgets and test_probe_limits_gpu.py stand on them; test_probe_gadgets_cpu.py reads them back from the sources.
PROBE_LIMITS = {
    "kQueue": 1024,         # k_probe: open rows a workgroup pools in LDS before it probes a chunk's rows where it finds them
    "kHubQueue": 256,       # k_probe: rows of hub destinations a workgroup sets aside for all its 16 wavefronts
    "kOpenGrid": 512,       # workgroups of 1024 threads k_probe / k_detect run at most: 8192 wavefronts
    "hub_step": 4 * 1024,   # k_probe: in-neighbours of a hub destination per step of the whole workgroup
    "probe_max_in": 4096,   # option: a destination with MORE in-neighbours is a hub destination
    "probe2_cap": 1 << 16,  # option: a pair whose two-hop walk holds MORE in-edges is left open by k_probe2
}


# ---- gadgets whose adjacency-list lengths sit on the kernels' own constants ----------------------------------------------

GADGET_DEGREES = (1, 2, 63, 64, 65, 319, 320, 321, 511, 512, 513, 4095, 4096, 4097)
GADGET_POSITIONS = ("first", "last", 63, 64, 319, 320)
GADGET_EXTRA_PAIRINGS = ((513, 4097),)
_POOL0, _POOL1, _DEAD = 320, 4096, 1024
# id regions, ascending: dead ends (sinks, roots) | path vertices that sort first | decoy pool 0 | path vertices at a numbered
# index | decoy pool 1 | path vertices that sort last | everything else (endpoints, inner path vertices)
_R_DEAD, _R_LOW, _R_P0, _R_MID, _R_P1, _R_HIGH, _R_ENDS = range(7)


def decoy_len(j):
    """List length of decoy j of a pool: 1..7, 0 in a cycle, and 255, 256, 257 three times in every 96 decoys."""
    return {13: 255, 45: 256, 77: 257}.get(j % 96, (j + 1) % 8)


def gadget_index(pos, n):
    """The list index a position names in a list of n entries, or None where the list is too short for it."""
    idx = 0 if pos == "first" else n - 1 if pos == "last" else pos
    return idx if idx < n else None


class Gadgets:
    """V, the edge table (src, dst: table order is slot order), the rows (rs, rd, dist with -1 = unreachable, tag) and one
    record per gadget: tag, k, a, b, pos, src, dst, paths (vertex lists), tie, row (index of its main row)."""

    def __init__(self, V, src, dst, rs, rd, dist, tag, gadgets):
        self.V, self.src, self.dst, self.rs, self.rd, self.dist, self.tag, self.gadgets = V, src, dst, rs, rd, dist, tag, gadgets

    def transposed(self):
        """Every edge and every row reversed: a and b swap, out-lists become in-lists, distances stay."""
        gs = [dict(g, a=g["b"], b=g["a"], src=g["dst"], dst=g["src"], paths=[p[::-1] for p in g["paths"]]) for g in self.gadgets]
        return Gadgets(self.V, self.dst, self.src, self.rd, self.rs, self.dist, self.tag, gs)

    def shifted(self, V):
        """The same graph on the last ids of [0, V)."""
        o = V - self.V
        assert o >= 0
        gs = [dict(g, src=g["src"] + o, dst=g["dst"] + o, paths=[[v + o for v in p] for p in g["paths"]]) for g in self.gadgets]
        return Gadgets(V, self.src + o, self.dst + o, self.rs + o, self.rd + o, self.dist, self.tag, gs)

    def main_rows(self, pick=lambda g: True):
        return np.array([g["row"] for g in self.gadgets if pick(g)], dtype=np.int64)


def degree_gadgets(degrees=GADGET_DEGREES, positions=GADGET_POSITIONS, extra_pairings=GADGET_EXTRA_PAIRINGS,
                   tie_degrees=(65, 513)):
    """One graph of gadgets, each a source `src` of out-degree a and a destination `dst` of in-degree b that are exactly k hops
    apart (k = 1 .. 4) by ONE shortest path, whose vertex sits at a chosen index of src's out-list and of dst's in-list; every
    other entry of the two lists is a decoy.  Forward decoys come from a shared pool: each has a short out-list (decoy_len) into
    a pool of sinks without out-edges.  Backward decoys mirror them: in-lists from roots without in-edges.  No decoy reaches or
    is reached from an endpoint of another gadget, so rows of different gadgets do not disturb each other, and the path
    vertices of different gadgets are disjoint.

    Out-lists are in table order (csr_arrays_from_rows), in-lists in source-id order; the path vertex's id comes from a region
    below, between or above the two decoy pools, and both lists of a gadget are emitted in ascending id order, so a position
    holds in both directions and in the transposed graph.  Pairings per k and degree x: (x, x) at every position the list is
    long enough for, (x, 1) and (1, x) at `last`, and `extra_pairings` at `last`.

    Tie gadgets (tag tie<n>_...): n = 2, 3 disjoint shortest paths through the first, the last (and a middle) slot of src's
    out-list, whose vertex ids DEscend in slot order, and ascend again on the destination's side for k >= 3.

    Extra rows per gadget: src -> a sink of one of its decoys and a root -> dst (distance 2), dst -> src (unreachable).

    Two parameter sets are in use.  The defaults sit on the constants of the unweighted search kernels
    (test_degree_gadgets_cpu.py, test_degree_edges_gpu.py); WEIGHTED_GADGETS sits on those of the cheapest-path relaxation
    and is given weights by weighted_gadgets (test_weighted_gadgets_cpu.py, test_weighted_gadgets_gpu.py).  A numbered position
    takes its decoys from pool 0 before it and from pool 1 behind it, so no degree may pass 4097 and no numbered position 320:
    a longer list would silently come out shorter."""
    enc = lambda region, serial: (np.int64(region) << 32) + np.asarray(serial, dtype=np.int64)
    count = [0] * 7

    def new(region, n=None):
        at = count[region]
        count[region] += 1 if n is None else n
        return int(enc(region, at)) if n is None else enc(region, np.arange(at, at + n))

    sinks, roots = new(_R_DEAD, _DEAD), new(_R_DEAD, _DEAD)
    f0, b0 = new(_R_P0, _POOL0), new(_R_P0, _POOL0)
    f1, b1 = new(_R_P1, _POOL1), new(_R_P1, _POOL1)
    fdec, bdec = np.concatenate([f0, f1]), np.concatenate([b0, b1])
    es, ed = [], []  # edge table, in pieces

    def edges(s, d):
        s, d = np.broadcast_arrays(np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64))
        es.append(s.ravel())
        ed.append(d.ravel())

    for j in range(len(fdec)):  # decoy j: decoy_len(j) consecutive dead ends, starting at 7 j
        dead = (7 * j + np.arange(decoy_len(j))) % _DEAD
        edges(fdec[j], sinks[dead])
        edges(roots[dead], bdec[j])

    def region_of(pos):
        return _R_LOW if pos == "first" else _R_HIGH if pos == "last" else _R_MID

    def side(n, pos, pv, pool0, pool1):
        """A list of n entries, ascending in id, with pv at gadget_index(pos, n)."""
        idx = gadget_index(pos, n)
        if n == 1:
            return np.array([pv], dtype=np.int64)
        if isinstance(pos, str):
            decoys = np.concatenate([pool0, pool1])[:n - 1]
            return np.concatenate([[pv], decoys] if pos == "first" else [decoys, [pv]]).astype(np.int64)
        return np.concatenate([pool0[:idx], [pv], pool1[:n - 1 - idx]]).astype(np.int64)

    rs, rd, dist, tag, gadgets = [], [], [], [], []

    def row(s, d, k, t):
        rs.append(s), rd.append(d), dist.append(k), tag.append(t)
        return len(rs) - 1

    def finish(t, k, a, b, pos, src, dst, paths, out_list, in_list, tie):
        if k == 1:  # one table row is the path: it keeps its place among src's rows and among the rows into dst
            ia, ib = int(np.flatnonzero(out_list == dst)[0]), int(np.flatnonzero(in_list == src)[0])
            edges(src, out_list[:ia])
            edges(in_list[:ib], dst)
            edges(src, dst)
            edges(src, out_list[ia + 1:])
            edges(in_list[ib + 1:], dst)
        else:
            edges(src, out_list)
            edges(in_list, dst)
        edges(dst, sinks[(3 * len(gadgets) + np.arange(3)) % _DEAD])  # the endpoints have lists against the direction too
        edges(roots[(3 * len(gadgets) + np.arange(3)) % _DEAD], src)
        r = row(src, dst, k, t)
        gadgets.append(dict(tag=t, k=k, a=a, b=b, pos=pos, src=src, dst=dst, paths=paths, tie=tie, row=r))
        for v in out_list:  # distance 2 through a decoy: the first one that has a list
            j = np.flatnonzero(fdec == v)
            if len(j) and decoy_len(int(j[0])):
                row(src, int(sinks[7 * int(j[0]) % _DEAD]), 2, t + "_sink")
                break
        for v in in_list:
            j = np.flatnonzero(bdec == v)
            if len(j) and decoy_len(int(j[0])):
                row(int(roots[7 * int(j[0]) % _DEAD]), dst, 2, t + "_root")
                break
        row(dst, src, -1, t + "_rev")

    def inner(k, m1, m2, serial):
        """The path between the two one-hop vertices (k >= 3) and a few dead ends beside it; returns the path's inner part."""
        t = serial % 4
        edges(m1, sinks[(5 * serial + np.arange(t)) % _DEAD])
        x = [new(_R_ENDS)] if k == 4 else []
        chain = [m1] + x + [m2]
        edges(chain[:-1], chain[1:])
        edges(roots[(5 * serial + np.arange(t)) % _DEAD], m2)
        return chain

    def gadget(k, a, b, pos):
        if gadget_index(pos, a) is None or gadget_index(pos, b) is None:
            return
        t = "k%d_a%d_b%d_%s" % (k, a, b, pos)
        reg = region_of(pos)
        if k == 1:
            src, dst = new(reg), new(reg)
            path, pv_out, pv_in = [src, dst], dst, src
        else:
            src, dst = new(_R_ENDS), new(_R_ENDS)
            m1 = new(reg)
            mids = [m1] if k == 2 else inner(k, m1, new(reg), len(gadgets))
            path, pv_out, pv_in = [src] + mids + [dst], mids[0], mids[-1]
        finish(t, k, a, b, pos, src, dst, [path], side(a, pos, pv_out, f0, f1), side(b, pos, pv_in, b0, b1), False)

    def tie(k, n, deg):
        src, dst = new(_R_ENDS), new(_R_ENDS)
        regs = [_R_HIGH, _R_LOW] if n == 2 else [_R_HIGH, _R_MID, _R_LOW]  # ids descend in slot order
        slots = [0, deg - 1] if n == 2 else [0, deg // 2, deg - 1]
        firsts = [new(r) for r in regs]
        if k == 2:
            lasts, paths = firsts, [[src, m, dst] for m in firsts]
        else:
            lasts = [new(r) for r in regs[::-1]]
            paths = [[src] + inner(k, m1, m2, 7 * len(gadgets) + i) + [dst] for i, (m1, m2) in enumerate(zip(firsts, lasts))]

        def fill(pvs, pool):
            out = np.empty(deg, dtype=np.int64)
            free = np.setdiff1d(np.arange(deg), slots)
            out[free] = pool[:len(free)]
            out[slots] = pvs
            return out

        finish("tie%d_k%d_d%d" % (n, k, deg), k, deg, deg, "tie", src, dst, paths, fill(firsts, fdec), fill(lasts, bdec), True)

    for k in (1, 2, 3, 4):
        for x in degrees:
            for pos in positions:  # (where `last` is also a numbered index — x = 64: index 63 — both are built)
                gadget(k, x, x, pos)
            if x > 1:
                gadget(k, x, 1, "last")
                gadget(k, 1, x, "last")
        for a, b in extra_pairings:
            gadget(k, a, b, "last")
    for k in (2, 3, 4):
        for n in (2, 3):
            for deg in tie_degrees:
                tie(k, n, deg)

    base = np.concatenate([[0], np.cumsum(count)])
    real = lambda v: base[np.asarray(v, dtype=np.int64) >> 32] + (np.asarray(v, dtype=np.int64) & 0xFFFFFFFF)
    for g in gadgets:
        g["src"], g["dst"] = int(real(g["src"])), int(real(g["dst"]))
        g["paths"] = [[int(v) for v in real(p)] for p in g["paths"]]
    return Gadgets(int(base[-1]), real(np.concatenate(es)), real(np.concatenate(ed)), real(rs), real(rd),
                   np.array(dist, dtype=np.int64), np.array(tag), gadgets)


# ---- the same gadgets on the constants of the cheapest-path relaxation (pgq_cheapest.hip), with weights by slot ------------
# k_relax walks eight edges per trip (7, 8, 9 / 15, 16, 17 / 71, 72, 73), sets a list of more than 128 edges aside and walks
# it in chunks of 64 (63 .. 65, 127 .. 130, 191 .. 193), and fills the chunk map 64 chunks per trip: 4097 edges are 65 chunks
WEIGHTED_GADGETS = dict(
    degrees=(1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 71, 72, 73, 127, 128, 129, 130, 191, 192, 193, 4095, 4096, 4097),
    positions=("first", "last", 7, 8, 63, 64, 127, 128, 191, 192),
    extra_pairings=((129, 4097),),
    tie_degrees=(9, 129))
WEIGHT_SCHEMES = ("ascending", "descending", "witness_heaviest", "zeros")
WEIGHT_DTYPES = ("int64", "double", "double_inexact")


def edge_slots(g):
    """Per edge-table row of a Gadgets object: its slot in its source's out-list (table order is slot order) and the
    list's length."""
    order = np.argsort(g.src, kind="stable")
    deg = np.bincount(g.src, minlength=g.V)
    start = np.concatenate([[0], np.cumsum(deg)])
    slot = np.empty(len(g.src), dtype=np.int64)
    slot[order] = np.arange(len(g.src), dtype=np.int64) - start[g.src[order]]
    return slot, deg[g.src].astype(np.int64)


def path_edge_rows(g):
    """The edge-table rows that lie on a gadget's path(s)."""
    key = g.src * g.V + g.dst
    on = {u * g.V + v for x in g.gadgets for p in x["paths"] for u, v in zip(p[:-1], p[1:])}
    return np.isin(key, np.fromiter(on, dtype=np.int64, count=len(on)))


def weighted_gadgets(g, scheme, dtype="int64"):
    """One weight per edge-table row of g, a function of the row's slot i in its source's out-list of length deg alone:
      ascending         1 + i: the weight-sorted rank is the slot, and 2^j / 2^j + 1 sit at slots 2^j - 1 / 2^j
      descending        deg - i: sorting reverses every list
      witness_heaviest  1, but deg + 1 on the edges of the gadgets' paths: such an edge sorts last, behind deg - 1 equal keys
      zeros             0 (doubles: +0.0 in even slots, -0.0 in odd ones)
    dtype: int64; double = the int64 weights x 0.125 (every sum exact); double_inexact = x 0.1 (sums round: only the left
    fold along the path gives the reference's bits).  Weights of g.transposed() go by ITS out-lists, the former in-lists."""
    slot, deg = edge_slots(g)
    if scheme == "ascending":
        w = 1 + slot
    elif scheme == "descending":
        w = deg - slot
    elif scheme == "witness_heaviest":
        w = np.where(path_edge_rows(g), deg + 1, 1)
    elif scheme == "zeros":
        w = np.zeros(len(slot), dtype=np.int64)
    else:
        raise ValueError(scheme)
    if dtype == "int64":
        return w.astype(np.int64)
    f = w.astype(np.float64) * {"double": 0.125, "double_inexact": 0.1}[dtype]
    if scheme == "zeros":
        f = np.where(slot % 2 == 1, -0.0, 0.0)
    return f


def weight_sort_keys(w):
    """The keys ensure_weight_sorted sorts a list by: the weight's bit pattern; for doubles without the sign of -0.0 and with
    NaN counted as +inf (k_weight_keys)."""
    w = np.ascontiguousarray(w)
    bits = w.view(np.uint64)
    if w.dtype.kind == "f":
        bits = np.minimum(bits & np.uint64(0x7FFFFFFFFFFFFFFF), np.uint64(0x7FF0000000000000))
    return bits


LCC_DEGREES = (2, 64, 65, 511, 512, 513)


def lcc_gadgets(big_rows=300):
    """Vertices of out-degree exactly d, d in LCC_DEGREES, whose only triangle-closing edge runs from the neighbour in the last
    slot to the neighbour in the first slot; the slots between hold leaves from a shared pool without out-edges.  Per degree
    three variants: plain, the last neighbour twice (slots d - 2 and d - 1), and a self loop in a middle slot.  `big_rows` more
    plain vertices of degree 513: more long rows than k_lcc_big has workgroups.  The first and last neighbours get the largest
    ids.  Returns (vertex count, src, dst, the rows' vertices, their degrees)."""
    pool = np.arange(513, dtype=np.int64)
    n = len(pool)
    specs = [(d, v) for d in LCC_DEGREES for v in ("plain", "dup", "loop")] + [(513, "plain")] * big_rows
    hubs = n + np.arange(len(specs), dtype=np.int64)
    firsts, lasts = hubs + len(specs), hubs + 2 * len(specs)
    es, ed = [], []
    for (d, variant), h, f, l in zip(specs, hubs, firsts, lasts):
        row = np.concatenate([[f], pool[:d - 2], [l]]) if d > 2 else np.array([f, l])
        if variant == "dup" and d > 2:
            row[d - 2] = l
        if variant == "loop" and d > 2:
            row[d // 2] = h
        es += [np.full(len(row), h), [l]]
        ed += [row, [f]]
    return int(lasts[-1]) + 1, np.concatenate(es).astype(np.int64), np.concatenate(ed).astype(np.int64), hubs, \
        np.array([d for d, _ in specs])


def spread_ids(rng, n, V):
    """n ascending ids of [0, V): 0, V // 2, every id of the last 32-vertex word of a V-bit map, random ones between."""
    top = (V - 1) // 32 * 32
    fixed = np.concatenate([[0, V // 2], np.arange(top, V)])
    ids = np.unique(np.concatenate([fixed, rng.choice(top, n, replace=False)]))
    drop = rng.choice(np.flatnonzero(~np.isin(ids, fixed)), len(ids) - n, replace=False)
    return np.delete(ids, drop).astype(np.int64)


# ---- gadgets on the limits of the lane batches' destination probes (k_probe, k_probe2) -------------------------------------
PROBE_DEGREES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193)
PROBE_POSITIONS = (0, 63, 64, 1023, 1024, 4095, 4096, "last")
PROBE2_FANS = (1, 15, 16, 17, 32, 33)       # in-degree of a two-hop gadget's destination
PROBE2_FAN_POSITIONS = (0, 15, 16, "last")  # where among them the one in-neighbour sits that leads on
PROBE2_LISTS = (65, 129)                    # length of that in-neighbour's own in-list ...
PROBE2_LIST_POSITIONS = (0, 63, 64, "last")  # ... and the witness's position in it
PROBE2_CAP = 4096                           # the probe2_cap the two-hop gadgets' walk sizes sit on
_PROBE_POOL = 8192


class ProbeGadgets:
    """V, the edge table (src, dst), the rows (rs, rd; dist with -1 = unreachable; tag; kind: one / two / indeg0 / self /
    decoys; b = in-degree of the destination, p = position of the one in-neighbour on the path in its in-list, both -1 where
    the row has none; walk = in-degree sum over N_in(dst) for two-hop rows, else -1) and one record per gadget."""

    def __init__(self, V, src, dst, rows, gadgets):
        self.V, self.src, self.dst, self.gadgets = V, src, dst, gadgets
        self.rs = np.array([r[0] for r in rows], dtype=np.int64)
        self.rd = np.array([r[1] for r in rows], dtype=np.int64)
        self.dist = np.array([r[2] for r in rows], dtype=np.int64)
        self.tag = np.array([r[3] for r in rows])
        self.kind = np.array([r[4] for r in rows])
        self.b = np.array([r[5] for r in rows], dtype=np.int64)
        self.p = np.array([r[6] for r in rows], dtype=np.int64)
        self.walk = np.array([r[7] for r in rows], dtype=np.int64)

    def rows_where(self, pick):
        return np.array([g["row"] for g in self.gadgets if pick(g)], dtype=np.int64)


def probe_gadgets(cap=PROBE2_CAP):
    """One graph of gadgets for the destination probes.  The reverse CSR orders an in-list by (source id, slot), so a vertex's
    position in N_in(dst) is its id's rank among the in-neighbours: a LOW pool of decoys holds the smallest ids, a HIGH pool
    the largest, sources, chains and destinations lie between.  A decoy has in-degree 0: it is in no frontier.  A list of n
    entries with its one live entry at position p takes p decoys from the low pool and n - 1 - p from the high pool.

    One-hop gadgets (kind one, tag one_k<k>_b<b>_p<p>): a chain source = c0 -> .. -> c(k-1) -> dst, k = 1, 2, 3, so dst is
    exactly k hops away by one path and c(k-1), the witness k_probe looks for at level k, sits at position p of the b entries
    of N_in(dst); b in PROBE_DEGREES, p in PROBE_POSITIONS where below b.

    Two-hop gadgets (kind two, tag two_k<k>_f<b1>_q<q>_n<n>_v<pv>_w<walk - cap>): dst has b1 in-neighbours u_0 .. u_(b1-1), in
    id order; only u_q has a live in-neighbour, the witness v, at position pv of u_q's n in-neighbours; v is k - 2 hops from
    the source (k = 2: the source itself).  The others' in-lists are decoys, sized so that the in-degree sum over N_in(dst) —
    k_probe2's walk — is cap - 1, cap or cap + 1 (b1 = 1: the walk is n).  Every (b1, q) has every (n, pv) at the cap and two of
    them at cap - 1 and cap + 1 for k = 2, one at each walk for k = 3.

    Other rows: indeg0 (a decoy as destination: nothing points at it), self (src == dst), decoys (a destination whose whole
    in-list of b entries is decoys: unreachable after a full scan, asked from the source of a k = 3 gadget)."""
    low = np.arange(_PROBE_POOL, dtype=np.int64)
    high = -1 - np.arange(_PROBE_POOL, dtype=np.int64)  # placed behind the last id between the pools at the end
    count = [_PROBE_POOL]
    es, ed, rows, gadgets = [], [], [], []

    def new(n=None):
        at = count[0]
        count[0] += 1 if n is None else n
        return at if n is None else np.arange(at, at + n, dtype=np.int64)

    def edges(s, d):
        s, d = np.broadcast_arrays(np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64))
        es.append(s.ravel())
        ed.append(d.ravel())

    def in_list(live, n, p):
        assert 0 <= p < n and p <= _PROBE_POOL and n - 1 - p <= _PROBE_POOL
        return np.concatenate([low[:p], [live], high[:n - 1 - p]]).astype(np.int64)

    def chain(k):  # k edges: k + 1 vertices
        c = [new() for _ in range(k + 1)]
        if k:
            edges(c[:-1], c[1:])
        return c

    def row(s, d, dist, tag, kind, b=-1, p=-1, walk=-1):
        rows.append((s, d, dist, tag, kind, b, p, walk))
        return len(rows) - 1

    def index(pos, n):
        idx = n - 1 if pos == "last" else pos
        return idx if idx < n else None

    # one-hop
    for k in (1, 2, 3):
        for b in PROBE_DEGREES:
            for p in sorted({index(pos, b) for pos in PROBE_POSITIONS} - {None}):
                c = chain(k - 1)
                d = new()
                edges(in_list(c[-1], b, p), d)
                t = "one_k%d_b%d_p%d" % (k, b, p)
                r = row(c[0], d, k, t, "one", b, p)
                gadgets.append(dict(tag=t, kind="one", k=k, b=b, p=p, src=c[0], dst=d, path=c + [d], row=r))
                if len(gadgets) % 7 == 0:
                    row(c[0], int(low[(p + 11 * len(gadgets)) % _PROBE_POOL]), -1, t + "_indeg0", "indeg0", 0)
                if len(gadgets) % 5 == 0:
                    row(c[0], c[0], 0, t + "_self_src", "self")
                    row(d, d, 0, t + "_self_dst", "self")
    far = [g for g in gadgets if g["k"] == 3]
    for i, b in enumerate((1, 64, 65, 1024, 4096, 4097, 8193)):
        d = new()
        edges(np.concatenate([low[:b // 2], high[:b - b // 2]]), d)
        for g in far[i::7][:3]:
            row(g["src"], d, -1, "decoys_b%d_from_%s" % (b, g["tag"]), "decoys", b)

    # two-hop
    def two_hop(k, b1, q, n, pv, walk):
        c = chain(k - 2)
        us = new(b1)
        d = new()
        edges(us, d)
        edges(in_list(c[-1], n, pv), us[q])
        if b1 == 1:
            walk = n
        else:
            rest, others = walk - n, np.delete(us, q)
            assert rest >= 0
            for i, u in enumerate(others):
                m = rest // len(others) + (1 if i < rest % len(others) else 0)
                edges(low[(7 * i + np.arange(m)) % _PROBE_POOL], u)
        t = "two_k%d_f%d_q%d_n%d_v%d_w%+d" % (k, b1, q, n, pv, walk - cap)
        r = row(c[0], d, k, t, "two", b1, q, walk)
        gadgets.append(dict(tag=t, kind="two", k=k, b=b1, p=q, n=n, pv=pv, walk=walk, src=c[0], dst=d,
                            path=c + [int(us[q]), d], row=r))

    cells = sorted({(n, index(pos, n)) for n in PROBE2_LISTS for pos in PROBE2_LIST_POSITIONS})
    turn = 0
    for b1 in PROBE2_FANS:
        for q in sorted({index(pos, b1) for pos in PROBE2_FAN_POSITIONS} - {None}):
            for n, pv in cells:
                two_hop(2, b1, q, n, pv, cap)
            if b1 == 1:
                continue
            for walk in (cap - 1, cap + 1):
                for _ in range(2):
                    two_hop(2, b1, q, *cells[turn % len(cells)], walk)
                    turn += 1
            for walk in (cap - 1, cap, cap + 1):
                two_hop(3, b1, q, *cells[turn % len(cells)], walk)
                turn += 1

    hi_base = count[0]
    V = hi_base + _PROBE_POOL
    real = lambda v: np.where(np.asarray(v, dtype=np.int64) < 0, hi_base - 1 - np.asarray(v, dtype=np.int64), v).astype(np.int64)
    return ProbeGadgets(V, real(np.concatenate(es)), real(np.concatenate(ed)), rows, gadgets)
