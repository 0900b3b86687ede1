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


# ---- gadgets on the partition limits of the lane batches' expansion kernels ---------------------------------------------
# Every constant the gadgets sit on, and where it was read (test_pull_gadgets_cpu.py reads them back from the sources):
PULL_LIMITS = dict(
    kPartRun=256,         # pgq_runtime.hip, `constexpr int kPartRun = 256;`: k_make_parts packs one run per thread
    part_vertices=16,     # k_make_parts, `v - begin >= 16`; `constexpr int NV = 16;` in k_pull_sparse and k_pull_lanes
    vertex_weight=8,      # k_make_parts, `const int64_t wv = d + 8;`
    part_weight=1024,     # pgq_internal.h, `int part_weight = 1024;`
    hub_chunk=4096,       # pgq_internal.h, `int hub_chunk = 4096;`
    push_chunk=256,       # pgq_internal.h, `int push_chunk = 256;`
    min_option=64,        # finish_upload / the batch worker: std::max(64, hub_chunk | part_weight | push_chunk)
    hub_slice_div=4,      # finish_upload, `slice = std::max<int64_t>(64, chunk / 4)`
    lanes_qcap=64,        # k_pull_lanes, `constexpr int QCAP = 64;`: queued records with more than two lane ids
    sparse_qcap=128,      # k_pull_sparse, `constexpr int QCAP = 128;`: spilled words per trip
    kInlineWords=3,       # pgq_msbfs.hip: words of a frontier record that need no second fetch
    kLaneFields=10,       # pgq_lanes.hip: lane ids a record holds; one more and the dense row is read
    rpk_pad=2048)         # pgq_internal.h, csr_arrays: `(En + 2048) * 4` bytes of rpk
PULL_UNROLLS = (1, 2, 4)  # lanes_unroll / sparse_unroll: a trip is 64 x UN in-slots
PULL_DEGREES = (1, 2, 3, 5, 16, 17, 32, 33, 48, 49, 63, 64, 65, 127, 128, 129)  # k_pull: 64 per trip, GRP breaks at r0 * NS
PUSH_DEGREES = (1, 63, 64, 65, 127, 128, 129, 192, 193)
_Z = 32  # symbolic ids: zone << 32 | index; zones in id order: targets, low pools, middle, high pools, top, tail


def pull_parts_model(roff, part_weight, hub_chunk, max_vertices=16):
    """k_make_parts's contract in plain Python: per run of 256 consecutive vertices a greedy pass, hubs (in-degree above the
    chunk) in no part, a part closed before the vertex that would be its 17th or would take its in-degree + 8 per vertex above
    the weight, unless the part is empty.  Returns (parts as [n, 2], hub vertices)."""
    W, C, run = max(64, part_weight), max(64, hub_chunk), PULL_LIMITS["kPartRun"]
    V = len(roff) - 1
    deg = np.diff(roff).tolist()
    parts, hubs = [], []
    for v0 in range(0, V, run):
        v1 = min(V, v0 + run)
        begin, acc = v0, 0
        for v in range(v0, v1):
            d = deg[v]
            if d > C:
                hubs.append(v)
                if v > begin:
                    parts.append((begin, v))
                begin, acc = v + 1, 0
                continue
            if v > begin and (acc + d + 8 > W or v - begin >= max_vertices):
                parts.append((begin, v))
                begin, acc = v, 0
            acc += d + 8
        if v1 > begin:
            parts.append((begin, v1))
    return np.array(parts, dtype=np.int64).reshape(-1, 2), np.array(hubs, dtype=np.int64)


def hub_slices_model(roff, hubs, hub_chunk):
    """finish_upload's hub items: every hub's in-list cut into slices of max(64, chunk / 4) entries, in vertex order."""
    S = max(64, max(64, hub_chunk) // PULL_LIMITS["hub_slice_div"])
    return np.array([(v, b, min(b + S, roff[v + 1])) for v in hubs for b in range(roff[v], roff[v + 1], S)],
                    dtype=np.int64).reshape(-1, 3)


class PullGadgets:
    """V, the edge table (src, dst), the rows (rs, rd, dist with -1 = unreachable, tag) and one record per gadget:
      tag, family, k (hops), rows (row indices; the first is (src, dst)), cut (per row, the edge without which the row's answer
      changes; None for a negative row), src, dst, path, b (in-degree of dst), p (in-slot of
      the witness path[-2] in N_in(dst)), live (decoys are frontier vertices) and, where the family fixes them, expect = a dict
      of v0 / own (part start, owner row) / closes (dst is its part's last vertex) / alone / hub / prel (part-relative
      in-slot) / mod4 (roff[v0] % 4) / slice, last_slice / out_deg, out_slot (of the witness edge in path[-2]'s out-list) /
      lanes (distinct sources the witness carries) / words (distinct 64-lane words of those sources in the spread call).
    fixed = rows that belong in every call (the decoy sources: they make the pools live), pairs = rows to call on their own
    (two lanes: the early exit), spread = rows of the call in which the spread witnesses' sources lie in different lane-words,
    negative = rows that a scan without the first trip's mask answers, stale = two calls to make one after the other (first, second):
    the second asks for a hub the first reached, from a source that does not reach it."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def rows_where(self, pick):
        return np.array([r for g in self.gadgets if pick(g) for r in g["rows"]], dtype=np.int64)

    def calls(self, words):
        """Row sets of at most 64 x words distinct sources (one batch), each holding the fixed rows; a gadget's rows stay
        together."""
        fixed = set(self.rs[self.fixed].tolist())
        room = 64 * words - len(fixed)
        out, cur, srcs = [], [], set()
        for g in self.gadgets:
            if g["family"] in ("spread", "spill"):
                continue
            s = set(self.rs[g["rows"]].tolist()) - fixed
            if len(srcs | s) > room:
                out.append(cur)
                cur, srcs = [], set()
            cur += g["rows"]
            srcs |= s
        out.append(cur)
        return [np.array(list(self.fixed) + c, dtype=np.int64) for c in out if c]


def pull_gadgets(part_weight=64, hub_chunk=64):
    """One graph of gadgets for the expansion kernels of the lane batches (k_push, k_pull, k_pull_sparse, k_pull_lanes,
    k_pull_hub) and the work partition of finish_upload, for a handle uploaded under `part_weight` and `hub_chunk`.

    A gadget is a row (s, t) whose only shortest path enters t through one in-edge, from the witness; s = c0 -> .. -> c(k-1)
    = witness -> t, k = 1, 2, 3 (5 in the push family).  In-lists are ordered by source id: the target zone has the smallest
    ids (so roff of a target is the sum of the target zone's in-degrees before it), then the LOW pools, the sources, chains and
    witnesses, the HIGH pools; a witness at in-slot p of b entries has p in-neighbours out of a LOW pool and b - 1 - p out of a
    HIGH pool.  Decoys are LIVE: pool k is in the frontier of level k - 1 with other lanes' bits (pool 1: eight + eight sources
    of rows of their own; pool 2: every vertex an out-neighbour of three sources D2 — three lane ids, a queued record in
    k_pull_lanes — and of the four spread sources; pool 3: two hops from a source D3; the D sources keep a row five hops long,
    so their lanes stay wanted).  A list longer than its pool, and the `cold` family, takes vertices nothing reaches.  Kind
    `detour`: a second path two hops longer enters t just before the witness, else a lost witness leaves the row unreachable.

    The target zone is cut into segments that begin at a multiple of 256 (a run of k_make_parts: a part begins there); the
    last vertex of the run before, the aligner, takes 0 .. 3 cold in-edges (or a part's weight of them: the heavy aligner of the
    `align` family, alone in its part) so that roff of the segment's first vertex has the wanted remainder mod 4."""
    L = PULL_LIMITS
    W, C, RUN, NV = max(L["min_option"], part_weight), max(L["min_option"], hub_chunk), L["kPartRun"], L["part_vertices"]
    S = max(64, C // L["hub_slice_div"])
    PC = L["min_option"]  # the push_chunk the push family stands on
    T, LOW, MID, HIGH, TOP, TAIL = (z << _Z for z in range(6))
    n1, NP, N3 = 8, max(1100, C + S + 8), 320
    count = {z: 0 for z in (LOW, MID, HIGH, TOP, TAIL)}
    tdeg = []  # in-degrees of the target zone, by id
    es, ed, rows, gadgets = [], [], [], []
    fixed, pairs, negative, tags = [], [], [], set()

    def new(zone=MID, n=None):
        at = zone + count[zone]
        count[zone] += 1 if n is None else n
        return at if n is None else at + np.arange(n, dtype=np.int64)

    def edges(s, d):
        s, d = np.broadcast_arrays(np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64))
        es.append(s.ravel().copy())
        ed.append(d.ravel().copy())

    def row(s, d, dist, tag):
        rows.append((int(s), int(d), dist, tag))
        return len(rows) - 1

    def chain(k, first=None):  # k edges from `first` (a new vertex if None): the k + 1 vertices
        c = [new() if first is None else first] + [new() for _ in range(k)]
        if k:
            edges(c[:-1], c[1:])
        return c

    # the pools
    pool = {}
    for zone, side in ((LOW, "low"), (HIGH, "high")):
        pool[side, 1] = new(zone, n1)
        pool[side, 2] = new(zone, NP)
        pool[side, 3] = new(zone, N3)
        pool[side, 0] = new(zone, NP)  # cold: nothing points at them
    d2, d3 = new(LOW, 3), new(LOW)
    spread = [None] * 4  # sources 64 ranks apart (below): their lanes lie in four lane-words

    def far_row(s, tag):  # keeps a decoy source's lane wanted for five levels
        row(s, chain(5, s)[-1], 5, tag)
        fixed.append(len(rows) - 1)

    sink1 = new()
    for side in ("low", "high"):
        for i, v in enumerate(pool[side, 1]):
            edges(v, sink1)
            fixed.append(row(v, sink1, 1, "pool1_%s%d" % (side, i)))
    for j, s in enumerate(d2):
        for side in ("low", "high"):
            edges(s, pool[side, 2])
        far_row(s, "d2_%d" % j)
    m3 = new()
    edges(d3, m3)
    for side in ("low", "high"):
        edges(m3, pool[side, 3])
    far_row(d3, "d3")
    # ballast: 63 rows one hop long between two spread sources
    ballast = []
    for i in range(4):
        spread[i] = new()
        if i < 3:
            for j in range(63):
                s, d = new(), new()
                edges(s, d)
                ballast.append(row(s, d, 1, "ballast%d_%d" % (i, j)))
    for s in spread:
        for side in ("low", "high"):
            edges(s, pool[side, 2])

    def in_list(k, b, p, live, before=()):
        """The in-neighbours of a list of b entries around a witness at in-slot p: low side, then `before`, [witness], high."""
        n_low, n_high = p - len(before), b - 1 - p
        assert n_low >= 0 and n_high >= 0, (b, p)
        out = []
        for side, n in (("low", n_low), ("high", n_high)):
            a = min(n, len(pool[side, k])) if live else 0
            assert n - a <= NP, (b, p)
            out.append(np.concatenate([pool[side, k][:a], pool[side, 0][:n - a]]).astype(np.int64))
        return out[0], out[1]

    # -- the target zone
    def tv(b):
        tdeg.append(b)
        return T + len(tdeg) - 1

    def segment(mod4=None, heavy=False):
        """Pads to the next multiple of 256; the last pad vertex is the aligner.  Returns it where it is heavy."""
        pad = RUN - len(tdeg) % RUN
        tdeg.extend([0] * (pad - 1))
        a = 0
        if heavy:
            a = W - L["vertex_weight"] + 1  # alone in its part: a + 8 > W whatever precedes it
        if mod4 is not None:
            a += (mod4 - sum(tdeg) - a) % 4
        assert a <= C
        v = tv(a)
        if a and not heavy:
            edges(pool["low", 0][:a], v)
        return v, a

    def gadget(family, k, b, p, live=True, detour=False, t=None, tag=None, expect=None, n_src=1, srcs=None):
        """s = c0 -> .. -> witness -> t.  n_src > 1: so many sources, each with an edge to c1 (k = 2: the witness), a row each."""
        t = tv(b) if t is None else t
        ss = [new() for _ in range(n_src)] if srcs is None else srcs
        before = []
        if detour:  # a path of k + 2 hops whose last vertex sits in the slot before the witness (the witness gets the next id)
            assert p >= 1
            before = [chain(k + 1, ss[0])[-1]]
        c = chain(k - 1, ss[0])
        for s in ss[1:]:
            assert k >= 2
            edges(s, c[1])
        lo, hi = in_list(min(k, 3), b, p, live, before)
        edges(np.concatenate([lo, before, [c[-1]], hi]).astype(np.int64), t)
        tag = tag or "%s_k%d_b%d_p%d%s%s" % (family, k, b, p, "" if live else "_cold", "_detour" if detour else "")
        if tag in tags:
            tag += "_n%d" % len(gadgets)
        tags.add(tag)
        rs_ = [row(s, t, k, tag if i == 0 else "%s_src%d" % (tag, i)) for i, s in enumerate(ss)]
        g = dict(tag=tag, family=family, k=k, b=b, p=p, live=live, detour=detour, src=ss[0], dst=t, path=c + [t], rows=rs_,
                 expect=dict(expect or {}))
        if n_src > 1:
            g["expect"]["lanes"] = n_src
        gadgets.append(g)
        return g

    last = lambda b: b - 1
    # run 0: nothing points at it; ids 62 .. 65 are sources of the push family (k_queue_from_dense takes 64 vertices per trip)
    tdeg.extend([0] * 66)
    # a. degrees: every kernel's 64-entry trip, k_pull's GRP loop (r0 * NS | + 1 entries in the last chunk, NS = 64 / words);
    #    above the chunk the same lists are hubs
    segment()
    for k in (1, 2, 3):
        for b in PULL_DEGREES:
            for p in sorted({0, last(b)} | ({63, 64} & set(range(b)))):
                gadget("deg", k, b, p, detour=(k == 2 and p == last(b) and b in (5, 64, 129)),
                       expect=dict(hub=b > C))
    for b in (5, 64, 65, 129):
        gadget("cold", 2, b, last(b), live=False, expect=dict(hub=b > C))
        gadget("cold", 3, b, 0, live=False, expect=dict(hub=b > C))
    for b in sorted({64 + x for x in (16, 17, 32, 33, 48, 49)}):
        gadget("deg", 2, b, last(b), expect=dict(hub=b > C))
    # b. part shapes
    n_fit = min(NV, W // (3 + L["vertex_weight"]))  # vertices of in-degree 3 a part takes: 16 under the defaults, 5 at weight 64
    v0 = segment()[0] + 1
    for j in range(n_fit + 1):  # the vertex after the full part opens the next one
        p = 0 if j in (0, n_fit) else 2
        gadget("full_part", 2, 3, p, expect=dict(v0=v0 + (n_fit if j == n_fit else 0), own=j % n_fit, closes=j == n_fit - 1,
                                                  full=n_fit == NV and j < n_fit, opens_next=j == n_fit))
    half = (W - 2 * L["vertex_weight"]) // 2  # two vertices of `half` in-edges weigh exactly W
    for over in (0, 1):
        v0 = segment()[0] + 1
        gadget("weight", 2, half, last(half), expect=dict(v0=v0, own=0, closes=bool(over)), tag="weight_first_over%d" % over)
        gadget("weight", 2, half + over, last(half + over), expect=dict(v0=v0 + over, own=1 - over), tag="weight_second_over%d" % over)
    v0 = segment()[0] + 1
    gadget("heavy", 2, 2, 1, expect=dict(v0=v0, own=0, closes=True))
    big = min(C, W + 36)  # heavier than a part on its own, and no hub
    gadget("heavy", 2, big, last(big), expect=dict(v0=v0 + 1, own=0, alone=True))
    gadget("heavy", 2, 2, 0, expect=dict(v0=v0 + 2, own=0))
    # the end of a run cuts a part: targets at ids 255 | 256 of a two-run segment
    v0 = segment()[0] + 1
    tdeg.extend([0] * (RUN - 1))
    gadget("run_end", 2, 3, 2, expect=dict(closes=True, run_last=True))
    gadget("run_end", 2, 3, 0, expect=dict(v0=v0 + RUN, own=0))
    # hubs inside a run: at its first vertex, two adjacent ones, at its last vertex; in-degree 0 inside a part
    v0 = segment()[0] + 1
    hb = C + 1
    gadget("hub_in_run", 2, hb, last(hb), expect=dict(hub=True), tag="hub_first_of_run")
    gadget("hub_in_run", 2, 2, 1, expect=dict(v0=v0 + 1, own=0))
    tv(0), tv(0)
    gadget("hub_in_run", 2, 2, 1, expect=dict(v0=v0 + 1, own=3, closes=True), tag="zero_degrees_inside")
    gadget("hub_in_run", 2, hb, 0, expect=dict(hub=True), tag="hub_adjacent_a")
    gadget("hub_in_run", 2, hb + 1, last(hb + 1), expect=dict(hub=True), tag="hub_adjacent_b")
    gadget("hub_in_run", 2, 2, 0, expect=dict(v0=v0 + 7, own=0), tag="after_two_hubs")
    tdeg.extend([0] * (RUN - 10))
    gadget("hub_in_run", 2, 2, 1, expect=dict(closes=True), tag="before_hub_last_of_run")
    gadget("hub_in_run", 2, hb, S, expect=dict(hub=True, run_last=True), tag="hub_last_of_run")
    # c. trip position: roff[v0] mod 4 with the witness in in-slot e0; the aligner before it is heavy and ends in a live
    #    witness of another lane, which a first trip that starts at e0 & ~3 without a mask credits to this part's owner row 0
    for r in range(4):
        av, a = segment(mod4=r, heavy=True)
        lo, _ = in_list(2, a, a - 1, False)
        sa, wa = new(), new()
        edges(sa, wa)
        edges(np.concatenate([lo, [wa]]), av)
        ra = row(sa, av, 2, "align_mod%d_aligner" % r)
        g = gadget("align", 2, 5, 0, expect=dict(v0=av + 1, own=0, mod4=r, prel=0))
        negative.append(row(sa, g["dst"], -1, "align_mod%d_negative" % r))
        gadgets.append(dict(tag="align_mod%d_aligner" % r, family="aligner", k=2, b=a, p=a - 1, live=False, detour=False, src=sa,
                            dst=av, path=[sa, wa, av], rows=[ra, negative[-1]], expect=dict(v0=av, own=0, alone=True)))
    # part-relative in-slots on the ends of the trips of 64 x UN entries (k_pull_lanes: two prologue trips, then the pipeline)
    slots = sorted({m * 64 * un - 1 for un in PULL_UNROLLS for m in (1, 2)} | {m * 64 * un for un in PULL_UNROLLS for m in (1, 2, 3)})
    longest = W - L["vertex_weight"]  # the longest list that is not alone in its part by weight
    for q in slots:
        if q < longest:
            v0 = segment(mod4=q % 3 + 1)[0] + 1
            gadget("trip", 2, longest, q, expect=dict(v0=v0, own=0, prel=q))
        elif q < C:  # (weight 64: a part's in-slots end before 64 unless one vertex holds them all) heavier than a part, no hub
            v0 = segment(mod4=q % 3 + 1)[0] + 1
            gadget("trip", 2, q + 1, q, expect=dict(v0=v0, own=0, prel=q, alone=True))
    # d. hubs: in-degrees around the chunk, last slices of 1, 63, 64 (a whole slice) and 65 = 64 + 1 entries, the witness in
    #    the first and last slot of the first, a middle and the last slice
    segment()
    gadget("hub", 2, C, last(C), expect=dict(hub=False), tag="hub_not_yet_last")
    gadget("hub", 2, C, 0, expect=dict(hub=False), tag="hub_not_yet_first")
    hub_degrees = [C + 1, C + 63, C + 64, C + 65, C + S] if C > 64 else [C + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S - 1, 3 * S, 3 * S + 1, 4 * S + 63]
    for b in hub_degrees:
        n_sl = (b + S - 1) // S
        for sl in sorted({0, n_sl // 2, n_sl - 1}):
            for p in sorted({sl * S, min(b, (sl + 1) * S) - 1}):
                gadget("hub", 2, b, p, expect=dict(hub=True, slice=sl, last_slice=sl == n_sl - 1, tail=b - (n_sl - 1) * S))
    gadget("hub", 3, hub_degrees[1], last(hub_degrees[1]), expect=dict(hub=True, last_slice=True))
    gadget("hub", 1, hub_degrees[1], last(hub_degrees[1]), expect=dict(hub=True, last_slice=True))
    gadget("hub", 2, hub_degrees[-1], last(hub_degrees[-1]), live=False, expect=dict(hub=True, last_slice=True), tag="hub_cold_last")
    # a hub reached in one call and asked for, from a source that does not reach it, in the next: the two calls' only sources
    # share lane 0, and the bottom-up levels' frontier buffers are never cleared between calls, so a k_pull_hub_zero that left the
    # hub's row of `next` alone would hand the second call the first call's bit (its other row, three hops long, keeps it running)
    gz = gadget("stale", 2, hub_degrees[0], last(hub_degrees[0]), live=False, expect=dict(hub=True, last_slice=True))
    sz = new()
    stale = dict(first=list(gz["rows"]), second=[row(sz, gz["dst"], -1, "stale_negative"), row(sz, chain(3, sz)[-1], 3, "stale_far")])
    # e. two lanes want one target: A is supplied in the first 64 in-slots, B only by the last one (the early exit of k_pull and
    #    k_pull_hub must wait for B).  Cold decoys; B's witness lies above the high pools.  `levels`: A arrives a level before B
    #    (k_pull_hub: `have`, `want` and the fold of a hub one lane has seen already)
    def pair(b, ka, tag):
        t = tv(b)
        ca, cb, wb = chain(ka - 1), [new()], new(TOP)
        edges(cb[0], wb)
        lo, hi = in_list(2, b - 1, 3, False)
        edges(np.concatenate([lo, [ca[-1]], hi, [wb]]).astype(np.int64), t)
        r = [row(cb[0], t, 2, tag + "_B"), row(ca[0], t, ka, tag + "_A")]
        gadgets.append(dict(tag=tag, family="pair", k=2, b=b, p=b - 1, live=False, detour=False, src=cb[0], dst=t, path=[cb[0], wb, t],
                            rows=r, expect=dict(hub=b > C, first=3), cut=[(wb, t), (ca[-1], t)]))
        pairs.append(r)

    for b in (65, 129, 4 * S + 1):
        pair(b, 2, "pair_b%d" % b)
        pair(b, 1, "pair_levels_b%d" % b)
    # f. frontier records: a witness that carries 1, 2, 3, 9, 10, 11 lanes (k_pull_lanes: two ids inline, the tail queue from
    #    the third, the dense row from the eleventh)
    segment()
    for m in (1, 2, 3, 9, 10, 11):
        gadget("lanes", 2, 3, 1, n_src=m, tag="lanes_%d" % m)
    # sources in 3 and in 4 lane-words (k_compact_frontier: three words inline, the fourth out of cw), and lists whose live
    # entries each spill a fourth word: under and over k_pull_sparse's queue (their decoys carry the four spread lanes)
    gadget("spread", 2, 3, 1, live=False, srcs=spread[:3], tag="spread_3words")
    gadget("spread", 2, 3, 1, live=False, srcs=spread, tag="spread_4words")
    for b in (100, 200):
        if b <= C and b + L["vertex_weight"] <= W:
            v0 = segment()[0] + 1
            gadget("spill", 2, b, last(b), expect=dict(v0=v0, own=0, prel=b - 1))
    # g. top-down: the witness edge in the last slot of the first, a middle and the last item of `push_chunk` out-edges
    sinks = new(MID, 256)
    push_src = [T + 62, T + 63, T + 64, T + 65]
    n_push = [0]

    def push(k, d, q, src=None):
        c = chain(k - 1, src)
        t = new()
        junk = sinks[(37 * n_push[0] + np.arange(d - 1)) % len(sinks)]
        n_push[0] += 1
        edges(c[-1], np.concatenate([junk[:q], [t], junk[q:]]).astype(np.int64))
        tag = "push_k%d_d%d_q%d" % (k, d, q)
        if tag in tags:
            tag += "_n%d" % len(gadgets)
        tags.add(tag)
        gadgets.append(dict(tag=tag, family="push", k=k, b=1, p=0, live=False, detour=False, src=c[0], dst=t, path=c + [t],
                            rows=[row(c[0], t, k, tag)], expect=dict(out_deg=d, out_slot=q, item=q // PC)))
        return gadgets[-1]

    for d in PUSH_DEGREES:
        items = (d + PC - 1) // PC
        for q in sorted({min(d, (i + 1) * PC) - 1 for i in (0, items // 2, items - 1)} | {0}):
            for k in (1, 2):
                push(k, d, q, src=push_src.pop() if push_src and k == 1 and q == d - 1 else None)
    for d, q in ((65, 64), (129, 128), (64, 63)):
        push(5, d, q)  # the fifth level's frontier is a handful of vertices: top-down after bottom-up levels
    # the tail: the last part ends at V, its in-slots are the last of the graph (rpk and rown are padded behind them), and
    # the last vertex is a source
    t_last = new(TAIL)
    gadget("tail", 2, 6, 5, t=t_last, expect=dict(closes=False, ends_at_V=True))
    push(1, 65, 64, src=new(TAIL))["expect"]["last_vertex"] = True

    base = np.concatenate([[0], np.cumsum([len(tdeg)] + [count[z] for z in (LOW, MID, HIGH, TOP, TAIL)])])
    real = lambda v: base[np.asarray(v, dtype=np.int64) >> _Z] + (np.asarray(v, dtype=np.int64) & 0xFFFFFFFF)
    for g in gadgets:
        # per row, the edge whose removal must change the row's answer (None: a negative row)
        cut = g.pop("cut", None) or [(g["path"][-2], g["path"][-1])] * len(g["rows"])
        g["cut"] = [None if r in negative else (int(real(u)), int(real(v))) for r, (u, v) in zip(g["rows"], cut)]
        g["src"], g["dst"] = int(real(g["src"])), int(real(g["dst"]))
        g["path"] = [int(v) for v in real(g["path"])]
        if "v0" in g["expect"]:
            g["expect"]["v0"] = int(real(g["expect"]["v0"]))
    src, dst = real(np.concatenate(es)), real(np.concatenate(ed))
    assert (np.bincount(dst, minlength=len(tdeg))[:len(tdeg)] == np.array(tdeg)).all(), "the target zone's in-degrees are the declared ones"
    spread_rows = fixed + ballast + [r for g in gadgets if g["family"] in ("spread", "spill") for r in g["rows"]]
    return PullGadgets(V=int(base[-1]), src=src, dst=dst, rs=real([r[0] for r in rows]), rd=real([r[1] for r in rows]),
                       dist=np.array([r[2] for r in rows], dtype=np.int64), tag=np.array([r[3] for r in rows]), gadgets=gadgets,
                       fixed=fixed, pairs=pairs, stale=stale, spread=np.array(spread_rows, dtype=np.int64), negative=negative,
                       part_weight=part_weight, hub_chunk=hub_chunk, n_targets=len(tdeg), spread_sources=[int(real(s)) for s in spread])


# ---- gadgets on the queue, list, cap and row limits of k_bibfs ------------------------------------------------------------
# Every constant the gadgets sit on, and where it was read (test_bibfs_gadgets_cpu.py reads them back from the sources):
BIBFS_LIMITS = dict(
    queue_floor=1024,   # pgq_meet.hip, `qcap = std::max(1024, ...bibfs_queue)` in the chain and in meet_bidirectional
    cap_floor=1,        # launch_bibfs, `std::max(1, options().bibfs_cap)`
    block=1024,         # `__launch_bounds__(1024) void k_bibfs(`: 16 wavefronts
    walk_stride=16,     # k_bibfs, `nf[side], wib, 16, xoff, xadj`: wavefront w takes the queue positions w + 16 * lane
    walk_lanes=64,      # pgq_walk.h, `pb += 64 * stride` and `min(64, (list_n - pb + stride - 1) / stride)`
    chunk=256,          # pgq_walk.h, `q += 256`: four entries per lane, from `b & ~3`
    depth=2,            # pgq_meet.hip, `#define PGQ_BIBFS_DEPTH 2`
    rows=256,           # pgq_internal.h, `int bibfs_rows = 256;`
    rows_max=16384,     # pgq_internal.h, `int bibfs_rows_max = 16384;`
    rows_edges=4096,    # the chain, `std::min<int64_t>(opt.bibfs_rows_max, c->E / 4096)`
    far_rows_start=1)   # pgq_internal.h, `meet_far_rows { 1 }`
BIBFS_HUB = 2304        # in-edges of the hub behind every guarded destination: more than any forward frontier has work (2049)
BIBFS_TEST_CAP = 300    # the bibfs_cap the `cap` family is built for
BIBFS_POSITIONS = {1024: (1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024), 2048: (1025, 2047, 2048)}
BIBFS_LENGTHS = (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 769, 1025)
BIBFS_TIES = (1, 5, 64)
BIBFS_FAR = (5, 6, 7, 8, 9)


class BibfsGadgets:
    """V, the edge table, and the rows as columns: rs, rd, dist (the builder's claim, -1 = no path; the tests take the oracle's),
    fam (family), q (the bibfs_queue the row is built for, 0: any), a and b (positions: F, i; slots: gadget, slot or -1 for the
    decoy row; queue: level size; cap: frontier work; tie: k; far: distance, kind).  slots: per gadget (L, start offset mod 4,
    frontier vertex, is it the last vertex with edges)."""

    def __init__(self, V, src, dst, rs, rd, dist, fam, q, a, b, slots):
        self.V, self.src, self.dst, self.rs, self.rd, self.dist, self.fam, self.q, self.a, self.b = V, src, dst, rs, rd, dist, fam, q, a, b
        self.slots = slots

    def transposed(self):
        """Every edge and every row reversed: the backward side walks what the forward side walked."""
        return BibfsGadgets(self.V, self.dst, self.src, self.rd, self.rs, self.dist, self.fam, self.q, self.a, self.b, self.slots)

    def rows_where(self, fam, q=None):
        return np.flatnonzero((self.fam == fam) & ((self.q == q) if q is not None else True))

    def tag(self, r):
        return "%s(%d, %d) for bibfs_queue %d" % (self.fam[r], self.a[r], self.b[r], self.q[r])


class _Builder:
    def __init__(self):
        self.n, self.es, self.ed, self.rows = 0, [], [], []

    def new(self, n=None):
        at = self.n
        self.n += 1 if n is None else n
        return at if n is None else np.arange(at, at + n, dtype=np.int64)

    def edge(self, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
        self.es.append(a.ravel()), self.ed.append(b.ravel())

    def n_edges(self):
        return sum(len(x) for x in self.es)

    def hub(self):
        """A vertex with BIBFS_HUB in-edges from eight sources nothing leads to: a destination with an in-edge from it has a
        backward side that costs more than any forward level here once it has been expanded by one level."""
        g = self.new()
        self.edge(np.repeat(self.new(8), BIBFS_HUB // 8), g)
        return g

    def row(self, s, d, dist, fam, q, a, b):
        self.rows.append((int(s), int(d), dist, fam, q, a, b))

    def finish(self, slots=()):
        col = lambda k, t: np.array([r[k] for r in self.rows], dtype=t)
        return BibfsGadgets(self.n, np.concatenate(self.es), np.concatenate(self.ed), col(0, np.int64), col(1, np.int64), col(2, np.int64),
                            col(3, object), col(4, np.int64), col(5, np.int64), col(6, np.int64), list(slots))


def bibfs_gadgets():
    """One graph, seven families (the `stale` family is bibfs_stale_gadgets: it needs ids of its own).  No family rests on where
    a vertex lands in the frontier queue: a family asks one row per member, and every queue position or list slot is the only
    witness of exactly one row.  A guarded destination t has two in-edges, one from its path and one from the hub: the backward
    side expands t once and is dearer than the forward side from then on, so the forward side walks the level under test and
    meets the path's last inner vertex there (test_bibfs_gadgets_cpu.py asserts this on the model's trace)."""
    B = _Builder()
    g = B.hub()
    sink = B.new()
    # positions: s -> f_i -> u_i -> t_i; the row (s, t_i) is met where the walk over the F queue positions reaches f_i's list
    for q, Fs in sorted(BIBFS_POSITIONS.items()):
        for F, thirds in [(F, False) for F in Fs] + ([(1024, True)] if q == 1024 else []):
            s, f, u, t = B.new(), B.new(F), B.new(F), B.new(F)
            live = np.arange(F) % 3 != 1 if thirds else np.ones(F, dtype=bool)  # every third f_i a dead end between live ones
            B.edge(s, f), B.edge(f[live], u[live]), B.edge(u, t), B.edge(g, t)
            for i in range(F):
                B.row(s, t[i], 3 if live[i] else -1, "positions", q, F + (1 << 20 if thirds else 0), i)
    # queue: a level of Q new vertices on the only path
    for q in (1024, 2048):
        for Q in (q, q + 1):
            s, f, m, t = B.new(), B.new(Q), B.new(4), B.new()
            B.edge(s, f), B.edge(f, m[0]), B.edge(m[:-1], m[1:]), B.edge(m[-1], t), B.edge(g, t)
            B.row(s, t, 6, "queue", q, Q, 0)
    # cap: the forward side's work is C when a + b = 6, on a path of 8 edges
    for C in (BIBFS_TEST_CAP, BIBFS_TEST_CAP + 1):
        s, p, y, m, t = B.new(), B.new(5), B.new(C), B.new(), B.new()
        B.edge(s, p[0]), B.edge(p[:-1], p[1:]), B.edge(p[-1], y), B.edge(y, m), B.edge(m, t), B.edge(g, t)
        B.row(s, t, 8, "cap", 0, C, 0)
    # tie: equal work on both sides and no path; the forward side covers 2 k entries, the backward side k
    for k in BIBFS_TIES:
        s, u, v, d, ds = B.new(), B.new(k), B.new(), B.new(), B.new(k)
        B.edge(s, u), B.edge(u, v), B.edge(ds, d)
        B.row(s, d, -1, "tie", 0, k, 0)
    # far: two fans of three joined by a chain
    ends = []
    for D in BIBFS_FAR:
        s, a, m, b, t = B.new(), B.new(3), B.new(D - 3), B.new(3), B.new()
        B.edge(s, a), B.edge(a, m[0]), B.edge(m[:-1], m[1:]), B.edge(m[-1], b), B.edge(b, t)
        B.row(s, t, D, "far", 0, D, 0), B.row(t, s, -1, "far", 0, D, 1), B.row(a[1], t, D - 1, "far", 0, D, 2)
        for s0, t0 in ends:
            B.row(s, t0, -1, "far", 0, D, 3), B.row(s0, t, -1, "far", 0, D, 3)
        ends.append((s, t))
    # slots: s -> f, f's list x_0 .. x_{L-1}, x_j -> t_j.  The lists of [aligner, pad, f, above] stand side by side at the end of
    # the adjacency: the aligner brings the offset to a multiple of 4, the pad's k entries put f's list at offset k mod 4, and
    # the pad's and the upper neighbour's entries are the decoy row's destination: an unmasked head or tail meets it
    todo = [(L, k, False) for L in BIBFS_LENGTHS for k in range(4)] + [(257, 3, True)]
    low = []
    for L, k, last in todo:
        s, x, t, dstar = B.new(), B.new(L), B.new(L), B.new()
        B.edge(x, t), B.edge(g, t), B.edge(g, dstar)
        low.append((s, x, t, dstar))
    at = B.n_edges() + len(todo)  # every edge of a source below the quads, the s -> f edges included
    slots = []
    for n, ((L, k, last), (s, x, t, dstar)) in enumerate(zip(todo, low)):
        al, pad, f = B.new(), B.new(), B.new()
        B.edge(s, f)
        B.edge(np.full(-at % 4, al), sink), B.edge(np.full(k, pad), dstar), B.edge(f, x)
        at += -at % 4 + k
        assert at % 4 == k
        at += L
        if not last:
            B.edge(np.full(3, B.new()), dstar)
            at += 3
        slots.append((L, k, f, last))
        for j in range(L):
            B.row(s, t[j], 3, "slots", 0, n, j)
        B.row(s, dstar, -1, "slots", 0, n, -1)
    return B.finish(slots)


BIBFS_SHIPPED_CAP = 8 << 20  # pgq_internal.h, `int bibfs_cap = 8 << 20;`


def bibfs_calls(g):
    """The calls the families are asked in: (name, family, bibfs_queue, bibfs_cap, row indices)."""
    out = []
    for fam, q in (("positions", 1024), ("positions", 2048), ("slots", 0), ("queue", 1024), ("queue", 2048), ("cap", 0), ("tie", 0), ("far", 0)):
        out.append(("%s_%d" % (fam, q) if q else fam, fam, q or 1024, BIBFS_TEST_CAP if fam == "cap" else BIBFS_SHIPPED_CAP, g.rows_where(fam, q)))
    return out


def bibfs_stale_gadgets(grid, qcap=1024):
    """Rows that leave a global map dirty, and behind each, on the same workgroup, a row that needs it clean.  Per variant
    (the dirty row lists qcap - 1, qcap, qcap + 1 words): a -> c_1 .. c_T -> d', every c_i alone in its map word; the dirty row
    (a, z) has no path and a dear backward side, so the forward side marks every c_i.  Victim (s', d') has no path and a dear
    forward side: its backward side reaches every c_i and meets nothing, unless a forward bit of the row before is still
    there.  Victim (s''_w, d') is two hops apart by s''_w -> c_w: a forward bit of c_w left behind drops c_w from its
    frontier.  d' stands in a's map word, so the last words listed are the c_i's.  Laid out as grid dirty rows, grid victims,
    grid dirty rows, grid victims of the second kind: workgroup w of a bulk call with `grid` workgroups runs one of each,
    in this order (the device queues rows per wavefront of 64 in the order their atomics land: a call whose wavefronts land out
    of order checks less, never wrongly).  Returns the gadgets (a: listed words, b: 0 dirty, 1, 2 the victims) and T per variant."""
    B = _Builder()
    dear = 1400  # entries of a dear side: more than T + grid, in lists of four vertices (a level of four)
    assert qcap - 2 + grid < dear and grid < qcap - 4
    Ts = {}
    for listed in (qcap - 1, qcap, qcap + 1):
        T = listed - 3  # the row's own two words, the c_i's, the spare word of the forward map
        Ts[listed] = T
        base = (B.n + 31) // 32 * 32
        B.n = base + 32 * (T + 2)
        a, dp, c = base, base + 1, base + 32 * np.arange(1, T + 1, dtype=np.int64)
        z, sp, s2 = B.new(), B.new(), B.new(grid)
        B.edge(a, c), B.edge(c, dp), B.edge(np.repeat(B.new(4), dear // 4), z), B.edge(sp, np.repeat(B.new(4), dear // 4)), B.edge(s2, c[:grid])
        for kind, (ss, dd, dist) in enumerate((([a] * grid, z, -1), ([sp] * grid, dp, -1), ([a] * grid, z, -1), (s2, dp, 2))):
            for s in ss:
                B.row(s, dd, dist, "stale", qcap, listed, (0, 1, 0, 2)[kind])
    return B.finish(), Ts


# ---- graphs for the upload's derived layout (tests/layout_model.py, test_layout_model_cpu.py, test_upload_layout_gpu.py) ------
# Four upload kernels walk 256 vertices per workgroup with a binary search over 257 LDS offsets (k_slot_sources, k_fill_padded,
# k_fill_packed<K>, k_two_hop_work); the grid-stride loops of the others take a second trip above LAYOUT_TRIPS.
LAYOUT_BLOCK_V = (1, 2, 255, 256, 257, 511, 512, 513, 769)
LAYOUT_LENGTHS = (0, 1, 2, 3, 4, 5, 30, 31, 32, 33, 62, 63, 64, 65, 127, 128, 129)
LAYOUT_LONG = 700                     # one list longer than two 256-thread trips
LAYOUT_PREFIX = (0, 64, 63, 129)      # lists of vertices 0 .. 3: see layout_blocks
LAYOUT_TRIPS = dict(
    slot_sources_v=2048 * 256,        # k_slot_sources: grid_for(V, 256, 256 * 8) workgroups of 256 rows
    degree_stats_v=1024 * 256,        # k_degree_stats: grid_for(V, 256, 1024) workgroups of 256 threads
    slots_e=4096 * 256,               # k_narrow_adj, k_check_rows, k_gather_rows, k_any_negative: grid_for(E) x 256 threads
    tail_v=257, tail_e=300,
)


class LayoutGraph:
    """An edge table in slot order of its forward CSR (rows sorted by source, stably)."""

    def __init__(self, name, V, src, dst):
        self.name, self.V = name, int(V)
        self.src, self.dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)

    def transposed(self):
        return LayoutGraph(self.name + "_T", self.V, self.dst, self.src)

    def csr(self):
        off, adj, _ = csr_arrays_from_rows(self.V, self.src, self.dst)
        return off, adj


def layout_blocks(V, seed=0):
    """Family a.  Out- and in-list lengths from LAYOUT_LENGTHS; one out-list and one in-list of LAYOUT_LONG entries; empty
    lists (both directions) at the first and the last vertex of every block of 256, so vertex 0 and vertex V - 1 have no
    in-edges and k_row_bounds closes a gap at both ends; at V = 769 the whole block 256 .. 511 is empty between two full ones.
    Vertices 1, 2, 3 have lists of 64, 63 and 129 entries in both directions: counted from the block's first slot, as
    k_two_hop_work's wavefront trips are, the first starts on lane 0 and ends on lane 63, the second starts on lane 0, the third
    starts on lane 63 of one trip and ends on lane 63 of the third.  One slack vertex per direction takes up the difference
    of the two degree sums (its length is the only one not in the list).  Destinations are a seeded permutation of the in-degree
    multiset: parallel edges and self loops occur (test_layout_model_cpu.py counts them).  V = 1 and V = 2 cannot have edges
    AND no in-edges at both ends: they are a vertex with five self loops, and two vertices with lists of 4 and 2."""
    if V == 1:
        return LayoutGraph("blocks_1", 1, np.zeros(5), np.zeros(5))
    if V == 2:
        return LayoutGraph("blocks_2", 2, [0, 0, 0, 0, 1, 1], [1, 1, 0, 1, 1, 0])
    rng = np.random.default_rng(1000 * V + seed)
    v = np.arange(V)
    edge = (v % 256 == 0) | (v % 256 == 255) | (v == V - 1)
    if V == 769:
        edge |= (v >= 256) & (v < 512)
    free = np.flatnonzero(~edge)
    free = free[free >= len(LAYOUT_PREFIX)]
    degs = []
    for _ in range(2):
        d = np.zeros(V, dtype=np.int64)
        d[free] = rng.choice(LAYOUT_LENGTHS, len(free))
        d[free[:len(LAYOUT_LENGTHS)]] = rng.permutation(LAYOUT_LENGTHS)  # every length at least once
        d[:len(LAYOUT_PREFIX)] = LAYOUT_PREFIX
        degs.append(d)
    out, ind = degs
    hubs = free[-4:]  # out hub, in hub, out slack, in slack: the last free vertices
    out[hubs[0]], ind[hubs[1]] = LAYOUT_LONG, LAYOUT_LONG
    out[hubs[2]] = ind[hubs[3]] = 0
    diff = int(out.sum() - ind.sum())
    if diff > 0:
        ind[hubs[3]] = diff
    else:
        out[hubs[2]] = -diff
    src = np.repeat(v, out)
    dst = rng.permutation(np.repeat(v, ind))
    return LayoutGraph("blocks_%d" % V, V, src, dst)


def layout_saturation():
    """Family b.  h has 65,536 parallel slots to w and w has 65,536 slots: h's two-hop walk holds 2^32 entries, its work
    saturates at 2^32 - 1.  The twin h2 has 65,535 slots to w2, w2 65,536: 2^32 - 65,536, the largest sum below.  w and w2 spread
    their slots over 32 sinks.  262,143 edges."""
    h, w, h2, w2, sinks = 1, 2, 3, 4, np.arange(8, 40)
    n = 1 << 16
    src = np.concatenate([np.full(n, h), np.full(n, w), np.full(n - 1, h2), np.full(n, w2)])
    dst = np.concatenate([np.full(n, w), sinks[np.arange(n) % 32], np.full(n - 1, w2), sinks[np.arange(n) % 32]])
    g = LayoutGraph("saturation", 64, src, dst)
    g.h, g.h2 = h, h2
    return g


def layout_second_trips(vb=LAYOUT_TRIPS["slot_sources_v"], eb=LAYOUT_TRIPS["slots_e"], tail_v=LAYOUT_TRIPS["tail_v"],
                        tail_e=LAYOUT_TRIPS["tail_e"]):
    """Family c.  V = vb + tail_v, E = eb + tail_e (eb = 2 vb): the first vb vertices have two slots each into the first vb
    vertices (in-degree 2 each), the last tail_v vertices own the last tail_e slots, which point at the last tail_v vertices:
    most of them at V - 2, which so has the largest in-degree, vertex V - 3 has the largest out-degree, and the very last slot
    points at V - 1.  A kernel that loses the trip past vb vertices or eb slots leaves exactly these unwritten."""
    assert eb == 2 * vb and tail_e >= tail_v + 8 and tail_v >= 8
    V = vb + tail_v
    a = np.arange(vb, dtype=np.int64)
    src = np.concatenate([np.repeat(a, 2), vb + np.arange(tail_v), np.full(tail_e - tail_v, V - 3)])
    dst = np.concatenate([np.stack([(a * 7 + 1) % vb, (a * 11 + 5) % vb], axis=1).ravel(),
                          np.where(np.arange(tail_v) % 3 == 0, vb + np.arange(tail_v), V - 2),
                          np.where(np.arange(tail_e - tail_v) % 2 == 0, V - 2, vb + np.arange(tail_e - tail_v) % tail_v)])
    order = np.argsort(src, kind="stable")
    src, dst = src[order], dst[order]
    dst[-1] = V - 1
    return LayoutGraph("second_trips_%d" % V, V, src, dst)


def layout_id_width(V):
    """Family d.  The top id V - 1 in every position of a 16-byte group of six (V <= 2^21) or five ids: vertex k's list of six
    has it at position k (the CSR's order, meet_pack_order = 0), vertex 8's list is six parallel edges to it (every position
    under either order), and the top vertex has a list of its own, so that its id stands in in-lists too.  A few dozen edges."""
    top = V - 1
    src, dst = [], []
    for k in range(6):
        lst = [100 + 10 * k + j for j in range(6)]
        lst[k] = top
        src += [k] * 6
        dst += lst
    src += [8] * 6 + [top] * 7
    dst += [top] * 6 + [0, 1, 2, 3, 100, 101, top]
    src, dst = np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64)
    order = np.argsort(src, kind="stable")
    return LayoutGraph("id_width_%d" % V, V, src[order], dst[order])


def layout_end_bit(V, seed=3):
    """Family d, the radix sorts' end_bit: a random graph on V = 2^k or 2^k + 1 vertices with edges into and out of vertex V - 1."""
    rng = np.random.default_rng(V + seed)
    src = np.concatenate([rng.integers(0, V, 6 * V), np.full(9, V - 1), rng.integers(0, V, 9)])
    dst = np.concatenate([rng.integers(0, V, 6 * V), rng.integers(0, V, 9), np.full(9, V - 1)])
    order = np.argsort(src, kind="stable")
    return LayoutGraph("end_bit_%d" % V, V, src[order], dst[order])


# ---- rows for k_src_ball (pgq_ball.h) at the line boundary of the fixed-stride in-list heads -----------------------------------
# rhead keeps a vertex's in-degree in word 31, the last word of its first 128-byte line, entries 0 .. 30 before it and entries
# 31 .. 62 in the second line; k_src_ball masks word 31 out of its membership test and reads entries 63 and on from rpadj.
BALL_LINE_DEGREES = (1, 30, 31, 32, 33, 62, 63, 64)
BALL_LINE_POSITIONS = (0, 30, 31, 61, 62, 63)
BALL_COUNT_DEGREES = (31, 32, 62, 63, 64)
_BALL_CORE, _BALL_POOL = 80, 80


def ball_line_gadgets():
    """A sibling of degree_gadgets for the heads.  Two families, each built as it stands and mirrored (every edge and row
    reversed), so that the graph and its transpose both hold them:

    line   s -> m1 -> m2 -> dst for every in-degree b of BALL_LINE_DEGREES and every position p of BALL_LINE_POSITIONS below b:
           m2 is entry p of dst's in-list and the only in-neighbour within two hops of s; the other b - 1 are decoys, roots
           nothing points at, p of them with ids below m2 and the rest above (in-lists are in source-id order).  One s, m1, m2
           for all of them: distance 3, the rows of one source side by side.
    count  s2 -> q -> {vertices 31, 32, 62, 63, 64}: the ids that are in-degrees lie in s2's two-hop set.  For every c of
           BALL_COUNT_DEGREES a destination of in-degree c whose in-neighbours are c decoys (unreachable), and one with c - 1
           decoys and x_c, where vertex c -> x_c: distance 4.  A kernel that tests the count word as an entry finds `c` in the
           set and answers 3.  s2's rows to every line destination too (unreachable; five of them have such an in-degree).

    Ids: 0 .. 79 the core (the count family's s2 = 0, q = 1, the five id-named vertices, the mirrored s2 = 2, q = 3, the rest
    isolated), then the low decoy pools (roots, sinks for the mirrored half), then every other vertex, then the high pools.
    Returns a Gadgets whose records have kind ('line' / 'count4' / 'count_unreachable'), a, b (the out-degree of the row's source
    and the in-degree of its destination: a mirrored record carries the degree in a until the graph is transposed), pos and
    mirrored."""
    n = [_BALL_CORE + 2 * _BALL_POOL]
    low = {False: np.arange(_BALL_CORE, _BALL_CORE + _BALL_POOL), True: np.arange(_BALL_CORE + _BALL_POOL, _BALL_CORE + 2 * _BALL_POOL)}

    def new():
        n[0] += 1
        return n[0] - 1

    es, ed, rs, rd, dist, tag, gadgets = [], [], [], [], [], [], []
    pending = []  # in-lists that take high decoys: the pools' ids are known at the end

    def edge(a, b, flip):
        es.append(b if flip else a), ed.append(a if flip else b)

    def row(a, b, k, t, flip, **rec):
        rs.append(b if flip else a), rd.append(a if flip else b), dist.append(k), tag.append(t)
        if rec:  # a, b: out-degree of the row's source, in-degree of its destination, as in degree_gadgets
            deg = rec.pop("deg")
            gadgets.append(dict(rec, tag=t, k=k, a=deg if flip else 1, b=1 if flip else deg, src=rs[-1], dst=rd[-1], tie=False,
                                row=len(rs) - 1, mirrored=flip))

    def in_list(dst, n_low, mid, n_high, flip):
        for v in low[flip][:n_low]:
            edge(int(v), dst, flip)
        if mid is not None:
            edge(mid, dst, flip)
        pending.append((dst, n_high, flip))

    for flip in (False, True):
        m = "_m" if flip else ""
        s, m1, m2 = new(), new(), new()
        edge(s, m1, flip), edge(m1, m2, flip)
        s2, q = (2, 3) if flip else (0, 1)
        edge(s2, q, flip)
        for c in BALL_COUNT_DEGREES:
            edge(q, c, flip)
        line_dsts = []
        for b in BALL_LINE_DEGREES:
            for p in BALL_LINE_POSITIONS:
                if p >= b:
                    continue
                d = new()
                in_list(d, p, m2, b - 1 - p, flip)
                row(s, d, 3, "line_b%d_p%d%s" % (b, p, m), flip, kind="line", deg=b, pos=p, paths=[[s, m1, m2, d][::-1 if flip else 1]])
                line_dsts.append((d, b, p))
        for c in BALL_COUNT_DEGREES:
            x, d4, du = new(), new(), new()
            edge(c, x, flip)
            in_list(d4, c // 2, x, c - 1 - c // 2, flip)
            in_list(du, c // 2, None, c - c // 2, flip)
            row(s2, d4, 4, "count_c%d_far%s" % (c, m), flip, kind="count4", deg=c, pos=c // 2, paths=[[s2, q, c, x, d4][::-1 if flip else 1]])
            row(s2, du, -1, "count_c%d_unreachable%s" % (c, m), flip, kind="count_unreachable", deg=c, pos=None, paths=[])
        for d, b, p in line_dsts:
            row(s2, d, -1, "count_line_b%d_p%d%s" % (b, p, m), flip)
    high = {False: np.arange(n[0], n[0] + _BALL_POOL), True: np.arange(n[0] + _BALL_POOL, n[0] + 2 * _BALL_POOL)}
    for dst, n_high, flip in pending:
        for v in high[flip][:n_high]:
            edge(int(v), dst, flip)
    V = n[0] + 2 * _BALL_POOL
    i64 = lambda a: np.array(a, dtype=np.int64)
    src, dst = i64(es), i64(ed)
    order = np.argsort(src, kind="stable")  # table order = slot order
    return Gadgets(V, src[order], dst[order], i64(rs), i64(rd), i64(dist), np.array(tag), gadgets)
