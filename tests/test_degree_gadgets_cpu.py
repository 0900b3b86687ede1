"""helpers.degree_gadgets and helpers.lcc_gadgets are what test_degree_edges_gpu.py assumes: checked here with numpy and the
CPU oracle alone.

Every gadget's endpoint degrees and the index of its path vertex in the out-list (table order) and in the in-list (source-id
order) are read back from the CSR arrays, for the graph and for its transpose; every row's distance is the oracle's; without
the first edge of its path a gadget's row is unreachable or farther, so the path through the chosen slot is the only shortest
one; and every (degree, position) cell of the issue's lists exists at each distance 1 .. 4, on the out- and on the in-side."""
import numpy as np
import pytest

from helpers import (BALL_COUNT_DEGREES, BALL_LINE_DEGREES, BALL_LINE_POSITIONS, GADGET_DEGREES, GADGET_POSITIONS, LCC_DEGREES,
                     LDS_LIMITS, ball_line_gadgets, csr_arrays_from_rows, decoy_len, degree_gadgets, gadget_index, lcc_gadgets,
                     spread_ids)
from oracle.pgq_oracle import OracleCSR


def oracle_dist(g, rs, rd, src=None, dst=None):
    ora = OracleCSR.from_edges(g.V, g.src if src is None else src, g.dst if dst is None else dst)
    ln, ok = ora.lean_iterativelength(g.V, rs, rd, nthreads=8)
    return np.where(ok, ln, -1)


class Built:
    def __init__(self, g):
        self.g = g
        self.off, self.adj, _ = csr_arrays_from_rows(g.V, g.src, g.dst)
        # in-lists as the upload builds them: the transpose's rows sorted by source id (stable)
        by_src = np.argsort(g.src, kind="stable")
        self.roff, self.radj, _ = csr_arrays_from_rows(g.V, g.dst[by_src], g.src[by_src])

    def out_list(self, v):
        return self.adj[self.off[v]:self.off[v + 1]]

    def in_list(self, v):
        return self.radj[self.roff[v]:self.roff[v + 1]]


@pytest.fixture(scope="module")
def both():
    g = degree_gadgets()
    return [Built(g), Built(g.transposed())]


def test_size_limits(both):
    g = both[0].g
    assert g.V < LDS_LIMITS["ball_2_per_cu"], "every LDS-map kernel keeps its map in LDS"
    assert 0.5e6 < len(g.src) < 1.1e6
    assert g.src.min() >= 0 and g.dst.min() >= 0 and g.src.max() < g.V and g.dst.max() < g.V
    assert len(set(g.tag.tolist())) == len(g.tag), "tags name one row each"


def test_decoy_lists_cover_every_group_fill_and_segment_start(both):
    lens = {decoy_len(j) for j in range(96)}
    assert lens == set(range(8)) | {255, 256, 257}
    for k in (4, 5, 6):  # ids per 16-byte group of the padded lists: every fill of the last group
        assert {n % k for n in lens if n} == set(range(k)), k
    for b in both:  # the lists of the decoys of one long list start at every offset mod 4
        g = next(x for x in b.g.gadgets if x["a"] == 4097 and x["b"] == 4097 and x["pos"] == "last" and x["k"] == 3)
        assert set((b.off[b.out_list(g["src"])] % 4).tolist()) == {0, 1, 2, 3}
        assert set((b.roff[b.in_list(g["dst"])] % 4).tolist()) == {0, 1, 2, 3}


def test_degrees_and_slots(both):
    for b in both:
        for g in b.g.gadgets:
            out, inn = b.out_list(g["src"]), b.in_list(g["dst"])
            assert len(out) == g["a"] and len(inn) == g["b"], g["tag"]
            if g["tie"]:
                firsts, lasts = {p[1] for p in g["paths"]}, {p[-2] for p in g["paths"]}
                assert out[0] in firsts and out[-1] in firsts and inn[0] in lasts and inn[-1] in lasts, g["tag"]
                continue
            (path,) = g["paths"]
            assert len(path) == g["k"] + 1
            ia, ib = gadget_index(g["pos"], g["a"]), gadget_index(g["pos"], g["b"])
            assert out[ia] == path[1] and (out == path[1]).sum() == 1, g["tag"]
            assert inn[ib] == path[-2] and (inn == path[-2]).sum() == 1, g["tag"]
            for u, v in zip(path[:-1], path[1:]):
                assert v in b.out_list(u), g["tag"]


def test_tie_gadgets_order_ids_against_slots(both):
    b = both[0]
    ties = [g for g in b.g.gadgets if g["tie"]]
    assert {(g["k"], len(g["paths"])) for g in ties} == {(k, n) for k in (2, 3, 4) for n in (2, 3)}
    for g in ties:
        out = b.out_list(g["src"])
        slots = [int(np.flatnonzero(out == p[1])[0]) for p in g["paths"]]
        ids = [p[1] for p in g["paths"]]
        assert slots == sorted(slots) and slots[0] == 0 and slots[-1] == g["a"] - 1, g["tag"]
        assert ids == sorted(ids, reverse=True), g["tag"]  # the first slot holds the largest id


def test_oracle_distances(both):
    for b in both:
        g = b.g
        got = oracle_dist(g, g.rs, g.rd)
        bad = np.flatnonzero(got != g.dist)
        assert len(bad) == 0, (g.tag[bad[0]], int(got[bad[0]]), int(g.dist[bad[0]]))
    assert {1, 2, 3, 4, -1} == set(both[0].g.dist.tolist())


def test_the_path_through_the_slot_is_the_only_shortest_one(both):
    # every gadget's first path edge removed at once (the gadgets' paths are disjoint): each row is unreachable or farther
    for b in both:
        g = b.g
        plain = [x for x in g.gadgets if not x["tie"]]
        cut = {(x["paths"][0][0], x["paths"][0][1]) for x in plain}
        key = g.src * g.V + g.dst
        keep = ~np.isin(key, [s * g.V + d for s, d in cut])
        assert (~keep).sum() == len(plain), "one table row per path edge"
        rows = np.array([x["row"] for x in plain])
        got = oracle_dist(g, g.rs[rows], g.rd[rows], g.src[keep], g.dst[keep])
        bad = [x["tag"] for x, d in zip(plain, got) if d != -1 and d <= x["k"]]
        assert not bad, bad[:5]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_threshold_and_position_at_each_distance(both, k):
    cells = 0
    for b in both:  # a cell counts on the out-side of src (a) and on the in-side of dst (b)
        have_a = {(g["a"], gadget_index(g["pos"], g["a"])) for g in b.g.gadgets if g["k"] == k and not g["tie"]}
        have_b = {(g["b"], gadget_index(g["pos"], g["b"])) for g in b.g.gadgets if g["k"] == k and not g["tie"]}
        for x in GADGET_DEGREES:
            for pos in GADGET_POSITIONS:
                idx = gadget_index(pos, x)
                if idx is None:
                    continue
                assert (x, idx) in have_a and (x, idx) in have_b, (k, x, pos)
                cells += 1
        pairs = {(g["a"], g["b"]) for g in b.g.gadgets if g["k"] == k}
        for x in GADGET_DEGREES:
            assert {(x, x), (x, 1), (1, x)} <= pairs, (k, x)
        assert (513, 4097) in pairs or (4097, 513) in pairs
    print("distance %d: %d (degree, position) cells present on both sides, in the graph and its transpose" % (k, cells))


def test_shifted_gadgets_keep_their_shape(both):
    g = both[0].g
    V = (1 << 21) + 1
    s = g.shifted(V)
    assert s.V == V and s.src.max() < V and s.rs.max() < V and (s.src - g.src == V - g.V).all()
    assert s.gadgets[5]["paths"][0][0] == g.gadgets[5]["paths"][0][0] + V - g.V


# ---- helpers.ball_line_gadgets: the rows for k_src_ball at the line boundary of the in-list heads ----------------------------
@pytest.fixture(scope="module")
def lines():
    g = ball_line_gadgets()
    return [Built(g), Built(g.transposed())]


def two_hop_set(b, s):
    one = b.out_list(s)
    two = np.concatenate([b.out_list(v) for v in one]) if len(one) else one
    return set(one.tolist()) | set(two.tolist()) | {int(s)}


def test_ball_line_gadgets(lines):
    assert (lines[0].g.rs >= 0).all() and lines[0].g.dst.max() < lines[0].g.V < 1000
    for side, b in enumerate(lines):
        g = b.g
        got = oracle_dist(g, g.rs, g.rd)
        bad = np.flatnonzero(got != g.dist)
        assert len(bad) == 0, (g.tag[bad[0]], int(got[bad[0]]), int(g.dist[bad[0]]))
        mine = [x for x in g.gadgets if x["mirrored"] == (side == 1)]  # the half whose in-lists this orientation holds
        cells, counts = set(), {}
        for x in mine:
            inn, ball = b.in_list(x["dst"]), two_hop_set(b, x["src"])
            assert len(inn) == x["b"], x["tag"]
            inside = [int(v) for v in inn if int(v) in ball]
            if x["kind"] == "line":
                m2 = x["paths"][0][-2]
                assert inside == [m2] and int(inn[x["pos"]]) == m2 and x["k"] == 3, x["tag"]  # the only witness, at its position
                assert all(len(b.in_list(v)) == 0 for v in inn if v != m2), x["tag"]       # the rest: roots nothing reaches
                cells.add((x["b"], x["pos"]))
            else:
                assert inside == [] and x["b"] in ball, x["tag"]  # no witness, and the vertex named like the count word is in the set
                counts.setdefault(x["b"], set()).add(x["kind"])
                if x["kind"] == "count4":
                    assert x["k"] == 4 and int(inn[x["pos"]]) == x["paths"][0][-2] and x["paths"][0][2] == x["b"]
                else:
                    assert x["k"] == -1
        assert cells == {(d, p) for d in BALL_LINE_DEGREES for p in BALL_LINE_POSITIONS if p < d}
        assert counts == {c: {"count4", "count_unreachable"} for c in BALL_COUNT_DEGREES}
        # s2's rows to the line destinations: unreachable, and every in-degree that is an id of its set occurs
        s2 = next(x["src"] for x in mine if x["kind"] == "count4")
        extra = [i for i, t in enumerate(g.tag) if t.startswith("count_line_") and t.endswith("_m") == (side == 1)]
        assert all(g.rs[i] == s2 and g.dist[i] == -1 for i in extra)
        assert {len(b.in_list(g.rd[i])) for i in extra} >= set(BALL_COUNT_DEGREES)
        # without the witness's edge into the destination every line row is unreachable: no other path
        cut = {(x["paths"][0][-2], x["dst"]) for x in mine if x["kind"] == "line"}
        keep = ~np.isin(g.src * g.V + g.dst, [s * g.V + d for s, d in cut])
        assert (~keep).sum() == len(cut)
        rows = np.array([x["row"] for x in mine if x["kind"] == "line"])
        assert (oracle_dist(g, g.rs[rows], g.rd[rows], g.src[keep], g.dst[keep]) == -1).all()


def test_lcc_gadgets():
    n, s, d, hubs, deg = lcc_gadgets()
    off, adj, _ = csr_arrays_from_rows(n, s, d)
    assert (np.diff(off)[hubs] == deg).all() and set(deg.tolist()) == set(LCC_DEGREES)
    assert (deg >= 513).sum() > 256, "more long rows than k_lcc_big has workgroups"
    ora = OracleCSR.from_edges(n, s, d)
    got = ora.local_clustering_coefficient(hubs)
    for k in range(3 * len(LCC_DEGREES), len(hubs), 50):  # plain rows: one closing edge, last slot -> first slot
        h = hubs[k]
        first, last = adj[off[h]], adj[off[h + 1] - 1]
        assert adj[off[last]:off[last + 1]].tolist() == [first]
        assert got[k] == np.float32(1.0) / (np.float32(513) * np.float32(512))
    assert (got[:3 * len(LCC_DEGREES)] > 0).all()
    for V in (LDS_LIMITS["lcc_big"], LDS_LIMITS["lcc_big"] + 1):
        ids = spread_ids(np.random.default_rng(V % 1000), n, V)
        assert len(ids) == n and (np.diff(ids) > 0).all() and ids[0] == 0 and ids[-1] == V - 1
        assert ((ids >= (V - 1) // 32 * 32).sum()) == V - (V - 1) // 32 * 32
        assert (ids[adj[off[hubs[-1] + 1] - 1]] >= (V - 1) // 32 * 32), "a last-slot neighbour in the map's last word"
