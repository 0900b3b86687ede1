"""k_meet3 settles distance-3 and distance-4 rows from the hub tables: every answer is the CPU oracle's and the
same bytes as the call on a handle uploaded with meet_hubs = 0, and the read-only counters meet_hub3_settled, meet_hub4_settled
and meet4_batch_settled say which kernel answered a row.

The graph is built from disjoint gadgets on 65,536 vertices (k_meet4d's batch pass needs a vertex map of 4 KB per row).  256
designated hubs h_0 .. h_255 have exactly 400 - r edges (out-lists into a pool of sinks), every other vertex fewer than 145: with
meet_hubs = 256, meet_hub_min_degree = 1 and meet_hub_min_count = 1 hub h_r is bit r.  Every gadget is symmetric under turning
all edges round, and every test runs on the graph and on its transpose: no outcome depends on the endpoint k_meet3 expands.

kind        edges                                                  distance  P3  P4   answered by
d1_p3       s -> d,  s -> a -> h -> d                               1        yes      the distance-1 test
d2_p3       s -> m -> d,  s -> a -> h -> d                          2        yes      the distance-2 test
far_bit r   s -> a -> h_r -> d   (r = 0, 63, 64, 255)               3        yes      hub tables (hub two hops from s, one from d)
near_bit r  s -> h_r -> c -> d                                      3        yes      hub tables (hub one hop from s, two from d)
d3_plain    s -> a -> b -> d                                        3        no  no   the two-hop walk
d4_p4       s -> a -> h -> c -> d                                   4        no  yes  hub tables, after the walk ran to its end
d4_plain    s -> a -> x -> c -> d                                   4        no  no   k_meet4d
d5          s -> a -> h -> h' -> c -> d                             5        no  no   the stages behind k_meet3
none        s -> a -> h,  h' -> c -> d                              -        no  no   the stages behind k_meet3
capped      s -> a_1 .. a_130 (50 sinks each), c_1 .. c_130 -> d (50 roots each), a_130 -> c_130, a_1 -> h -> c_1
                                                                    3        no  yes  k_meet4d: under meet_cap = 64 the walk is cut
                                                                                      long before a_130's list, and a cut walk must
                                                                                      not be answered 4"""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from oracle.pgq_oracle import OracleCSR
from test_within_gpu import clamp

import hub_model

pytestmark = pytest.mark.gpu

KEYS = ("meet", "meet_bias", "meet_cap", "meet_cap_small", "meet4", "meet4_batch", "meet_pack", "meet_pack_order", "meet_small_rows",
        "meet_wide_rows", "meet_wide_rows_always", "meet_grid_mult", "meet_rows_per_wave", "meet_tail_rows", "ball", "route_memo",
        "route_timing", "calibration_cache", "meet_calibrate", "chunk_zero_copy", "streams", "lanes", "bibfs_rows",
        "meet_hubs", "meet_hub_min_degree", "meet_hub_min_count", "meet_hub_mb")
V, H = 65536, 256
SENTINEL = -7
BITS = (0, 63, 64, H - 1)


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    # k_meet3 sees every row of every call; k_meet4d's batch pass runs on every launch
    for k, v in (("meet", 1), ("meet_bias", 1e9), ("ball", 0), ("route_memo", 0), ("meet_small_rows", 0), ("meet4_batch", 2)):
        pgq.set_option(k, v)
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


class Builder:
    def __init__(self):
        self.n = 0
        self.es, self.ed, self.rows = [], [], []  # rows: (s, d, valid, kind, distance or -1, P3, P4)
        self.hubs = self.new(H)
        self.sinks, self.roots, self.leaves = self.new(2048), self.new(2048), self.new(4096)
        self.free_hubs = [r for r in range(H) if r not in BITS]
        self.serial = 0
        for r in BITS:
            self.far_bit(r)
        for r in (1, 65, 200):
            self.near_bit(r)
        for copy in range(2):
            self.d1_p3(), self.d2_p3(), self.d3_plain(), self.d4_p4(), self.d4_plain(), self.d5(), self.none()
        self.capped()
        s, a = self.new(), self.new()  # trivial rows: a NULL source, src == dst with and without edges, empty lists
        self.edge(s, a)
        self.row(s, a, "null", 1, False, False, valid=False)
        self.row(s, s, "same", 0, False, False)
        self.row(V - 1, V - 1, "same", 0, False, False)
        self.row(V - 2, a, "empty", -1, False, False)
        self.row(s, V - 3, "empty", -1, False, False)
        self.row(a, s, "empty", -1, False, False)  # a has no out-edge
        deg = np.bincount(np.concatenate(self.es + self.ed), minlength=V)
        at = 0
        for r, h in enumerate(self.hubs):  # hub r has exactly 400 - r edges
            extra = 400 - r - int(deg[h])
            assert extra > 0
            self.edge(np.full(extra, h), self.leaves[(at + np.arange(extra)) % len(self.leaves)])
            at += extra
        assert self.n < V - 8

    def new(self, n=None):
        at = self.n
        self.n += 1 if n is None else n
        return at if n is None else np.arange(at, at + n, dtype=np.int64)

    def hub(self):
        return self.hubs[self.free_hubs.pop(0)]

    def edge(self, s, d):
        s, d = np.broadcast_arrays(np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64))
        self.es.append(s.ravel()), self.ed.append(d.ravel())

    def chain(self, *v):
        for a, b in zip(v[:-1], v[1:]):
            self.edge(a, b)

    def row(self, s, d, kind, dist, p3, p4, valid=True):
        self.rows.append((int(s), int(d), valid, kind, dist, p3, p4))

    def far_bit(self, r):
        s, a, d = self.new(), self.new(), self.new()
        self.chain(s, a, self.hubs[r], d)
        self.row(s, d, "hub3", 3, True, False)

    def near_bit(self, r):
        s, c, d = self.new(), self.new(), self.new()
        self.chain(s, self.hubs[r], c, d)
        self.row(s, d, "hub3", 3, True, False)

    def d1_p3(self):
        s, a, d = self.new(), self.new(), self.new()
        self.edge(s, d), self.chain(s, a, self.hub(), d)
        self.row(s, d, "d1_p3", 1, True, False)

    def d2_p3(self):
        s, m, a, d = self.new(), self.new(), self.new(), self.new()
        self.chain(s, m, d), self.chain(s, a, self.hub(), d)
        self.row(s, d, "d2_p3", 2, True, False)

    def d3_plain(self):
        s, a, b, d = self.new(), self.new(), self.new(), self.new()
        self.chain(s, a, b, d)
        self.row(s, d, "d3_plain", 3, False, False)

    def d4_p4(self):
        s, a, c, d = self.new(), self.new(), self.new(), self.new()
        self.chain(s, a, self.hub(), c, d)
        self.row(s, d, "hub4", 4, False, True)

    def d4_plain(self):
        s, a, x, c, d = (self.new() for _ in range(5))
        self.chain(s, a, x, c, d)
        self.row(s, d, "d4_plain", 4, False, False)

    def d5(self):
        s, a, c, d = self.new(), self.new(), self.new(), self.new()
        self.chain(s, a, self.hub(), self.hub(), c, d)
        self.row(s, d, "d5", 5, False, False)

    def none(self):
        s, a, c, d = self.new(), self.new(), self.new(), self.new()
        self.chain(s, a, self.hub()), self.chain(self.hub(), c, d)
        self.row(s, d, "none", -1, False, False)

    def capped(self):
        s, d, a, c = self.new(), self.new(), self.new(130), self.new(130)
        self.edge(s, a), self.edge(c, d)
        for j in range(130):
            self.edge(a[j], self.sinks[(50 * j + np.arange(50)) % len(self.sinks)])
            self.edge(self.roots[(50 * j + np.arange(50)) % len(self.roots)], c[j])
        self.edge(a[-1], c[-1])
        self.chain(a[0], self.hub(), c[0])
        self.row(s, d, "capped", 3, False, True)


class Graph:
    """The gadget graph (or its transpose) on two handles, with hub tables and without, and the oracle's distances."""

    def __init__(self, transpose):
        b = Builder()
        src, dst = np.concatenate(b.es), np.concatenate(b.ed)
        rs, rd = np.array([r[0] for r in b.rows], dtype=np.int64), np.array([r[1] for r in b.rows], dtype=np.int64)
        if transpose:
            src, dst, rs, rd = dst, src, rd, rs
        self.rs, self.rd = rs, rd
        self.valid = np.array([r[2] for r in b.rows])
        self.kind = np.array([r[3] for r in b.rows])
        built = np.array([r[4] for r in b.rows])
        ln, ok = OracleCSR.from_edges(V, src, dst).lean_iterativelength(V, rs, rd, nthreads=8)
        self.dist = np.where(ok, ln, -1)
        assert (self.dist == built).all(), "the builder's distances are the oracle's"
        # the hubs are where the builder put them, and the proofs are the ones the gadgets were built for
        ids = hub_model.select_hubs(V, src, dst, H, min_degree=1, min_count=1)
        assert (ids == b.hubs).all()
        p3, p4 = hub_model.proofs(hub_model.build_tables(V, src, dst, ids), rs, rd)
        assert (p3 == np.array([r[5] for r in b.rows])).all() and (p4 == np.array([r[6] for r in b.rows])).all()
        self.block = len(rs)
        self.handles = {}
        for name, hubs in (("hubs", H), ("plain", 0)):
            for k, v in (("meet_hubs", hubs), ("meet_hub_min_degree", 1), ("meet_hub_min_count", 1)):
                pgq.set_option(k, v)
            st = pgq.PgqState()
            st.build_csr(0, V, src, dst)
            self.handles[name] = (st, st.device_csr(0))
        assert (self.handles["hubs"][1].hub_tables()["ids"] == ids).all()
        with pytest.raises(pgq.PgqError):
            self.handles["plain"][1].hub_sizes()

    def want(self, idx, bound=None):
        if bound is None:
            return np.where(self.valid[idx], self.dist[idx], -1).astype(np.int64)
        return clamp(self.dist[idx], self.valid[idx], bound)

    def bulk(self, name, idx, bound=None):
        """One call through the device-pointer form over a pre-filled result buffer (NULL sources are src < 0):
        (answers, rows settled as 3 from the tables, as 4 from the tables, by k_meet4d's batch pass)."""
        import torch
        dev = self.handles[name][1]
        t_s = torch.from_numpy(np.where(self.valid[idx], self.rs[idx], -1)).cuda()
        t_d = torch.from_numpy(self.rd[idx]).cuda()
        t_o = torch.full((len(idx),), SENTINEL, dtype=torch.int64, device="cuda")
        before = [pgq.get_option(k) for k in ("meet_hub3_settled", "meet_hub4_settled", "meet4_batch_settled")]
        if bound is None:
            dev.iterativelength_bulk_ptr(len(idx), t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr())
        else:
            dev.iterativelength_within_bulk_ptr(len(idx), t_s.data_ptr(), t_d.data_ptr(), bound, t_o.data_ptr())
        after = [pgq.get_option(k) for k in ("meet_hub3_settled", "meet_hub4_settled", "meet4_batch_settled")]
        return (t_o.cpu().numpy(),) + tuple(int(a - b) for a, b in zip(after, before))

    def both(self, idx, what, bound=None):
        """The call on both handles: the oracle's answers, no row unwritten, the same bytes.  Returns the counters of the two calls."""
        want = self.want(idx, bound)
        got, *hub_counts = self.bulk("hubs", idx, bound)
        plain, *plain_counts = self.bulk("plain", idx, bound)
        for name, x in (("hub tables", got), ("meet_hubs = 0", plain)):
            bad = np.flatnonzero(x != want)
            assert len(bad) == 0, "%s, %s: %d of %d rows differ, first: row %d (%s) got %d, expected %d" % (
                what, name, len(bad), len(want), bad[0], self.kind[idx][bad[0]], x[bad[0]], want[bad[0]])
        assert got.tobytes() == plain.tobytes()
        assert plain_counts[0] == 0 and plain_counts[1] == 0, "a handle without tables settled rows from them"
        return hub_counts, plain_counts

    def count(self, idx, *kinds):
        return int(np.isin(self.kind[idx], kinds).sum())


@pytest.fixture(scope="module", params=[False, True], ids=["forward", "transposed"])
def graph(request):
    saved = {k: pgq.get_option(k) for k in KEYS}
    try:
        return Graph(request.param)
    finally:
        for k, v in saved.items():
            pgq.set_option(k, v)


def test_every_row_alone(graph):
    """One row per call: the tables answer exactly the rows built for them, the walk and k_meet4d the others."""
    g = graph
    for i in range(g.block):
        idx = np.array([i])
        (hub3, hub4, batch), (_, _, plain_batch) = g.both(idx, "row %d (%s)" % (i, g.kind[i]))
        assert (hub3, hub4) == (g.count(idx, "hub3"), g.count(idx, "hub4")), g.kind[i]
        assert batch == g.count(idx, "d4_plain"), g.kind[i]  # a row the tables answered 4 never reaches k_meet4d
        assert plain_batch == g.count(idx, "d4_plain", "hub4"), g.kind[i]  # ... without tables it does


@pytest.mark.parametrize("small", [False, True], ids=["grouped", "small_call"])
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_schedules(graph, R, small):
    """Row counts 1, R + 1 and five whole groups, a partial one and three tail rows, under every meet_rows_per_wave, through the
    grouped instantiation and the one for small calls (one row per wavefront, four list requests in flight)."""
    g = graph
    T = 3
    pgq.set_option("meet_rows_per_wave", R)
    pgq.set_option("meet_tail_rows", T)
    if small:
        pgq.set_option("meet_small_rows", 1 << 20)
        pgq.set_option("meet_wide_rows", 0)
    for n in (1, R + 1, 5 * R + 3 + T, 3 * g.block + 1):
        for rot in (0, 5):
            idx = (rot + np.arange(n)) % g.block
            (hub3, hub4, _), _ = g.both(idx, "R %d, n %d, rotation %d" % (R, n, rot))
            assert (hub3, hub4) == (g.count(idx, "hub3"), g.count(idx, "hub4"))


@pytest.mark.parametrize("bound", [1, 2, 3, 4, 5])
def test_bounded_calls(graph, bound):
    """max_hops 2: the distance tests decide, P3 is not consulted and its rows are NULL; 3: a walk that ran to its end is NULL even
    where P4 holds; 4: a P4 row is 4."""
    g = graph
    idx = np.arange(2 * g.block) % g.block
    (hub3, hub4, _), _ = g.both(idx, "max_hops %d" % bound, bound)
    assert hub3 == (g.count(idx, "hub3") if bound >= 3 else 0)
    assert hub4 == (g.count(idx, "hub4") if bound >= 4 else 0)
    got = g.bulk("hubs", idx, bound)[0]
    assert (got[g.kind[idx] == "hub3"] == (3 if bound >= 3 else -1)).all()
    assert (got[g.kind[idx] == "hub4"] == (4 if bound >= 4 else -1)).all()


def test_a_cut_walk_is_not_answered_from_the_tables(graph):
    """meet_cap = 64: the capped row's walk is cut (its 130 lists hold 6,500 entries, the witness is in the last), P4 holds, the
    distance is 3.  Alone, in a group, as a small call."""
    g = graph
    for k in ("meet_cap", "meet_cap_small"):
        pgq.set_option(k, 64)
    at = int(np.flatnonzero(g.kind == "capped")[0])
    for small in (0, 1 << 20):
        pgq.set_option("meet_small_rows", small)
        pgq.set_option("meet_wide_rows", 0)
        for idx in (np.array([at]), (at - 3 + np.arange(8)) % g.block, np.arange(g.block)):
            (hub3, hub4, _), _ = g.both(idx, "meet_cap 64, %d rows" % len(idx))
            assert (hub3, hub4) == (g.count(idx, "hub3"), g.count(idx, "hub4"))


def test_an_id_out_of_range_beside_settled_rows(graph):
    """An id outside [0, V) fails the call as before, whatever its neighbours in the group are; the next call is untouched."""
    import torch
    g = graph
    dev = g.handles["hubs"][1]
    idx = np.flatnonzero(g.kind == "hub3")[:4]
    for bad_src, bad_dst in ((V, 0), (0, V + 5), (0, -1)):
        t_s = torch.from_numpy(np.concatenate([g.rs[idx], [bad_src], g.rs[idx]])).cuda()
        t_d = torch.from_numpy(np.concatenate([g.rd[idx], [bad_dst], g.rd[idx]])).cuda()
        t_o = torch.full((len(t_s),), SENTINEL, dtype=torch.int64, device="cuda")
        with pytest.raises(pgq.PgqError):
            dev.iterativelength_bulk_ptr(len(t_s), t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr())
    g.both(np.arange(g.block), "after the failed calls")
