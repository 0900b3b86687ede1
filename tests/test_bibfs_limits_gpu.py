"""k_bibfs at its queue, list, cap and row limits (helpers.bibfs_gadgets, helpers.BIBFS_LIMITS).

The random graphs of the other files reach k_bibfs with a few rows among thousands, and what it wrongly leaves open the lane
batches answer correctly behind it.  Here every queue position, list slot, chunk boundary and cap value is the only witness of
one row, on the graph and on its transpose (the backward side walks what the forward side walked), and beside the answers the
tests check WHO answered: meet_pairs, levels and edges_scanned against tests/bibfs_model.py, the kernel restated in Python
(test_bibfs_gadgets_cpu.py holds that model to the oracle and shows which family tells each of its mutants apart).  Every
expected answer is the oracle's; every comparison is exact; no number comes from the kernel under test."""
import numpy as np
import pytest

import bibfs_model as M
import duckpgq_extension_amd as pgq
from helpers import BIBFS_FAR, bibfs_calls, bibfs_gadgets, bibfs_stale_gadgets, csr_arrays_from_rows
from oracle.pgq_oracle import OracleCSR
from test_degree_edges_gpu import KEYS
from test_within_gpu import Rows, clamp, payload

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


class Side:
    """A gadget graph (or its transpose), the oracle's distances of its rows, and the model's account of every call."""

    def __init__(self, g):
        self.g = g
        self.ora = OracleCSR.from_edges(g.V, g.src, g.dst)
        self.dist = self.distances(g.rs, g.rd)
        self.mg = M.Graph(g.V, g.src, g.dst)
        self.calls = {name: (rows, q, cap) + self.model(g.rs[rows], g.rd[rows], self.dist[rows], cap, q) for name, fam, q, cap, rows in bibfs_calls(g)}

    def distances(self, ps, pd):
        ln, ok = self.ora.lean_iterativelength(self.g.V, ps, pd, nthreads=8)
        return np.where(ok, ln, -1)

    def model(self, ps, pd, dist, cap, q, bound=None):
        """(the model's rows, how many it leaves open); what it answers is the oracle's distance."""
        res = M.solve(self.mg, (ps, pd), cap, q, bound=bound)
        ans = np.array([r.answer for r in res])
        opn = ans == M.OPEN
        want = dist if bound is None else np.where(dist > bound, -1, dist)
        assert (ans[~opn] == want[~opn]).all()
        return res, int(opn.sum())

    def upload(self):
        st = pgq.PgqState()
        st.build_csr(0, self.g.V, self.g.src, self.g.dst)
        return st


@pytest.fixture(scope="module")
def sides():
    g = bibfs_gadgets()
    return [Side(g), Side(g.transposed())]


def orient(k):
    return "graph" if k == 0 else "transpose"


def run_form(st, form, V, ps, pd):
    import torch
    dev = st.device_csr(0)
    if form == "bulk":
        t_s, t_d = torch.from_numpy(ps).cuda(), torch.from_numpy(pd).cuda()
        t_o = torch.full((len(ps),), -7, dtype=torch.int64, device="cuda")
        dev.iterativelength_bidirectional_bulk_ptr(len(ps), t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr())
        return t_o.cpu().numpy()
    if form == "chunk":
        return payload(*dev.iterativelength_bidirectional(ps, pd))
    return payload(*st.iterativelength(0, V, ps, pd, variant=3))


def check(got, want, what, tags):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: %d of %d rows differ, first: %s got %d, expected %d" % (what, len(bad), len(want), tags(bad[0]), got[bad[0]], want[bad[0]])


def check_who(stats, n, n_open, what):
    print("%s: %d rows, open: model %d, device %d, levels %d" % (what, n, n_open, n - stats["meet_pairs"], stats["levels"]))
    assert stats["meet_pairs"] == n - n_open, "%s: k_bibfs answered %d of %d rows, the model %d" % (what, stats["meet_pairs"], n, n - n_open)
    assert (stats["levels"] == 0) == (n_open == 0), "%s: levels %d with %d rows open in the model" % (what, stats["levels"], n_open)


# ---- the bidirectional entry points: every row is k_bibfs's --------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1], ids=["graph", "transpose"])
@pytest.mark.parametrize("lds_kb", [150, 0], ids=["lds_maps", "global_maps"])
def test_bidirectional_entry_points(sides, lds_kb, k):
    side = sides[k]
    g = side.g
    st = side.upload()
    pgq.set_option("meet4_lds_kb", lds_kb)
    for name, (rows, q, cap, res, n_open) in side.calls.items():
        pgq.set_option("bibfs_queue", q)
        pgq.set_option("bibfs_cap", cap)
        for form in ("bulk", "chunk", "udf"):
            what = "%s, %s, meet4_lds_kb %d, %s form" % (orient(k), name, lds_kb, form)
            pgq.reset_stats()
            got = run_form(st, form, g.V, g.rs[rows], g.rd[rows])
            stats = pgq.get_stats()
            check(got, side.dist[rows], what, lambda b: g.tag(rows[b]))
            check_who(stats, len(rows), n_open, what)
            assert stats["launches"]["bibfs"] == 1 and stats["lds_map_launches"]["bibfs"] == (1 if lds_kb else 0), what
        # rows that end without a meeting are walked to the end: the entries covered are the model's, exactly
        quiet = np.array([i for i, r in enumerate(res) if r.answer == M.NULL and r.sides], dtype=np.int64)
        if len(quiet):
            pgq.reset_stats()
            got = run_form(st, "bulk", g.V, g.rs[rows[quiet]], g.rd[rows[quiet]])
            stats = pgq.get_stats()
            assert (got == -1).all()
            assert stats["edges_scanned"] == sum(res[i].entries for i in quiet), "%s, %s, meet4_lds_kb %d: entries covered by %d rows without a meeting" % (
                orient(k), name, lds_kb, len(quiet))
    st.delete_csr(0)


# ---- the touched-word list of the global maps: a dirty row, then a row that needs a clean map ----------------------------
@pytest.mark.parametrize("k", [0, 1], ids=["graph", "transpose"])
@pytest.mark.parametrize("lds_kb", [0, 150], ids=["global_maps", "lds_maps"])
def test_stale_words(lds_kb, k):
    import torch
    grid = torch.cuda.get_device_properties(0).multi_processor_count  # meet_bidirectional: min(n, CUs) workgroups
    g, Ts = bibfs_stale_gadgets(grid)
    g = g if k == 0 else g.transposed()
    ln, ok = OracleCSR.from_edges(g.V, g.src, g.dst).lean_iterativelength(g.V, g.rs, g.rd, nthreads=8)
    dist = np.where(ok, ln, -1)
    assert (dist == g.dist).all() and len(g.rs) == 12 * grid
    # the model, with the maps carried from row i to row i + grid: the answers are the oracle's, and the dirty rows list what they claim
    res = M.solve(M.Graph(g.V, g.src, g.dst), (g.rs, g.rd), int(pgq.get_default_option("bibfs_cap")), 1024, grid=grid, gm=True)
    assert [r.answer for r in res] == dist.tolist()
    assert {(int(a), r.listed) for a, b, r in zip(g.a, g.b, res) if b == 0} == {(n, n) for n in (1023, 1024, 1025)}
    st = pgq.PgqState()
    st.build_csr(0, g.V, g.src, g.dst)
    pgq.set_option("meet4_lds_kb", lds_kb)
    pgq.set_option("bibfs_queue", 1024)
    for rep in range(2):  # the second call finds the maps as the first one left them
        pgq.reset_stats()
        got = run_form(st, "bulk", g.V, g.rs, g.rd)
        stats = pgq.get_stats()
        what = "%s, meet4_lds_kb %d, call %d" % (orient(k), lds_kb, rep)
        check(got, dist, what, lambda b: g.tag(b) + (", a dirty row", ", behind a dirty row: the other side's map", ", behind a dirty row: its own side's map")[g.b[b]])
        check_who(stats, len(g.rs), 0, what)
    st.delete_csr(0)


# ---- the pre-pass chain: k_bibfs behind k_meet3 and k_meet4d, with and without a bound -------------------------------------
def chain_options(rows):
    for key, v in (("meet", 1), ("meet_bias", 1e9), ("ball", 0), ("bibfs_rows", rows)):
        pgq.set_option(key, v)


@pytest.mark.parametrize("k", [0, 1], ids=["graph", "transpose"])
@pytest.mark.parametrize("lds_kb", [150, 0], ids=["lds_maps", "global_maps"])
@pytest.mark.parametrize("name", ["far", "queue_1024", "queue_2048", "cap"])
def test_chain(sides, name, lds_kb, k):
    side = sides[k]
    g = side.g
    rows, q, cap, res, n_open = side.calls[name]
    ps, pd, dist = g.rs[rows], g.rd[rows], side.dist[rows]
    assert (dist[dist >= 0] >= 4).all() and (dist >= 5).any()
    chain_options(4096)
    pgq.set_option("meet4_lds_kb", lds_kb)
    pgq.set_option("bibfs_queue", q)
    pgq.set_option("bibfs_cap", cap)
    st = side.upload()  # a fresh handle: k_bibfs is in its chain, and these rows keep it there
    r = Rows(st, g.V, ps, pd)
    what = "%s, %s, meet4_lds_kb %d" % (orient(k), name, lds_kb)
    pgq.reset_stats()
    check(r.unbounded(), dist, what + ", unbounded", lambda b: g.tag(rows[b]))
    stats = pgq.get_stats()
    print("%s, unbounded: open in the model %d, levels %d" % (what, n_open, stats["levels"]))
    assert stats["launches"]["bibfs"] == 1, what
    assert (stats["levels"] == 0) == (n_open == 0), (what, stats["levels"], n_open)  # a row 5 hops or more apart is nobody else's
    bounds = sorted({int(d) + e for d in dist[dist >= 5] for e in (-1, 0, 1)} | ({6} if name == "cap" else set()))
    for U in bounds:
        m_open = side.model(ps, pd, dist, cap, q, bound=U)[1]
        for form in ("chunk", "bulk"):
            pgq.reset_stats()
            check(getattr(r, form)(U), clamp(dist, r.valid, U), "%s, %s form, max_hops %d" % (what, form, U), lambda b: g.tag(rows[b]))
            stats = pgq.get_stats()
            print("%s, %s form, max_hops %d: open in the model %d, levels %d" % (what, form, U, m_open, stats["levels"]))
            assert stats["launches"]["bibfs"] == 1, (what, form, U)
            if m_open == 0:
                assert stats["levels"] == 0, (what, form, U, stats["levels"])
    if name == "cap":  # the bound closes the row in front of the cap test: NULL from k_bibfs, both rows, not a row left open
        assert side.model(ps, pd, dist, cap, q, bound=6)[1] == 0 and n_open == 1
    st.delete_csr(0)


def far_rows(side, n):
    """n rows 5 .. 9 hops apart (the far family's main rows, over and over): open behind the two-hop kernels whatever they do."""
    g = side.g
    main = [r for r in g.rows_where("far") if g.b[r] == 0]
    assert sorted(side.dist[main].tolist()) == list(BIBFS_FAR)
    rows = np.resize(np.array(main, dtype=np.int64), n)
    return g.rs[rows], g.rd[rows], side.dist[rows]


def near_rows(side, n):
    """n rows one hop apart: each far source and its first out-neighbour."""
    g = side.g
    off, adj, _ = csr_arrays_from_rows(g.V, g.src, g.dst)
    ps = np.resize(far_rows(side, len(BIBFS_FAR))[0], n)
    return ps, adj[off[ps]], np.ones(n, dtype=np.int64)


@pytest.mark.parametrize("k", [0, 1], ids=["graph", "transpose"])
def test_row_limit(sides, k):
    side = sides[k]
    limit = 64
    assert len(side.g.src) // 4096 < limit  # max(bibfs_rows, min(bibfs_rows_max, E / 4096)) is bibfs_rows here
    chain_options(limit)
    st = side.upload()
    dev = st.device_csr(0)
    for n in (limit, limit + 1, limit):
        ps, pd, dist = far_rows(side, n)
        pgq.reset_stats()
        got = payload(*dev.iterativelength(ps, pd))
        stats = pgq.get_stats()
        assert (got == dist).all(), (orient(k), n)
        assert stats["launches"]["bibfs"] == 1, (orient(k), n)  # launched either way: it counts the rows itself
        assert (stats["levels"] == 0) == (n <= limit), "%s: %d rows open under bibfs_rows %d, levels %d" % (orient(k), n, limit, stats["levels"])
    st.delete_csr(0)


def test_switch(sides):
    side = sides[0]
    chain_options(4096)
    st = side.upload()
    dev = st.device_csr(0)
    near, far = near_rows(side, 20), far_rows(side, 20)

    def call(rows, U=None):
        pgq.reset_stats()
        got = payload(*(dev.iterativelength(rows[0], rows[1]) if U is None else dev.iterativelength_within(rows[0], rows[1], U)))
        assert (got == (rows[2] if U is None else clamp(rows[2], np.ones(len(got), dtype=bool), U))).all()
        stats = pgq.get_stats()
        return stats["launches"]["bibfs"], stats["levels"]

    assert call(near) == (1, 0)      # a handle starts with k_bibfs in its chain; nothing was open at its place: off
    assert call(near) == (0, 0)
    assert call(far, U=9)[0] == 0    # a bounded call neither uses what is off nor switches it on
    assert call(near) == (0, 0)
    n, levels = call(far)            # off: the lane batches answer, and the call switches it on for the next
    assert n == 0 and levels > 0
    assert call(near, U=3) == (1, 0)  # bounded, nothing open at its place: the switch stays as it is
    assert call(far) == (1, 0)
    st.delete_csr(0)
