"""k_meet4d's batch pass (option meet4_batch): proven-far rows, one per wavefront, settled by a 512-entry set against a
4096-entry walk; what it cannot settle goes through the whole-workgroup procedure in the same launch.

The graphs are disjoint gadgets built in numpy and padded with isolated vertices to the V wanted (the pass's batch size is
min(16, map bytes / 4096), the map has one bit per vertex).  A gadget is a source s with out-neighbours a_1 .. a_p whose
out-lists are sinks (no out-edges) and a destination d with one in-neighbour b whose in-list is roots (no in-edges); one
vertex w sits in a chosen slot of a chosen a_i's list and in b's in-list: s -> a_i -> w -> b -> d is the only path, the row is at
distance exactly 4.  b's in-list is the longer side, so the set side is the forward one and w's slot decides whether it lies in
the set's 512-entry prefix; the transposed graph turns the sides round.  Every expected value is the CPU oracle's, every
comparison is exact, and meet4_batch = 2 (the pass on every launch) and 1 (as shipped: when more than two proven-far rows are
queued per workgroup) must give what meet4_batch = 0 gives.  The read-only option meet4_batch_settled counts the rows the pass
answered: only the pass advances it."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from oracle.pgq_oracle import OracleCSR
from test_within_gpu import clamp, payload

pytestmark = pytest.mark.gpu

KEYS = ("meet", "meet_bias", "meet_cap", "meet_cap_small", "meet4", "meet4_cap", "meet4_test_cap", "meet4_lds_kb", "meet4_global_mb",
        "meet4_grid_mult", "meet4_batch", "meet_layout", "meet_align", "meet_pack", "meet_pack_align", "meet_pack_order", "meet_small_rows",
        "meet_wide_rows", "meet_wide_rows_always", "meet_grid_mult", "bibfs_rows", "bibfs_rows_max", "ball", "route_memo", "route_timing",
        "calibration_cache", "meet_calibrate", "chunk_zero_copy", "streams", "words", "max_words", "lanes")
SIZES = (16_384, 65_536, 1 << 18, 524_288 + 128)  # map of 2 KB (pass off), then batches of 2, 8 and 16 rows
_LOW, _HIGH, _ROOTS = 1024, 1024, 2048  # sinks with the smallest ids, sinks with the largest ids, roots
_BACK = 1500  # entries of b's in-list: over every set side below (so the set side is s's), under the pass's 4096-entry walk


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    for k, v in (("meet", 1), ("meet_bias", 1e9), ("ball", 0)):  # the pre-pass takes every call
        pgq.set_option(k, v)
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def batch_of(V):
    """Rows per batch at V vertices: one 4-KB filter per wavefront inside the map of ceil(V / 128) * 16 bytes."""
    return min(16, (V + 127) // 128 * 16 // 4096)


# kind: (out-list lengths of a_1 .. a_p without w, list that holds w, w's slot in it, expected: the pass settles the row)
#   near       w is the first entry of the first list
#   at511      w is the last entry of the prefix (slot 511 of one list)
#   at512      w is the first entry behind the prefix: the wavefront misses, the workgroup answers 4
#   beyond     w far behind the prefix
#   cut_in     the prefix ends in the middle of a_2's list (a_1: 300 entries, padded to at most 320), w before the cut
#   cut_out    ... w behind the cut
#   short      the whole two-hop neighbourhood is 3 entries
KINDS = {
    "near": ((40, 50), 0, 0, True),
    "at511": ((640,), 0, 511, True),
    "at512": ((640,), 0, 512, False),
    "beyond": ((300, 300, 200), 2, 150, False),
    "cut_in": ((300, 400), 1, 100, True),
    "cut_out": ((300, 400), 1, 300, False),
    "short": ((1, 1), 1, 1, True),
}


class Far:
    """The gadget graph: V, edge table (src, dst), rows (rs, rd), per row its kind, built distance (-1: unreachable) and
    whether the batch pass can settle it."""

    def __init__(self, plan, hub_rows=0):
        self.es, self.ed, self.rs, self.rd, self.kind, self.dist, self.settles = [], [], [], [], [], [], []
        self.n = _LOW + _ROOTS
        self.low, self.roots = np.arange(_LOW, dtype=np.int64), _LOW + np.arange(_ROOTS, dtype=np.int64)
        self.high = -1 - np.arange(_HIGH, dtype=np.int64)  # placed behind every other id by finish()
        for kind, copies in plan:
            for c in range(copies):
                self.gadget(kind, len(self.rs))
        for c in range(hub_rows):
            self.hub(len(self.rs))

    def new(self, n=1):
        at = self.n
        self.n += n
        return at if n == 1 else np.arange(at, at + n, dtype=np.int64)

    def edges(self, s, d):
        s, d = np.broadcast_arrays(np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64))
        self.es.append(s.ravel())
        self.ed.append(d.ravel())

    def row(self, s, d, kind, dist, settles):
        self.rs.append(s), self.rd.append(d), self.kind.append(kind), self.dist.append(dist), self.settles.append(settles)

    def gadget(self, kind, serial):
        far = kind.split(":")[0]  # "d5:near": the same lists, but w -> w2 -> b (distance 5); "none:near": no connection
        lens, wi, wj, settles = KINDS[kind.split(":")[-1]]
        s, d, b, w = self.new(), self.new(), self.new(), self.new()
        for i, n in enumerate(lens):
            a = self.new()
            self.edges(s, a)
            # ascending ids, so that the slots are the same in the out-list (table order) and, transposed, in the in-list (id order)
            k = wj if i == wi else n // 2
            lo = np.sort(self.low[(7 * serial + 13 * i + np.arange(k)) % _LOW])
            hi = np.sort(self.high[(5 * serial + 11 * i + np.arange(n - k)) % _HIGH])[::-1]
            self.edges(a, np.concatenate([lo, [w], hi] if i == wi else [lo, hi]))
        self.edges(self.roots[(5 * serial + np.arange(_BACK)) % _ROOTS], b)
        self.edges(b, d)
        if far == "d5":
            w2 = self.new()
            self.edges(w, w2)
            self.edges(w2, b)
            self.row(s, d, kind, 5, False)
        elif far == "none":
            self.row(s, d, kind, -1, False)
        else:
            self.edges(w, b)
            self.row(s, d, kind, 4, settles)

    def hub(self, serial):
        """Both one-hop lists over the register set of k_meet3 (513 > 512): such a row comes from the FRONT of k_meet4d's queue
        and is the whole workgroup's; distance 4 through the last slots."""
        s, d, w = self.new(), self.new(), self.new()
        a, b = self.new(513), self.new(513)
        self.edges(s, a)
        self.edges(b, d)
        self.edges(a[:-1], self.low[(3 * serial + np.arange(512)) % _LOW])
        self.edges(self.roots[(3 * serial + np.arange(512)) % _ROOTS], b[:-1])
        self.edges(a[-1], w)
        self.edges(w, b[-1])
        self.row(s, d, "hub", 4, False)

    def finish(self, V, transpose=False):
        """The graph on the LAST ids of [0, V) (the filter and the map see high id bits), isolated vertices before it."""
        o = V - self.n - _HIGH
        assert o >= 0, "V too small for the gadgets"
        real = lambda v: np.where(np.asarray(v, dtype=np.int64) < 0, self.n - 1 - np.asarray(v, dtype=np.int64), v) + o
        src, dst = real(np.concatenate(self.es)), real(np.concatenate(self.ed))
        rs, rd = real(self.rs), real(self.rd)
        if transpose:
            src, dst, rs, rd = dst, src, rd, rs
        return Graph(V, src, dst, rs, rd, np.array(self.kind), np.array(self.dist), np.array(self.settles))


class Graph:
    def __init__(self, V, src, dst, rs, rd, kind, built, settles):
        self.V, self.src, self.dst, self.rs, self.rd, self.kind, self.built, self.settles = V, src, dst, rs, rd, kind, built, settles
        ora = OracleCSR.from_edges(V, src, dst)
        ln, ok = ora.lean_iterativelength(V, rs, rd, nthreads=8)
        self.dist = np.where(ok, ln, -1)
        assert (self.dist == built).all(), "the builder's distances are the oracle's"
        self.st = pgq.PgqState()
        self.st.build_csr(0, V, src, dst)

    def run(self, batch, rows=slice(None), bound=None):
        """(payloads, rows the batch pass settled, meet4 launches) of one call under meet4_batch = batch."""
        pgq.set_option("meet4_batch", batch)
        before = pgq.get_option("meet4_batch_settled")
        pgq.reset_stats()
        if bound is None:
            got = payload(*self.st.iterativelength(0, self.V, self.rs[rows], self.rd[rows]))
        else:
            got = payload(*self.st.iterativelength_within(0, self.V, self.rs[rows], self.rd[rows], bound))
        return got, int(pgq.get_option("meet4_batch_settled") - before), pgq.get_stats()["launches"]["meet4"]

    def check(self, got, what, rows=slice(None), bound=None):
        want = self.dist[rows] if bound is None else clamp(self.dist[rows], np.ones(len(self.dist[rows]), dtype=bool), bound)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "%s: %d of %d rows differ, first: %s got %d, expected %d" % (
            what, len(bad), len(want), self.kind[rows][bad[0]], got[bad[0]], want[bad[0]])

    def both(self, what, rows=slice(None), bound=None):
        """The call with the pass on every launch (meet4_batch = 2), as shipped (1: when more than two proven-far rows are queued
        per workgroup) and without it (0): all the oracle's answers, byte for byte the same.  Returns the pass's count under 2;
        self.shipped is its count under 1: all of that or nothing."""
        on, settled, launches = self.run(2, rows, bound)
        dflt, self.shipped, _ = self.run(1, rows, bound)
        off, settled_off, _ = self.run(0, rows, bound)
        self.check(on, what + ", meet4_batch 2", rows, bound)
        self.check(dflt, what + ", meet4_batch 1", rows, bound)
        self.check(off, what + ", meet4_batch 0", rows, bound)
        assert on.tobytes() == off.tobytes() and dflt.tobytes() == off.tobytes()
        assert settled_off == 0, "meet4_batch = 0 is the whole-workgroup path alone"
        assert self.shipped in (0, settled)
        assert launches >= 1
        print("%s: %d rows, the pass settled %d (as shipped: %d)" % (what, len(on), settled, self.shipped))
        return settled

    def close(self):
        self.st.delete_csr(0)


PLAN = [(k, 6) for k in KINDS] + [("d5:near", 4), ("d5:beyond", 4), ("none:near", 4), ("none:cut_out", 4)]


@pytest.fixture(scope="module")
def far():
    return Far(PLAN)


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("V", SIZES)
def test_every_kind_on_both_sides_of_the_pass_limit(far, V, transpose):
    g = far.finish(V, transpose)
    what = "V = %d%s" % (V, ", transposed" if transpose else "")
    can = int(g.settles.sum())
    settled = g.both(what)
    if batch_of(V) == 0:
        assert settled == 0, "a map under 4 KB has no room for a filter: the pass is off"
    else:
        assert settled == can, "the pass settles exactly the rows whose only witness lies in the 512-entry prefix"
    # one kind at a time: a witness at slot 512 or behind a cut is the whole workgroup's (the pass settles nothing there)
    for kind in KINDS:
        rows = np.flatnonzero(g.kind == kind)
        settled = g.both(what + ", " + kind, rows)
        assert settled == (len(rows) if KINDS[kind][3] and batch_of(V) else 0), kind
    # under the bound 4 the rows farther apart are NULL; under 3 every row of the graph is
    for bound in (4, 3):
        settled = g.both(what + ", bound %d" % bound, bound=bound)
        assert settled == (can if bound == 4 and batch_of(V) else 0)
    g.close()


@pytest.mark.parametrize("V", SIZES[1:])
def test_fewer_rows_than_a_batch_and_more_than_the_grid_takes(V):
    B = batch_of(V)
    many = 40 * B + 3
    g = Far([("near", many), ("at512", 5), ("d5:near", 3)]).finish(V)
    near = np.flatnonzero(g.kind == "near")
    for n in (1, max(1, B - 1), many):  # one row; one short of a batch; a small call's grid is max(16, rows / 16) workgroups: B x grid < rows
        assert n < B or n == 1 or n > B * max(16, n // 16)
        assert g.both("V = %d, %d near rows" % (V, n), near[:n]) == n
        # as shipped the pass runs when more than two such rows are queued per workgroup (a wavefront alone takes longer over a
        # row than the workgroup does)
        assert g.shipped == (n if n > 2 * min(n, max(16, n // 16)) else 0)
    assert g.both("V = %d, every row" % V) == many
    g.close()


def test_front_rows_and_back_rows_in_one_workgroup():
    # 40 rows for the front of the queue (lists over the register set) on a grid of 16 workgroups: every workgroup takes whole
    # rows first and batches behind them
    V = 1 << 18
    g = Far([("near", 150), ("cut_out", 30), ("none:near", 10)], hub_rows=40).finish(V)
    assert max(16, len(g.rs) // 16) < 40
    assert g.both("front and back rows") == 150
    g.close()


def test_grid_multipliers_agree():
    V = 1 << 18
    g = Far([("near", 500), ("cut_in", 200), ("beyond", 200), ("d5:cut_in", 50), ("none:beyond", 50)], hub_rows=24).finish(V)
    pgq.set_option("meet_small_rows", 0)  # not a small call: the grid is meet4_grid_mult workgroups per CU (at most one per row)
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    ref = None
    for mult in (1, 2, 3):
        pgq.set_option("meet4_grid_mult", mult)
        on, settled, _ = g.run(2)
        g.check(on, "meet4_grid_mult %d" % mult)
        assert settled == 700
        assert g.both("meet4_grid_mult %d" % mult) == 700
        assert g.shipped == (700 if 1000 > 2 * min(1024, ncu * mult) else 0)  # (256 CUs: 1000 proven-far rows on 256 / 512 / 768 workgroups)
        ref = on if ref is None else ref
        assert on.tobytes() == ref.tobytes()
    g.close()


def test_the_counter_is_read_only():
    with pytest.raises(pgq.PgqError):
        pgq.set_option("meet4_batch_settled", 0)
