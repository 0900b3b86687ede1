"""cheapest_path_length with list lengths ON the relaxation's own constants and the only cheapest path in a chosen slot.

helpers.degree_gadgets(**WEIGHTED_GADGETS) builds sources of out-degree a and destinations of in-degree b, a and b in 1, 2,
7 .. 9, 15 .. 17, 63 .. 65, 71 .. 73, 127 .. 130, 191 .. 193, 4095 .. 4097, k = 1 .. 4 edges apart by one path whose vertex is
the first, the last, or the 8th / 9th, 64th / 65th, 128th / 129th, 192nd / 193rd entry of the list; helpers.weighted_gadgets
gives every edge a weight by its slot, so that the path is also at a known rank of the weight-sorted list and its edges sit on
and one above the caps of the light-edges-first phases (test_weighted_gadgets_cpu.py proves all of that on the CPU, and that a
relaxation which loses a trip's eighth edge, the one-edge last chunk, chunk 64 of a 4097-edge list, the edge at the cap or the
pairing of sorted neighbours and weights answers a gadget row wrongly).  The random graphs of the other files have other
witnesses for any single lost edge.  Every expected value is the CPU oracle's; every comparison is exact: validity, int64
values, doubles as bit patterns.  The chain kernels get directed paths and rings of 8,200 vertices of their own."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from duckpgq_extension_amd.binding import _check, _p, make_vec, unpack_validity
from helpers import WEIGHT_DTYPES, WEIGHT_SCHEMES, WEIGHTED_GADGETS, csr_arrays_from_rows, degree_gadgets, weighted_gadgets
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

# every option these calls depend on, at the value a test starts from (another file may have left its own); SHIPPED: the
# library's own value, read from it
SHIPPED = ("chain_cap", "wbibfs_rows", "wbibfs_delta_div", "wbibfs_cap", "wbibfs_queue", "wbibfs_far", "wbibfs_prune",
           "wbibfs_mem_mb", "relax_light", "relax_light_div", "relax_light_min_degree", "relax_labels32", "relax_split",
           "relax_small_limit", "relax_bidir_rows", "relax_bidir_c0_div", "relax_bidir_step_div")
KEYS = {"streams": 1, "relax_streams": 0, "chain": 0, "wbibfs": 0, "relax_delta_div": 0, "relax_bidir": 0}


@pytest.fixture(autouse=True)
def _options():
    start = dict(KEYS, **{k: pgq.get_default_option(k) for k in SHIPPED})
    saved = {k: pgq.get_option(k) for k in start}
    for k, v in start.items():
        pgq.set_option(k, v)
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def options(**kw):
    for k, v in kw.items():
        pgq.set_option(k, v)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def differing(out, ok, want_out, want_ok):
    """Rows whose validity differs, or whose value does where both are valid (int64 values, doubles as bit patterns)."""
    return np.flatnonzero((ok != want_ok) | (ok & want_ok & (bits(out) != bits(want_out))))


class Case:
    """One orientation of the gadgets under one weight scheme and type: the device handle, the oracle and its answers."""

    def __init__(self, g, csr, scheme, dtype, name):
        self.g, self.name = g, "%s, %s %s" % (name, scheme, dtype)
        off, adj, order = csr
        w = weighted_gadgets(g, scheme, dtype)[order]
        eid = np.arange(len(adj), dtype=np.int64)
        self.dev = pgq.DeviceCSR(g.V, off, adj, eid, w)
        self.ora = OracleCSR.adopt(g.V, off, adj, eid, w)
        self.out, self.ok = self.ora.lean_cheapest_path_length(g.V, g.rs, g.rd)
        assert (self.ok == (g.dist >= 0)).all()
        self.deg = np.diff(off)

    def check(self, out, ok, what, rows=None):
        rows = np.arange(len(self.g.rs)) if rows is None else rows
        bad = differing(out, ok, self.out[rows], self.ok[rows])
        assert len(bad) == 0, "%s, %s: %d of %d rows differ, first: gadget %s got %r (valid %s), expected %r (valid %s)" % (
            self.name, what, len(bad), len(rows), self.g.tag[rows[bad[0]]], out[bad[0]], ok[bad[0]], self.out[rows[bad[0]]],
            self.ok[rows[bad[0]]])

    def run(self, what, rows=None):
        g = self.g
        r = slice(None) if rows is None else rows
        out, ok = self.dev.cheapest_path_length(g.rs[r], g.rd[r])
        self.check(out, ok, what, rows)


class World:
    def __init__(self):
        g = degree_gadgets(**WEIGHTED_GADGETS)
        self.sides = [g, g.transposed()]
        self.csr = [csr_arrays_from_rows(x.V, x.src, x.dst) for x in self.sides]
        self.cases = {}

    def case(self, k, scheme, dtype="int64"):
        if (k, scheme, dtype) not in self.cases:
            self.cases[k, scheme, dtype] = Case(self.sides[k], self.csr[k], scheme, dtype, ("graph", "transpose")[k])
        return self.cases[k, scheme, dtype]


@pytest.fixture(scope="module")
def world():
    return World()


# ---- 1. plain rounds: every edge of a changed vertex, lists over 128 edges in chunks of 64, few changed vertices on the device -
@pytest.mark.parametrize("dtype", ["int64", "double_inexact"])
def test_plain_rounds(world, dtype):
    options(relax_light=0, chain=0)
    for k in (0, 1):
        c = world.case(k, "ascending", dtype)
        for split in (1, 0):
            for small in (0, 2048):
                options(relax_split=split, relax_small_limit=small)
                pgq.reset_stats()
                c.run("plain rounds, relax_split %d, relax_small_limit %d" % (split, small))
                assert pgq.get_stats()["batches"] == 25  # 1,553 distinct sources


# ---- 2. light edges first: weight-sorted lists under a doubling cap ---------------------------------------------------------
# (relax_light, relax_labels32, relax_split, relax_light_div): every value of every axis with 4-byte and with 8-byte labels;
# doubles always have 8-byte labels.  1 << 20: the first int64 cap is 1 and the caps are the powers of two, so the
# ascending witness weights 8, 64, 128, 4096 equal a cap and 9, 65, 129, 4097 are one above it
# (`zeros`: the mean weight is clamped to 1e-300 and the largest weight is 0, so the light path is taken but ends after one phase
# with every cap and stop rule degenerate: that scheme checks first improvements among equal labels, not the caps)
LIGHT_INT = ((None, 1, 1, None), (2, 0, 0, 1 << 20), (2, 1, 0, 1 << 20), (None, 0, 1, None))
LIGHT_DOUBLE = ((None, 1, 1, None), (2, 1, 0, 1 << 20))


@pytest.mark.parametrize("dtype", WEIGHT_DTYPES)
@pytest.mark.parametrize("scheme", WEIGHT_SCHEMES)
def test_light_edges_first(world, scheme, dtype):
    options(chain=0)
    shipped = {key: pgq.get_default_option(key) for key in ("relax_light", "relax_light_div")}
    assert shipped["relax_light"] == 1
    for k in (0, 1):
        c = world.case(k, scheme, dtype)
        for light, labels32, split, div in (LIGHT_INT if dtype == "int64" else LIGHT_DOUBLE):
            light = shipped["relax_light"] if light is None else light
            div = shipped["relax_light_div"] if div is None else div
            options(relax_light=light, relax_labels32=labels32, relax_split=split, relax_light_div=div)
            pgq.reset_stats()
            c.run("light edges first, relax_light %d, relax_labels32 %d, relax_split %d, relax_light_div %d" % (light, labels32, split, div))
            assert pgq.get_stats()["batches"] == 25


# ---- 3. ordered rounds: only labels under a threshold that advances by a band ---------------------------------------------
# 100000: a band of one unit (int64) or less than one weight step (double), so every distinct label is a band of its own: a
# call is about 31,000 (int64) or 62,000 (double) rounds.  That the option took effect shows in the rounds: far more of them
# than with a band of the mean weight
@pytest.mark.parametrize("k", [0, 1], ids=["graph", "transpose"])
@pytest.mark.parametrize("dtype", ["int64", "double"])
@pytest.mark.parametrize("delta_div", [1, 8, 100000])
def test_ordered_rounds(world, delta_div, dtype, k):
    options(chain=0, relax_small_limit=0)  # (the device-side small rounds know no threshold)
    c = world.case(k, "ascending", dtype)
    for light in (0, 2):
        rounds = {}
        for div in sorted({1, delta_div}):
            options(relax_light=light, relax_delta_div=div)
            pgq.reset_stats()
            c.run("ordered rounds, relax_delta_div %d, relax_light %d" % (div, light))
            rounds[div] = pgq.get_stats()["levels"]
        assert delta_div == 1 or rounds[delta_div] > rounds[1] > 0, (c.name, light, rounds)


# ---- 4. batches of 64 lanes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [1, 3])
def test_batch_edges(world, streams):
    options(chain=0, streams=streams)
    for k in (0, 1):
        c = world.case(k, "ascending")
        g = c.g
        srcs = np.unique(g.rs)
        first = next(x["src"] for x in g.gadgets if x["a"] == 4097 and x["pos"] == "last" and x["k"] == 2)
        srcs = np.concatenate([[first], srcs[srcs != first]])  # a list of 4097 edges among the first, whatever U
        for U in (1, 63, 64, 65, 128, 129):
            rows = np.flatnonzero(np.isin(g.rs, srcs[:U]))
            assert len(np.unique(g.rs[rows])) == U and c.deg[first] == 4097
            pgq.reset_stats()
            c.run("the first %d distinct sources, streams %d" % (U, streams), rows)
            assert pgq.get_stats()["batches"] == (U + 63) // 64, (U, pgq.get_stats()["batches"])


# ---- 5. the heavy pass keeps every chunk once ---------------------------------------------------------------------------
def test_heavy_pass_scans_what_the_plain_walk_scans(world):
    options(chain=0, relax_light=0, relax_delta_div=0, relax_small_limit=0)
    for k in (0, 1):
        c = world.case(k, "ascending")
        g = c.g
        for n in (128, 129, 192, 193, 4096, 4097):
            (x,) = [x for x in g.gadgets if x["k"] == 2 and (x["a"], x["b"]) == (n, n) and x["pos"] == "last"]
            row = np.array([x["row"]])
            scanned = {}
            for split in (1, 0):
                options(relax_split=split)
                pgq.reset_stats()
                c.run("one row of gadget %s, relax_split %d" % (x["tag"], split), row)
                scanned[split] = pgq.get_stats()["edges_scanned"]
            print("%s, %s: edges_scanned %d with the heavy pass, %d without" % (c.name, x["tag"], scanned[1], scanned[0]))
            assert scanned[1] == scanned[0] and scanned[1] >= n, (c.name, x["tag"], scanned)


# ---- 6. two-ended relaxation: BidirBatches shares k_relax -----------------------------------------------------------------
@pytest.mark.parametrize("scheme", WEIGHT_SCHEMES)
def test_two_ended_relaxation(world, scheme):
    options(chain=0, relax_bidir=1, relax_light=2, relax_bidir_rows=4)
    shipped = [int(pgq.get_default_option(key)) for key in ("relax_bidir_c0_div", "relax_bidir_step_div")]
    n = len(world.sides[0].rs)
    assert n <= 4 * len(np.unique(world.sides[0].rs)) and n <= 4 * len(np.unique(world.sides[1].rs))  # the rows qualify
    # four of the eight (orientation, label width, caps) combinations, cut as a Latin square: every value of each axis meets
    # every value of each other axis once, the full product is not run
    for k, labels32, (c0, step) in ((0, 1, shipped), (0, 0, (1 << 30, 1 << 30)), (1, 1, (1 << 30, 1 << 30)), (1, 0, shipped)):
        c = world.case(k, scheme)
        options(relax_labels32=labels32, relax_bidir_c0_div=c0, relax_bidir_step_div=step)
        pgq.reset_stats()
        c.run("two-ended, relax_labels32 %d, relax_bidir_c0_div %d, relax_bidir_step_div %d" % (labels32, c0, step))
        # a batch of the two-ended search is 64 ROWS (every row here needs a search), one of the one-sided search 64 sources
        assert pgq.get_stats()["batches"] == (n + 63) // 64 != 25


# ---- 7. k_wbibfs walks the lists its own way -------------------------------------------------------------------------------
@pytest.mark.parametrize("delta_div", [8, 100000])
def test_weighted_pair_search(world, delta_div):
    options(chain=1, wbibfs_rows=1 << 20, wbibfs_delta_div=delta_div)
    for scheme in WEIGHT_SCHEMES:
        for k in (0, 1):
            c = world.case(k, scheme)
            settled = {}
            for wbibfs in (0, 1):  # meet_pairs counts the rows the chain walk settles, too: k_wbibfs must add to them
                options(wbibfs=wbibfs)
                pgq.reset_stats()
                c.run("wbibfs %d, wbibfs_delta_div %d" % (wbibfs, delta_div))
                settled[wbibfs] = pgq.get_stats()["meet_pairs"]
            assert settled[1] > settled[0] > 0, (c.name, settled)


# ---- 8. long chains --------------------------------------------------------------------------------------------------------
CHAIN_V = 8200
LONG_ENDS, SHORT_ENDS = (1, 4095, 4096, 4097, 8191, 8192, 8193, 8199), (1, 150, 298, 299)


def chain_graph(n, ring, double):
    s = np.arange(n - 1 + ring, dtype=np.int64)
    d = (s + 1) % n
    w = 1 + s % 7
    return s, d, (w * 0.1 if double else w)


@pytest.fixture(scope="module")
def chains():
    """(name, V, device handle, rows, the oracle's answers): a directed path and the same path closed into a ring, int64 and
    inexact double weights, over 8,200 vertices and over a prefix of 300."""
    out = []
    for n, ends in ((CHAIN_V, LONG_ENDS), (300, SHORT_ENDS)):
        ps = np.array([0] * len(ends) + [n - 1], dtype=np.int64)
        pd = np.array(list(ends) + [0], dtype=np.int64)  # the last row runs against the direction
        for ring in (0, 1):
            for double in (False, True):
                s, d, w = chain_graph(n, ring, double)
                off, adj, order = csr_arrays_from_rows(n, s, d)
                eid = np.arange(len(s), dtype=np.int64)
                want = OracleCSR.adopt(n, off, adj, eid, w[order]).lean_cheapest_path_length(n, ps, pd)
                assert want[1][:-1].all() and want[1][-1] == bool(ring)
                name = "%s of %d vertices, %s" % ("ring" if ring else "path", n, "double" if double else "int64")
                out.append((name, n, pgq.DeviceCSR(n, off, adj, eid, w[order]), ps, pd, want))
    return out


def run_chains(chains, n, what):
    for name, V, dev, ps, pd, (want, wok) in chains:
        if V != n:
            continue
        out, ok = dev.cheapest_path_length(ps, pd)
        bad = differing(out, ok, want, wok)
        assert len(bad) == 0, "%s, %s: first differing row %d -> %d got %r (valid %s), expected %r (valid %s)" % (
            name, what, ps[bad[0]], pd[bad[0]], out[bad[0]], ok[bad[0]], want[bad[0]], wok[bad[0]])
        yield name


def test_long_chain_small_rounds_are_started_again(chains):
    # k_relax_small ends a launch after 4096 rounds; a path of 8,199 edges needs 8,200
    options(chain=0, relax_light=0, relax_small_limit=2048)
    pgq.reset_stats()
    for name in run_chains(chains, CHAIN_V, "device-side rounds"):
        stats = pgq.get_stats()
        assert stats["levels"] >= CHAIN_V - 1 and stats["launches"]["relax"] >= 3, (name, stats["levels"], stats["launches"]["relax"])
        pgq.reset_stats()


def run_chain_walk(chains, n, chain_cap, ends):
    """k_chain_walk answers a row of d steps if d <= chain_cap and hands it over at step >= chain_cap; the row against the
    direction ends at once, at a vertex without out-edges (path) or after one step (ring).  meet_pairs counts what the walk
    settled; with every row settled no relaxation round runs."""
    settled = sum(d <= chain_cap for d in ends) + 1
    pgq.reset_stats()
    for name in run_chains(chains, n, "chain_cap %d" % chain_cap):
        stats = pgq.get_stats()
        assert stats["meet_pairs"] == settled, (name, chain_cap, stats["meet_pairs"], settled)
        assert (stats["levels"] == 0) == (settled == len(ends) + 1), (name, chain_cap, stats["levels"])
        pgq.reset_stats()


@pytest.mark.parametrize("chain_cap", [4095, 4096, 4097, CHAIN_V])
def test_long_chain_hand_over_at_the_cap(chains, chain_cap):
    # rows at 4095, 4096 and 4097 steps on both sides of the cap; on the ring no row ends at a vertex without out-edges
    options(chain=1, chain_cap=chain_cap, relax_light=0, relax_small_limit=2048)
    run_chain_walk(chains, CHAIN_V, chain_cap, LONG_ENDS)


def test_short_chain_host_rounds(chains):
    options(chain=0, relax_light=0, relax_small_limit=0)
    pgq.reset_stats()
    assert len(list(run_chains(chains, 300, "host rounds"))) == 4
    assert pgq.get_stats()["levels"] >= 4 * 299
    for chain_cap in (149, 150, 151, 300):  # the hand-over again, into rounds the host drives
        options(chain=1, chain_cap=chain_cap)
        run_chain_walk(chains, 300, chain_cap, SHORT_ENDS)


# ---- 9. both entry forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int64", "double_inexact"])
def test_chunk_form_with_selection_and_nulls_equals_bulk_form(world, dtype):
    import torch
    for key in KEYS:  # as shipped, the chain pre-pass included
        pgq.set_option(key, pgq.get_default_option(key))
    rng = np.random.default_rng(99)
    for k in (0, 1):
        c = world.case(k, "ascending", dtype)
        g = c.g
        n = len(g.rs)
        sel = rng.permutation(n).astype(np.uint32)  # the same selection on both sides: every row stays a gadget row
        valid = np.arange(n) % 7 != 3               # per position of the data, not per row
        keep = []
        sv, dv = make_vec(g.rs, sel=sel, valid=valid, keep=keep), make_vec(g.rd, sel=sel, keep=keep)
        out = np.zeros(n, dtype=c.out.dtype)
        ov = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
        _check(c.dev.L.pgq_cheapest_path_length(c.dev.h, g.V, n, sv, dv, _p(out), _p(ov)))
        ok = unpack_validity(ov, n)
        want_ok = c.ok[sel] & valid[sel]
        bad = differing(out, ok, c.out[sel], want_ok)
        assert len(bad) == 0, "%s, chunk form: %d rows differ, first: gadget %s" % (c.name, len(bad), g.tag[sel[bad[0]]])
        assert (~valid[sel]).sum() > 300 and not ok[~valid[sel]].any()
        d_src = torch.from_numpy(np.where(valid[sel], g.rs[sel], -1)).cuda()  # a NULL source of the bulk form
        d_dst = torch.from_numpy(g.rd[sel]).cuda()
        d_val = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        c.dev.cheapest_bulk_ptr(n, d_src.data_ptr(), d_dst.data_ptr(), d_val.data_ptr(), d_ok.data_ptr())
        bval, bok = d_val.cpu().numpy(), d_ok.cpu().numpy().astype(bool)
        bad = differing(bval, bok, c.out[sel], want_ok)
        assert len(bad) == 0, "%s, bulk form: %d rows differ, first: gadget %s" % (c.name, len(bad), g.tag[sel[bad[0]]])
        assert (bok == ok).all() and (bits(bval)[ok] == bits(out)[ok]).all()
