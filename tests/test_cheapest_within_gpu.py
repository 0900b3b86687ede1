"""cheapest_path_length_within on the GPU: the cost of the cheapest walk of at most K edges, in every entry form.

The CPU oracle has no bounded form (the reference's Bellman-Ford sweeps in place: its rounds are not hops), so bounded
expectations come from the Python model of cheapest_within_model.py, which test_cheapest_within_cpu.py checks against a
brute-force enumeration of walks and whose mutants the fixtures used here catch.  Two kinds of expectation come from the
oracle instead: K >= V - 2, where the bounded answer IS the unbounded one, and the degree gadgets of
helpers.degree_gadgets(**WEIGHTED_GADGETS) — each gadget's endpoints are joined by paths of one length only and its decoys
are dead ends, so a gadget row is valid iff 0 <= dist <= K and then equals the oracle's unbounded value.  That claim was
checked with the model on the CPU (test_cheapest_within_cpu.py::test_gadget_rows_cost_what_the_unbounded_search_says): it
holds for every main and reversed row and for all side rows (an endpoint and a shared dead end, two edges apart) but ONE — in
the transposed graph under `ascending` weights the dead end of k4_a129_b1_last_sink is also one the gadget's own far endpoint
points to, and the five-edge walk round the gadget costs 68 where the two-edge walk costs 592.  The gadget rows are therefore
compared with the model, all of them, and the oracle's value is asserted beside it on every row the model agrees on.
Every comparison is exact: validity, int64 values, doubles as bit patterns."""
import ctypes as C

import numpy as np
import pytest

import cheapest_within_model as M
import duckpgq_extension_amd as pgq
from duckpgq_extension_amd.binding import _p, make_vec, unpack_validity
from helpers import WEIGHTED_GADGETS, csr_arrays_from_rows, degree_gadgets, weighted_gadgets
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

INT64_MAX = np.iinfo(np.int64).max
# every option these calls depend on, at the value a test starts from (another file may have left its own); SHIPPED: the
# library's own value, read from it
SHIPPED = ("chain_cap", "wbibfs_rows", "wbibfs_delta_div", "wbibfs_cap", "wbibfs_queue", "wbibfs_far", "wbibfs_prune",
           "wbibfs_mem_mb", "relax_light", "relax_light_div", "relax_light_min_degree", "relax_labels32", "relax_split",
           "relax_small_limit", "relax_bidir_rows", "relax_bidir_c0_div", "relax_bidir_step_div", "chain", "wbibfs")
KEYS = {"streams": 1, "relax_streams": 0, "relax_delta_div": 0, "relax_bidir": 0}


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


def device(V, off, adj, w):
    return pgq.DeviceCSR(V, off, adj, np.arange(len(adj), dtype=np.int64), w)


def oracle(V, off, adj, w):
    return OracleCSR.adopt(V, off, adj, np.arange(len(adj), dtype=np.int64), w)


def expect(got, want, what, rs, rd):
    bad = M.differing(got[0], got[1], want[0], want[1])
    assert len(bad) == 0, "%s: %d of %d rows differ, first: %d -> %d got %r (valid %s), expected %r (valid %s)" % (
        what, len(bad), len(rs), rs[bad[0]], rd[bad[0]], got[0][bad[0]], got[1][bad[0]], want[0][bad[0]], want[1][bad[0]])


# ---- 1. the bound changes the value -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True], ids=["int64", "double"])
def test_bound_changes_the_value(double):
    V, off, adj, w = M.shortcut_path(double)
    dev = device(V, off, adj, w)
    for K, want in enumerate((None, 60, 51, 42, 33, 24, 6)):
        out, ok = dev.cheapest_path_length_within([0], [6], K)
        if want is None:
            assert not ok[0], (K, out)
        else:
            assert ok[0] and out[0] == want and out.dtype == (np.float64 if double else np.int64), (K, out, ok)
    out, ok = dev.cheapest_path_length([0], [6])
    assert ok[0] and out[0] == 6
    dev.close()


# ---- 2. one edge per round ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True], ids=["int64", "double"])
def test_one_edge_per_round(double):
    V, off, adj, w, rs, rd = M.path_graph(200, double)
    fold = [0.0]
    for _ in range(5):
        fold.append(fold[-1] + 0.1)  # left to right: 0.1 + 0.1 + 0.1 is not 3 * 0.1
    value = np.array(fold)[rd - rs] if double else rd - rs
    dev = device(V, off, adj, w)
    for K in range(1, 5):
        pgq.reset_stats()
        got = dev.cheapest_path_length_within(rs, rd, K)
        within = rd - rs <= K
        expect(got, (np.where(within, value, 0), within), "path of 200, K = %d" % K, rs, rd)
        stats = pgq.get_stats()
        assert stats["batches"] == 4 and stats["levels"] == 4 * K, (K, stats["batches"], stats["levels"])  # 199 sources; every queue lives on
    dev.close()
    V, off, adj, w, rs, rd, t = M.zero_ring(130, double)
    dev = device(V, off, adj, w)
    for K in range(1, 5):
        got = dev.cheapest_path_length_within(rs, rd, K)  # (returns: a zero-weight cycle improves nothing, so requeues nothing)
        expect(got, (np.zeros(len(rs), dtype=w.dtype), t <= K), "ring of 130, K = %d" % K, rs, rd)
    dev.close()


# ---- 3. lane and batch edges -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lanes_graph():
    V, off, adj, w = M.random_graph(500, 3500, "int_small", seed=3)
    return V, off, adj, w, device(V, off, adj, w)


@pytest.mark.parametrize("U", [63, 64, 65, 129])
def test_lane_and_batch_edges(lanes_graph, U):
    V, off, adj, w, dev = lanes_graph
    rng = np.random.default_rng(U)
    rs = np.repeat(rng.choice(V, U, replace=False), 3).astype(np.int64)
    rd = (rs + 1 + rng.integers(0, V - 1, len(rs))) % V  # never the source itself: every source needs a lane
    perm = rng.permutation(len(rs))
    rs, rd = rs[perm], rd[perm]
    want = M.bounded_cheapest(V, off, adj, w, rs, rd, [2])[2]
    assert want[1].any() and not want[1].all()
    pgq.reset_stats()
    expect(dev.cheapest_path_length_within(rs, rd, 2), want, "%d distinct sources, K = 2" % U, rs, rd)
    assert pgq.get_stats()["batches"] == (U + 63) // 64


# ---- 4. list lengths on the walk's constants ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gadget_sides():
    g = degree_gadgets(**WEIGHTED_GADGETS)
    sides = [g, g.transposed()]
    return [(x, csr_arrays_from_rows(x.V, x.src, x.dst)) for x in sides]


@pytest.mark.parametrize("dtype", ["int64", "double_inexact"])
@pytest.mark.parametrize("scheme", ["ascending", "witness_heaviest"])
def test_list_lengths(gadget_sides, scheme, dtype):
    """Lists of 7 .. 9, 15 .. 17, 63 .. 65 and 4095 .. 4097 edges (among others), the only path in the first, last, 8th and 9th
    slot: a trip's eighth edge, the one-edge last trip, the lists one wavefront walks alone.  Every row is compared with the
    model; the oracle's unbounded value where 0 <= dist <= K is the same thing on every row but the side rows the model says
    otherwise about (see the file's docstring), at most one per orientation."""
    for name, (g, (off, adj, order)) in zip(("graph", "transpose"), gadget_sides):
        w = weighted_gadgets(g, scheme, dtype)[order]
        dev = device(g.V, off, adj, w)
        out, ok = oracle(g.V, off, adj, w).lean_cheapest_path_length(g.V, g.rs, g.rd)
        assert (ok == (g.dist >= 0)).all()
        model = M.bounded_cheapest(g.V, off, adj, w, g.rs, g.rd, range(1, 5))
        for K in range(1, 5):
            within = (g.dist >= 0) & (g.dist <= K)
            other = M.differing(model[K][0], model[K][1], out, within)
            assert len(other) <= 1 and all(g.tag[i].endswith(("_sink", "_root")) for i in other), (name, K, g.tag[other])
            got = dev.cheapest_path_length_within(g.rs, g.rd, K)
            bad = M.differing(got[0], got[1], model[K][0], model[K][1])
            assert len(bad) == 0, "%s, %s %s, K = %d: %d rows differ, first: gadget %s got %r (valid %s), expected %r (valid %s)" % (
                name, scheme, dtype, K, len(bad), g.tag[bad[0]], got[0][bad[0]], got[1][bad[0]], model[K][0][bad[0]], model[K][1][bad[0]])
        dev.close()


# ---- 5. random graphs ---------------------------------------------------------------------------------------------------------------
RANDOM_V, RANDOM_E = 2000, 14000
BOUNDED_KS = (0, 1, 2, 3, 5)


class RandomCase:
    def __init__(self, kind):
        self.kind = kind
        self.V, self.off, self.adj, self.w = M.random_graph(RANDOM_V, RANDOM_E, kind)
        self.rs, self.rd = M.random_rows(self.V)
        self.dev = device(self.V, self.off, self.adj, self.w)
        self.ora = oracle(self.V, self.off, self.adj, self.w)
        self.model = M.bounded_cheapest(self.V, self.off, self.adj, self.w, self.rs, self.rd, BOUNDED_KS)  # once, shared, never changed
        self.unbounded = self.ora.cheapest_path_length(self.V, self.rs, self.rd)  # the literal Bellman-Ford restatement


@pytest.fixture(scope="module")
def random_cases():
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = RandomCase(kind)
        return cache[kind]
    return get


@pytest.mark.parametrize("kind", ["int_small", "int_wide", "double_special"])
def test_random_graphs(random_cases, kind):
    c = random_cases(kind)
    valid = {K: int(c.model[K][1].sum()) for K in BOUNDED_KS}
    assert 0 < valid[0] < valid[1] < valid[2] < valid[3] < valid[5] <= int(c.unbounded[1].sum()), valid
    changed = M.differing(c.model[3][0], c.model[3][1], c.unbounded[0], c.model[3][1])
    assert len(changed) > 0  # rows whose cheapest walk of at most 3 edges costs more than the cheapest walk
    for K in BOUNDED_KS:
        expect(c.dev.cheapest_path_length_within(c.rs, c.rd, K), c.model[K], "%s, K = %d" % (kind, K), c.rs, c.rd)
    for K in (c.V - 2, c.V - 1, INT64_MAX):
        expect(c.dev.cheapest_path_length_within(c.rs, c.rd, K), c.unbounded, "%s, K = %d" % (kind, K), c.rs, c.rd)


@pytest.mark.parametrize("kind", ["int_ones", "double_ones"])
def test_unit_weights_count_hops(random_cases, kind):
    c = random_cases(kind)
    hops, reach = c.ora.lean_iterativelength(c.V, c.rs, c.rd)
    for K in BOUNDED_KS + (c.V - 2,):
        within = reach & (hops <= K)
        want = np.where(within, hops, 0).astype(c.w.dtype)
        expect(c.dev.cheapest_path_length_within(c.rs, c.rd, K), (want, within), "%s, K = %d" % (kind, K), c.rs, c.rd)


# ---- 6. every form gives the same rows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("kind", ["int_small", "double_special"])
def test_every_form_gives_the_same_rows(random_cases, kind, streams):
    import torch
    options(streams=streams)
    c = random_cases(kind)
    K = 3
    want_out, want_ok = c.model[K]
    n = len(c.rs)
    rng = np.random.default_rng(5)
    # the chunk form: a selection vector, NULL sources and NULL destinations (validity is per position of the data)
    sel = rng.permutation(n).astype(np.uint32)
    src_valid, dst_valid = np.arange(n) % 7 != 3, np.arange(n) % 11 != 5
    live = (src_valid & dst_valid)[sel]
    out, ok = c.dev.cheapest_path_length_within(c.rs, c.rd, K, src_valid=src_valid, dst_valid=dst_valid, src_sel=sel, dst_sel=sel)
    expect((out, ok), (want_out[sel], want_ok[sel] & live), "%s, chunk form" % kind, c.rs[sel], c.rd[sel])
    assert (~live).sum() > 100 and not ok[~live].any()
    # the bulk-device form (a NULL source is -1 there)
    d_src = torch.from_numpy(np.where(live, c.rs[sel], -1)).cuda()
    d_dst = torch.from_numpy(c.rd[sel]).cuda()
    d_val = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    c.dev.cheapest_within_bulk_ptr(n, d_src.data_ptr(), d_dst.data_ptr(), K, d_val.data_ptr(), d_ok.data_ptr())
    bval, bok = d_val.cpu().numpy().view(c.w.dtype), d_ok.cpu().numpy().astype(bool)
    expect((bval, bok), (want_out[sel], want_ok[sel] & live), "%s, bulk form" % kind, c.rs[sel], c.rd[sel])
    # every enabled device, here the same one twice: the second shard runs on the replica
    assert pgq.init_devices([0, 0]) == 2
    try:
        expect(c.dev.cheapest_path_length_within_multi(c.rs, c.rd, K), (want_out, want_ok), "%s, multi form" % kind, c.rs, c.rd)
    finally:
        pgq.init_devices([0])
    # the UDF layer: rows in slot order build the same CSR
    st = pgq.PgqState()
    es = np.repeat(np.arange(c.V, dtype=np.int64), np.diff(c.off))
    st.build_csr(0, c.V, es, c.adj, np.arange(len(c.adj), dtype=np.int64), w=c.w)
    out, ok = st.cheapest_path_length_within(0, c.V, c.rs, c.rd, K, src_valid=src_valid, dst_valid=dst_valid, src_sel=sel, dst_sel=sel)
    expect((out, ok), (want_out[sel], want_ok[sel] & live), "%s, PgqState" % kind, c.rs[sel], c.rd[sel])


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------
def raw_calls(dev, rs, rd, K):
    """(status, message) of the chunk and the bulk form, bounded (K an int) or unbounded (K None)."""
    import torch
    L = dev.L
    n = len(rs)
    keep = []
    sv, dv = make_vec(np.asarray(rs, dtype=np.int64), keep=keep), make_vec(np.asarray(rd, dtype=np.int64), keep=keep)
    out, ov = np.zeros(n, dtype=np.int64), np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
    d_src, d_dst = torch.tensor(rs, dtype=torch.int64).cuda(), torch.tensor(rd, dtype=torch.int64).cuda()
    d_val, d_ok = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    res = []
    if K is None:
        res.append((L.pgq_cheapest_path_length(dev.h, dev.V, n, sv, dv, _p(out), _p(ov)), L.pgq_last_error().decode()))
        res.append((L.pgq_cheapest_path_length_bulk_device(dev.h, n, ptr(d_src), ptr(d_dst), ptr(d_val), ptr(d_ok)), L.pgq_last_error().decode()))
    else:
        res.append((L.pgq_cheapest_path_length_within(dev.h, dev.V, n, sv, dv, K, _p(out), _p(ov)), L.pgq_last_error().decode()))
        res.append((L.pgq_cheapest_path_length_within_bulk_device(dev.h, n, ptr(d_src), ptr(d_dst), K, ptr(d_val), ptr(d_ok)), L.pgq_last_error().decode()))
    return res


def test_errors():
    V, off, adj, w = M.shortcut_path(False)
    dev = device(V, off, adj, w)
    for rc, msg in raw_calls(dev, [0], [6], -1):
        assert rc == -4 and msg == "max_hops must not be negative", (rc, msg)  # PGQ_ERR_INVALID_ARG
    with pytest.raises(pgq.PgqError, match="max_hops must not be negative"):
        dev.cheapest_path_length_within_multi([0], [6], -1)
    # an id >= V, an unweighted CSR, a negative weight: status and message of the unbounded call
    bad_id = raw_calls(dev, [0, 0], [6, V], 3)
    assert bad_id == raw_calls(dev, [0, 0], [6, V], None) and all(rc == -4 for rc, _ in bad_id), bad_id
    plain = pgq.DeviceCSR(V, off, adj, np.arange(len(adj), dtype=np.int64))
    unweighted = raw_calls(plain, [0], [6], 3)
    assert unweighted == raw_calls(plain, [0], [6], None), unweighted
    assert all(rc == -5 and "Need to initialize CSR before doing cheapest path" in msg for rc, msg in unweighted), unweighted
    wn = w.copy()
    wn[3] = -1
    negative = device(V, off, adj, wn)
    neg = raw_calls(negative, [0], [6], 3)
    assert neg == raw_calls(negative, [0], [6], None), neg
    assert all(rc == -6 and "negative edge weights are not supported" in msg for rc, msg in neg), neg
    for d in (dev, plain, negative):
        d.close()


# ---- 8. the search stops at the bound -----------------------------------------------------------------------------------------------
def test_stops_at_the_bound(random_cases):
    c = random_cases("int_small")
    pgq.reset_stats()
    expect(c.dev.cheapest_path_length_within(c.rs, c.rd, 2), c.model[2], "K = 2", c.rs, c.rd)
    stats = pgq.get_stats()
    assert 0 < stats["levels"] <= 2 * stats["batches"], (stats["levels"], stats["batches"])
    assert stats["edges_scanned"] > 0 and stats["launches"]["relax"] >= stats["levels"]  # (a round enqueued behind an empty queue is none)
    pgq.reset_stats()
    expect(c.dev.cheapest_path_length_within(c.rs, c.rd, 0), c.model[0], "K = 0", c.rs, c.rd)
    stats = pgq.get_stats()
    assert stats["levels"] == 0 and stats["launches"]["relax"] == 0 and stats["batches"] > 0, stats


# ---- 9. a bounded call leaves the workspace sound ------------------------------------------------------------------------------------
def test_leaves_the_workspace_sound():
    """The snapshot rows live in the label array of the two-ended search's backward side: a two-ended call behind a bounded
    one must fill that array again, and a bounded call behind it must not trust what it left."""
    V, off, adj, w = M.random_graph(RANDOM_V, RANDOM_E, "int_small", seed=21)
    rng = np.random.default_rng(21)
    rs = np.repeat(rng.permutation(V)[:200], 2).astype(np.int64)  # two destinations per source: the two-ended search takes them
    rd = rng.integers(0, V, 400)
    model = M.bounded_cheapest(V, off, adj, w, rs, rd, [3])[3]
    unbounded = oracle(V, off, adj, w).lean_cheapest_path_length(V, rs, rd)
    before = pgq.live_device_blocks()
    dev = device(V, off, adj, w)
    expect(dev.cheapest_path_length_within(rs, rd, 3), model, "bounded, first", rs, rd)
    options(chain=0, wbibfs=0, relax_bidir=1, relax_light=2, relax_bidir_rows=4)
    pgq.reset_stats()
    expect(dev.cheapest_path_length(rs, rd), unbounded, "two-ended, unbounded", rs, rd)
    assert pgq.get_stats()["batches"] > 4  # batches of 64 ROWS, not of 64 of the 200 sources: the two-ended drivers ran
    expect(dev.cheapest_path_length_within(rs, rd, 3), model, "bounded, again", rs, rd)
    dev.close()
    assert pgq.live_device_blocks() == before
