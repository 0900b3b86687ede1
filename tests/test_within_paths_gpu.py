"""shortestpath_within(src, dst, max_hops): shortestpath, except that a row whose path has more than max_hops hops is NULL
and takes no room in the child payload.

Expected value everywhere: the CPU oracle's lean_shortestpath list P = [src, e1, v1, ..., ek, dst] per row; the row's
expectation is P when the row is valid, P is not None and (len(P) - 1) // 2 <= max_hops, else None.  Lists compare element
for element (vertices and edge ids).  Checked through the chunk form (DeviceCSR.shortestpath_within: the lists land in the
library's own child buffer), the bulk form (shortestpath_within_bulk_ptr: the caller's child buffer — the C entry point takes
no other), the scalar-function form (PgqState.shortestpath_within) and the multi form, by the pre-pass chain with both
k_meet4<paths> map variants and by the lane batches, with the caps at their smallest, and with conditions on the statistics
and on the child payload's size that only hold when the search stops at the bound and lays out no list beyond it."""
import ctypes as C

import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from helpers import LDS_LIMITS, degree_gadgets, sparse_ids_graph
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

BOUNDS = (0, 1, 2, 3, 4, 5, 8)
UNBOUNDED = 2 ** 62

KEYS = ("meet", "meet_bias", "meet_cap", "meet_cap_small", "meet_cap_paths", "meet4", "meet4_cap", "meet4_test_cap",
        "meet4_lds_kb", "meet4_global_mb", "meet_layout", "meet_small_rows", "meet_wide_rows", "meet_wide_rows_always",
        "paths_reserve_mb", "bibfs_rows", "bibfs_cap", "bibfs_queue", "bibfs_grid", "ball", "ball_head_mb", "ball_cap",
        "ball_test_cap", "ball_grid", "ball_bias", "ball_sort", "ball_seg_kb", "words", "lanes", "force_mode", "force_pull",
        "sparse_lds", "blocks_per_cu", "probe", "defer", "route_timing", "route_timing_rows", "route_try_factor", "route_memo",
        "calibration_cache", "spec_levels", "chunk_zero_copy")


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def hops(p):
    return (len(p) - 1) // 2


def expect(paths, valid, U):
    """Expected lists: the oracle's where the row is valid and the path has at most U hops, else None (NULL)."""
    return [p if (ok and p is not None and hops(p) <= U) else None for p, ok in zip(paths, valid)]


def need_of(want):
    return sum(len(p) for p in want if p is not None)


def upload(V, s, d):
    st = pgq.PgqState()
    st.build_csr(0, V, s, d)
    return st


def lists_of(ln, off, child):
    return [None if ln[i] < 0 else child[off[i]:off[i] + 2 * ln[i] + 1].tolist() for i in range(len(ln))]


class Rows:
    """The forms of one call on the same rows (valid: the rows' src validity)."""

    def __init__(self, st, V, ps, pd, valid=None):
        import torch
        self.st, self.V, self.ps, self.pd = st, V, np.asarray(ps, dtype=np.int64), np.asarray(pd, dtype=np.int64)
        self.n = len(self.ps)
        self.valid = np.ones(self.n, dtype=bool) if valid is None else np.asarray(valid)
        self.dev = st.device_csr(0)
        self.h_s = np.where(self.valid, self.ps, -1).astype(np.int64)  # bulk and multi forms: src < 0 is a NULL row
        self.t_s = torch.from_numpy(self.h_s).cuda()
        self.t_d = torch.from_numpy(self.pd).cuda()

    def chunk(self, U):
        return self.dev.shortestpath_within(self.ps, self.pd, U, src_valid=self.valid)

    def chunk_raw(self, U):
        return self.dev.shortestpath_within(self.ps, self.pd, U, src_valid=self.valid, raw=True)

    def udf(self, U):
        return self.st.shortestpath_within(0, self.V, self.ps, self.pd, U, src_valid=self.valid)

    def bulk_raw(self, U, cap):
        """(rc, child_used, lengths, offsets, child) of the bulk form with a child buffer of `cap` elements; U None: unbounded."""
        import torch
        t_len = torch.full((self.n,), -7, dtype=torch.int64, device="cuda")
        t_off = torch.full((self.n,), -7, dtype=torch.int64, device="cuda")
        t_child = torch.full((max(cap, 1),), -7, dtype=torch.int64, device="cuda")
        args = (t_len.data_ptr(), t_off.data_ptr(), t_child.data_ptr(), cap)
        if U is None:
            rc, used = self.dev.shortestpath_bulk_ptr(self.n, self.t_s.data_ptr(), self.t_d.data_ptr(), *args)
        else:
            rc, used = self.dev.shortestpath_within_bulk_ptr(self.n, self.t_s.data_ptr(), self.t_d.data_ptr(), U, *args)
        return rc, used, t_len.cpu().numpy(), t_off.cpu().numpy(), t_child.cpu().numpy()

    def roomy(self):
        return 64 * self.n + 1024  # elements: room for a list of 31 hops per row

    def bulk(self, U):
        """The bulk form's lists, from a buffer every call fits."""
        rc, used, ln, off, child = self.bulk_raw(U, self.roomy())
        assert rc == 0, rc
        got = lists_of(ln, off, child)
        assert used == need_of(got), "child_used counts the lists of the rows within the bound only"
        assert (child[used:] == -7).all(), "nothing is written behind child_used"
        return got


def assert_lists(got, want, rows, what):
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert len(got) == len(want) and not bad, "%s: %d of %d lists differ, first (src %d, dst %d): got %s, expected %s" % (
        what, len(bad), len(want), rows.ps[bad[0]], rows.pd[bad[0]], got[bad[0]], want[bad[0]])


def check_forms(rows, paths, bounds, forms=("chunk", "bulk", "udf"), what=""):
    for U in bounds:
        want = expect(paths, rows.valid, U)
        for form in forms:
            assert_lists(getattr(rows, form)(U), want, rows, "%s %s form, max_hops %d" % (what, form, U))


class Case:
    """The graph and rows of test_within_gpu.Case: random pairs, every chain pair both ways, ~1 % src == dst, ~3 % NULL src;
    with the oracle's list of every row."""

    def __init__(self, V, seed):
        rng = self.rng = np.random.default_rng(seed)
        self.V = V
        act, s, d, hubs, chains = sparse_ids_graph(rng, V, 12000, 30000, hubs=1, chains=8, chain_len=10)
        self.act, self.s, self.d, self.hubs, self.chains = act, s, d, hubs, chains
        self.ora = OracleCSR.from_edges(V, s, d)
        top = V - 1
        ends = np.array([0, V - 1, V - 2, V // 2, top // 32 * 32, top // 128 * 128, hubs[0]], dtype=np.int64)
        ps = [act[rng.integers(0, len(act), 1500)], np.repeat(ends, 8), rng.choice(ends, 60)]
        pd = [act[rng.integers(0, len(act), 1500)], rng.choice(act, 8 * len(ends)), np.repeat(ends, 60 // len(ends) + 1)[:60]]
        cs, cd = [], []
        for c in chains:  # every pair along a chain (distance j - i) and against it (unreachable)
            i, j = np.triu_indices(len(c), 1)
            cs += [c[i], c[j]]
            cd += [c[j], c[i]]
        self.chain_s, self.chain_d = np.concatenate(cs).astype(np.int64), np.concatenate(cd).astype(np.int64)
        ps, pd = np.concatenate(ps + cs).astype(np.int64), np.concatenate(pd + cd).astype(np.int64)
        same = rng.random(len(ps)) < 0.01
        pd[same] = ps[same]
        perm = rng.permutation(len(ps))
        self.ps, self.pd = ps[perm], pd[perm]
        self.valid = rng.random(len(ps)) > 0.03
        self.dist = self.distances(self.ps, self.pd)

    def distances(self, ps, pd):
        oln, ook = self.ora.lean_iterativelength(self.V, ps, pd, nthreads=8)
        return np.where(ook, oln, -1)

    def paths_of(self, ps, pd):
        return self.ora.lean_shortestpath(self.V, ps, pd)


@pytest.fixture(scope="module")
def case():
    c = Case(20000, seed=20000)
    d = c.dist
    # what the sweep relies on, on the oracle, before any GPU call
    assert (d == 4).any() and (d >= 5).sum() >= 100 and (d < 0).any()
    for U in BOUNDS:
        assert (d == U).any() and (d == U + 1).any(), U
    c.paths = c.paths_of(c.ps, c.pd)  # computed once, shared, never changed
    assert [(-1 if p is None else hops(p)) for p in c.paths] == d.tolist()
    return c


# ---- 1: the parity sweep ------------------------------------------------------------------------------------------------
def test_parity_sweep_all_forms(case):
    st = upload(case.V, case.s, case.d)
    rows = Rows(st, case.V, case.ps, case.pd, case.valid)
    check_forms(rows, case.paths, BOUNDS + (UNBOUNDED,), what="sweep")
    # the LIST vector as DuckDB sees it
    for U in BOUNDS + (UNBOUNDED,):
        want = expect(case.paths, case.valid, U)
        off, ln, ov, child = rows.chunk_raw(U)
        ok = pgq.binding.unpack_validity(ov, rows.n)
        assert (ok == np.array([p is not None for p in want])).all(), U
        within = (case.dist >= 0) & (case.dist <= U) & case.valid
        assert len(child) == int((2 * case.dist[within] + 1).sum()), "child_len at max_hops %d" % U
        assert (off[~ok] == 0).all() and (ln[~ok] == 0).all(), "a NULL row's entry is {0, 0}"
        o, l = off[ok].astype(np.int64), ln[ok].astype(np.int64)
        assert (l == 2 * case.dist[ok] + 1).all() and (o + l <= len(child)).all(), U
        order = np.argsort(o, kind="stable")
        assert (o[order][1:] >= (o + l)[order][:-1]).all(), "no two lists overlap (max_hops %d)" % U
    # 2^62 is the unbounded search: same lists, same payload size, in every form
    unb = rows.dev.shortestpath(case.ps, case.pd, src_valid=case.valid)
    assert unb == expect(case.paths, case.valid, UNBOUNDED)
    for form in ("chunk", "bulk", "udf"):
        assert getattr(rows, form)(UNBOUNDED) == unb, form
    assert len(rows.chunk_raw(UNBOUNDED)[3]) == len(rows.dev.shortestpath(case.ps, case.pd, src_valid=case.valid, raw=True)[3])
    cap = rows.roomy()
    rc_b, used_b = rows.bulk_raw(UNBOUNDED, cap)[:2]
    rc_u, used_u = rows.bulk_raw(None, cap)[:2]
    assert rc_b == 0 and rc_u == 0 and used_b == used_u == need_of(unb)
    st.delete_csr(0)


# ---- 2: per route -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [1, 8])
def test_route_lane_batches(case, words):
    pgq.set_option("meet", 0)
    pgq.set_option("words", words)
    st = upload(case.V, case.s, case.d)
    rows = Rows(st, case.V, case.ps, case.pd, case.valid)
    pgq.reset_stats()
    check_forms(rows, case.paths, BOUNDS + (UNBOUNDED,), forms=("chunk", "bulk"), what="meet = 0, words = %d" % words)
    stats = pgq.get_stats()
    assert stats["levels"] > 0 and stats["meet_pairs"] == 0
    st.delete_csr(0)


def test_route_prepass_chain(case):
    pgq.set_option("meet", 1)
    pgq.set_option("meet_bias", 1e9)
    st = upload(case.V, case.s, case.d)
    rows = Rows(st, case.V, case.ps, case.pd, case.valid)
    pgq.reset_stats()
    check_forms(rows, case.paths, BOUNDS + (UNBOUNDED,), forms=("chunk", "bulk"), what="meet = 1, meet_bias = 1e9")
    stats = pgq.get_stats()
    assert stats["meet_pairs"] > 0 and stats["launches"]["meet"] >= 1 and stats["launches"]["meet4"] >= 1
    st.delete_csr(0)


def test_route_chunk_sized_call(case):
    pick = np.concatenate([np.flatnonzero(case.dist == k)[:3] for k in (-1, 0, 1, 2, 3, 4, 5, 9)])[:24]
    assert len(pick) == 24
    st = upload(case.V, case.s, case.d)
    rows = Rows(st, case.V, case.ps[pick], case.pd[pick], case.valid[pick])
    check_forms(rows, [case.paths[i] for i in pick], BOUNDS + (UNBOUNDED,), what="24 rows")
    st.delete_csr(0)


# ---- 3: both k_meet4<paths> map variants ------------------------------------------------------------------------------------
@pytest.mark.parametrize("above", [0, 1], ids=["at_limit", "limit_plus_1"])
def test_meet4_map_variants(above):
    V = LDS_LIMITS["meet4"] + above
    c = Case(V, seed=V % 100_003)
    pgq.set_option("meet", 1)
    pgq.set_option("meet_bias", 1e9)
    pgq.set_option("ball", 0)
    ps, pd = np.concatenate([c.chain_s, c.ps[:300]]), np.concatenate([c.chain_d, c.pd[:300]])
    valid = np.concatenate([np.ones(len(c.chain_s), dtype=bool), c.valid[:300]])
    dist = c.distances(ps, pd)
    for U in (3, 4, 5):
        assert (dist == U).any() and (dist == U + 1).any() and (dist < 0).any()
    paths = c.paths_of(ps, pd)
    st = upload(V, c.s, c.d)
    rows = Rows(st, V, ps, pd, valid)
    pgq.reset_stats()
    check_forms(rows, paths, (3, 4, 5), forms=("chunk", "bulk"), what="k_meet4<paths> at V = %d" % V)
    stats = pgq.get_stats()
    n, in_lds = stats["launches"]["meet4"], stats["lds_map_launches"]["meet4"]
    assert n >= 1 and in_lds == (0 if above else n), (V, n, in_lds)
    assert stats["meet_pairs"] > 0
    st.delete_csr(0)


# ---- 4: list lengths on the kernels' thresholds -----------------------------------------------------------------------------
def test_degree_thresholds():
    g = degree_gadgets()
    main = g.main_rows()
    ps, pd, k = g.rs[main], g.rd[main], g.dist[main]
    assert set(k.tolist()) == {1, 2, 3, 4}
    ora = OracleCSR.from_edges(g.V, g.src, g.dst)
    paths = ora.lean_shortestpath(g.V, ps, pd)
    assert [hops(p) for p in paths] == k.tolist()
    pgq.set_option("meet", 1)
    pgq.set_option("meet_bias", 1e9)
    pgq.set_option("ball", 0)
    st = upload(g.V, g.src, g.dst)
    rows = Rows(st, g.V, ps, pd)
    pgq.reset_stats()
    for U in (0, 1, 2, 3, 4):
        got = rows.bulk(U)
        for i in np.flatnonzero(k == U + 1):
            assert got[i] is None, "gadget %s (%d hops) under max_hops %d: %s" % (g.tag[main[i]], k[i], U, got[i])
        for i in np.flatnonzero(k == U):
            assert got[i] == paths[i], "gadget %s (%d hops) under max_hops %d: got %s, expected %s" % (g.tag[main[i]], k[i], U, got[i], paths[i])
        assert_lists(got, expect(paths, rows.valid, U), rows, "gadgets, max_hops %d" % U)
    stats = pgq.get_stats()
    assert stats["meet_pairs"] > 0 and stats["launches"]["meet4"] >= 1
    st.delete_csr(0)


# ---- 5: capped rows are not closed by the bound ------------------------------------------------------------------------------
@pytest.mark.parametrize("meet4_cap", [None, 1], ids=["meet4_cap_default", "meet4_cap_1"])
def test_capped_rows_stay_open(case, meet4_cap):
    # the caps at the smallest value the library takes: every walk is cut, so no stage may conclude "farther than the bound"
    for key in ("meet_cap_paths", "meet_cap", "meet_cap_small", "meet4_test_cap"):
        pgq.set_option(key, 1)
    if meet4_cap is not None:
        pgq.set_option("meet4_cap", meet4_cap)
    hub = int(case.hubs[0])
    out_n = np.unique(case.d[case.s == hub])[:40]
    in_n = np.unique(case.s[case.d == hub])[:40]
    in2 = np.setdiff1d(np.unique(case.s[np.isin(case.d, in_n)]), np.concatenate([in_n, [hub]]))[:40]  # two hops in front of the hub
    assert len(out_n) == 40 and len(in_n) == 40 and len(in2) == 40
    ps = np.concatenate([np.full(40, hub), in_n, out_n, in_n, in_n[::-1], in2, in2]).astype(np.int64)
    pd = np.concatenate([out_n, np.full(40, hub), in_n, out_n, out_n, out_n, np.full(40, hub)]).astype(np.int64)
    dist = case.distances(ps, pd)
    for U in (2, 3, 4):
        assert ((dist >= 1) & (dist <= U)).any(), U
    assert (dist == 2).any() and (dist == 3).any()
    paths = case.paths_of(ps, pd)
    for bias in (None, 1e9):  # the route the library picks, and the pre-pass chain for certain
        if bias is not None:
            pgq.set_option("meet", 1)
            pgq.set_option("meet_bias", bias)
        st = upload(case.V, case.s, case.d)
        rows = Rows(st, case.V, ps, pd)
        check_forms(rows, paths, (2, 3, 4), what="caps at their smallest, meet_bias %s" % bias)
        st.delete_csr(0)


# ---- 6: the search really stops ---------------------------------------------------------------------------------------------
CHAINS, CHAIN_V = 16, 200


def chain_graph():
    ids = np.arange(CHAINS * CHAIN_V, dtype=np.int64).reshape(CHAINS, CHAIN_V)
    return CHAINS * CHAIN_V, ids[:, :-1].ravel().copy(), ids[:, 1:].ravel().copy(), ids[:, 0].copy(), ids[:, -1].copy()


def chain_call(U):
    """The 16 (first, last) rows on a fresh handle; returns (lists, child_len, statistics of the call)."""
    V, s, d, first, last = chain_graph()
    st = upload(V, s, d)
    dev = st.device_csr(0)
    pgq.reset_stats()
    if U is None:
        off, ln, ov, child = dev.shortestpath(first, last, raw=True)
    else:
        off, ln, ov, child = dev.shortestpath_within(first, last, U, raw=True)
    stats = pgq.get_stats()
    got = pgq.binding._lists(off, ln, pgq.binding.unpack_validity(ov, len(first)), child)
    st.delete_csr(0)
    return got, len(child), stats


def test_unbounded_chain_search_runs_every_level():
    far, child_len, s_far = chain_call(None)
    assert all(p is not None and len(p) == 2 * (CHAIN_V - 1) + 1 for p in far) and child_len == CHAINS * (2 * CHAIN_V - 1)
    assert s_far["batches"] >= 1 and s_far["levels"] > 6 * s_far["batches"], (s_far["levels"], s_far["batches"])


@pytest.mark.parametrize("U", [1, 2, 3, 4])
def test_nothing_reaches_the_lanes_under_a_small_bound(U):
    near, child_len, s_near = chain_call(U)
    assert near == [None] * CHAINS and child_len == 0
    # nothing was capped, so the pre-pass closes every row itself
    assert s_near["batches"] == 0 and s_near["levels"] == 0, (U, s_near["batches"], s_near["levels"])


def test_lane_batches_launch_no_level_past_the_bound():
    pgq.set_option("meet", 0)
    near, child_len, s_near = chain_call(6)
    assert near == [None] * CHAINS and child_len == 0
    assert s_near["batches"] >= 1 and s_near["levels"] <= 6 * s_near["batches"], (s_near["levels"], s_near["batches"])


# ---- 7: child buffer accounting ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meet", [None, 1, 0], ids=["default_route", "prepass", "lanes"])
def test_child_buffer_accounting(case, meet):
    if meet is not None:
        pgq.set_option("meet", meet)
        pgq.set_option("meet_bias", 1e9)
    st = upload(case.V, case.s, case.d)
    rows = Rows(st, case.V, case.ps, case.pd, case.valid)
    want = expect(case.paths, case.valid, 3)
    need = need_of(want)
    want_len = np.array([-1 if p is None else hops(p) for p in want], dtype=np.int64)
    rc, used, ln, off, child = rows.bulk_raw(3, need)
    assert rc == 0 and used == need
    assert_lists(lists_of(ln, off, child), want, rows, "child_cap == need")
    rc, used, ln, off, child = rows.bulk_raw(3, need - 1)
    assert rc == -4 and used == need, (rc, used, need)
    assert (ln == want_len).all(), "the lengths are complete and correct when the lists did not fit"
    rc, used_unbounded = rows.bulk_raw(None, rows.roomy())[:2]
    assert rc == 0 and need < used_unbounded
    # the second emission: the pre-pass reserves 4 KB, finds its lists do not fit and writes them again at their exact size
    pgq.set_option("paths_reserve_mb", 0)
    assert_lists(rows.chunk(3), want, rows, "paths_reserve_mb 0")
    st.delete_csr(0)


# ---- 8: off the record --------------------------------------------------------------------------------------------------------
def test_bounded_path_calls_leave_the_routing_state_alone():
    # As test_within_gpu.test_bounded_calls_leave_the_routing_state_alone: large grouped calls are timed per graph (two through
    # the source-centric kernel, then — route_try_factor = 0 — two through the lane batches).  A handle that has answered
    # bounded shortestpath calls first must route the same unbounded iterativelength calls exactly like a fresh one.
    import torch
    rng = np.random.default_rng(71)
    V, E = 20000, 400000
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    for k, v in (("meet", 1), ("ball", 1), ("ball_seg_kb", 16), ("calibration_cache", 0), ("route_timing", 1),
                 ("route_timing_rows", 16384), ("route_try_factor", 0.0)):
        pgq.set_option(k, v)
    ps = np.repeat(rng.choice(V, 70, replace=False), 1000).astype(np.int64)
    pd = rng.integers(0, V, len(ps)).astype(np.int64)
    ora = OracleCSR.from_edges(V, s, d)
    oln, ook = ora.lean_iterativelength(V, ps, pd, nthreads=8)
    dist = np.where(ook, oln, -1)
    want_len = np.where((dist >= 0) & (dist <= 3), dist, -1)
    need = int((2 * want_len[want_len >= 0] + 1).sum())
    some = np.arange(0, len(ps), 233)  # the lists of a sample of the rows, element for element
    some_want = expect(ora.lean_shortestpath(V, ps[some], pd[some]), np.ones(len(some), dtype=bool), 3)
    t_s, t_d = torch.from_numpy(ps).cuda(), torch.from_numpy(pd).cuda()

    def routes(bounded_first):
        st = upload(V, s, d)
        dev = st.device_csr(0)
        t_o = torch.full((len(ps),), -7, dtype=torch.int64, device="cuda")
        t_off = torch.zeros(len(ps), dtype=torch.int64, device="cuda")
        t_child = torch.zeros(need + 8, dtype=torch.int64, device="cuda")
        for _ in range(bounded_first):
            rc, used = dev.shortestpath_within_bulk_ptr(len(ps), t_s.data_ptr(), t_d.data_ptr(), 3, t_o.data_ptr(), t_off.data_ptr(),
                                                        t_child.data_ptr(), need + 8)
            assert rc == 0 and used == need
            ln, off, child = t_o.cpu().numpy(), t_off.cpu().numpy(), t_child.cpu().numpy()
            assert (ln == want_len).all()
            assert [None if ln[i] < 0 else child[off[i]:off[i] + 2 * ln[i] + 1].tolist() for i in some] == some_want
        seen = []
        for _ in range(4):
            pgq.reset_stats()
            dev.iterativelength_bulk_ptr(len(ps), t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr())
            assert (t_o.cpu().numpy() == dist).all()
            stt = pgq.get_stats()
            seen.append((stt["ball_calls"] >= 1, stt["levels"] > 0))
        st.delete_csr(0)
        return seen

    fresh = routes(0)
    assert fresh[0] == fresh[1] == (True, False) and fresh[2] == fresh[3] == (False, True), fresh  # the premise: the timing is live
    assert routes(3) == fresh


# ---- 9: the multi form on one device ----------------------------------------------------------------------------------------
def test_multi_form_on_one_device(case):
    st = upload(case.V, case.s, case.d)
    rows = Rows(st, case.V, case.ps, case.pd, case.valid)
    single = {U: rows.bulk(U) for U in (3, UNBOUNDED)}
    for U in (3, UNBOUNDED):
        assert_lists(single[U], expect(case.paths, case.valid, U), rows, "bulk form, max_hops %d" % U)
    assert pgq.init_devices([0, 0]) == 2
    try:
        for U in (3, UNBOUNDED):
            ln, off, child = rows.dev.shortestpath_within_multi(rows.h_s, rows.pd, U)
            got = lists_of(ln, off, child)
            assert_lists(got, single[U], rows, "multi form, max_hops %d" % U)
            assert len(child) == need_of(single[U]), "the gathered payload holds the lists within the bound only"
        ln, off, child = rows.dev.shortestpath_multi(rows.h_s, rows.pd)
        assert lists_of(ln, off, child) == single[UNBOUNDED]
    finally:
        pgq.init_devices([0])
        st.delete_csr(0)


# ---- 10: argument checks -----------------------------------------------------------------------------------------------------
def test_argument_checks():
    import torch
    V, s, d, first, last = chain_graph()
    st = upload(V, s, d)
    dev = st.device_csr(0)
    with pytest.raises(pgq.PgqError, match="error -4.*max_hops"):
        dev.shortestpath_within(first, last, -1)
    with pytest.raises(pgq.PgqError, match="max_hops"):
        st.shortestpath_within(0, V, first, last, -1)
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    L = pgq.load_hip()
    rc, _ = dev.shortestpath_within_bulk_ptr(4, t.data_ptr(), t.data_ptr(), -1, t.data_ptr(), t.data_ptr(), t.data_ptr(), 64)
    assert rc == -4 and b"max_hops" in L.pgq_last_error()
    with pytest.raises(pgq.PgqError, match="error -4.*max_hops"):
        dev.shortestpath_within_multi(first, last, -1)
    # empty input
    empty = np.zeros(0, dtype=np.int64)
    assert dev.shortestpath_within(empty, empty, 3) == []
    assert st.shortestpath_within(0, V, empty, empty, 3) == []
    rc, used = dev.shortestpath_within_bulk_ptr(0, 0, 0, 3, 0, 0, 0, 0)
    assert rc == 0 and used == 0
    ln, off, child = dev.shortestpath_within_multi(empty, empty, 3)
    assert len(ln) == 0 and len(child) == 0
    # ids out of range, as for shortestpath
    with pytest.raises(pgq.PgqError, match="out of range"):
        dev.shortestpath_within(np.array([0, V]), np.array([1, 1]), 3)
    # src == dst is [src] under every bound, 0 included
    assert dev.shortestpath_within(first, first, 0) == [[int(v)] for v in first]
    assert st.shortestpath_within(0, V, first, first, 0) == [[int(v)] for v in first]
    # a NULL handle: the texts of shortestpath's own checks
    vec = pgq.binding.make_vec(first, keep=[])
    o, l = np.zeros(len(first), dtype=np.uint64), np.zeros(len(first), dtype=np.uint64)
    ov = np.zeros(2, dtype=np.uint64)
    child, clen = C.c_void_p(), C.c_uint64()
    rc = L.pgq_shortestpath_within(None, V, len(first), vec, vec, 3, o.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p),
                                   ov.ctypes.data_as(C.c_void_p), C.byref(child), C.byref(clen))
    assert rc == -4 and b"Need to initialize CSR before doing shortest path" in L.pgq_last_error()
    used = C.c_int64(0)
    assert L.pgq_shortestpath_within_bulk_device(None, 0, None, None, 3, None, None, None, 0, C.byref(used)) == -4
    assert b"NULL csr" in L.pgq_last_error()
    assert L.pgq_shortestpath_within_multi(None, 0, None, None, 3, None, None, None, 0, C.byref(used)) == -4
    assert b"NULL csr" in L.pgq_last_error()
    st.delete_csr(0)
