"""iterativelength_within(src, dst, max_hops): iterativelength, except that a row farther apart than max_hops is NULL.

Expected value everywhere: the CPU oracle's lean_iterativelength distance d; the row's value is d when the row is valid and
0 <= d <= max_hops, else NULL (payload -1).  Checked through the chunk form (DeviceCSR.iterativelength_within), the bulk form
(iterativelength_within_bulk_ptr) and the scalar-function form (PgqState.iterativelength_within), by every route — the
source-centric kernel, the pair-centric chain with each k_bibfs map variant, the lane batches, the chunk-sized k_meet3w —
with every cap at its smallest (a capped row must stay open whatever the bound), and with conditions on the statistics that
only hold when the search really stops at the bound."""
import ctypes as C

import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from helpers import LDS_LIMITS, sparse_ids_graph
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

BOUNDS = (0, 1, 2, 3, 4, 5, 8)
UNBOUNDED = 2 ** 62

KEYS = ("meet", "meet_bias", "meet_cap", "meet_cap_small", "meet_cap_paths", "meet4", "meet4_cap", "meet4_test_cap",
        "meet4_lds_kb", "meet4_global_mb", "meet_layout", "meet_small_rows", "meet_wide_rows", "meet_wide_rows_always",
        "bibfs_rows", "bibfs_cap", "bibfs_queue", "bibfs_grid", "ball", "ball_head_mb", "ball_cap", "ball_test_cap",
        "ball_grid", "ball_bias", "ball_sort", "ball_seg_kb", "words", "lanes", "force_mode", "force_pull", "sparse_lds",
        "blocks_per_cu", "route_timing", "route_timing_rows", "route_try_factor", "route_memo", "calibration_cache",
        "spec_levels", "chunk_zero_copy")


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def clamp(dist, valid, U):
    """Expected payloads: the distance where the row is valid and 0 <= d <= U, else -1 (NULL)."""
    d = np.asarray(dist)
    return np.where((d >= 0) & (d <= U) & np.asarray(valid), d, -1).astype(np.int64)


def payload(out, ok):
    out, ok = np.asarray(out), np.asarray(ok)
    assert (out[~ok] == -1).all(), "a NULL row's payload is -1"
    return np.where(ok, out, -1).astype(np.int64)


def upload(V, s, d):
    st = pgq.PgqState()
    st.build_csr(0, V, s, d)
    return st


class Rows:
    """The three forms of one call on the same rows (valid: the rows' src validity)."""

    def __init__(self, st, V, ps, pd, valid=None):
        import torch
        self.st, self.V, self.ps, self.pd = st, V, np.asarray(ps, dtype=np.int64), np.asarray(pd, dtype=np.int64)
        self.valid = np.ones(len(self.ps), dtype=bool) if valid is None else valid
        self.dev = st.device_csr(0)
        self.t_s = torch.from_numpy(np.where(self.valid, self.ps, -1)).cuda()  # bulk form: src < 0 is a NULL row
        self.t_d = torch.from_numpy(self.pd).cuda()

    def chunk(self, U):
        return payload(*self.dev.iterativelength_within(self.ps, self.pd, U, src_valid=self.valid))

    def udf(self, U):
        return payload(*self.st.iterativelength_within(0, self.V, self.ps, self.pd, U, src_valid=self.valid))

    def bulk(self, U):
        import torch
        t_o = torch.full((len(self.ps),), -7, dtype=torch.int64, device="cuda")
        self.dev.iterativelength_within_bulk_ptr(len(self.ps), self.t_s.data_ptr(), self.t_d.data_ptr(), U, t_o.data_ptr())
        return t_o.cpu().numpy()

    def unbounded(self):
        return payload(*self.dev.iterativelength(self.ps, self.pd, src_valid=self.valid))


def check_forms(rows, dist, bounds, forms=("chunk", "bulk", "udf"), what=""):
    for U in bounds:
        want = clamp(dist, rows.valid, U)
        for form in forms:
            got = getattr(rows, form)(U)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, "%s %s form, max_hops %d: %d rows differ, first (src %d, dst %d): got %d, expected %d (distance %d)" % (
                what, form, U, len(bad), rows.ps[bad[0]], rows.pd[bad[0]], got[bad[0]], want[bad[0]], np.asarray(dist)[bad[0]])


class Case:
    """One graph, its oracle, and rows built like test_lds_limits_gpu.Case: random pairs, every chain pair both ways, ~1 %
    src == dst, ~3 % NULL src."""

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


@pytest.fixture(scope="module")
def case():
    c = Case(20000, seed=20000)
    d = c.dist
    # what the sweep relies on, on the oracle, before any GPU call
    assert (d == 4).any() and (d >= 5).sum() >= 100 and (d < 0).any()
    for U in BOUNDS:
        assert (d == U).any() and (d == U + 1).any(), U
    return c


# ---- 1: the parity sweep ------------------------------------------------------------------------------------------------
def test_parity_sweep_all_forms(case):
    st = upload(case.V, case.s, case.d)
    rows = Rows(st, case.V, case.ps, case.pd, case.valid)
    check_forms(rows, case.dist, BOUNDS + (UNBOUNDED,), what="sweep")
    unb = rows.unbounded()
    for form in ("chunk", "bulk", "udf"):
        assert (getattr(rows, form)(UNBOUNDED) == unb).all(), form
    assert (unb == clamp(case.dist, case.valid, UNBOUNDED)).all()
    st.delete_csr(0)


# ---- 2: the same sweep per route ------------------------------------------------------------------------------------------
def cross_product(case):
    rng = np.random.default_rng(5)
    srcs = np.concatenate([[case.hubs[0], case.chains[0][0], case.chains[1][3], 0, case.V - 1], case.act[rng.integers(0, len(case.act), 27)]])
    pool = np.concatenate([case.act] + case.chains)
    ps = np.repeat(np.sort(srcs), 256).astype(np.int64)
    pd = pool[rng.integers(0, len(pool), len(ps))].astype(np.int64)
    pd[::97] = ps[::97]
    return ps, pd


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted_by_source", "shuffled"])
def test_route_source_centric(case, shuffled):
    ps, pd = cross_product(case)
    if shuffled:
        perm = np.random.default_rng(6).permutation(len(ps))
        ps, pd = ps[perm], pd[perm]
    dist = case.distances(ps, pd)
    for U in (2, 3, 4):
        assert (dist == U).any() and (dist == U + 1).any(), U
    pgq.set_option("meet", 1)
    pgq.set_option("meet_bias", 1e9)
    pgq.set_option("ball", 2)
    st = upload(case.V, case.s, case.d)
    rows = Rows(st, case.V, ps, pd)
    pgq.reset_stats()
    check_forms(rows, dist, BOUNDS + (UNBOUNDED,), what="ball = 2")
    if not shuffled:
        assert pgq.get_stats()["ball_calls"] >= 1
    st.delete_csr(0)


@pytest.mark.parametrize("words", [1, 8])
def test_route_lane_batches(case, words):
    pgq.set_option("meet", 0)
    pgq.set_option("words", words)
    st = upload(case.V, case.s, case.d)
    rows = Rows(st, case.V, case.ps, case.pd, case.valid)
    pgq.reset_stats()
    check_forms(rows, case.dist, BOUNDS + (UNBOUNDED,), forms=("chunk", "bulk"), what="meet = 0, words = %d" % words)
    stats = pgq.get_stats()
    assert stats["levels"] > 0 and stats["meet_pairs"] == 0
    st.delete_csr(0)


@pytest.mark.parametrize("wide", [0, 1], ids=["default_options", "k_meet3w"])
def test_route_chunk_sized_call(case, wide):
    # 24 rows under the default options; meet_wide_rows_always = 1: the chunk-sized k_meet3w (several wavefronts per row) takes
    # them on a graph of any size, as it does by itself on one whose adjacency is past the caches
    pgq.set_option("meet_wide_rows_always", wide)
    pick = np.concatenate([np.flatnonzero(case.dist == k)[:3] for k in (-1, 0, 1, 2, 3, 4, 5, 9)])[:24]
    assert len(pick) == 24
    st = upload(case.V, case.s, case.d)
    rows = Rows(st, case.V, case.ps[pick], case.pd[pick], case.valid[pick])
    check_forms(rows, case.dist[pick], BOUNDS + (UNBOUNDED,), what="24 rows")
    st.delete_csr(0)


# ---- 3: capped rows are not closed by the bound ------------------------------------------------------------------------------
def test_capped_rows_stay_open(case):
    # every cap at the smallest value the library takes: every walk is cut, so no stage may conclude "farther than the bound"
    for k in ("meet_cap_small", "meet_cap", "meet4_test_cap", "ball_test_cap", "bibfs_cap", "bibfs_queue"):
        pgq.set_option(k, 1)
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
    for ball in (0, 2):
        pgq.set_option("ball", ball)
        order = np.argsort(ps, kind="stable") if ball else np.arange(len(ps))
        st = upload(case.V, case.s, case.d)
        rows = Rows(st, case.V, ps[order], pd[order])
        check_forms(rows, dist[order], (2, 3, 4), what="caps at their smallest, ball = %d" % ball)
        st.delete_csr(0)


# ---- 4: both k_bibfs map variants --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("above", [0, 1], ids=["at_limit", "limit_plus_1"])
def test_bibfs_map_variants(above):
    V = LDS_LIMITS["bibfs"] + above
    c = Case(V, seed=V % 100_003)
    pgq.set_option("meet", 1)
    pgq.set_option("meet_bias", 1e9)
    pgq.set_option("ball", 0)
    pgq.set_option("bibfs_rows", 4096)  # every open row of these calls
    dist = c.distances(c.chain_s, c.chain_d)
    for U in (5, 7):
        assert (dist == U).any() and (dist == U + 1).any() and (dist < 0).any()
    st = upload(V, c.s, c.d)
    rows = Rows(st, V, c.chain_s, c.chain_d)
    pgq.reset_stats()
    check_forms(rows, dist, (5, 7), what="k_bibfs at V = %d" % V)
    stats = pgq.get_stats()
    n, in_lds = stats["launches"]["bibfs"], stats["lds_map_launches"]["bibfs"]
    assert n >= 1 and in_lds == (0 if above else n), (V, n, in_lds)
    st.delete_csr(0)


# ---- 5: the search really stops ---------------------------------------------------------------------------------------------
CHAINS, CHAIN_V = 16, 200


def chain_graph():
    ids = np.arange(CHAINS * CHAIN_V, dtype=np.int64).reshape(CHAINS, CHAIN_V)
    return CHAINS * CHAIN_V, ids[:, :-1].ravel().copy(), ids[:, 1:].ravel().copy(), ids[:, 0].copy(), ids[:, -1].copy()


def chain_call(U):
    """The 16 (first, last) rows on a fresh handle; returns (payloads, statistics of the call)."""
    V, s, d, first, last = chain_graph()
    st = upload(V, s, d)
    dev = st.device_csr(0)
    pgq.reset_stats()
    got = payload(*(dev.iterativelength(first, last) if U is None else dev.iterativelength_within(first, last, U)))
    stats = pgq.get_stats()
    st.delete_csr(0)
    return got, stats


def test_stops_reading_edges_at_the_bound():
    far, s_far = chain_call(None)
    assert (far == CHAIN_V - 1).all()
    assert s_far["edges_scanned"] >= CHAINS * (CHAIN_V - 1)  # a path of 199 edges cannot be found without reading each once
    near, s_near = chain_call(6)
    assert (near == -1).all()
    print("edges_scanned: unbounded %d, max_hops 6: %d" % (s_far["edges_scanned"], s_near["edges_scanned"]))
    assert s_near["edges_scanned"] * 2 <= s_far["edges_scanned"], (s_near["edges_scanned"], s_far["edges_scanned"])


def test_lane_batches_launch_no_level_past_the_bound():
    pgq.set_option("meet", 0)
    far, s_far = chain_call(None)
    assert (far == CHAIN_V - 1).all()
    assert s_far["batches"] >= 1 and s_far["levels"] > 6 * s_far["batches"], (s_far["levels"], s_far["batches"])
    near, s_near = chain_call(6)
    assert (near == -1).all()
    assert s_near["batches"] >= 1 and s_near["levels"] <= 6 * s_near["batches"], (s_near["levels"], s_near["batches"])


def test_bounded_calls_leave_the_routing_state_alone():
    # There is no accessor for the route memo / route timing / calibration figures, so this compares behaviour: large grouped
    # calls are timed per graph (two through the source-centric kernel, then — route_try_factor = 0 — two through the lane
    # batches).  A handle that has answered bounded calls first must route the same unbounded calls exactly like a fresh one.
    import torch
    rng = np.random.default_rng(71)
    V, E = 20000, 400000
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    for k, v in (("meet", 1), ("ball", 1), ("ball_seg_kb", 16), ("calibration_cache", 0), ("route_timing", 1),
                 ("route_timing_rows", 16384), ("route_try_factor", 0.0)):
        pgq.set_option(k, v)
    ps = np.repeat(rng.choice(V, 70, replace=False), 1000).astype(np.int64)
    pd = rng.integers(0, V, len(ps)).astype(np.int64)
    oln, ook = OracleCSR.from_edges(V, s, d).lean_iterativelength(V, ps, pd, nthreads=8)
    dist = np.where(ook, oln, -1)
    t_s, t_d = torch.from_numpy(ps).cuda(), torch.from_numpy(pd).cuda()

    def routes(bounded_first):
        st = upload(V, s, d)
        dev = st.device_csr(0)
        t_o = torch.full((len(ps),), -7, dtype=torch.int64, device="cuda")
        for _ in range(bounded_first):
            dev.iterativelength_within_bulk_ptr(len(ps), t_s.data_ptr(), t_d.data_ptr(), 3, t_o.data_ptr())
            assert (t_o.cpu().numpy() == clamp(dist, True, 3)).all()
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


# ---- 6: argument checks -------------------------------------------------------------------------------------------------------
def test_argument_checks():
    V, s, d, first, last = chain_graph()
    st = upload(V, s, d)
    dev = st.device_csr(0)
    with pytest.raises(pgq.PgqError, match="error -4.*max_hops"):
        dev.iterativelength_within(first, last, -1)
    with pytest.raises(pgq.PgqError, match="max_hops"):
        st.iterativelength_within(0, V, first, last, -1)
    import torch
    t = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(pgq.PgqError, match="error -4.*max_hops"):
        dev.iterativelength_within_bulk_ptr(4, t.data_ptr(), t.data_ptr(), -1, t.data_ptr())
    empty = np.zeros(0, dtype=np.int64)
    out, ok = dev.iterativelength_within(empty, empty, 3)
    assert len(out) == 0 and len(ok) == 0
    dev.iterativelength_within_bulk_ptr(0, 0, 0, 3, 0)
    out, ok = st.iterativelength_within(0, V, empty, empty, 3)
    assert len(out) == 0
    # ids out of range, as for iterativelength
    with pytest.raises(pgq.PgqError, match="out of range"):
        dev.iterativelength_within(np.array([0, V]), np.array([1, 1]), 3)
    # src == dst is 0 under every bound, 0 included
    out, ok = dev.iterativelength_within(first, first, 0)
    assert ok.all() and (out == 0).all()
    # a NULL handle: the text of iterativelength's own check
    L = pgq.load_hip()
    vec = pgq.binding.make_vec(first, keep=[])
    o = np.zeros(len(first), dtype=np.int64)
    ov = np.zeros(2, dtype=np.uint64)
    rc = L.pgq_iterativelength_within(None, V, len(first), vec, vec, 3, o.ctypes.data_as(C.c_void_p), ov.ctypes.data_as(C.c_void_p))
    assert rc == -4 and b"Need to initialize CSR before doing shortest path" in L.pgq_last_error()
    assert L.pgq_iterativelength_within_bulk_device(None, 0, None, None, 3, None) == -4 and b"NULL csr" in L.pgq_last_error()
    st.delete_csr(0)
