"""The search kernels with adjacency-list lengths ON their own constants and the only shortest path in a chosen slot.

helpers.degree_gadgets builds sources of out-degree a and destinations of in-degree b, a and b in 1, 2, 63 .. 65, 319 .. 321,
511 .. 513, 4095 .. 4097, exactly k = 1 .. 4 hops apart by one path whose vertex is the first, the last, the 64th / 65th or the
320th / 321st entry of the list; everything else in the lists is a decoy (test_degree_gadgets_cpu.py proves that on the CPU).
A kernel that loses the last lane of a register round, the ninth round, the descriptor at index 64 or 320 or the 4097th
neighbour answers such a row wrongly, where the random graphs of the other files have other witnesses.  Every expected value
is the CPU oracle's; every comparison is exact.  helpers.lcc_gadgets does the same for k_lcc / k_lcc_big at 512 / 513."""
import numpy as np
import pytest

import duckpgq_extension_amd as pgq
from helpers import LDS_LIMITS, ball_line_gadgets, csr_arrays_from_rows, degree_gadgets, lcc_gadgets, spread_ids
from oracle.pgq_oracle import OracleCSR
from test_within_gpu import Rows, clamp

pytestmark = pytest.mark.gpu

# every option these tests depend on: the library's defaults first (another file may have left its own values)
KEYS = ("meet", "meet_bias", "meet_cap", "meet_cap_small", "meet_cap_paths", "meet4", "meet4_cap", "meet4_test_cap",
        "meet4_lds_kb", "meet4_global_mb", "meet_layout", "meet_align", "meet_pack", "meet_pack_align", "meet_small_rows",
        "meet_wide_rows", "meet_wide_rows_always", "meet_spin_wait", "paths_reserve_mb", "bibfs_rows", "bibfs_rows_max", "bibfs_cap",
        "bibfs_queue", "bibfs_grid", "wbibfs", "ball", "ball_head_mb", "ball_cap", "ball_test_cap", "ball_grid", "ball_bias",
        "ball_sort", "ball_seg_kb", "ball_seg_rows_small", "words", "max_words", "lanes", "lanes_unroll", "force_mode",
        "force_pull", "sparse_lds", "blocks_per_cu", "hub_chunk", "push_chunk", "push_div", "probe", "probe2", "defer", "streams",
        "route_timing", "route_timing_rows", "route_try_factor", "route_memo", "calibration_cache", "meet_calibrate",
        "spec_levels", "chunk_zero_copy")


@pytest.fixture(autouse=True)
def _options():
    saved = {k: pgq.get_option(k) for k in KEYS}
    for k in KEYS:
        pgq.set_option(k, pgq.get_default_option(k))
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def prepass():
    for k, v in (("meet", 1), ("meet_bias", 1e9), ("ball", 0)):
        pgq.set_option(k, v)


class Side:
    """A gadget graph (or its transpose), its oracle and the oracle's answers for its rows."""

    def __init__(self, g):
        self.g = g
        self.ora = OracleCSR.from_edges(g.V, g.src, g.dst)
        ln, ok = self.ora.lean_iterativelength(g.V, g.rs, g.rd, nthreads=8)
        self.dist = np.where(ok, ln, -1)
        self._paths = None

    def paths(self):
        if self._paths is None:
            self.near = np.flatnonzero((self.dist >= 0) & (self.dist <= 4))
            self._paths = self.ora.lean_shortestpath(self.g.V, self.g.rs[self.near], self.g.rd[self.near])
        return self._paths

    def upload(self):
        st = pgq.PgqState()
        st.build_csr(0, self.g.V, self.g.src, self.g.dst)
        return st

    def check(self, out, ok, what, rows=slice(None)):
        got = np.where(ok, out, -1)
        want, tags = self.dist[rows], self.g.tag[rows]
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "%s: %d of %d rows differ, first: gadget %s got %d, expected %d" % (
            what, len(bad), len(want), tags[bad[0]], got[bad[0]], want[bad[0]])


@pytest.fixture(scope="module")
def sides():
    g = degree_gadgets()
    out = [Side(g), Side(g.transposed())]
    for s in out:  # the builder's own distances (test_degree_gadgets_cpu.py) — the expected values are the oracle's
        assert (s.dist == g.dist).all()
    return out


def orient(k):
    return "graph" if k == 0 else "transpose"


# ---- k_meet3 / k_meet3w, hop counts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack,pack_k", [(1, 6), (0, 4)])
def test_meet3_hop_counts(sides, pack, pack_k):
    prepass()
    pgq.set_option("meet_pack", pack)  # read at upload
    for k, side in enumerate(sides):
        g = side.g
        st = side.upload()
        assert st.device_csr(0).pack_k == pack_k
        for wide in (0, 1):
            pgq.set_option("meet_wide_rows_always", wide)
            pgq.reset_stats()
            ln, ok = st.iterativelength(0, g.V, g.rs, g.rd)
            side.check(ln, ok, "%s, meet_pack %d, wide %d" % (orient(k), pack, wide))
            assert pgq.get_stats()["meet_pairs"] > 0
        st.delete_csr(0)


# ---- K = 5 and the filter that folds high id bits --------------------------------------------------------------------------
@pytest.mark.parametrize("V,pack,pack_k", [((1 << 21) + 1, 2, 5), ((1 << 20) + 1, 1, 6)])
def test_meet3_hop_counts_top_of_the_id_range(sides, V, pack, pack_k):
    prepass()
    pgq.set_option("meet_pack", pack)
    for k, side in enumerate(sides):
        g = side.g.shifted(V)
        st = pgq.PgqState()
        st.build_csr(0, V, g.src, g.dst)
        assert st.device_csr(0).pack_k == pack_k
        for wide in (0, 1):
            pgq.set_option("meet_wide_rows_always", wide)
            ln, ok = st.iterativelength(0, V, g.rs, g.rd)
            side.check(ln, ok, "%s at the top of V = %d, wide %d" % (orient(k), V, wide))  # distances do not move with the ids
        st.delete_csr(0)


# ---- hand-over at 512 and 4096 -----------------------------------------------------------------------------------------------
def test_hand_over_to_meet4(sides):
    prepass()
    pgq.set_option("bibfs_rows", 0)
    cap = int(min(pgq.get_option("meet_cap"), pgq.get_option("meet_cap_small")))
    for k, side in enumerate(sides):
        g = side.g
        st = side.upload()
        over = g.main_rows(lambda x: {x["a"], x["b"]} in ({513}, {4097}, {513, 4097}) and x["a"] > 1 and x["b"] > 1 and not x["tie"])
        assert len(over) >= 4 * 6 * 2 + 4
        # k_meet4d's testing walk of a distance-4 row stops after meet4_test_cap entries (shipped: 2^15) and leaves the row to the
        # stages behind it: the lists of 4097 decoys hold about 47,000, the witness is in the last one.  Under the shipped
        # cap the answers must be right; with room for every list (8 entries of padding each) every row is the pre-pass's
        off, adj, _ = csr_arrays_from_rows(g.V, g.src, g.dst)
        deg = np.diff(off)
        room = max(int((deg[adj[off[x["src"]]:off[x["src"] + 1]]] + 8).sum()) for x in g.gadgets if x["a"] == 4097)
        assert room < 1 << 20
        for test_cap in (int(pgq.get_default_option("meet4_test_cap")), 1 << 20):
            pgq.set_option("meet4_test_cap", test_cap)
            pgq.reset_stats()
            ln, ok = st.iterativelength(0, g.V, g.rs[over], g.rd[over])
            side.check(ln, ok, "%s, both lists over the limit, meet4_test_cap %d" % (orient(k), test_cap), over)
            stats = pgq.get_stats()
            print("%s, meet4_test_cap %d: meet_pairs %d of %d rows" % (orient(k), test_cap, stats["meet_pairs"], len(over)))
            assert stats["launches"]["meet4"] >= 1
        assert stats["meet_pairs"] == len(over), "the pre-pass answers every such row (k_meet4d), not the lane batches"
        pgq.set_option("meet4_test_cap", pgq.get_default_option("meet4_test_cap"))
        # at the limit k_meet3 keeps the row: (512, 512) up to distance 3 (a distance-4 row is k_meet4d's anyway), and (4096, 1)
        # up to distance 2 (its distance-3 walk over 4096 lists runs into the walk cap)
        at = g.main_rows(lambda x: ((x["a"], x["b"]) == (512, 512) and x["k"] <= 3) or
                         ({x["a"], x["b"]} == {4096, 1} and x["k"] <= 2))
        assert len(at) >= 3 * 6 + 2
        for x in g.gadgets:  # the cap does not cut a (512, 512) walk: list lengths plus 8 entries of padding each
            if (x["a"], x["b"]) == (512, 512) and x["k"] <= 3:
                assert (deg[adj[off[x["src"]]:off[x["src"] + 1]]] + 8).sum() < cap, x["tag"]
        # the chain launches k_meet4d straight behind k_meet3 whether or not a row is open (it reads the count on the device), so
        # its launch count says nothing here: with the bit-map kernels switched off k_meet3 is the whole pre-pass, and every
        # row it answers it kept
        pgq.set_option("meet4", 0)
        pgq.reset_stats()
        ln, ok = st.iterativelength(0, g.V, g.rs[at], g.rd[at])
        side.check(ln, ok, "%s, lists at the limit" % orient(k), at)
        stats = pgq.get_stats()
        assert stats["launches"]["meet4"] == 0 and stats["meet_pairs"] == len(at), (stats["launches"], stats["meet_pairs"])
        pgq.set_option("meet4", pgq.get_default_option("meet4"))
        every = g.main_rows(lambda x: (x["a"], x["b"]) == (512, 512) or {x["a"], x["b"]} == {4096, 1})
        ln, ok = st.iterativelength(0, g.V, g.rs[every], g.rd[every])
        side.check(ln, ok, "%s, lists at the limit, every distance" % orient(k), every)
        st.delete_csr(0)


# ---- paths ---------------------------------------------------------------------------------------------------------------
def check_paths(side, got, what):
    want = side.paths()
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, "%s: %d of %d lists differ, first: gadget %s got %s, expected %s" % (
        what, len(bad), len(want), side.g.tag[side.near[bad[0]]], got[bad[0]], want[bad[0]])


def test_shortestpath_every_row_up_to_four_hops(sides):
    # ties included: the oracle's tie-break, with ids ordered against the slots; 0 MB: the smallest reservation (4 KB), the lists
    # are written a second time at their exact size
    for k, side in enumerate(sides):
        g = side.g
        side.paths()
        ps, pd = g.rs[side.near], g.rd[side.near]
        assert len(ps) > 1000 and any(t.startswith("tie3_k4") for t in g.tag[side.near])
        st = side.upload()
        prepass()
        for mb in (int(pgq.get_default_option("paths_reserve_mb")), 0):
            pgq.set_option("paths_reserve_mb", mb)
            pgq.reset_stats()
            check_paths(side, st.shortestpath(0, g.V, ps, pd), "%s, pre-pass, paths_reserve_mb %d" % (orient(k), mb))
            stats = pgq.get_stats()
            assert stats["meet_pairs"] > 0 and stats["launches"]["meet"] >= 1 and stats["launches"]["meet4"] >= 1
        pgq.set_option("meet", 0)
        for words in (1, 8):
            pgq.set_option("words", words)
            check_paths(side, st.shortestpath(0, g.V, ps, pd), "%s, lane batches, words %d" % (orient(k), words))
        st.delete_csr(0)


# ---- source-centric: k_ball_segments + k_src_ball ---------------------------------------------------------------------------
def ball_rows(side, rng):
    """Rows grouped by source: nine runs of 1023 / 1024 / 1025 rows of one source of out-degree 4095 / 4096 / 4097 holding 15 / 16
    / 17 rows at distance >= 4 or unreachable, short runs of other sources between them."""
    g = side.g
    off, adj, _ = csr_arrays_from_rows(g.V, g.src, g.dst)
    big = [x for x in g.gadgets if x["k"] == 4 and x["a"] == x["b"] and x["a"] in (4095, 4096, 4097)]
    big.sort(key=lambda x: str(x["pos"]))  # by position, then 4095, 4096, 4097 in turn
    small = [x for x in g.gadgets if x["k"] == 3 and x["a"] in (63, 64, 65)]
    others = np.array([x["dst"] for x in g.gadgets if x["k"] >= 2], dtype=np.int64)
    ps, pd, runs = [], [], []
    for i, (r, f) in enumerate((r, f) for r in (1023, 1024, 1025) for f in (15, 16, 17)):
        x = big[i]
        one = adj[off[x["src"]]:off[x["src"] + 1]]
        two = np.concatenate([adj[off[v]:off[v + 1]] for v in one[:64]])  # their sinks
        near = np.concatenate([one[-400:], one[:r - f - 400 - 200], two[:200]])
        far = np.concatenate([[x["dst"]], rng.choice(others[others != x["dst"]], f - 1, replace=False)])  # distance 4, unreachable
        d = np.concatenate([near, far])
        assert len(d) == r
        d = d[rng.permutation(r)]
        ps.append(np.full(r, x["src"], dtype=np.int64)), pd.append(d), runs.append((r, f, x["a"]))
        y = small[i]
        ps.append(np.full(5, y["src"], dtype=np.int64)), pd.append(np.array([y["dst"], y["paths"][0][1], y["paths"][0][2], y["src"], x["dst"]]))
        runs.append((5, None, y["a"]))
    ps, pd = np.concatenate(ps), np.concatenate(pd).astype(np.int64)
    ln, ok = side.ora.lean_iterativelength(g.V, ps, pd, nthreads=8)
    dist = np.where(ok, ln, -1)
    at = 0
    for r, f, _ in runs:  # the runs are what they are meant to be, on the oracle's distances
        far = (dist[at:at + r] < 0) | (dist[at:at + r] >= 4)
        assert f is None or far.sum() == f, (r, f, int(far.sum()))
        at += r
    assert {a for r, f, a in runs if f} == {4095, 4096, 4097}
    assert {(r, f) for r, f, a in runs if f} == {(r, f) for r in (1023, 1024, 1025) for f in (15, 16, 17)}
    return ps, pd, dist


def test_source_centric_runs(sides):
    pgq.set_option("meet", 1)
    pgq.set_option("meet_bias", 1e9)
    pgq.set_option("ball", 2)
    for k, side in enumerate(sides):
        g = side.g
        ps, pd, dist = ball_rows(side, np.random.default_rng(5 + k))
        for head_mb in (512, 0):
            pgq.set_option("ball_head_mb", head_mb)  # read at upload and launch
            st = side.upload()
            pgq.reset_stats()
            ln, ok = st.iterativelength(0, g.V, ps, pd)
            got = np.where(ok, ln, -1)
            bad = np.flatnonzero(got != dist)
            assert len(bad) == 0, "%s, ball_head_mb %d: %d rows differ, first: row %d (src %d, dst %d) got %d, expected %d" % (
                orient(k), head_mb, len(bad), bad[0], ps[bad[0]], pd[bad[0]], got[bad[0]], dist[bad[0]])
            stats = pgq.get_stats()
            assert stats["ball_calls"] >= 1 and stats["launches"]["ball"] >= 1
            # the gadget rows themselves, each source's rows side by side
            pgq.reset_stats()
            ln, ok = st.iterativelength(0, g.V, g.rs, g.rd)
            side.check(ln, ok, "%s, ball = 2, ball_head_mb %d" % (orient(k), head_mb))
            assert pgq.get_stats()["ball_calls"] >= 1
            st.delete_csr(0)


# ---- source-centric: the fixed-stride heads at their line boundary (helpers.ball_line_gadgets) --------------------------------
def test_source_centric_head_lines():
    # rhead: word 31 is the in-degree, entries 31 .. 62 sit one word further on, entry 63 and on come from rpadj.  The only witness
    # of a row is in-list entry 0, 30, 31, 61, 62 or 63 of a destination of in-degree 1, 30 .. 33, 62 .. 64; the count rows have
    # the vertex whose id IS the in-degree in the source's two-hop set.  Under max_hops = 3 a row whose scan shows no witness is
    # NULL in k_src_ball itself: a lost entry is a wrong answer there, no kernel behind repairs it
    g0 = ball_line_gadgets()
    pgq.set_option("meet", 1)
    pgq.set_option("meet_bias", 1e9)
    pgq.set_option("ball", 2)
    for k, g in enumerate((g0, g0.transposed())):
        side = Side(g)
        assert (side.dist == g.dist).all()
        by_src = np.argsort(g.rs, kind="stable")  # each source's rows side by side
        ps, pd, dist, tags = g.rs[by_src], g.rd[by_src], side.dist[by_src], g.tag[by_src]
        for head_mb in (512, 0):
            pgq.set_option("ball_head_mb", head_mb)  # read at upload and launch
            st = side.upload()
            lay = st.device_csr(0).meet_layout_sizes()
            assert lay["has_rhead"] == (1 if head_mb else 0)
            for U in (None, 2, 3, 4):
                pgq.reset_stats()
                if U is None:
                    ln, ok = st.iterativelength(0, g.V, ps, pd)
                    want = dist
                else:
                    ln, ok = st.iterativelength_within(0, g.V, ps, pd, U)
                    want = clamp(dist, np.ones(len(ps), dtype=bool), U)
                got = np.where(ok, ln, -1)
                bad = np.flatnonzero(got != want)
                assert len(bad) == 0, "%s, ball_head_mb %d, max_hops %s: %d of %d rows differ, first: %s got %d, expected %d" % (
                    orient(k), head_mb, U, len(bad), len(ps), tags[bad[0]], got[bad[0]], want[bad[0]])
                stats = pgq.get_stats()
                assert stats["ball_calls"] >= 1 and stats["launches"]["ball"] >= 1, (orient(k), head_mb, U)
            st.delete_csr(0)


# ---- lane batches ------------------------------------------------------------------------------------------------------------
def test_lane_batches(sides):
    pgq.set_option("meet", 0)
    pgq.set_option("hub_chunk", 64)  # read at upload: a list of 4097 entries is 65 slices
    pgq.set_option("push_chunk", 64)
    for k, side in enumerate(sides):
        g = side.g
        st = side.upload()
        for words in (1, 32):
            for mode in (0, 1, 2):  # adaptive, always top-down, always bottom-up
                pgq.set_option("words", words)
                pgq.set_option("force_mode", mode)
                pgq.reset_stats()
                ln, ok = st.iterativelength(0, g.V, g.rs, g.rd)
                side.check(ln, ok, "%s, lane batches, words %d, force_mode %d" % (orient(k), words, mode))
                stats = pgq.get_stats()
                assert stats["levels"] > 0 and stats["meet_pairs"] == 0
        st.delete_csr(0)


# ---- bounds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ball", [None, 2], ids=["default_options", "ball_2"])
def test_bounds(sides, ball):
    if ball is not None:
        for k, v in (("meet", 1), ("meet_bias", 1e9), ("ball", ball)):
            pgq.set_option(k, v)
    for k, side in enumerate(sides):
        g = side.g
        st = side.upload()
        rows = Rows(st, g.V, g.rs, g.rd)
        for U in (1, 2, 3, 4):
            want = clamp(side.dist, rows.valid, U)
            for form in ("chunk", "bulk"):
                bad = np.flatnonzero(getattr(rows, form)(U) != want)
                assert len(bad) == 0, "%s, ball %s, %s form, max_hops %d: %d rows differ, first: gadget %s (distance %d)" % (
                    orient(k), ball, form, U, len(bad), g.tag[bad[0]], side.dist[bad[0]])
        st.delete_csr(0)


# ---- local clustering coefficient: k_lcc / k_lcc_big at 512 / 513, both map placements -------------------------------------
def run_lcc(V, ids):
    n, s, d, hubs, deg = lcc_gadgets()
    s, d = ids[s], ids[d]
    rows = np.concatenate([ids[hubs], ids[:40], ids[-40:], ids[hubs[::-1]]])  # leaves of degree 0 and 1 among them
    want = OracleCSR.from_edges(V, s, d).local_clustering_coefficient(rows)
    assert (want > 0).sum() == 2 * len(hubs)
    st = pgq.PgqState()
    st.build_csr(0, V, s, d)
    out, ok = st.local_clustering_coefficient(0, rows)
    st.delete_csr(0)
    assert ok.all()
    bad = np.flatnonzero(out.view(np.uint32) != want.view(np.uint32))
    label = np.concatenate([deg, np.zeros(80, dtype=np.int64), deg[::-1]])  # 0: a leaf
    assert len(bad) == 0, "V = %d: %d rows differ, first: row %d (out-degree %d) got %r, expected %r" % (
        V, len(bad), bad[0], label[bad[0]], out[bad[0]], want[bad[0]])


def test_lcc_at_512_and_513():
    n = lcc_gadgets()[0]
    run_lcc(n, np.arange(n, dtype=np.int64))


@pytest.mark.parametrize("above", [0, 1], ids=["lds_map", "global_slices"])
def test_lcc_big_map_placement(above):
    # V = the limit: the map of k_lcc_big in LDS; one vertex more: a slice of global memory per workgroup.  Results only: no
    # kernel class counts k_lcc_big's launches (helpers.LDS_LIMITS["lcc_big"], recomputed in test_lds_budget_cpu.py)
    V = LDS_LIMITS["lcc_big"] + above
    run_lcc(V, spread_ids(np.random.default_rng(V % 1000), lcc_gadgets()[0], V))
