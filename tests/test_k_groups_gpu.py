"""k_shortest_groups (SHORTEST k GROUP) on the GPU, in every entry form (bulk, chunk, UDF), against the Python model
(k_groups_model.groups_model — checked on the CPU against a brute-force enumeration of walks filtered by the mode and grouped by
length; the fixtures used here catch its mutants there).  Every comparison is exact: lists, npaths, ngroups, counts, hops, offsets,
payload sizes, the rounds and, under a mode, the steps the search took."""
import numpy as np
import pytest

import all_shortest_model as A
import duckpgq_extension_amd as pgq
import k_groups_model as G
import k_walks_model as W
import path_modes_model as M
from duckpgq_extension_amd.binding import PgqError

pytestmark = pytest.mark.gpu

ALL = G.P_ALL
FIXTURES = G.gpu_fixtures()
_want, _state = {}, {}


def want_of(name, lo, K, g, P, mode):
    """The model's answer, computed once and left unchanged."""
    key = (name, lo, K, g, P, mode)
    if key not in _want:
        _want[key] = G.groups_model(*FIXTURES[name][0], lo, K, g, P, mode, state=_state.setdefault(name, {}))
    return _want[key]


def device(fx):
    V, off, adj, eid = fx[:4]
    return pgq.DeviceCSR(V, off, adj, eid)


def udf_state(fx):
    V, off, adj, eid = fx[:4]
    st = pgq.PgqState()
    st.build_csr(0, V, A.slot_sources(V, off), adj, eid)
    return st


def bulk_raw(dev, rs, rd, lo, K, g, P, mode, path_cap, child_cap):
    """(rc, walks needed, elements needed, hops, counts, first, npaths, ngroups, walk offsets, walk hops, child) of the bulk form."""
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    row = [torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda") for _ in range(5)]
    t_po = torch.full((max(path_cap, 1),), -7, dtype=torch.int64, device="cuda")
    t_ph = torch.full((max(path_cap, 1),), -7, dtype=torch.int64, device="cuda")
    t_ch = torch.full((max(child_cap, 1),), -7, dtype=torch.int64, device="cuda")
    rc, paths, used = dev.k_shortest_groups_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, K, g, P, mode, row[0].data_ptr(), row[1].data_ptr(),
                                                     row[2].data_ptr(), row[3].data_ptr(), row[4].data_ptr(), t_po.data_ptr(), t_ph.data_ptr(), path_cap,
                                                     t_ch.data_ptr(), child_cap)
    return (rc, paths, used) + tuple(t.cpu().numpy()[:n] for t in row) + (t_po.cpu().numpy(), t_ph.cpu().numpy(), t_ch.cpu().numpy())


def needs(lists):
    return sum(len(ps) for ps in lists if ps is not None), sum(len(q) for ps in lists if ps is not None for q in ps)


def expected_steps(want, mode):
    return (0, 0) if mode in (G.NONE, G.WALK) else (sum(want["steps1"]) + sum(want["steps2"]), max(want["steps1"]))


def bulk(dev, rs, rd, lo, K, g, P, mode, want):
    """The bulk form's lists from buffers of exactly the size the expected lists need; every per-row array, the layout, the rounds and
    the steps."""
    lists = want["lists"]
    Pn, C = needs(lists)
    pgq.binding.reset_stats()
    rc, paths, used, ln, cnt, first, npaths, ngroups, po, ph, ch = bulk_raw(dev, rs, rd, lo, K, g, P, mode, Pn, C)
    assert rc == 0 and (paths, used) == (Pn, C), (rc, paths, used, Pn, C)
    assert ln.tolist() == want["len"] and cnt.tolist() == want["count"], (ln.tolist(), want["len"], cnt.tolist(), want["count"])
    assert npaths.tolist() == want["npaths"] and ngroups.tolist() == want["ngroups"], (ngroups.tolist(), want["ngroups"])
    assert first.tolist() == (np.cumsum(npaths) - npaths).tolist()  # packed in row order ...
    assert ph[:Pn].tolist() == [len(q) // 2 for ps in lists if ps is not None for q in ps]
    width = 2 * ph[:Pn] + 1
    assert po[:Pn].tolist() == (np.cumsum(width) - width).tolist()  # ... and so are the walks' elements
    assert pgq.get_stats()["levels"] == want["rounds"], (pgq.get_stats()["levels"], want["rounds"])
    assert pgq.mode_steps() == expected_steps(want, mode), (pgq.mode_steps(), expected_steps(want, mode))
    return [None if ps is None else [ch[po[j]:po[j] + 2 * ph[j] + 1].tolist() for j in range(first[i], first[i] + npaths[i])]
            for i, ps in enumerate(lists)]


def same(got, want, rs, rd, what):
    bad = [i for i in range(len(rs)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d rows differ, first: %d -> %d got %r, expected %r" % (
        what, len(bad), len(rs), rs[bad[0]], rd[bad[0]], got[bad[0]], want[bad[0]])


def check_all_forms(name, dev=None, st=None, runs=None):
    fx, fx_runs = FIXTURES[name]
    V, off, adj, eid, rs, rd = fx
    own = dev is None
    dev = dev or device(fx)
    st = st or udf_state(fx)
    try:
        for lo, K, gs, Ps, modes in runs or fx_runs:
            for mode in modes:
                for g in gs:
                    for P in Ps:
                        want = want_of(name, lo, K, g, P, mode)
                        what = "%s, {%d,%d}, groups = %d, max_paths = %d, %s" % (name, lo, K, g, P, G.MODE_NAMES[mode])
                        same(bulk(dev, rs, rd, lo, K, g, P, mode, want), want["lists"], rs, rd, what + ", bulk form")
                        for form, (lists, ngroups) in (("chunk", dev.k_shortest_groups(rs, rd, lo, K, g, P, mode)),
                                                       ("udf", st.k_shortest_groups(0, V, rs, rd, lo, K, g, P, mode))):
                            same(lists, want["lists"], rs, rd, what + ", %s form" % form)
                            assert ngroups.tolist() == want["ngroups"], (what, form)
                            assert pgq.mode_steps() == expected_steps(want, mode), (what, form)
    finally:
        if own:
            dev.close()


# ---- 1. the random multigraph: every (src, dst); the model's expectation is the grouped enumeration itself -----------------------------------
def test_random_multigraph_against_the_grouped_enumeration():
    check_all_forms("tiny0")
    fx = FIXTURES["tiny0"][0]
    brute = {}
    for mode in G.ALL_MODES:
        want = want_of("tiny0", 0, 3, 2, 3, mode)
        enum = G.brute_groups(*fx, 0, 3, 2, 3, mode, brute=brute)
        assert all(want[k] == enum[k] for k in enum)


# ---- 2. in-lists of 63 .. 129 entries: the second group's only parent in the last slot and at the head of the second trip ---------------------
@pytest.mark.parametrize("deg", [63, 64, 65, 128, 129])
def test_in_list_lengths_and_the_second_group(deg):
    name = "in_list_%d" % deg
    check_all_forms(name)
    want = want_of(name, 0, 3, 2, ALL, G.WALK)
    assert want["npaths"] == [2, 2, 0] and want["ngroups"] == [2, 2, 0] and want["count"] == [2, 2, 0]
    assert [len(p) // 2 for p in want["lists"][0]] == [2, 3]


# ---- 3. batch boundaries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_batch_boundaries(n):
    check_all_forms("sources_%d" % n)
    check_all_forms("gap", runs=((0, 5, (2,), (ALL,), (G.WALK, G.ACYCLIC)),))  # a smaller graph on the same thread afterwards


# ---- 4. which lengths are groups ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bipartite", "ring5", "self_loop", "detour"])
def test_empty_lengths_rings_loops_and_lo_above_the_distance(name):
    check_all_forms(name)


def test_what_the_lengths_are():
    assert [len(p) // 2 for p in want_of("bipartite", 0, 6, 3, ALL, G.WALK)["lists"][0]] == [2, 2, 4, 4, 6, 6]  # d, d + 2, d + 4
    assert [len(p) // 2 for p in want_of("ring5", 0, 12, 3, ALL, G.WALK)["lists"][1]] == [2, 7, 12]  # d, d + n, d + 2 n
    assert want_of("self_loop", 0, 4, G.G_ALL, ALL, G.WALK)["ngroups"][0] == 5  # every length
    assert want_of("ring5", 0, 12, 2, ALL, G.ACYCLIC)["lists"][0] == [[0]]  # src == dst, lo = 0: the empty walk, under ACYCLIC the only group
    assert [len(p) // 2 for p in want_of("ring5", 0, 12, 2, ALL, G.SIMPLE)["lists"][0]] == [0, 5]  # ... SIMPLE admits the ring
    assert [len(p) // 2 for p in want_of("ring5", 1, 12, 2, ALL, G.WALK)["lists"][0]] == [5, 10]  # lo = 1
    assert [len(p) // 2 for p in want_of("bipartite", 3, 7, 2, ALL, G.NONE)["lists"][0]] == [4, 4, 6, 6]  # lo above the distance


# ---- 5. groups and max_paths around |A| and around a group boundary ----------------------------------------------------------------------------------
def test_max_paths_around_the_answer_and_around_a_group_boundary():
    check_all_forms("boundary")
    rows = lambda lo, K, g, P: tuple(want_of("boundary", lo, K, g, P, G.WALK)[k][0] for k in ("npaths", "ngroups", "count"))  # noqa: E731
    assert [rows(0, 5, 2, P) for P in (5, 6, 7)] == [(5, 2, 6), (6, 2, 6), (6, 2, 6)]  # |A| = 6
    assert [rows(0, 5, 2, P) for P in (2, 3, 4)] == [(2, 1, 3), (3, 1, 4), (4, 2, 5)]  # the boundary at 3, a later length inside K
    assert [rows(2, 2, 2, P) for P in (2, 3, 4)] == [(2, 1, 3), (3, 1, 3), (3, 1, 3)]  # ... and none
    assert [rows(0, 5, g, ALL)[1] for g in (1, 2, 3)] == [1, 2, 3]
    assert [want_of("boundary", 0, 5, g, 7, G.TRAIL)["ngroups"][0] for g in (1, 2, 3)] == [1, 2, 2]  # groups below, at and above the row's lengths


# ---- 6. the path modes -------------------------------------------------------------------------------------------------------------------------
def test_a_refused_length_between_two_admitted_ones():
    check_all_forms("gap")
    assert [[len(p) // 2 for p in want_of("gap", 0, 5, 3, ALL, m)["lists"][0]] for m in (G.WALK, G.TRAIL, G.SIMPLE, G.ACYCLIC)] == [
        [1, 2, 3], [1, 2, 4], [1, 4], [1, 4]]


def test_undirected_edges_share_an_id():
    check_all_forms("pair_and_triangle")


@pytest.mark.parametrize("P", [63, 64, 65, 129])
def test_a_run_of_parallel_slots_under_trail(P):
    name = "parallel_run_%d" % P
    check_all_forms(name)
    assert want_of(name, 3, 3, 1, P, G.TRAIL)["count"] == [0, P + 1, 0, 0] and want_of(name, 3, 3, 1, P, G.WALK)["count"][1] == P + 1


def test_a_chain_of_64_edges_with_a_chord_and_a_ring_of_64():
    check_all_forms("chain64")
    check_all_forms("ring64")
    assert [len(q) // 2 for q in want_of("chain64", 0, 64, 2, ALL, G.ACYCLIC)["lists"][0]] == [63, 64]
    assert want_of("ring64", 1, 64, 2, 3, G.ACYCLIC)["lists"][0] is None and len(want_of("ring64", 1, 64, 2, 3, G.SIMPLE)["lists"][0][0]) == 129


# ---- 7. the three identities -----------------------------------------------------------------------------------------------------------------------
def test_the_identities_hold_on_the_device():
    fx = FIXTURES["sources_65"][0]
    V, off, adj, eid, rs, rd = fx
    dev = device(fx)
    sp = dev.shortestpath(rs, rd)
    for lo, K, P in ((1, 3, 7), (0, 4, 2)):
        asp = dev.all_shortestpaths(rs, rd, K, P)
        hops = A.solve(*fx, K, P)[1]
        for mode in (G.NONE, G.WALK):  # 1. one group is ALL SHORTEST
            got = dev.k_shortest_groups(rs, rd, lo, K, 1, P, mode)[0]
            rows = [i for i in range(len(rs)) if rs[i] != rd[i] and hops[i] >= lo]
            assert len(rows) > 20 and all(got[i] == asp[i] for i in rows)
        for mode in G.ALL_MODES:  # 2. every group is SHORTEST k
            for g in (K - lo + 1, G.G_ALL):
                assert dev.k_shortest_groups(rs, rd, lo, K, g, P, mode)[0] == dev.k_shortest_walks(rs, rd, lo, K, P, path_mode=mode)
            got = dev.k_shortest_groups(rs, rd, lo, K, 2, 1, mode)[0]  # 3. one path is shortestpath's
            rows = [i for i in range(len(rs)) if rs[i] != rd[i] and hops[i] >= lo]
            assert all(got[i] == [sp[i]] for i in rows)
    dev.close()


# ---- 8. special rows ----------------------------------------------------------------------------------------------------------------------------
def test_null_rows_selections_and_empty_calls():
    fx = FIXTURES["sources_65"][0]
    V, off, adj, eid, rs, rd = fx
    rs, rd = rs[:60].copy(), rd[:60].copy()
    rd[::11] = rs[::11]  # closed rows among the others
    dev, st = device(fx), udf_state(fx)
    sv, dv = np.ones(len(rs), dtype=bool), np.ones(len(rs), dtype=bool)
    sv[3::7] = False
    dv[5::7] = False
    null = ~(sv & dv)
    sel = np.array([7, 7, 0, 59, 12, 3, 12], dtype=np.uint32)
    for mode in (G.WALK, G.SIMPLE):
        want = G.groups_model(V, off, adj, eid, rs, rd, 1, 3, 2, 3, mode)
        masked = [None if null[i] else ps for i, ps in enumerate(want["lists"])]
        for obj, args in ((dev, ()), (st, (0, V))):
            lists, ngroups = obj.k_shortest_groups(*args, rs, rd, 1, 3, 2, 3, mode, src_valid=sv, dst_valid=dv)
            assert lists == masked and ngroups.tolist() == [0 if null[i] else g for i, g in enumerate(want["ngroups"])]
            lists, ngroups = obj.k_shortest_groups(*args, rs, rd, 1, 3, 2, 3, mode, src_sel=sel, dst_sel=sel)
            assert lists == [want["lists"][i] for i in sel] and ngroups.tolist() == [want["ngroups"][i] for i in sel]
        (first, npaths, ov, po, pl, ch), _ = dev.k_shortest_groups(rs, rd, 1, 3, 2, 3, mode, src_valid=sv, dst_valid=dv, raw=True)
        for i, ps in enumerate(masked):
            if ps is None:  # NULL: no inner list, no payload
                assert first[i] == 0 and npaths[i] == 0 and not (int(ov[i >> 6]) >> (i & 63)) & 1
        assert (len(po), len(ch)) == needs(masked)
        brs = rs.copy()  # bulk form: a negative src is a NULL row with count -1
        brs[4::9] = -1
        bwant = G.groups_model(V, off, adj, eid, brs, rd, 1, 3, 2, 3, mode)
        assert -1 in bwant["count"] and bulk(dev, brs, rd, 1, 3, 2, 3, mode, bwant) == bwant["lists"]
        lists, ngroups = dev.k_shortest_groups([], [], 1, 3, 2, 3, mode)
        assert lists == [] and len(ngroups) == 0
    dev.close()


# ---- 9. the capacity protocol -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [G.WALK, G.ACYCLIC])
def test_capacity_protocol(mode):
    fx = FIXTURES["sources_65"][0]
    V, off, adj, eid, rs, rd = fx
    want = want_of("sources_65", 1, 3, 2, 2, mode)
    Pn, C = needs(want["lists"])
    dev = device(fx)
    for path_cap, child_cap in ((Pn - 1, C), (Pn, C - 1), (0, 0)):
        rc, paths, used, ln, cnt, first, npaths, ngroups, po, ph, ch = bulk_raw(dev, rs, rd, 1, 3, 2, 2, mode, path_cap, child_cap)
        assert rc == -4 and (paths, used) == (Pn, C), (path_cap, child_cap)
        assert ln.tolist() == want["len"] and cnt.tolist() == want["count"] and npaths.tolist() == want["npaths"] and ngroups.tolist() == want["ngroups"]
    assert "too small" in pgq.load_hip().pgq_last_error().decode()
    same(bulk(dev, rs, rd, 1, 3, 2, 2, mode, want), want["lists"], rs, rd, "exact size")
    dev.close()


# ---- 10. every error code -------------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    fx = W.chain8()
    V, off, adj, eid, rs, rd = fx
    dev, st = device(fx), udf_state(fx)
    err = lambda: pgq.load_hip().pgq_last_error().decode()  # noqa: E731
    untouched = lambda out: all((a == -7).all() for a in out[3:])  # noqa: E731
    for lo, K, g, P, mode in ((-1, 3, 1, 1, G.TRAIL), (3, 2, 1, 1, G.TRAIL), (1, 3, 0, 1, G.TRAIL), (1, 3, 1, 0, G.TRAIL), (1, 3, 1, 1, 5), (1, 3, 1, 1, -1),
                              (1, 3, 0, 1, G.WALK), (1, 3, 1, 0, G.WALK), (1, 3, -2, 4, G.NONE)):
        out = bulk_raw(dev, rs, rd, lo, K, g, P, mode, 10, 10)  # PGQ_ERR_INVALID_ARG
        assert out[0] == -4 and untouched(out), (lo, K, g, P, mode)
        with pytest.raises(PgqError):
            dev.k_shortest_groups(rs, rd, lo, K, g, P, mode)
        with pytest.raises(PgqError):
            st.k_shortest_groups(0, V, rs, rd, lo, K, g, P, mode)
    with pytest.raises(PgqError, match="groups must be at least 1"):
        dev.k_shortest_groups(rs, rd, 1, 3, 0, 1, G.TRAIL)
    with pytest.raises(PgqError, match="max_paths must be at least 1"):
        dev.k_shortest_groups(rs, rd, 1, 3, 1, 0, G.WALK)
    for K in (G.MAX_HOPS + 1, W.INT64_MAX):  # PGQ_ERR_UNSUPPORTED: walks need an upper bound
        for mode in (G.WALK, G.SIMPLE):
            out = bulk_raw(dev, rs, rd, 0, K, 1, 1, mode, 10, 10)
            assert out[0] == -6 and "upper bound" in err() and untouched(out)
            with pytest.raises(PgqError, match="upper bound"):
                dev.k_shortest_groups(rs, rd, 0, K, 1, 1, mode)
            with pytest.raises(PgqError, match="upper bound"):
                st.k_shortest_groups(0, V, rs, rd, 0, K, 1, 1, mode)
    # more than 2^31 - 1 emitted walks: 8192 rows of 8^6 = 2^18 walks each in one group; nothing is written
    many_s, many_d = np.zeros(8192, dtype=np.int64), np.full(8192, 6, dtype=np.int64)
    out = bulk_raw(dev, many_s, many_d, 0, 8, 1, ALL, G.WALK, 16, 16)
    assert out[0] == -6 and "2^31-1 walks" in err() and out[1:3] == (0, 0) and untouched(out)
    with pytest.raises(PgqError):
        dev.k_shortest_groups([0, V], [1, 1], 1, 3, 2, 2, G.TRAIL)  # an id outside the graph
    assert bulk_raw(dev, np.array([0, V]), np.array([1, 1]), 1, 3, 2, 2, G.WALK, 10, 10)[0] == -4
    # a saturated W is a group like any other: count is capped without overflow
    lists, ngroups = dev.k_shortest_groups(rs[:3], rd[:3], 0, G.MAX_HOPS, 2, 3, G.WALK)
    want = G.groups_model(V, off, adj, eid, rs[:3], rd[:3], 0, G.MAX_HOPS, 2, 3, G.WALK)
    assert lists == want["lists"] and want["count"] == [4, 4, 4]
    dev.close()


# ---- 11. the work limit ---------------------------------------------------------------------------------------------------------------------------
def test_step_cap():
    name, lo, K, g, P, mode = "parallel_run_65", 3, 3, 1, 65, G.TRAIL
    fx = FIXTURES[name][0]
    V, off, adj, eid, rs, rd = fx
    want = want_of(name, lo, K, g, P, mode)
    row_max = max(want["steps1"])
    assert row_max > 100 and pgq.get_default_option("mode_step_cap") == 1 << 24
    Pn, C = needs(want["lists"])
    dev = device(fx)
    dev.set_option("mode_step_cap", row_max - 1)  # this handle's option: the process-wide one stays
    out = bulk_raw(dev, rs, rd, lo, K, g, P, mode, Pn, C)
    msg = pgq.load_hip().pgq_last_error().decode()
    assert out[0] == -6 and "mode_step_cap = %d" % (row_max - 1) in msg and out[1:3] == (0, 0) and all((a == -7).all() for a in out[3:])
    with pytest.raises(PgqError, match="mode_step_cap"):
        dev.k_shortest_groups(rs, rd, lo, K, g, P, mode)
    dev.set_option("mode_step_cap", row_max)  # per row and pass: the counting pass is the longer one
    assert bulk(dev, rs, rd, lo, K, g, P, mode, want) == want["lists"]
    dev.close()


# ---- 12. the rounds ---------------------------------------------------------------------------------------------------------------------------------
def test_rounds_stop_by_groups():
    """A chain with 8 parallel edges per hop that ends at vertex 22: (0, 1) has 8 walks, all of one edge.  A row that is closed stops
    its batch at its distance; one that is open — also with cum == max_paths on the boundary — runs until the queue is empty."""
    fx = W.chain8()
    V, off, adj, eid, rs, rd = fx
    dev = device(fx)
    row = (np.array([0]), np.array([1]))
    for mode, g, P, closed in ((G.WALK, 1, 1, True), (G.WALK, 2, 7, True), (G.WALK, 2, 8, False), (G.NONE, 2, 9, False), (G.ACYCLIC, 1, 8, True),
                               (G.ACYCLIC, 2, 7, True), (G.ACYCLIC, 2, 8, False), (G.TRAIL, 2, 9, False), (G.SIMPLE, 1, 1, True)):
        want = G.groups_model(V, off, adj, eid, *row, 0, 30, g, P, mode)
        assert (want["rounds"] == 1) if closed else (22 <= want["rounds"] <= 23), (mode, g, P, want["rounds"])
        assert want["count"] == [min(8, P + 1)] and want["ngroups"] == [1]
        assert bulk(dev, *row, 0, 30, g, P, mode, want) == want["lists"]  # (compares the rounds)
    far = (np.array([0]), np.array([5]))
    want = G.groups_model(V, off, adj, eid, *far, 0, G.MAX_HOPS, 1, 100, G.WALK)
    assert want["rounds"] == 5 and want["count"] == [101] and bulk(dev, *far, 0, G.MAX_HOPS, 1, 100, G.WALK, want) == want["lists"]  # d rounds, not K
    want = G.groups_model(V, off, adj, eid, *far, 6, G.MAX_HOPS, 1, 100, G.WALK)  # lo above the only length: open to the chain's end
    assert want["rounds"] >= 22 and want["count"] == [0] and bulk(dev, *far, 6, G.MAX_HOPS, 1, 100, G.WALK, want) == want["lists"]
    dev.close()


# ---- 13. the neighbours on the shared workspace ------------------------------------------------------------------------------------------------------
def test_neighbours_unchanged_and_nothing_left_behind():
    V, off, adj, eid, rs, rd = FIXTURES["sources_65"][0]
    w = np.random.default_rng(3).integers(1, 9, len(adj))
    before_handle = pgq.live_device_blocks()
    dev = pgq.DeviceCSR(V, off, adj, eid, w)

    def neighbours():
        out = [dev.k_shortest_walks(rs, rd, 1, 3, 3), dev.all_shortestpaths(rs, rd, 3, 7), dev.shortestpath(rs, rd)]
        for mode in M.MODES:
            out.append(dev.k_shortest_walks(rs, rd, 1, 3, 2, path_mode=mode))
            out.append(pgq.mode_steps())
        return out

    first = neighbours()
    assert first[0] == W.solve(V, off, adj, eid, rs, rd, 1, 3, 3)[2] and first[1] == A.solve(V, off, adj, eid, rs, rd, 3, 7)[2]
    mwant = M.search_model(V, off, adj, eid, rs, rd, 1, 3, 2, M.SIMPLE)
    assert first[3] == mwant[2] and first[4] == (sum(mwant[3]) + sum(mwant[4]), max(mwant[3]))  # the existing search takes the steps it took
    for mode in (G.WALK, G.SIMPLE):
        want = want_of("sources_65", 1, 3, 2, 2, mode)
        Pn, C = needs(want["lists"])
        assert dev.k_shortest_groups(rs, rd, 1, 3, 2, 2, mode)[0] == want["lists"]
        assert neighbours() == first
        assert bulk_raw(dev, rs, rd, 1, 3, 2, 2, mode, Pn - 1, C - 1)[0] == -4  # a call that failed with a too-small buffer
        assert neighbours() == first
        assert bulk_raw(dev, rs, rd, 1, 3, 0, 2, mode, Pn, C)[0] == -4  # ... one that failed its checks
        if mode == G.SIMPLE:
            dev.set_option("mode_step_cap", 1)
            assert bulk_raw(dev, rs, rd, 1, 3, 2, 2, mode, Pn, C)[0] == -6  # ... and one that went over the step cap
            dev.set_option("mode_step_cap", 1 << 24)
        assert neighbours() == first
        assert bulk(dev, rs, rd, 1, 3, 2, 2, mode, want) == want["lists"]
    dev.close()
    assert pgq.live_device_blocks() == before_handle
