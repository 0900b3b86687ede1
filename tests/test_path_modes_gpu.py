"""k_shortest_walks_mode and walk_count_mode on the GPU, in every entry form (bulk, chunk, UDF), against the Python model of the
kernel's search (path_modes_model.search_model — checked on the CPU against a brute-force enumeration of walks filtered by the mode;
the fixtures used here catch its mutants there).  Every comparison is exact: counts, hops, whole lists, offsets, payload sizes and
the steps the search took."""
import numpy as np
import pytest

import all_shortest_model as A
import duckpgq_extension_amd as pgq
import k_walks_model as W
import path_modes_model as M
from duckpgq_extension_amd.binding import PgqError

pytestmark = pytest.mark.gpu

ALL = M.K_ALL
FIXTURES = M.gpu_fixtures()
_want, _state = {}, {}


def want_of(name, lo, K, k, mode):
    """(counts, hops, lists, counting steps, emitting steps, rounds) of the model, computed once and left unchanged."""
    if (name, lo, K, k, mode) not in _want:
        _want[name, lo, K, k, mode] = M.search_model(*FIXTURES[name][0], lo, K, k, mode, state=_state.setdefault(name, {}))
    return _want[name, lo, K, k, mode]


def device(fx):
    V, off, adj, eid = fx[:4]
    return pgq.DeviceCSR(V, off, adj, eid)


def udf_state(fx):
    V, off, adj, eid = fx[:4]
    st = pgq.PgqState()
    st.build_csr(0, V, A.slot_sources(V, off), adj, eid)
    return st


def bulk_count(dev, rs, rd, lo, K, limit, mode):
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    t_c = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    dev.walk_count_mode_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, K, limit, mode, t_c.data_ptr())
    return t_c.cpu().numpy()[:n].tolist()


def bulk_raw(dev, rs, rd, lo, K, k, mode, path_cap, child_cap):
    """(rc, walks needed, elements needed, hops, counts, first, npaths, walk offsets, walk hops, child) of the bulk form."""
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    row = [torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda") for _ in range(4)]
    t_po = torch.full((max(path_cap, 1),), -7, dtype=torch.int64, device="cuda")
    t_ph = torch.full((max(path_cap, 1),), -7, dtype=torch.int64, device="cuda")
    t_ch = torch.full((max(child_cap, 1),), -7, dtype=torch.int64, device="cuda")
    rc, paths, used = dev.k_shortest_walks_mode_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, K, k, mode, row[0].data_ptr(), row[1].data_ptr(),
                                                         row[2].data_ptr(), row[3].data_ptr(), t_po.data_ptr(), t_ph.data_ptr(), path_cap,
                                                         t_ch.data_ptr(), child_cap)
    return (rc, paths, used) + tuple(t.cpu().numpy()[:n] for t in row) + (t_po.cpu().numpy(), t_ph.cpu().numpy(), t_ch.cpu().numpy())


def needs(lists):
    return sum(len(ps) for ps in lists if ps is not None), sum(len(q) for ps in lists if ps is not None for q in ps)


def bulk(dev, rs, rd, lo, K, k, mode, want):
    """The bulk form's lists from buffers of exactly the size the expected lists need; every per-row array, the layout and the steps."""
    counts, hops, lists, steps1, steps2 = want[:5]
    P, C = needs(lists)
    rc, paths, used, ln, cnt, first, npaths, po, ph, ch = bulk_raw(dev, rs, rd, lo, K, k, mode, P, C)
    assert rc == 0 and (paths, used) == (P, C), (rc, paths, used, P, C)
    assert ln.tolist() == hops and cnt.tolist() == counts
    assert npaths.tolist() == [max(c, 0) for c in counts]  # min(a, k); a NULL row: count -1, no walk
    assert first.tolist() == (np.cumsum(npaths) - npaths).tolist()  # packed in row order ...
    assert ph[:P].tolist() == [len(q) // 2 for ps in lists if ps is not None for q in ps]
    width = 2 * ph[:P] + 1
    assert po[:P].tolist() == (np.cumsum(width) - width).tolist()  # ... and so are the walks' elements
    assert pgq.mode_steps() == (sum(steps1) + sum(steps2), max(steps1)), (pgq.mode_steps(), sum(steps1), sum(steps2), max(steps1))
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
        for lo, K, ks, modes in runs or fx_runs:
            for mode in modes:
                for k in ks:
                    want = want_of(name, lo, K, k, mode)
                    what = "%s, {%d,%d}, k = %d, %s" % (name, lo, K, k, M.MODE_NAMES[mode])
                    same(bulk(dev, rs, rd, lo, K, k, mode, want), want[2], rs, rd, what + ", bulk form")
                    same(dev.k_shortest_walks(rs, rd, lo, K, k, path_mode=mode), want[2], rs, rd, what + ", chunk form")
                    same(st.k_shortest_walks(0, V, rs, rd, lo, K, k, path_mode=mode), want[2], rs, rd, what + ", udf form")
                    # the count form: the same search with nothing emitted, k its limit
                    same(bulk_count(dev, rs, rd, lo, K, k, mode), want[0], rs, rd, what + ", count, bulk form")
                    assert pgq.mode_steps() == (sum(want[3]), max(want[3])), what
                    for form, (out, ok) in (("chunk", dev.walk_count(rs, rd, lo, K, limit=k, path_mode=mode)),
                                            ("udf", st.walk_count(0, V, rs, rd, lo, K, limit=k, path_mode=mode))):
                        assert ok.all(), (what, form)
                        same(out.tolist(), want[0], rs, rd, what + ", count, %s form" % form)
    finally:
        if own:
            dev.close()


# ---- 1. the random multigraph: every (src, dst), the model's expectation is the filtered enumeration itself --------------------------------
def test_random_multigraph_against_the_filtered_enumeration():
    check_all_forms("tiny0")
    fx = FIXTURES["tiny0"][0]
    brute = {}
    for mode in M.MODES:
        assert want_of("tiny0", 0, 3, ALL, mode)[:3] == M.filter_model(*fx, 0, 3, ALL, mode, brute=brute)


def test_none_and_walk_go_to_the_existing_calls():
    fx = FIXTURES["tiny0"][0]
    V, off, adj, eid, rs, rd = fx
    dev, st = device(fx), udf_state(fx)
    for lo, K, k in ((0, 3, 3), (2, 4, ALL)):
        counts, hops, lists, counts_k = W.solve(*fx, lo, K, k)
        P, C = needs(lists)
        for mode in (M.NONE, M.WALK):
            rc, paths, used, ln, cnt, first, npaths, po, ph, ch = bulk_raw(dev, rs, rd, lo, K, k, mode, P, C)
            assert rc == 0 and (paths, used) == (P, C) and ln.tolist() == hops and cnt.tolist() == counts_k  # d_out_count as that call defines it
            assert npaths.tolist() == [0 if ps is None else len(ps) for ps in lists]
            assert dev.k_shortest_walks(rs, rd, lo, K, k, path_mode=mode) == lists == st.k_shortest_walks(0, V, rs, rd, lo, K, k, path_mode=mode)
            for limit in (1, 4, ALL):
                cut = [min(c, limit) for c in counts]
                assert bulk_count(dev, rs, rd, lo, K, limit, mode) == cut
                assert dev.walk_count(rs, rd, lo, K, limit=limit, path_mode=mode)[0].tolist() == cut
                assert st.walk_count(0, V, rs, rd, lo, K, limit=limit, path_mode=mode)[0].tolist() == cut
            assert pgq.mode_steps() == (0, 0)
    dev.close()


# ---- 2. in-lists of 63 .. 129 entries: the last slot, the first slot of the second trip, two in one trip, two in neighbouring trips ----------
@pytest.mark.parametrize("deg", [63, 64, 65, 128, 129])
def test_in_list_lengths_and_the_cursor(deg):
    name = "in_list_%d" % deg
    check_all_forms(name)
    counts, hops, lists = want_of(name, 0, 2, ALL, M.TRAIL)[:3]
    assert counts == [1, 1, 2, 2, 0] and hops == [2, 2, 2, 2, -1]
    assert want_of(name, 0, 2, 1, M.TRAIL)[0] == [1, 1, 1, 1, 0]


# ---- 3. the full stack depth ------------------------------------------------------------------------------------------------------------------
def test_a_chain_of_64_edges_with_a_chord_and_a_ring_of_64():
    check_all_forms("chain64")
    check_all_forms("ring64")
    assert [len(q) // 2 for q in want_of("chain64", 0, 64, 3, M.ACYCLIC)[2][0]] == [63, 64]
    assert want_of("ring64", 1, 64, 2, M.ACYCLIC)[2][0] is None and len(want_of("ring64", 1, 64, 2, M.SIMPLE)[2][0][0]) == 129


# ---- 4. cycles under each mode; src == dst rows with and without a lane --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring5", "self_loop", "two_loops", "detour"])
def test_cycles_under_each_mode(name):
    check_all_forms(name)


def test_what_the_modes_say_about_loops():
    assert want_of("self_loop", 1, 3, ALL, M.SIMPLE)[2][0] == [[0, 1000, 0]] and want_of("self_loop", 1, 3, ALL, M.ACYCLIC)[2][0] is None
    assert want_of("self_loop", 0, 3, ALL, M.ACYCLIC)[2][0] == [[0]] and want_of("self_loop", 0, 3, 1, M.TRAIL)[2][5] == [[2]]  # (2, 2): no lane
    assert want_of("two_loops", 1, 5, ALL, M.TRAIL)[0] == [4] and want_of("two_loops", 1, 5, ALL, M.SIMPLE)[0] == [2]
    assert want_of("ring5", 1, 10, 3, M.SIMPLE)[0][0] == 1 and want_of("ring5", 1, 10, 3, M.TRAIL)[0][0] == 1
    # a row whose distance is below lo: its shortest admitted walk is longer than its shortest walk
    assert want_of("detour", 2, 3, 1, M.ACYCLIC)[1][0] == 3 and want_of("detour", 2, 3, 1, M.TRAIL)[1][0] == 2


# ---- 5. TRAIL: runs of parallel slots, ids against slots ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [63, 64, 65, 129])
def test_a_run_of_parallel_slots_under_trail(P):
    name = "parallel_run_%d" % P
    check_all_forms(name)
    assert want_of(name, 3, 3, ALL, M.TRAIL)[0] == [0, P * (P - 1), 0, 0]


def test_undirected_edges_share_an_id():
    check_all_forms("pair_and_triangle")
    assert want_of("pair_and_triangle", 2, 4, ALL, M.TRAIL)[2][0] is None  # 0 - 1 - 0 goes back over the one edge
    assert want_of("pair_and_triangle", 3, 3, ALL, M.TRAIL)[0][3] == 2  # round the triangle, both ways


# ---- 6. batch boundaries -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_batch_boundaries(n):
    check_all_forms("sources_%d" % n)
    check_all_forms("detour", runs=((2, 3, (1,), (M.ACYCLIC,)),))  # a smaller graph on the same thread afterwards


# ---- 7. k and limit at a - 1, a, a + 1 ------------------------------------------------------------------------------------------------------------
def test_k_and_limit_around_the_number_of_admitted_walks():
    check_all_forms("parallel")
    fx = FIXTURES["parallel"][0]
    V, off, adj, eid, rs, rd = fx
    dev = device(fx)
    for mode in M.MODES:
        full = M.search_model(*fx, 0, 3, ALL, mode)
        a = full[0][0]
        assert a >= 2
        for k in (a - 1, a, a + 1):
            want = M.search_model(*fx, 0, 3, k, mode)
            assert want[0][0] == min(a, k) and want[2][0] == full[2][0][:k]
            assert bulk(dev, rs, rd, 0, 3, k, mode, want) == want[2]
            assert bulk_count(dev, rs, rd, 0, 3, k, mode) == want[0]
    dev.close()


# ---- 8. special rows --------------------------------------------------------------------------------------------------------------------------
def test_null_rows_selections_and_empty_calls():
    fx = FIXTURES["sources_65"][0]
    V, off, adj, eid, rs, rd = fx
    rs, rd = rs[:60].copy(), rd[:60].copy()
    rd[::11] = rs[::11]  # closed rows among the others
    counts, hops, lists = M.search_model(V, off, adj, eid, rs, rd, 1, 3, 2, M.SIMPLE)[:3]
    dev, st = device(fx), udf_state(fx)
    sv, dv = np.ones(len(rs), dtype=bool), np.ones(len(rs), dtype=bool)
    sv[3::7] = False
    dv[5::7] = False
    null = ~(sv & dv)
    masked = [None if null[i] else ps for i, ps in enumerate(lists)]
    sel = np.array([7, 7, 0, 59, 12, 3, 12], dtype=np.uint32)
    for obj, args in ((dev, ()), (st, (0, V))):
        assert obj.k_shortest_walks(*args, rs, rd, 1, 3, 2, src_valid=sv, dst_valid=dv, path_mode=M.SIMPLE) == masked
        out, ok = obj.walk_count(*args, rs, rd, 1, 3, src_valid=sv, dst_valid=dv, limit=2, path_mode=M.SIMPLE)
        assert (ok == ~null).all() and out[ok].tolist() == [c for c, z in zip(counts, null) if not z]
        assert obj.k_shortest_walks(*args, rs, rd, 1, 3, 2, src_sel=sel, dst_sel=sel, path_mode=M.SIMPLE) == [lists[i] for i in sel]
    first, npaths, ov, po, pl, ch = dev.k_shortest_walks(rs, rd, 1, 3, 2, src_valid=sv, dst_valid=dv, raw=True, path_mode=M.SIMPLE)
    for i, ps in enumerate(masked):
        if ps is None:  # NULL: no inner list, no payload
            assert first[i] == 0 and npaths[i] == 0 and not (int(ov[i >> 6]) >> (i & 63)) & 1
    assert (len(po), len(ch)) == needs(masked)
    brs = rs.copy()  # bulk form: a negative src is a NULL row with count -1
    brs[4::9] = -1
    bwant = M.search_model(V, off, adj, eid, brs, rd, 1, 3, 2, M.TRAIL)
    assert bulk_count(dev, brs, rd, 1, 3, 2, M.TRAIL) == bwant[0] and -1 in bwant[0]
    assert bulk(dev, brs, rd, 1, 3, 2, M.TRAIL, bwant) == bwant[2]
    assert dev.k_shortest_walks([], [], 1, 3, 2, path_mode=M.TRAIL) == [] and len(dev.walk_count([], [], 1, 3, limit=1, path_mode=M.TRAIL)[0]) == 0
    dev.close()


# ---- 9. the capacity protocol -------------------------------------------------------------------------------------------------------------------
def test_capacity_protocol():
    fx = FIXTURES["sources_65"][0]
    V, off, adj, eid, rs, rd = fx
    want = want_of("sources_65", 1, 3, 2, M.ACYCLIC)
    counts, hops, lists = want[:3]
    P, C = needs(lists)
    dev = device(fx)
    for path_cap, child_cap in ((P - 1, C), (P, C - 1), (0, 0)):
        rc, paths, used, ln, cnt, first, npaths, po, ph, ch = bulk_raw(dev, rs, rd, 1, 3, 2, M.ACYCLIC, path_cap, child_cap)
        assert rc == -4 and (paths, used) == (P, C), (path_cap, child_cap)
        assert ln.tolist() == hops and cnt.tolist() == counts and npaths.tolist() == counts
    assert "too small" in pgq.load_hip().pgq_last_error().decode()
    same(bulk(dev, rs, rd, 1, 3, 2, M.ACYCLIC, want), lists, rs, rd, "exact size")
    dev.close()


# ---- 10. every error code -------------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    fx = W.chain8()
    V, off, adj, eid, rs, rd = fx
    dev, st = device(fx), udf_state(fx)
    err = lambda: pgq.load_hip().pgq_last_error().decode()  # noqa: E731
    untouched = lambda out: all((a == -7).all() for a in out[3:])  # noqa: E731
    for lo, K, k, mode in ((-1, 3, 1, M.TRAIL), (3, 2, 1, M.TRAIL), (1, 3, 0, M.TRAIL), (1, 3, 1, 5), (1, 3, 1, -1), (1, 3, 0, M.WALK), (1, 3, 1, 7)):
        out = bulk_raw(dev, rs, rd, lo, K, k, mode, 10, 10)  # PGQ_ERR_INVALID_ARG
        assert out[0] == -4 and untouched(out), (lo, K, k, mode)
        with pytest.raises(PgqError):
            dev.k_shortest_walks(rs, rd, lo, K, k, path_mode=mode)
        with pytest.raises(PgqError):
            st.k_shortest_walks(0, V, rs, rd, lo, K, k, path_mode=mode)
        with pytest.raises(PgqError):
            dev.walk_count(rs, rd, lo, K, limit=k, path_mode=mode)
        with pytest.raises(PgqError):
            st.walk_count(0, V, rs, rd, lo, K, limit=k, path_mode=mode)
        with pytest.raises(PgqError):
            bulk_count(dev, rs, rd, lo, K, k, mode)
    with pytest.raises(PgqError, match="limit must be at least 1"):
        dev.walk_count(rs, rd, 1, 3, limit=0, path_mode=M.TRAIL)
    for K in (M.MAX_HOPS + 1, W.INT64_MAX):  # PGQ_ERR_UNSUPPORTED: an unbounded upper is not built under a mode either
        for mode in (M.WALK, M.SIMPLE):
            out = bulk_raw(dev, rs, rd, 0, K, 1, mode, 10, 10)
            assert out[0] == -6 and "upper bound" in err() and untouched(out)
            with pytest.raises(PgqError, match="upper bound"):
                dev.walk_count(rs, rd, 0, K, limit=1, path_mode=mode)
            with pytest.raises(PgqError, match="upper bound"):
                st.k_shortest_walks(0, V, rs, rd, 0, K, 1, path_mode=mode)
    # more than 2^31 - 1 emitted walks: 8192 rows of 8^6 = 2^18 trails each; the counting pass finds them, nothing is written
    many_s, many_d = np.zeros(8192, dtype=np.int64), np.full(8192, 6, dtype=np.int64)
    out = bulk_raw(dev, many_s, many_d, 6, 6, ALL, M.TRAIL, 16, 16)
    assert out[0] == -6 and "2^31-1 walks" in err() and out[1:3] == (0, 0) and untouched(out)
    assert bulk_count(dev, many_s[:2], many_d[:2], 6, 6, ALL, M.TRAIL) == [8 ** 6] * 2  # the count form emits nothing
    for bad_call in (lambda: dev.k_shortest_walks([0, V], [1, 1], 1, 3, 2, path_mode=M.TRAIL),
                     lambda: dev.walk_count([0], [V], 1, 3, limit=1, path_mode=M.TRAIL)):
        with pytest.raises(PgqError):
            bad_call()
    assert bulk_raw(dev, np.array([0, V]), np.array([1, 1]), 1, 3, 2, M.TRAIL, 10, 10)[0] == -4
    with pytest.raises(PgqError, match="go together"):
        dev.walk_count(rs, rd, 1, 3, limit=2)
    dev.close()


# ---- 11. the work limit ---------------------------------------------------------------------------------------------------------------------------
def test_step_cap():
    name, lo, K, k, mode = "parallel_run_65", 3, 3, ALL, M.TRAIL
    fx = FIXTURES[name][0]
    V, off, adj, eid, rs, rd = fx
    want = want_of(name, lo, K, k, mode)
    row_max = max(want[3])
    assert row_max > 1000 and pgq.get_default_option("mode_step_cap") == 1 << 24
    P, C = needs(want[2])
    dev = device(fx)
    dev.set_option("mode_step_cap", row_max - 1)  # this handle's option: the process-wide one stays
    assert dev.get_option("mode_step_cap") == row_max - 1 and pgq.get_option("mode_step_cap") == 1 << 24
    out = bulk_raw(dev, rs, rd, lo, K, k, mode, P, C)
    msg = pgq.load_hip().pgq_last_error().decode()
    assert out[0] == -6 and "mode_step_cap = %d" % (row_max - 1) in msg and out[1:3] == (0, 0) and all((a == -7).all() for a in out[3:])
    with pytest.raises(PgqError, match="mode_step_cap"):
        dev.walk_count(rs, rd, lo, K, limit=k, path_mode=mode)
    with pytest.raises(PgqError, match="mode_step_cap"):
        dev.k_shortest_walks(rs, rd, lo, K, k, path_mode=mode)
    assert dev.k_shortest_walks(rs, rd, lo, K, 1, path_mode=mode) == want_of(name, lo, K, 1, mode)[2]  # a cheaper call under the same cap
    dev.set_option("mode_step_cap", row_max)
    assert bulk(dev, rs, rd, lo, K, k, mode, want) == want[2]  # the next call succeeds
    dev.close()


# ---- 12. the rounds stop by distance ----------------------------------------------------------------------------------------------------------------
def test_rounds_stop_at_the_distance():
    fx = W.chain8()
    V, off, adj, eid, rs, rd = fx
    dev = device(fx)
    row = (np.array([0]), np.array([5]))
    for mode in M.MODES:
        want = M.search_model(V, off, adj, eid, *row, 0, M.MAX_HOPS, 1, mode)
        assert want[5] == [5]
        pgq.binding.reset_stats()
        assert dev.k_shortest_walks(*row, 0, M.MAX_HOPS, 1, path_mode=mode) == want[2]
        assert pgq.get_stats()["levels"] == 5  # d rounds, not K
    pgq.binding.reset_stats()
    assert dev.walk_count(*row, 6, M.MAX_HOPS, limit=1, path_mode=M.TRAIL)[0].tolist() == [0]  # lo > d: open to the chain's end
    assert 22 <= pgq.get_stats()["levels"] <= 23
    dev.close()
    # a row at distance 1 < lo = 2 with W_1[dst] >= k must not close the batch: its walks have 2 and 3 edges
    fx = FIXTURES["detour"][0]
    dev = device(fx)
    row = (np.array([0]), np.array([1]))
    pgq.binding.reset_stats()
    assert dev.k_shortest_walks(*row, 2, 3, 1, path_mode=M.ACYCLIC) == [[[0, 1002, 2, 1003, 3, 1004, 1]]]
    assert pgq.get_stats()["levels"] == 3
    dev.close()


# ---- 13. the neighbours on the shared workspace ------------------------------------------------------------------------------------------------------
def test_neighbours_unchanged_and_nothing_left_behind():
    V, off, adj, eid, rs, rd = FIXTURES["sources_65"][0]
    w = np.random.default_rng(3).integers(1, 9, len(adj))
    before_handle = pgq.live_device_blocks()
    dev = pgq.DeviceCSR(V, off, adj, eid, w)

    def neighbours():
        return (dev.k_shortest_walks(rs, rd, 1, 3, 3), dev.walk_count(rs, rd, 2, 4)[0].tolist(), dev.all_shortestpaths(rs, rd, 3, 7),
                dev.cheapest_path(rs, rd), dev.shortestpath(rs, rd))

    first = neighbours()
    assert first[0] == W.solve(V, off, adj, eid, rs, rd, 1, 3, 3)[2] and first[2] == A.solve(V, off, adj, eid, rs, rd, 3, 7)[2]
    want = want_of("sources_65", 1, 3, 2, M.SIMPLE)
    P, C = needs(want[2])
    for _ in range(2):
        assert dev.k_shortest_walks(rs, rd, 1, 3, 2, path_mode=M.SIMPLE) == want[2]
        assert neighbours() == first
        assert dev.walk_count(rs, rd, 1, 3, limit=2, path_mode=M.SIMPLE)[0].tolist() == want[0]
        assert bulk_raw(dev, rs, rd, 1, 3, 2, M.SIMPLE, P - 1, C - 1)[0] == -4  # a call that failed with a too-small buffer
        assert neighbours() == first
        dev.set_option("mode_step_cap", 1)
        assert bulk_raw(dev, rs, rd, 1, 3, 2, M.SIMPLE, P, C)[0] == -6  # ... and one that went over the step cap
        dev.set_option("mode_step_cap", 1 << 24)
        assert neighbours() == first
        assert bulk(dev, rs, rd, 1, 3, 2, M.SIMPLE, want) == want[2]
    dev.close()
    assert pgq.live_device_blocks() == before_handle
