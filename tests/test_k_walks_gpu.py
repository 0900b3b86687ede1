"""walk_count and k_shortest_walks on the GPU, in every entry form (bulk, chunk, UDF), against the Python model of their contract
(k_walks_model.py — checked on the CPU against a brute-force enumeration of walks, all_shortestpaths' model and the oracle; the
fixtures used here catch its mutants there).  Every comparison is exact: counts, hops, whole lists, offsets and payload sizes."""
import numpy as np
import pytest

import all_shortest_model as A
import duckpgq_extension_amd as pgq
import k_walks_model as M
from duckpgq_extension_amd.binding import PgqError

pytestmark = pytest.mark.gpu

INT64_MAX = M.INT64_MAX
ALL = M.K_ALL
FIXTURES = M.gpu_fixtures()
_want, _state = {}, {}


def want_of(name, lo, K, k):
    """(counts, hops, lists, counts_k) of the model, computed once and left unchanged."""
    if (name, lo, K, k) not in _want:
        _want[name, lo, K, k] = M.solve(*FIXTURES[name][0], lo, K, k, state=_state.setdefault(name, {}))
    return _want[name, lo, K, k]


def device(fx):
    V, off, adj, eid = fx[:4]
    return pgq.DeviceCSR(V, off, adj, eid)


def udf_state(fx):
    V, off, adj, eid = fx[:4]
    st = pgq.PgqState()
    st.build_csr(0, V, A.slot_sources(V, off), adj, eid)
    return st


def bulk_count(dev, rs, rd, lo, K):
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    t_c = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    dev.walk_count_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, K, t_c.data_ptr())
    return t_c.cpu().numpy()[:n].tolist()


def bulk_raw(dev, rs, rd, lo, K, k, path_cap, child_cap):
    """(rc, walks needed, elements needed, hops, counts, first, npaths, walk offsets, walk hops, child) of the bulk form."""
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    row = [torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda") for _ in range(4)]
    t_po = torch.full((max(path_cap, 1),), -7, dtype=torch.int64, device="cuda")
    t_ph = torch.full((max(path_cap, 1),), -7, dtype=torch.int64, device="cuda")
    t_ch = torch.full((max(child_cap, 1),), -7, dtype=torch.int64, device="cuda")
    rc, paths, used = dev.k_shortest_walks_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, K, k, row[0].data_ptr(), row[1].data_ptr(), row[2].data_ptr(),
                                                    row[3].data_ptr(), t_po.data_ptr(), t_ph.data_ptr(), path_cap, t_ch.data_ptr(), child_cap)
    return (rc, paths, used) + tuple(t.cpu().numpy()[:n] for t in row) + (t_po.cpu().numpy(), t_ph.cpu().numpy(), t_ch.cpu().numpy())


def needs(lists):
    return sum(len(ps) for ps in lists if ps is not None), sum(len(q) for ps in lists if ps is not None for q in ps)


def bulk(dev, rs, rd, lo, K, k, want):
    """The bulk form's lists from buffers of exactly the size the expected lists need; every per-row array and the layout checked."""
    counts, hops, lists, counts_k = want
    P, C = needs(lists)
    rc, paths, used, ln, cnt, first, npaths, po, ph, ch = bulk_raw(dev, rs, rd, lo, K, k, P, C)
    assert rc == 0 and (paths, used) == (P, C), (rc, paths, used, P, C)
    assert ln.tolist() == hops and cnt.tolist() == counts_k
    assert npaths.tolist() == [0 if ps is None else len(ps) for ps in lists]
    assert first.tolist() == (np.cumsum(npaths) - npaths).tolist()  # packed in row order ...
    assert ph[:P].tolist() == [len(q) // 2 for ps in lists if ps is not None for q in ps]
    width = 2 * ph[:P] + 1
    assert po[:P].tolist() == (np.cumsum(width) - width).tolist()  # ... and so are the walks' elements
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
        for lo, K, ks in runs or fx_runs:
            counts = want_of(name, lo, K, ks[0])[0]
            what = "%s, {%d,%d}" % (name, lo, K)
            same(bulk_count(dev, rs, rd, lo, K), counts, rs, rd, what + ", count, bulk form")
            for form, (out, ok) in (("chunk", dev.walk_count(rs, rd, lo, K)), ("udf", st.walk_count(0, V, rs, rd, lo, K))):
                assert ok.all(), (what, form)
                same(out.tolist(), counts, rs, rd, what + ", count, %s form" % form)
            for k in ks:
                want = want_of(name, lo, K, k)
                what = "%s, {%d,%d}, k = %d" % (name, lo, K, k)
                same(bulk(dev, rs, rd, lo, K, k, want), want[2], rs, rd, what + ", bulk form")
                same(dev.k_shortest_walks(rs, rd, lo, K, k), want[2], rs, rd, what + ", chunk form")
                same(st.k_shortest_walks(0, V, rs, rd, lo, K, k), want[2], rs, rd, what + ", udf form")
    finally:
        if own:
            dev.close()


# ---- 1. the brute-force graph and the random multigraph, (lo, K) in {(0,0), (0,3), (1,3), (2,4), (3,3)}, k in {1, 3, all} --------------
@pytest.mark.parametrize("name", ["tiny0", "random"])
def test_random_and_brute_force_graphs(name):
    check_all_forms(name)
    V, off, adj, eid, rs, rd = FIXTURES[name][0]
    if name == "tiny0":  # the model's expectation is the enumeration of all walks itself
        brute = {s: M.brute_force(V, off, adj, eid, s, 4) for s in range(V)}
        lists = want_of(name, 2, 4, ALL)[2]
        assert all(lists[i] == ([p for p in brute[s][d] if len(p) >= 5] or None) for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())))


def test_leading_walks_are_all_shortestpaths_lists():
    """For src != dst and lo <= d <= K the walks of length d are all_shortestpaths' lists in its order, walk 0 shortestpath's."""
    fx = FIXTURES["random"][0]
    V, off, adj, eid, rs, rd = fx
    dev = device(fx)
    walks = dev.k_shortest_walks(rs, rd, 1, 3, ALL)
    shortest = dev.all_shortestpaths(rs, rd, 3, A.MAX_PATHS_ALL)
    plain = dev.shortestpath_within(rs, rd, 3)
    checked = 0
    for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
        if s != d and shortest[i] is not None:
            assert walks[i][:len(shortest[i])] == shortest[i] and walks[i][0] == plain[i], (s, d)
            checked += 1
    assert checked >= 40
    dev.close()


# ---- 2. in-lists and out-lists of 63 .. 129 entries, walks of d and d + c edges ---------------------------------------------------------
@pytest.mark.parametrize("deg", [63, 64, 65, 127, 128, 129])
def test_list_lengths_around_the_wavefront_width(deg):
    name = "in_list_%d" % deg
    check_all_forms(name)
    counts, hops, lists, _ = want_of(name, 0, 3, ALL)
    x_parents = [q[-3] for q in lists[0]]
    assert counts[0] == len(lists[0]) > deg // 3 and x_parents[0] == min(x_parents) and x_parents[-1] == max(x_parents)  # first .. last position
    assert sorted({len(q) // 2 for q in want_of(name, 3, 7, 200)[2][0]}) == [3, 4, 7]


# ---- 3. batch boundaries; the next call sees a clean workspace ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_batch_boundaries(n):
    check_all_forms("sources_%d" % n)
    check_all_forms("tiny0", runs=((1, 3, (3,)),))  # a smaller graph on the same thread afterwards


# ---- 4. parallel edges, per-row limits: k = count - 1, count, count + 1 ---------------------------------------------------------------
def test_parallel_edges_and_per_row_limits():
    check_all_forms("parallel")
    for k, emitted in ((1, 1), (9, 9), (10, 10), (11, 10)):
        counts, _, lists, counts_k = want_of("parallel", 0, 3, k)
        assert counts[0] == counts_k[0] == 10 and len(lists[0]) == emitted
    nine = want_of("parallel", 0, 3, 11)[2][0][1:]
    assert len({tuple(q) for q in nine}) == 9 and len({e for q in nine for e in (q[1], q[3])}) == 6


@pytest.mark.parametrize("P", [63, 64, 65, 129])
def test_a_run_of_parallel_slots(P):
    """The m-th of P parallel slots, m up to P - 1: the run crosses position 64 of the in-list, its edges lie at other positions
    of the parent's out-list, past its first 64 entries."""
    name = "parallel_run_%d" % P
    check_all_forms(name)
    counts, hops, lists, _ = want_of(name, 2, 2, ALL)
    assert counts == [1 + P, 0] and hops == [2, -1] and len({q[-2] for q in lists[0]}) == 1 + P
    assert want_of(name, 1, 2, ALL)[0] == [1 + P, P]


# ---- 5. cycles: a ring of 5, a self-loop; rows without a lane ---------------------------------------------------------------------------
def test_ring_and_self_loop():
    check_all_forms("ring5")
    check_all_forms("self_loop")
    counts, hops, lists, _ = want_of("ring5", 1, 10, 3)
    assert counts[0] == 2 and [len(q) // 2 for q in lists[0]] == [5, 10]  # (a, a) with lo = 1: the closed walks
    assert want_of("ring5", 0, 10, 3)[2][0][0] == [0] and want_of("ring5", 1, 4, 1)[2][0] is None
    assert want_of("self_loop", 0, 3, ALL)[0][:2] == [4, 3]  # (0, 0): the loop 0..3 times; (0, 1): 0..2 loops, then the edge


def test_rows_without_a_lane_and_special_rows():
    check_all_forms("dead_ends")  # no out-edge at src, no in-edge at dst, src == dst with neither
    assert want_of("dead_ends", 0, 2, 1)[0] == [0, 0, 2, 1, 0, 0, 1, 1] and want_of("dead_ends", 0, 2, 1)[2][3] == [[4]]
    assert want_of("dead_ends", 1, 2, 1)[0] == [0, 0, 2, 0, 0, 0, 0, 0] and want_of("dead_ends", 1, 2, 1)[2][3] is None
    fx = FIXTURES["random"][0]
    V, off, adj, eid, rs, rd = fx
    rs, rd = rs[:60].copy(), rd[:60].copy()
    rd[::11] = rs[::11]  # closed rows among the others
    counts, hops, lists, counts_k = M.solve(V, off, adj, eid, rs, rd, 1, 3, 2)
    dev, st = device(fx), udf_state(fx)
    sv, dv = np.ones(len(rs), dtype=bool), np.ones(len(rs), dtype=bool)
    sv[3::7] = False
    dv[5::7] = False
    null = ~(sv & dv)
    masked = [None if null[i] else ps for i, ps in enumerate(lists)]
    sel = np.array([7, 7, 0, 59, 12, 3, 12], dtype=np.uint32)
    for obj, args in ((dev, ()), (st, (0, V))):
        assert obj.k_shortest_walks(*args, rs, rd, 1, 3, 2, src_valid=sv, dst_valid=dv) == masked
        out, ok = obj.walk_count(*args, rs, rd, 1, 3, src_valid=sv, dst_valid=dv)
        assert (ok == ~null).all() and out[ok].tolist() == [c for c, z in zip(counts, null) if not z]
        assert obj.k_shortest_walks(*args, rs, rd, 1, 3, 2, src_sel=sel, dst_sel=sel) == [lists[i] for i in sel]
        assert obj.walk_count(*args, rs, rd, 1, 3, src_sel=sel, dst_sel=sel)[0].tolist() == [counts[i] for i in sel]
    first, npaths, ov, po, pl, ch = dev.k_shortest_walks(rs, rd, 1, 3, 2, src_valid=sv, dst_valid=dv, raw=True)
    for i, ps in enumerate(masked):
        if ps is None:  # NULL: no inner list, no payload
            assert first[i] == 0 and npaths[i] == 0 and not (int(ov[i >> 6]) >> (i & 63)) & 1
    assert (len(po), len(ch)) == needs(masked)
    brs = rs.copy()  # bulk form: a negative src is a NULL row with count -1
    brs[4::9] = -1
    bwant = M.solve(V, off, adj, eid, brs, rd, 1, 3, 2)
    assert bulk_count(dev, brs, rd, 1, 3) == bwant[0] and -1 in bwant[0]
    assert bulk(dev, brs, rd, 1, 3, 2, bwant) == bwant[2]
    assert dev.k_shortest_walks([], [], 1, 3, 2) == [] and len(dev.walk_count([], [], 1, 3)[0]) == 0
    dev.close()


# ---- 6. saturation --------------------------------------------------------------------------------------------------------------------
def test_saturation():
    for name in ("chain8", "two_loops", "loops_and_fan"):
        check_all_forms(name)
    assert want_of("chain8", 0, M.MAX_HOPS, 3)[0][:3] == [2 ** 60, INT64_MAX, INT64_MAX]
    assert want_of("two_loops", 0, 62, 3)[0] == [INT64_MAX] == want_of("two_loops", 0, 63, 3)[0] and sum(2 ** t for t in range(63)) == INT64_MAX
    assert want_of("loops_and_fan", 1, 62, 3)[0][0] == INT64_MAX and want_of("loops_and_fan", 1, 61, 3)[0][0] == 3 * (2 ** 61 - 1)
    assert all(len(ps) == 3 for ps in want_of("chain8", 0, M.MAX_HOPS, 3)[2])  # the first three walks of each still unrank


# ---- 7. the capacity protocol -----------------------------------------------------------------------------------------------------------
def test_capacity_protocol():
    fx = FIXTURES["random"][0]
    V, off, adj, eid, rs, rd = fx
    want = want_of("random", 1, 3, 3)
    counts, hops, lists, counts_k = want
    P, C = needs(lists)
    dev = device(fx)
    for path_cap, child_cap in ((P - 1, C), (P, C - 1), (0, 0)):
        rc, paths, used, ln, cnt, first, npaths, po, ph, ch = bulk_raw(dev, rs, rd, 1, 3, 3, path_cap, child_cap)
        assert rc == -4 and (paths, used) == (P, C), (path_cap, child_cap)
        assert ln.tolist() == hops and cnt.tolist() == counts_k and npaths.tolist() == [0 if ps is None else len(ps) for ps in lists]
    assert "too small" in pgq.load_hip().pgq_last_error().decode()
    same(bulk(dev, rs, rd, 1, 3, 3, want), lists, rs, rd, "exact size")
    dev.close()


# ---- 8. bounds ------------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    fx = FIXTURES["chain8"][0]
    V, off, adj, eid, rs, rd = fx
    dev, st = device(fx), udf_state(fx)
    err = lambda: pgq.load_hip().pgq_last_error().decode()  # noqa: E731
    for lo, K, k in ((-1, 3, 1), (3, 2, 1), (1, 3, 0)):  # PGQ_ERR_INVALID_ARG
        assert bulk_raw(dev, rs, rd, lo, K, k, 10, 10)[0] == -4
        with pytest.raises(PgqError):
            dev.k_shortest_walks(rs, rd, lo, K, k)
        with pytest.raises(PgqError):
            st.k_shortest_walks(0, V, rs, rd, lo, K, k)
    for lo, K in ((-1, 3), (3, 2)):
        with pytest.raises(PgqError):
            dev.walk_count(rs, rd, lo, K)
        with pytest.raises(PgqError):
            st.walk_count(0, V, rs, rd, lo, K)
    for K in (M.MAX_HOPS + 1, INT64_MAX):  # PGQ_ERR_UNSUPPORTED: walks need an upper bound
        out = bulk_raw(dev, rs, rd, 0, K, 1, 10, 10)
        assert out[0] == -6 and "upper bound" in err() and all((a == -7).all() for a in out[3:])
        with pytest.raises(PgqError, match="upper bound"):
            dev.walk_count(rs, rd, 0, K)
        with pytest.raises(PgqError, match="upper bound"):
            st.k_shortest_walks(0, V, rs, rd, 0, K, 1)
    # two rows of 2^31 - 1 emitted walks each: more than a call may emit; nothing is written
    out = bulk_raw(dev, rs, rd, 0, 30, ALL, 16, 16)
    assert out[0] == -6 and "2^31-1 walks" in err() and out[1:3] == (0, 0) and all((a == -7).all() for a in out[3:])
    with pytest.raises(PgqError, match="2\\^31-1 walks"):
        dev.k_shortest_walks(rs, rd, 0, 30, ALL)
    assert dev.walk_count(rs, rd, 0, 30)[0].tolist() == want_of("chain8", 0, 30, 1)[0]  # the count itself has no such limit
    for bad_call in (lambda: dev.k_shortest_walks([0, V], [1, 1], 1, 3, 2), lambda: dev.walk_count([0], [V], 1, 3)):
        with pytest.raises(PgqError):
            bad_call()
    assert bulk_raw(dev, np.array([0, V]), np.array([1, 1]), 1, 3, 2, 10, 10)[0] == -4
    dev.close()


# ---- 9. the rounds stop when no row is short of k ------------------------------------------------------------------------------------------
def test_early_stop():
    fx = FIXTURES["chain8"][0]
    V, off, adj, eid, rs, rd = fx
    dev = device(fx)
    row = (np.array([0]), np.array([5]))
    pgq.binding.reset_stats()
    assert dev.k_shortest_walks(*row, 0, M.MAX_HOPS, 1) == [want_of("chain8", 0, M.MAX_HOPS, 1)[2][3]]
    assert pgq.get_stats()["levels"] == 5  # d rounds, not K
    pgq.binding.reset_stats()
    assert dev.walk_count(*row, 0, M.MAX_HOPS)[0].tolist() == [8 ** 5]
    assert 22 <= pgq.get_stats()["levels"] <= 23  # to the chain's end (and the round that activates nothing)
    dev.close()


# ---- 10. the neighbours on the shared workspace ------------------------------------------------------------------------------------------
def test_neighbours_unchanged_and_nothing_left_behind():
    V, off, adj, eid, rs, rd = FIXTURES["random"][0]
    w = np.random.default_rng(3).integers(1, 9, len(adj))
    before_handle = pgq.live_device_blocks()
    dev = pgq.DeviceCSR(V, off, adj, eid, w)

    def neighbours():
        return (dev.shortestpath(rs, rd), dev.all_shortestpaths(rs, rd, 3, 7), dev.cheapest_path(rs, rd), dev.cheapest_path_within(rs, rd, 3))

    first = neighbours()
    assert first[1] == A.solve(V, off, adj, eid, rs, rd, 3, 7)[2]
    want = want_of("random", 1, 3, 3)
    P, C = needs(want[2])
    for _ in range(2):
        assert dev.k_shortest_walks(rs, rd, 1, 3, 3) == want[2]
        assert neighbours() == first
        assert dev.walk_count(rs, rd, 2, 4)[0].tolist() == want_of("random", 2, 4, 1)[0]
        assert bulk_raw(dev, rs, rd, 1, 3, 3, P - 1, C - 1)[0] == -4  # a call that failed with a too-small buffer
        assert neighbours() == first
        assert bulk(dev, rs, rd, 1, 3, 3, want) == want[2]
    dev.close()
    assert pgq.live_device_blocks() == before_handle
