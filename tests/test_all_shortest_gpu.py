"""shortestpath_count and all_shortestpaths on the GPU, in every entry form (bulk, chunk, UDF), against the Python model of their
contract (all_shortest_model.py — checked on the CPU against a brute-force enumeration of walks and the oracle; the fixtures
used here catch its mutants there).  Every comparison is exact: counts, hops, whole lists, offsets and payload sizes."""
import numpy as np
import pytest

import all_shortest_model as M
import duckpgq_extension_amd as pgq
from duckpgq_extension_amd.binding import PgqError
from oracle.pgq_oracle import OracleCSR

pytestmark = pytest.mark.gpu

INT64_MAX = M.INT64_MAX
ALL = M.MAX_PATHS_ALL
FIXTURES = M.gpu_fixtures()
_full, _state = {}, {}


def want_of(name, h, p):
    """(counts, hops, lists) of the model, computed once and left unchanged.  Every path of a row is computed once per (fixture,
    max_hops) and cut to max_paths — except for the diamond chains, whose rows have 2^62 paths and more."""
    fx = FIXTURES[name][0]
    state = _state.setdefault(name, {})
    if name.startswith("diamonds"):
        return M.solve(*fx, h, p, state=state)
    if (name, h) not in _full:
        _full[name, h] = M.solve(*fx, h, ALL, state=state)
    counts, hops, lists = _full[name, h]
    return counts, hops, [None if ps is None else ps[:p] for ps in lists]


def device(fx):
    V, off, adj, eid = fx[:4]
    return pgq.DeviceCSR(V, off, adj, eid)


def udf_state(fx):
    V, off, adj, eid = fx[:4]
    st = pgq.PgqState()
    st.build_csr(0, V, M.slot_sources(V, off), adj, eid)
    return st


def bulk_count(dev, rs, rd, h):
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    t_c = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    dev.shortestpath_count_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), h, t_c.data_ptr())
    return t_c.cpu().numpy()[:n].tolist()


def bulk_raw(dev, rs, rd, h, p, path_cap, child_cap):
    """(rc, paths needed, elements needed, hops, counts, first, npaths, path offsets, child) of the bulk form."""
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    row = [torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda") for _ in range(4)]
    t_po = torch.full((max(path_cap, 1),), -7, dtype=torch.int64, device="cuda")
    t_ch = torch.full((max(child_cap, 1),), -7, dtype=torch.int64, device="cuda")
    rc, paths, used = dev.all_shortestpaths_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), h, p, row[0].data_ptr(), row[1].data_ptr(), row[2].data_ptr(),
                                                     row[3].data_ptr(), t_po.data_ptr(), path_cap, t_ch.data_ptr(), child_cap)
    return (rc, paths, used) + tuple(t.cpu().numpy()[:n] for t in row) + (t_po.cpu().numpy(), t_ch.cpu().numpy())


def needs(lists):
    return sum(len(ps) for ps in lists if ps is not None), sum(len(q) for ps in lists if ps is not None for q in ps)


def bulk(dev, rs, rd, h, p, want):
    """The bulk form's lists from buffers of exactly the size the expected lists need; every per-row array and the layout checked."""
    counts, hops, lists = want
    P, C = needs(lists)
    rc, paths, used, ln, cnt, first, npaths, po, ch = bulk_raw(dev, rs, rd, h, p, P, C)
    assert rc == 0 and (paths, used) == (P, C), (rc, paths, used, P, C)
    assert ln.tolist() == hops and cnt.tolist() == counts
    assert npaths.tolist() == [0 if ps is None else len(ps) for ps in lists]
    assert first.tolist() == (np.cumsum(npaths) - npaths).tolist()  # packed in row order ...
    width = np.repeat(np.where(ln >= 0, 2 * ln + 1, 0), npaths)
    assert po[:P].tolist() == (np.cumsum(width) - width).tolist()  # ... and so are the paths' elements
    return [None if ps is None else [ch[po[k]:po[k] + 2 * ln[i] + 1].tolist() for k in range(first[i], first[i] + npaths[i])]
            for i, ps in enumerate(lists)]


def same(got, want, rs, rd, what):
    bad = [i for i in range(len(rs)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d rows differ, first: %d -> %d got %r, expected %r" % (
        what, len(bad), len(rs), rs[bad[0]], rd[bad[0]], got[bad[0]], want[bad[0]])


def check_all_forms(name, dev=None, st=None, hops=None, paths=None):
    fx, fx_hops, fx_paths = FIXTURES[name]
    V, off, adj, eid, rs, rd = fx
    own = dev is None
    dev = dev or device(fx)
    st = st or udf_state(fx)
    try:
        for h in hops or fx_hops:
            counts = want_of(name, h, 1)[0]
            what = "%s, max_hops = %d" % (name, h)
            same(bulk_count(dev, rs, rd, h), counts, rs, rd, what + ", count, bulk form")
            for form, (out, ok) in (("chunk", dev.shortestpath_count(rs, rd, h)), ("udf", st.shortestpath_count(0, V, rs, rd, h))):
                assert ok.all(), (what, form)
                same(out.tolist(), counts, rs, rd, what + ", count, %s form" % form)
            for p in paths or fx_paths:
                want = want_of(name, h, p)
                what = "%s, max_hops = %d, max_paths = %d" % (name, h, p)
                same(bulk(dev, rs, rd, h, p, want), want[2], rs, rd, what + ", bulk form")
                same(dev.all_shortestpaths(rs, rd, h, p), want[2], rs, rd, what + ", chunk form")
                same(st.all_shortestpaths(0, V, rs, rd, h, p), want[2], rs, rd, what + ", udf form")
    finally:
        if own:
            dev.close()


# ---- 1. the random fixture and the brute-force graphs ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random"] + ["tiny%d" % s for s in range(6)])
def test_random_and_brute_force_graphs(name):
    check_all_forms(name)
    V, off, adj, eid, rs, rd = FIXTURES[name][0]
    if name.startswith("tiny"):  # the model's expectation is the enumeration of all walks itself
        lists = want_of(name, INT64_MAX, ALL)[2]
        assert all(lists[i] == M.brute_force(V, off, adj, eid, s, d) for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())))


@pytest.mark.parametrize("name", ["random", "tiny0", "tiny3"])
def test_one_path_is_the_oracles_shortestpath(name):
    fx = FIXTURES[name][0]
    V, off, adj, eid, rs, rd = fx
    plain = OracleCSR.adopt(V, off, adj, eid).shortestpath(V, rs, rd)
    dev, st = device(fx), udf_state(fx)
    for h in M.HOPS:
        want = [None if q is None or len(q) // 2 > h else [q] for q in plain]
        same(dev.all_shortestpaths(rs, rd, h, 1), want, rs, rd, "%s, max_hops = %d, chunk form" % (name, h))
        same(st.all_shortestpaths(0, V, rs, rd, h, 1), want, rs, rd, "%s, max_hops = %d, udf form" % (name, h))
        same(bulk(dev, rs, rd, h, 1, want_of(name, h, 1)), want, rs, rd, "%s, max_hops = %d, bulk form" % (name, h))
        # ... and shortestpath_within's lists, validity and payload, one level deeper
        o, ln, ov, child = dev.shortestpath_within(rs, rd, h, raw=True)
        first, npaths, ov2, po, pl, ch = dev.all_shortestpaths(rs, rd, h, 1, raw=True)
        n = len(rs)
        # (shortestpath's payload is not packed in row order, so the lists are compared through their entries)
        assert (ov[:(n + 63) // 64] == ov2[:(n + 63) // 64]).all() and len(child) == len(ch) and sorted(child.tolist()) == sorted(ch.tolist())
        valid = pgq.binding.unpack_validity(ov, n)
        k = first[valid].astype(np.int64)
        assert (npaths == valid).all() and (pl[k] == ln[valid]).all()
        assert all(ch[int(a):int(a) + int(w)].tolist() == child[int(b):int(b) + int(w)].tolist() for a, b, w in zip(po[k], o[valid], ln[valid]))
    dev.close()


def test_the_random_fixture_is_not_answered_by_single_paths_or_nulls_alone():
    counts, hops, _ = want_of("random", INT64_MAX, 1)
    bounded = want_of("random", 2, 1)[0]
    assert sum(c >= 2 for c in counts) >= 40 and sum(h >= 3 for h in hops) >= 40
    assert sum(c > 0 and b == 0 for c, b in zip(counts, bounded)) >= 40


# ---- 2. in-lists and out-lists of 63 .. 129 entries --------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [63, 64, 65, 127, 128, 129])
def test_list_lengths_around_the_wavefront_width(deg):
    name = "in_list_%d" % deg
    check_all_forms(name)
    counts, hops, lists = want_of(name, INT64_MAX, ALL)
    x_parents = [q[-3] for q in lists[0]]
    assert counts[0] == len(lists[0]) > deg // 3 and x_parents[0] == min(x_parents) and x_parents[-1] == max(x_parents)  # first .. last position


# ---- 3. parallel edges, per-row limits ----------------------------------------------------------------------------------------------
def test_parallel_edges_and_per_row_limits():
    check_all_forms("parallel")  # max_paths in {1, sigma - 1, sigma, sigma + 1} for sigma = 10
    for p, emitted in ((1, 1), (9, 9), (10, 10), (11, 10)):
        counts, _, lists = want_of("parallel", INT64_MAX, p)
        assert counts[0] == 10 and len(lists[0]) == emitted
    nine = want_of("parallel", INT64_MAX, 11)[2][0][1:]
    assert len({tuple(q) for q in nine}) == 9 and len({e for q in nine for e in (q[1], q[3])}) == 6


@pytest.mark.parametrize("P", [63, 64, 65, 129])
def test_a_run_of_parallel_slots(P):
    """The m-th of P parallel slots, m up to P - 1: the run crosses position 64 of the in-list, its edges lie at other positions
    of the parent's out-list, past its first 64 entries."""
    name = "parallel_run_%d" % P
    check_all_forms(name)
    counts, hops, lists = want_of(name, INT64_MAX, ALL)
    assert counts == [1 + P, P] and hops == [2, 1] and len({q[-2] for q in lists[0]}) == 1 + P


# ---- 4. batch boundaries: later batches walk what earlier ones touched; the next call sees a clean workspace ------------------
@pytest.mark.parametrize("k", [63, 64, 65, 129])
def test_batch_boundaries(k):
    check_all_forms("sources_%d" % k)
    check_all_forms("tiny1", hops=(INT64_MAX,), paths=(7,))  # a smaller graph on the same thread afterwards


# ---- 5. saturation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [62, 63, 64])
def test_diamond_chains(k):
    name = "diamonds_%d" % k
    check_all_forms(name)
    counts, hops, lists = want_of(name, INT64_MAX, 3)
    assert counts[0] == {62: 4611686018427387904, 63: INT64_MAX, 64: INT64_MAX}[k] and hops[0] == 2 * k
    assert len(lists[0]) == 3 and all(len(q) == 4 * k + 1 for q in lists[0])
    assert want_of(name, 2 * k - 1, 3)[0][0] == 0  # one hop short of the chain


def test_more_paths_than_a_call_may_emit():
    """Two rows of 2^62 and 2^31 paths under max_paths = 2^31 - 1: PGQ_ERR_UNSUPPORTED, and nothing is written."""
    V, off, adj, eid, rs, rd = fx = FIXTURES["diamonds_62"][0]
    counts = want_of("diamonds_62", INT64_MAX, 3)[0]
    assert counts[0] == 2 ** 62 and counts[1] == 2 ** 31
    dev = device(fx)
    rc, paths, used, ln, cnt, first, npaths, po, ch = bulk_raw(dev, rs, rd, INT64_MAX, ALL, 16, 16)
    assert rc == -6 and "2^31-1 paths" in pgq.load_hip().pgq_last_error().decode()
    assert (paths, used) == (0, 0) and all((a == -7).all() for a in (ln, cnt, first, npaths, po, ch))
    with pytest.raises(PgqError, match="2\\^31-1 paths"):
        dev.all_shortestpaths(rs, rd, INT64_MAX, ALL)
    assert dev.shortestpath_count(rs, rd, INT64_MAX)[0].tolist() == counts  # the count itself has no such limit
    dev.close()


# ---- 6. the capacity protocol ---------------------------------------------------------------------------------------------------------
def test_capacity_protocol():
    fx = FIXTURES["random"][0]
    V, off, adj, eid, rs, rd = fx
    want = want_of("random", 3, 2)
    counts, hops, lists = want
    P, C = needs(lists)
    dev = device(fx)
    for path_cap, child_cap in ((P - 1, C), (P, C - 1), (0, 0)):
        rc, paths, used, ln, cnt, first, npaths, po, ch = bulk_raw(dev, rs, rd, 3, 2, path_cap, child_cap)
        assert rc == -4 and (paths, used) == (P, C), (path_cap, child_cap)
        assert ln.tolist() == hops and cnt.tolist() == counts and npaths.tolist() == [0 if ps is None else len(ps) for ps in lists]
    assert "too small" in pgq.load_hip().pgq_last_error().decode()
    same(bulk(dev, rs, rd, 3, 2, want), lists, rs, rd, "exact size")  # (checks that the offsets are packed in row order)
    dev.close()


# ---- 7. special rows --------------------------------------------------------------------------------------------------------------------
def test_special_rows():
    check_all_forms("dead_ends")  # no out-edge at src, no in-edge at dst, src == dst under max_hops = 0
    counts, hops, lists = want_of("dead_ends", 0, 1)
    assert counts == [0, 0, 0, 1, 0, 0, 1, 1] and lists[3] == [[4]] and lists[6] == [[3]] and lists[2] is None
    assert want_of("dead_ends", 5, 3)[2][2] == [[0, 1000, 1, 1002, 3], [0, 1001, 2, 1003, 3]]
    fx = FIXTURES["random"][0]
    V, off, adj, eid, rs, rd = fx
    rs, rd = rs[:60], rd[:60]
    counts, hops, lists = M.solve(V, off, adj, eid, rs, rd, 3, 2)
    dev, st = device(fx), udf_state(fx)
    sv, dv = np.ones(len(rs), dtype=bool), np.ones(len(rs), dtype=bool)
    sv[3::7] = False
    dv[5::7] = False
    null = ~(sv & dv)
    masked = [None if null[i] else ps for i, ps in enumerate(lists)]
    sel = np.array([7, 7, 0, 59, 12, 3, 12], dtype=np.uint32)
    for obj, args in ((dev, ()), (st, (0, V))):
        assert obj.all_shortestpaths(*args, rs, rd, 3, 2, src_valid=sv, dst_valid=dv) == masked
        out, ok = obj.shortestpath_count(*args, rs, rd, 3, src_valid=sv, dst_valid=dv)
        assert (ok == ~null).all() and out[ok].tolist() == [c for c, z in zip(counts, null) if not z]
        assert obj.all_shortestpaths(*args, rs, rd, 3, 2, src_sel=sel, dst_sel=sel) == [lists[i] for i in sel]
        assert obj.shortestpath_count(*args, rs, rd, 3, src_sel=sel, dst_sel=sel)[0].tolist() == [counts[i] for i in sel]
    first, npaths, ov, po, pl, ch = dev.all_shortestpaths(rs, rd, 3, 2, src_valid=sv, dst_valid=dv, raw=True)
    for i, ps in enumerate(masked):
        if ps is None:  # NULL: no inner list, no payload
            assert first[i] == 0 and npaths[i] == 0 and not (int(ov[i >> 6]) >> (i & 63)) & 1
    assert (len(po), len(ch)) == needs(masked)
    brs = rs.copy()  # bulk form: a negative src is a NULL row with count -1
    brs[4::9] = -1
    bwant = M.solve(V, off, adj, eid, brs, rd, 3, 2)
    assert bulk_count(dev, brs, rd, 3) == bwant[0] and -1 in bwant[0]
    assert bulk(dev, brs, rd, 3, 2, bwant) == bwant[2]
    assert dev.all_shortestpaths([], [], 3, 2) == [] and len(dev.shortestpath_count([], [], 3)[0]) == 0
    # arguments out of range
    for bad_call in (lambda: dev.all_shortestpaths(rs, rd, -1, 2), lambda: dev.all_shortestpaths(rs, rd, 3, 0), lambda: dev.shortestpath_count(rs, rd, -1),
                     lambda: st.all_shortestpaths(0, V, rs, rd, 3, 0), lambda: st.shortestpath_count(0, V, rs, rd, -1),
                     lambda: dev.all_shortestpaths([0, V], [1, 1], 3, 2), lambda: dev.shortestpath_count([0], [V], 3)):
        with pytest.raises(PgqError):
            bad_call()
    assert bulk_raw(dev, rs, rd, -1, 2, 10, 10)[0] == -4 and bulk_raw(dev, rs, rd, 3, 0, 10, 10)[0] == -4
    assert bulk_raw(dev, np.array([0, V]), np.array([1, 1]), 3, 2, 10, 10)[0] == -4
    dev.close()


# ---- 8. the neighbours on the shared workspace ----------------------------------------------------------------------------------------
def test_neighbours_unchanged_and_nothing_left_behind():
    V, off, adj, eid, rs, rd = FIXTURES["random"][0]
    w = np.random.default_rng(3).integers(1, 9, len(adj))
    before_handle = pgq.live_device_blocks()
    dev = pgq.DeviceCSR(V, off, adj, eid, w)

    def neighbours():
        return (dev.shortestpath(rs, rd), [a.tolist() for a in dev.iterativelength_within(rs, rd, 3)], dev.cheapest_path(rs, rd),
                dev.cheapest_path_within(rs, rd, 3))

    first = neighbours()
    want = want_of("random", INT64_MAX, 7)
    for _ in range(2):
        assert dev.all_shortestpaths(rs, rd, INT64_MAX, 7) == want[2]
        assert dev.shortestpath_count(rs, rd, 2)[0].tolist() == want_of("random", 2, 1)[0]
        assert bulk(dev, rs, rd, INT64_MAX, 7, want) == want[2]
        assert neighbours() == first
    dev.close()
    assert pgq.live_device_blocks() == before_handle
