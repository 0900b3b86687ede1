"""cheapest_walk_length / cheapest_walk on the GPU: the cost and the list of the cheapest walk of lower..upper edges in every entry
form (bulk, chunk, UDF), against the Python model of the contract (cheapest_walk_model.py — held on the CPU to a brute-force
enumeration of walks, to the _within models and to walk_length / k_shortest_walks; the fixtures used here catch its mutants
there).  Every comparison is exact: values as bit patterns, validity, whole lists, lengths, offsets and payload sizes."""
import re

import numpy as np
import pytest

import cheapest_path_model as P
import cheapest_walk_model as M
import cheapest_within_model as W
import duckpgq_extension_amd as pgq
from cheapest_within_model import bits
from duckpgq_extension_amd.binding import PgqError

pytestmark = pytest.mark.gpu

SHIPPED = ("chain_cap", "relax_light", "relax_light_div", "relax_light_min_degree", "relax_labels32", "relax_split",
           "relax_small_limit", "relax_bidir_rows", "chain", "wbibfs")
KEYS = {"streams": 1, "relax_streams": 0, "relax_delta_div": 0, "relax_bidir": 0}
BOTH = pytest.mark.parametrize("double", [False, True], ids=["int64", "double"])
INT64_MAX = M.INT64_MAX


@pytest.fixture(autouse=True)
def _options():
    start = dict(KEYS, **{k: pgq.get_default_option(k) for k in SHIPPED})
    saved = {k: pgq.get_option(k) for k in start}
    for k, v in start.items():
        pgq.set_option(k, v)
    yield
    for k, v in saved.items():
        pgq.set_option(k, v)


def device(fx):
    V, off, adj, eid, w = fx[:5]
    return pgq.DeviceCSR(V, off, adj, eid, w)


def udf_state(fx):
    V, off, adj, eid, w = fx[:5]
    st = pgq.PgqState()
    st.build_csr(0, V, P.slot_sources(V, off), adj, eid, w)
    return st


def bulk_length(dev, w, rs, rd, lo, K):
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    t_out = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    t_ok = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
    dev.cheapest_walk_length_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, K, t_out.data_ptr(), t_ok.data_ptr())
    return t_out.cpu().numpy()[:n].view(w.dtype), t_ok.cpu().numpy()[:n].astype(bool)


def bulk_raw(dev, rs, rd, lo, K, cap):
    """(rc, child_used, lengths, offsets, child) of the bulk list form with a child buffer of `cap` elements."""
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    t_len = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    t_off = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    t_child = torch.full((max(cap, 1),), -7, dtype=torch.int64, device="cuda")
    rc, used = dev.cheapest_walk_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, K, t_len.data_ptr(), t_off.data_ptr(), t_child.data_ptr(), cap)
    return rc, used, t_len.cpu().numpy(), t_off.cpu().numpy(), t_child.cpu().numpy()


def bulk_lists(dev, rs, rd, lo, K, want, hops):
    """The bulk form's lists from a buffer of exactly the size the expected lists need; lengths (h), offsets and payload checked."""
    need = sum(len(p) for p in want if p is not None)
    rc, used, ln, off, child = bulk_raw(dev, rs, rd, lo, K, need)
    assert rc == 0 and used == need, (rc, used, need)
    assert ln.tolist() == list(hops)
    valid = ln >= 0
    sizes = np.where(valid, 2 * ln + 1, 0)
    assert (off[valid] == (np.cumsum(sizes) - sizes)[valid]).all()  # packed in row order
    return [None if ln[i] < 0 else child[off[i]:off[i] + 2 * ln[i] + 1].tolist() for i in range(len(rs))]


def same_values(got, want, what):
    out, ok = got
    bad = W.differing(np.ascontiguousarray(out), ok, want[0], want[1])
    assert len(bad) == 0, "%s: %d rows differ, first: row %d got %r / %r, expected %r / %r" % (
        what, len(bad), bad[0], out[bad[0]], ok[bad[0]], want[0][bad[0]], want[1][bad[0]])


def same_lists(got, want, rs, rd, what):
    bad = [i for i in range(len(rs)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d rows differ, first: %d -> %d got %r, expected %r" % (
        what, len(bad), len(rs), rs[bad[0]], rd[bad[0]], got[bad[0]], want[bad[0]])


def check_all_forms(fx, bounds, what, dev=None, forms=("bulk", "chunk", "udf"), model=None):
    """Both calls in the bulk, chunk and UDF form of one fixture against the model under every (lo, K); {(lo, K): the model's answer}."""
    V, off, adj, eid, w, rs, rd = fx
    own = dev is None
    dev = dev or device(fx)
    st = udf_state(fx) if "udf" in forms else None
    wants = {}
    try:
        for lo, K in bounds:
            want = wants[(lo, K)] = model(lo, K) if model else M.solve(V, off, adj, eid, w, rs, rd, lo, K)
            tag = "%s, {%d,%d}" % (what, lo, K)
            if "bulk" in forms:
                same_values(bulk_length(dev, w, rs, rd, lo, K), want, tag + ", length, bulk")
                same_lists(bulk_lists(dev, rs, rd, lo, K, want[3], want[2]), want[3], rs, rd, tag + ", list, bulk")
            if "chunk" in forms:
                same_values(dev.cheapest_walk_length(rs, rd, lo, K), want, tag + ", length, chunk")
                same_lists(dev.cheapest_walk(rs, rd, lo, K), want[3], rs, rd, tag + ", list, chunk")
            if st is not None:
                same_values(st.cheapest_walk_length(0, V, rs, rd, lo, K), want, tag + ", length, udf")
                same_lists(st.cheapest_walk(0, V, rs, rd, lo, K), want[3], rs, rd, tag + ", list, udf")
    finally:
        if own:
            dev.close()
    return wants


# ---- 1. the small fixtures: one property of the contract each ------------------------------------------------------------------
SMALL = ("bound_binds", "path4", "odd_walks", "loops_alone", "loops_shared", "dead_ends", "stale_gadget", "tied_parents", "parallel_edges",
         "zero_ring")


@BOTH
@pytest.mark.parametrize("name", SMALL)
def test_small_fixtures(name, double):
    fx, bounds = M.gpu_fixtures(double)[name]
    wants = check_all_forms(fx, bounds, name)
    assert any(ok.any() for _, ok, *_ in wants.values()) and any(not ok.all() for _, ok, *_ in wants.values()), name


@BOTH
def test_the_bound_binds(double):
    fx = M.bound_binds(double)
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)
    for (lo, K), (value, h) in M.BOUND_BINDS_EXPECTED.items():
        out, ok = dev.cheapest_walk_length(rs[:1], rd[:1], lo, K)
        got = dev.cheapest_walk(rs[:1], rd[:1], lo, K)[0]
        assert ok[0] and out[0] == value and len(got) == 2 * h + 1, (lo, K, out, got)
    assert dev.cheapest_walk(rs[:1], rd[:1], 2, 3)[0][::2] == [0, 4, 5, 3]
    within, wok = dev.cheapest_path_length_within(rs[:1], rd[:1], 3)
    assert wok[0] and within[0] == 1  # what a filter around the _within call would start from
    dev.close()


@BOTH
def test_the_reset(double):
    fx = M.path4(double)
    dev = device(fx)
    out, ok = dev.cheapest_walk_length(fx[5], fx[6], 2, 3)
    assert ok.tolist() == [False, True, True, True, False, False]
    assert dev.cheapest_walk(fx[5], fx[6], 2, 3)[0] is None
    dev.close()
    fx = M.odd_walks(double)
    dev = device(fx)
    assert not dev.cheapest_walk_length(fx[5], fx[6], 2, 2)[1][0]
    assert dev.cheapest_walk(fx[5], fx[6], 2, 3)[0][::2] == [0, 1, 2, 1]
    dev.close()


@BOTH
def test_dead_end_rows_are_null_not_zero(double):
    fx = M.dead_ends(double)
    dev = device(fx)
    for lo in (1, 2):
        assert dev.cheapest_walk_length(fx[5], fx[6], lo, 4)[1].tolist() == [False, False, False, True, True, True]
        assert [p is not None for p in dev.cheapest_walk(fx[5], fx[6], lo, 4)] == [False, False, False, True, True, True]
    out, ok = dev.cheapest_walk_length(fx[5], fx[6], 0, 4)
    assert ok.all() and (bits(out)[:4] == 0).all()  # lo == 0: the empty walk, +0.0
    assert dev.cheapest_walk(fx[5], fx[6], 0, 4)[:3] == [[2], [3], [4]]
    dev.close()


# ---- 2. lanes and batches, long lists, round groups ---------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("m", M.SOURCES)
def test_many_sources(m, double):
    fx, bounds = M.gpu_fixtures(double)["sources_%d" % m]
    pgq.reset_stats()
    dev = device(fx)
    dev.cheapest_walk_length(fx[5], fx[6], 2, 3)
    assert pgq.get_stats()["batches"] == (m + 63) // 64
    wants = check_all_forms(fx, bounds, "%d sources" % m, dev)
    dev.close()
    assert wants[(2, 3)][1][:m].all() and wants[(3, 4)][1][m]  # every source reaches m + 2 in three edges; (0, 0) closes in four


@BOTH
@pytest.mark.parametrize("n", M.OUT_LIST)
def test_long_out_lists(n, double):
    fx, bounds = M.gpu_fixtures(double)["out_list_%d" % n]
    want = check_all_forms(fx, bounds, "out-list of %d" % n)[(2, 3)]
    assert want[3][0][-2:] == [1001 + n, 3]  # the tight slot is the last of n


@BOTH
@pytest.mark.parametrize("n", M.IN_LIST)
def test_long_in_lists(n, double):
    fx, bounds = M.gpu_fixtures(double)["in_list_%d" % n]
    want = check_all_forms(fx, bounds, "in-list of %d" % n)[(2, 3)]
    assert want[3][0][-3:] == [n, 1000 + 2 * n, n + 2]  # the parent in the last position of the in-list, past the smaller decoys


def levels_of(call):
    pgq.reset_stats()
    call()
    return pgq.get_stats()["levels"]


@BOTH
def test_round_groups_and_levels(double):
    fx = M.chain(20, double)
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)
    check_all_forms(fx, M.CHAIN_BOUNDS, "chain of 20", dev)
    for lo, K in M.CHAIN_BOUNDS:  # one source: one batch, the model's rounds
        rounds = M.solve(V, off, adj, eid, w, rs, rd, lo, K)[4][0]
        assert levels_of(lambda: dev.cheapest_walk_length(rs, rd, lo, K)) == rounds, (lo, K)
        assert levels_of(lambda: dev.cheapest_walk(rs, rd, lo, K)) == rounds, (lo, K)
    dev.close()
    fx = M.ring(5, double)
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)
    check_all_forms(fx, M.RING_BOUNDS, "ring of 5", dev)
    for lo, K in [b for b in M.RING_BOUNDS if b[0] >= 1]:  # K stops the first two with the queue still full; lo == 0 is the _within call, whose K >= V - 1 takes other rounds
        rounds = M.solve(V, off, adj, eid, w, rs, rd, lo, K)[4][0]
        assert levels_of(lambda: dev.cheapest_walk_length(rs, rd, lo, K)) == rounds, (lo, K)
        assert levels_of(lambda: dev.cheapest_walk(rs, rd, lo, K)) == rounds, (lo, K)
    check_all_forms(M.chain(20, double), ((3, INT64_MAX),), "chain after the ring")  # nothing of the stopped batches is left behind
    dev.close()


# ---- 3. arithmetic ----------------------------------------------------------------------------------------------------------------
def test_absorbed_sum_with_a_lower_bound():
    fx, bounds = M.gpu_fixtures(True)["absorbed_shortcut"]
    wants = check_all_forms(fx, bounds, "2^53")
    assert wants[(2, 3)][3][0][::2] == [0, 2, 3] and wants[(3, 3)][3][0][::2] == [0, 1, 2, 3]
    assert wants[(2, 3)][0][0] == wants[(3, 3)][0][0] == 2.0 ** 53


def test_int64_sums_that_reach_inf():
    fx, bounds = M.gpu_fixtures(False)["near_inf"]
    wants = check_all_forms(fx, bounds, "near INF")
    assert wants[(2, 2)][0][0] == M.inf_of(fx[4]) - 1 and not wants[(2, 2)][1][1]


_MODEL = {}


def model_of(kind, fx, lo, K):
    """The model's answer for a random case, computed once."""
    if (kind, lo, K) not in _MODEL:
        _MODEL[(kind, lo, K)] = M.solve(*fx, lo, K)
    return _MODEL[(kind, lo, K)]


@pytest.fixture(scope="module", params=W.RANDOM_WEIGHTS[:4])
def random_case(request):
    V, off, adj, w = W.random_graph(600, 3600, request.param)
    rs, rd = W.random_rows(V, scattered=120, group=8)
    eid = 1000 + np.arange(len(adj), dtype=np.int64)[::-1].copy()
    fx = (V, off, adj, eid, w, rs, rd)
    dev = device(fx)
    yield request.param, fx, dev
    dev.close()


RANDOM_BOUNDS = ((1, 3), (2, 4), (3, 3), (2, INT64_MAX))


def test_random_graphs_against_the_model(random_case):
    kind, fx, dev = random_case
    wants = check_all_forms(fx, RANDOM_BOUNDS, kind, dev, model=lambda lo, K: model_of(kind, fx, lo, K))
    assert wants[(2, 4)][1].sum() > 50 and (~wants[(3, 3)][1]).sum() > 5


# ---- 4. the identities, through the library alone ------------------------------------------------------------------------------
def test_identity_1_lo_zero_is_the_within_calls(random_case):
    kind, fx, dev = random_case
    V, off, adj, eid, w, rs, rd = fx
    for K in (0, 3, INT64_MAX):
        a, b = dev.cheapest_walk_length(rs, rd, 0, K), dev.cheapest_path_length_within(rs, rd, K)
        assert (a[1] == b[1]).all() and (bits(a[0]) == bits(b[0])).all()
        ra, rb = dev.cheapest_walk(rs, rd, 0, K, raw=True), dev.cheapest_path_within(rs, rd, K, raw=True)
        assert all(np.array_equal(x, y) for x, y in zip(ra, rb))  # offsets, lengths, validity words, payload


def test_identity_2_the_fold_of_the_list_is_the_value(random_case):
    kind, fx, dev = random_case
    V, off, adj, eid, w, rs, rd = fx
    for lo, K in RANDOM_BOUNDS:
        out, ok = dev.cheapest_walk_length(rs, rd, lo, K)
        got = dev.cheapest_walk(rs, rd, lo, K)
        assert [p is not None for p in got] == ok.tolist()
        assert all(lo <= len(p) // 2 <= K for p in got if p is not None)
        folds = np.array([P.fold(w, eid, p) if p is not None else 0 for p in got], dtype=w.dtype)
        assert (bits(folds)[ok] == bits(np.ascontiguousarray(out))[ok]).all()
        _, _, ln, _, _ = bulk_raw(dev, rs, rd, lo, K, 1 << 16)
        assert ln.tolist() == [-1 if p is None else len(p) // 2 for p in got]  # h is the bulk form's d_out_len


def test_identity_3_rows_the_bound_does_not_bind(random_case):
    kind, fx, dev = random_case
    V, off, adj, eid, w, rs, rd = fx
    free = 0
    for lo, K in RANDOM_BOUNDS:
        out, ok = dev.cheapest_walk_length(rs, rd, lo, K)
        got = dev.cheapest_walk(rs, rd, lo, K)
        w_out, w_ok = dev.cheapest_path_length_within(rs, rd, K)
        w_got = dev.cheapest_path_within(rs, rd, K)
        model = model_of(kind, fx, lo, K)[3]
        for i, p in enumerate(w_got):
            if p is not None and len(p) // 2 >= lo:
                assert ok[i] and bits(out[i:i + 1])[0] == bits(w_out[i:i + 1])[0]
                assert got[i] == (p if w.dtype.kind == "i" else model[i])  # doubles: an absorbed sum may differ; the model decides
                free += 1
    assert free > 50


@pytest.mark.parametrize("c", [1, 7])
def test_identity_4_unit_weights(c):
    V, off, adj, _ = W.random_graph(600, 3600, "int_ones")
    w = np.full(len(adj), c, dtype=np.int64)
    rs, rd = W.random_rows(V, scattered=120, group=8)
    eid = 1000 + np.arange(len(adj), dtype=np.int64)
    dev = pgq.DeviceCSR(V, off, adj, eid, w)
    for lo, K in ((0, 3), (1, 3), (2, 4), (3, 3), (5, 64)):
        out, ok = dev.cheapest_walk_length(rs, rd, lo, K)
        ln, lok = dev.walk_length(rs, rd, lo, K)
        assert (ok == lok).all() and (out[ok] == c * ln[lok]).all(), (lo, K)
        walks = dev.k_shortest_walks(rs, rd, lo, K, 1)
        assert dev.cheapest_walk(rs, rd, lo, K) == [None if x is None else x[0] for x in walks], (lo, K)
    dev.close()


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------------------
@BOTH
def test_null_rows_and_selection_vectors(double):
    fx = P.random_weighted(200, 1200, double, rows=40)
    V, off, adj, eid, w, rs, rd = fx
    out, ok, hops, lists, _ = M.solve(V, off, adj, eid, w, rs, rd, 2, 3)
    dev, st = device(fx), udf_state(fx)
    sv, dv = np.ones(len(rs), dtype=bool), np.ones(len(rs), dtype=bool)
    sv[3::7] = False
    dv[5::7] = False
    keep = sv & dv
    masked = [p if keep[i] else None for i, p in enumerate(lists)]
    want = (np.where(keep, out, 0).astype(w.dtype), ok & keep)
    same_values(dev.cheapest_walk_length(rs, rd, 2, 3, src_valid=sv, dst_valid=dv), want, "valid, chunk")
    same_values(st.cheapest_walk_length(0, V, rs, rd, 2, 3, src_valid=sv, dst_valid=dv), want, "valid, udf")
    assert dev.cheapest_walk(rs, rd, 2, 3, src_valid=sv, dst_valid=dv) == masked
    assert st.cheapest_walk(0, V, rs, rd, 2, 3, src_valid=sv, dst_valid=dv) == masked
    sel = np.array([7, 7, 0, 39, 12, 3, 12], dtype=np.uint32)
    same_values(dev.cheapest_walk_length(rs, rd, 2, 3, src_sel=sel, dst_sel=sel), (out[sel], ok[sel]), "sel, chunk")
    same_values(st.cheapest_walk_length(0, V, rs, rd, 2, 3, src_sel=sel, dst_sel=sel), (out[sel], ok[sel]), "sel, udf")
    assert dev.cheapest_walk(rs, rd, 2, 3, src_sel=sel, dst_sel=sel) == [lists[i] for i in sel]
    assert st.cheapest_walk(0, V, rs, rd, 2, 3, src_sel=sel, dst_sel=sel) == [lists[i] for i in sel]
    brs, brd = rs.copy(), rd.copy()  # bulk form: a negative src is a NULL row
    brs[4::9] = -1
    brd[6::9] = brs[6::9]
    bwant = M.solve(V, off, adj, eid, w, brs, brd, 2, 3)
    same_values(bulk_length(dev, w, brs, brd, 2, 3), bwant, "NULL rows, bulk")
    assert bulk_lists(dev, brs, brd, 2, 3, bwant[3], bwant[2]) == bwant[3]
    assert dev.cheapest_walk(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 2, 3) == []
    assert len(dev.cheapest_walk_length(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 2, 3)[0]) == 0
    dev.close()


@pytest.mark.parametrize("streams", [1, 3])
def test_worker_streams(streams):
    fx, _ = M.gpu_fixtures(False)["sources_129"]
    V, off, adj, eid, w, rs, rd = fx
    pgq.set_option("relax_streams", streams)
    dev = device(fx)
    for lo, K in ((2, 3), (3, 4), (1, INT64_MAX)):
        same_values(dev.cheapest_walk_length(rs, rd, lo, K), M.solve(V, off, adj, eid, w, rs, rd, lo, K), "%d streams" % streams)
    dev.close()


def test_child_capacity(random_case):
    kind, fx, dev = random_case
    V, off, adj, eid, w, rs, rd = fx
    want = model_of(kind, fx, 2, 4)
    need = sum(len(p) for p in want[3] if p is not None)
    rc, used, ln, _, _ = bulk_raw(dev, rs, rd, 2, 4, need - 1)
    assert rc == -4 and used == need, (rc, used, need)  # PGQ_ERR_INVALID_ARG, and what to provide
    assert ln.tolist() == want[2]
    rc, used, ln, o, child = bulk_raw(dev, rs, rd, 2, 4, used)
    assert rc == 0 and used == need
    assert [None if ln[i] < 0 else child[o[i]:o[i] + 2 * ln[i] + 1].tolist() for i in range(len(rs))] == want[3]


def status(call):
    try:
        call()
    except PgqError as e:
        return int(re.search(r"error (-?\d+)", str(e)).group(1))
    return 0


def test_errors_and_a_failed_call_writes_nothing():
    import torch
    fx = P.diamond(False)
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)
    st = udf_state(fx)
    for lo, K, code in ((-1, 3, -4), (3, 2, -4), (65, 70, -6), (65, INT64_MAX, -6), (-1, -1, -4)):
        assert status(lambda: dev.cheapest_walk_length(rs, rd, lo, K)) == code, (lo, K)
        assert status(lambda: dev.cheapest_walk(rs, rd, lo, K)) == code, (lo, K)
        rc, used, ln, o, child = bulk_raw(dev, rs, rd, lo, K, 64)
        assert rc == code and used == 0 and (ln == -7).all() and (o == -7).all() and (child == -7).all()
        n = len(rs)
        t_s, t_d = torch.from_numpy(rs).cuda(), torch.from_numpy(rd).cuda()
        t_out = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        t_ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        assert status(lambda: dev.cheapest_walk_length_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, K, t_out.data_ptr(), t_ok.data_ptr())) == code
        assert (t_out.cpu().numpy() == -7).all() and (t_ok.cpu().numpy() == 9).all()
        with pytest.raises(PgqError):
            st.cheapest_walk_length(0, V, rs, rd, lo, K)
        with pytest.raises(PgqError):
            st.cheapest_walk(0, V, rs, rd, lo, K)
    assert status(lambda: dev.cheapest_walk_length(rs, rd, 64, 64)) == 0  # PGQ_WALK_MAX_HOPS itself is served
    for bad_s, bad_d in (([V], [0]), ([0], [V])):
        bs, bd = np.array(bad_s, dtype=np.int64), np.array(bad_d, dtype=np.int64)
        assert status(lambda: dev.cheapest_walk_length(bs, bd, 1, 2)) == status(lambda: dev.cheapest_path_length_within(bs, bd, 2)) == -4
        assert status(lambda: dev.cheapest_walk(bs, bd, 1, 2)) == -4
    other = pgq.DeviceCSR(V + 1, np.append(off, off[-1]), adj, eid, w)
    L = pgq.load_hip()  # a V that does not match the handle's
    keep = []
    sv, dv, n = dev._vecs(rs, rd, None, None, None, None, keep)
    out, ov = np.full(n, -7, dtype=np.int64), np.zeros(2, dtype=np.uint64)
    assert L.pgq_cheapest_walk_length(other.h, V, n, sv, dv, 1, 2, out.ctypes.data, ov.ctypes.data) == -4 and (out == -7).all()
    other.close()
    want = M.solve(V, off, adj, eid, w, rs, rd, 1, 2)  # the handle works on after the refused calls
    same_values(dev.cheapest_walk_length(rs, rd, 1, 2), want, "after the errors")
    assert dev.cheapest_walk(rs, rd, 1, 2) == want[3]
    dev.close()
    plain = pgq.DeviceCSR(V, off, adj, eid, None)
    assert status(lambda: plain.cheapest_walk_length(rs, rd, 1, 2)) == status(lambda: plain.cheapest_path_length(rs, rd)) == -5
    assert status(lambda: plain.cheapest_walk(rs, rd, 1, 2)) == -5
    plain.close()
    neg = pgq.DeviceCSR(V, off, adj, eid, -w)
    assert status(lambda: neg.cheapest_walk_length(rs, rd, 1, 2)) == status(lambda: neg.cheapest_path_length(rs, rd)) == -6
    assert status(lambda: neg.cheapest_walk(rs, rd, 1, 2)) == -6
    neg.close()


# ---- 6. the neighbours are left as they were -------------------------------------------------------------------------------------
@BOTH
def test_no_side_effect_on_the_other_calls(double):
    fx = P.random_weighted(200, 1200, double)
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)

    def others():
        a, b = dev.cheapest_path_length(rs, rd), dev.cheapest_path_length_within(rs, rd, 3)
        ln, lok = dev.walk_length(rs, rd, 1, 3)
        return ([bits(a[0]).tolist(), a[1].tolist(), bits(b[0]).tolist(), b[1].tolist(), ln.tolist(), lok.tolist()],
                dev.cheapest_path(rs, rd), dev.cheapest_path_within(rs, rd, 3))

    before = others()
    want = M.solve(V, off, adj, eid, w, rs, rd, 2, 4)
    same_values(dev.cheapest_walk_length(rs, rd, 2, 4), want, "first call")
    assert dev.cheapest_walk(rs, rd, 2, 4) == want[3]
    assert others() == before
    dev.cheapest_walk_length(rs, rd, 2, 2)  # stopped at the bound, the queues still full
    dev.cheapest_walk(rs, rd, 2, 2)
    assert others() == before
    need = sum(len(p) for p in want[3] if p is not None)
    assert bulk_raw(dev, rs, rd, 2, 4, need - 1)[0] == -4  # a call that failed behind its rounds
    assert status(lambda: dev.cheapest_walk_length(rs, rd, 3, 2)) == -4  # and one that failed before them
    assert others() == before
    same_values(dev.cheapest_walk_length(rs, rd, 2, 4), want, "again")
    assert dev.cheapest_walk(rs, rd, 2, 4) == want[3]
    dev.close()
