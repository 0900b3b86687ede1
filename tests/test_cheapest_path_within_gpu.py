"""cheapest_path_within on the GPU: the cheapest walk of at most max_hops edges as a list, in every entry form (bulk, chunk,
UDF), against the Python model of its contract (cheapest_path_within_model.py — checked on the CPU against a brute-force
enumeration of walks, the model of cheapest_path_length_within and the oracle's shortestpath; the fixtures used here catch its
mutants there).  Every comparison is exact: whole lists, lengths, offsets and payload sizes."""
import re

import numpy as np
import pytest

import cheapest_path_model as P
import cheapest_path_within_model as M
import cheapest_within_model as W
import duckpgq_extension_amd as pgq
from cheapest_within_model import bits
from duckpgq_extension_amd.binding import PgqError

pytestmark = pytest.mark.gpu

SHIPPED = ("chain_cap", "relax_light", "relax_light_div", "relax_light_min_degree", "relax_labels32", "relax_split",
           "relax_small_limit", "relax_bidir_rows", "chain", "wbibfs")
KEYS = {"streams": 1, "relax_streams": 0, "relax_delta_div": 0, "relax_bidir": 0}
BOTH = pytest.mark.parametrize("double", [False, True], ids=["int64", "double"])
INT64_MAX = int(np.iinfo(np.int64).max)


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


def want_of(fx, K):
    V, off, adj, eid, w, rs, rd = fx
    return M.bounded_paths(V, off, adj, eid, w, rs, rd, K)


def bulk_raw(dev, rs, rd, K, cap):
    """(rc, child_used, lengths, offsets, child) of the bulk form with a child buffer of `cap` elements."""
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    t_len = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    t_off = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    t_child = torch.full((max(cap, 1),), -7, dtype=torch.int64, device="cuda")
    rc, used = dev.cheapest_path_within_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), K, t_len.data_ptr(), t_off.data_ptr(), t_child.data_ptr(), cap)
    return rc, used, t_len.cpu().numpy(), t_off.cpu().numpy(), t_child.cpu().numpy()


def bulk(dev, rs, rd, K, want):
    """The bulk form's lists from a buffer of exactly the size the expected lists need; lengths, offsets and payload checked."""
    need = sum(len(p) for p in want if p is not None)
    rc, used, ln, off, child = bulk_raw(dev, rs, rd, K, need)
    assert rc == 0 and used == need, (rc, used, need)
    assert ln.tolist() == [-1 if p is None else len(p) // 2 for p in want]
    valid = ln >= 0
    assert (off[valid] == (np.cumsum(np.where(valid, 2 * ln + 1, 0)) - np.where(valid, 2 * ln + 1, 0))[valid]).all()  # packed in row order
    return [None if ln[i] < 0 else child[off[i]:off[i] + 2 * ln[i] + 1].tolist() for i in range(len(rs))]


def udf_state(fx):
    V, off, adj, eid, w = fx[:5]
    st = pgq.PgqState()
    st.build_csr(0, V, P.slot_sources(V, off), adj, eid, w)
    return st


def same(got, want, rs, rd, what):
    bad = [i for i in range(len(rs)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d rows differ, first: %d -> %d got %r, expected %r" % (
        what, len(bad), len(rs), rs[bad[0]], rd[bad[0]], got[bad[0]], want[bad[0]])


def check_all_forms(fx, Ks, what, dev=None):
    """Bulk, chunk and UDF form of one fixture against the model for every K of Ks; returns {K: the expected lists}."""
    V, off, adj, eid, w, rs, rd = fx
    own = dev is None
    dev = dev or device(fx)
    st = udf_state(fx)
    wants = {}
    try:
        for K in Ks:
            want = wants[K] = want_of(fx, K)
            same(bulk(dev, rs, rd, K, want), want, rs, rd, "%s, K = %d, bulk form" % (what, K))
            same(dev.cheapest_path_within(rs, rd, K), want, rs, rd, "%s, K = %d, chunk form" % (what, K))
            same(st.cheapest_path_within(0, V, rs, rd, K), want, rs, rd, "%s, K = %d, udf form" % (what, K))
    finally:
        if own:
            dev.close()
    return wants


def all_ks(V):
    return [0, 1, 2, 3, V - 1, INT64_MAX]


# ---- 1. the small fixtures: one property of the contract each --------------------------------------------------------------
def small(double):
    fx = dict(P.small_fixtures(double), long_out_list_65=M.long_out_list(65, double))
    if double:
        fx["absorbed_shortcut"] = M.absorbed_shortcut()
    return fx


@BOTH
def test_small_fixtures(double):
    for name, fx in small(double).items():
        wants = check_all_forms(fx, all_ks(fx[0]), name)
        assert any(p is not None and len(p) >= 3 for p in wants[INT64_MAX]), name


@BOTH
def test_special_rows(double):
    fx = P.random_weighted(200, 1200, double, rows=40)
    V, off, adj, eid, w, rs, rd = fx
    want = want_of(fx, 3)
    dev = device(fx)
    sv, dv = np.ones(len(rs), dtype=bool), np.ones(len(rs), dtype=bool)
    sv[3::7] = False
    dv[5::7] = False
    masked = [p if sv[i] and dv[i] else None for i, p in enumerate(want)]
    assert dev.cheapest_path_within(rs, rd, 3, src_valid=sv, dst_valid=dv) == masked
    assert udf_state(fx).cheapest_path_within(0, V, rs, rd, 3, src_valid=sv, dst_valid=dv) == masked
    sel = np.array([7, 7, 0, 39, 12, 3, 12], dtype=np.uint32)
    assert dev.cheapest_path_within(rs, rd, 3, src_sel=sel, dst_sel=sel) == [want[i] for i in sel]
    assert udf_state(fx).cheapest_path_within(0, V, rs, rd, 3, src_sel=sel, dst_sel=sel) == [want[i] for i in sel]
    o, ln, ov, child = dev.cheapest_path_within(rs, rd, 3, src_valid=sv, dst_valid=dv, raw=True)
    for i, p in enumerate(masked):
        if p is None:
            assert o[i] == 0 and ln[i] == 0 and not (int(ov[i >> 6]) >> (i & 63)) & 1
        else:
            assert child[int(o[i]):int(o[i]) + int(ln[i])].tolist() == p
    assert len(child) == sum(len(p) for p in masked if p is not None)
    brs, brd = rs.copy(), rd.copy()  # bulk form: a negative src is a NULL row; src == dst is [src], also at K = 0
    brs[4::9] = -1
    brd[6::9] = brs[6::9]
    for K in (0, 3):
        bwant = M.bounded_paths(V, off, adj, eid, w, brs, brd, K)
        assert bulk(dev, brs, brd, K, bwant) == bwant
        assert any(p is None and s >= 0 for p, s in zip(bwant, brs)) and any(p is not None and len(p) == 1 for p in bwant)
    assert dev.cheapest_path_within([], [], 3) == []
    dev.close()


@BOTH
def test_shortcut_path_changes_with_every_bound(double):
    fx = M.shortcut_path(double)
    wants = check_all_forms(fx, range(7), "shortcut path")
    assert len({tuple(wants[K][0] or ()) for K in range(7)}) == 7
    assert wants[3][0] == [0, 1008, 4, 1004, 5, 1005, 6]  # vertices 4, 5, 6 were improved again in later rounds


def test_absorbed_shortcut_beside_cheapest_path():
    fx = M.absorbed_shortcut()
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)
    assert dev.cheapest_path_within(rs, rd, INT64_MAX) == [[0, 1000, 2, 1003, 3], [0, 1001, 1, 1002, 2]]
    assert dev.cheapest_path(rs, rd) == [[0, 1001, 1, 1002, 2, 1003, 3], [0, 1001, 1, 1002, 2]]  # documented: the two differ
    dev.close()


# ---- 2. long lists, lane batches, round groups ---------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("n", [64, 65, 128, 129])
def test_long_lists(n, double):
    want = check_all_forms(P.long_in_list(n, double), [3], "in-list of %d" % n)[3]
    assert want[0][-3:] == [n, 1000 + 2 * n, n + 2]  # the parent in the last slot of the in-list, past the smaller decoys
    want = check_all_forms(M.long_out_list(n, double), [3], "out-list of %d" % n)[3]
    assert want[0][-2:] == [1001 + n, 3]  # the tight slot is the last of n


@pytest.mark.parametrize("m", [63, 64, 65, 129])
def test_many_sources(m):
    fx = M.many_sources(m, False)
    pgq.reset_stats()
    dev = device(fx)
    want = want_of(fx, 3)
    same(bulk(dev, fx[5], fx[6], 3, want), want, fx[5], fx[6], "%d sources" % m)
    assert pgq.get_stats()["batches"] == (m + 63) // 64
    check_all_forms(fx, [2, 3], "%d sources" % m, dev)
    dev.close()
    assert all(p is not None and len(p) == 7 for p in want[:m])


@BOTH
def test_directed_path_around_a_round_group(double):
    fx = M.directed_path(20, double)
    wants = check_all_forms(fx, [7, 8, 9, 19], "path of 20")
    for K in (7, 8, 9, 19):
        assert wants[K][K] is not None and len(wants[K][K]) == 2 * K + 1 and (K == 19 or wants[K][K + 1] is None)


def test_stops_at_the_bound():
    fx = M.directed_path(20, False)
    dev = device(fx)
    pgq.reset_stats()
    dev.cheapest_path_within(fx[5], fx[6], 3)
    stats = pgq.get_stats()
    dev.close()
    assert 0 < stats["levels"] <= 3 * stats["batches"], (stats["levels"], stats["batches"])
    assert stats["launches"]["relax"] > 0 and stats["launches"]["recon"] > 0


# ---- 3. random graphs: ties everywhere -------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["int64", "double"])
def random_case(request):
    fx = P.random_weighted(200, 1200, request.param)
    dev = device(fx)
    yield fx, dev, {K: want_of(fx, K) for K in (2, 3, 4)}
    dev.close()


def test_random_weighted(random_case):
    fx, dev, wants = random_case
    assert check_all_forms(fx, [2, 3, 4], "random, weights 0..3", dev) == wants
    assert sum(p is not None and len(p) > 3 for p in wants[3]) > 40 and sum(p is None for p in wants[3]) > 40


def test_double_special_weights():
    V, off, adj, w = W.random_graph(2000, 14000, "double_special")
    rs, rd = W.random_rows(V)
    eid = 1000 + np.arange(len(adj), dtype=np.int64)
    fx = (V, off, adj, eid, w, rs, rd)
    wants = check_all_forms(fx, [3], "double_special")
    assert sum(p is not None and len(p) > 3 for p in wants[3]) > 100


# ---- 4. consistency through the library ----------------------------------------------------------------------------------------
def test_fold_of_returned_edges_is_the_bounded_length(random_case):
    fx, dev, _ = random_case
    V, off, adj, eid, w, rs, rd = fx
    for K in (2, 3, 4):
        out, ok = dev.cheapest_path_length_within(rs, rd, K)
        got = dev.cheapest_path_within(rs, rd, K)
        assert [p is not None for p in got] == ok.tolist()
        assert all(len(p) // 2 <= K for p in got if p is not None)
        folds = np.array([M.fold(w, eid, p) if p is not None else 0 for p in got], dtype=w.dtype)
        assert (bits(folds)[ok] == bits(out)[ok]).all()


def test_a_large_bound_is_cheapest_path_for_int64_weights():
    fx = P.random_weighted(200, 1200, False)
    dev = device(fx)
    assert dev.cheapest_path_within(fx[5], fx[6], INT64_MAX) == dev.cheapest_path(fx[5], fx[6])
    dev.close()


def test_unit_weights_give_shortestpath_within():
    fx = P.random_weighted(200, 1200, False, unit=True)
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)
    for K in (1, 2, 3, 4):
        assert dev.cheapest_path_within(rs, rd, K) == dev.shortestpath_within(rs, rd, K), K
    dev.close()


# ---- 5. state left behind ----------------------------------------------------------------------------------------------------------
@BOTH
def test_no_side_effect_on_the_other_calls(double):
    fx = P.random_weighted(200, 1200, double)
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)

    def others():
        res = [dev.cheapest_path_length_within(rs, rd, 3), dev.cheapest_path_length(rs, rd)]
        for k, v in (("chain", 0), ("wbibfs", 0), ("relax_bidir", 1), ("relax_light", 2), ("relax_bidir_rows", 4)):
            pgq.set_option(k, v)
        res.append(dev.cheapest_path_length(rs, rd))  # the two-ended search, where the weights are int64
        for k in ("chain", "wbibfs", "relax_light", "relax_bidir_rows"):
            pgq.set_option(k, pgq.get_default_option(k))
        pgq.set_option("relax_bidir", 0)
        return res, dev.cheapest_path(rs, rd)

    before, path_before = others()
    first = dev.cheapest_path_within(rs, rd, 3)
    after, path_after = others()
    for (o0, k0), (o1, k1) in zip(before, after):
        assert (k0 == k1).all() and (bits(o0) == bits(o1)).all()
    assert path_before == path_after
    assert dev.cheapest_path_within(rs, rd, 3) == first == want_of(fx, 3)
    dev.close()


# ---- 6. the child-capacity protocol -------------------------------------------------------------------------------------------
def test_child_capacity(random_case):
    fx, dev, wants = random_case
    V, off, adj, eid, w, rs, rd = fx
    want = wants[3]
    need = sum(len(p) for p in want if p is not None)
    rc, used, ln, _, _ = bulk_raw(dev, rs, rd, 3, need - 1)
    assert rc == -4 and used == need, (rc, used, need)  # PGQ_ERR_INVALID_ARG, and what to provide
    assert ln.tolist() == [-1 if p is None else len(p) // 2 for p in want]
    rc, used, ln, o, child = bulk_raw(dev, rs, rd, 3, used)
    assert rc == 0 and used == need
    assert [None if ln[i] < 0 else child[o[i]:o[i] + 2 * ln[i] + 1].tolist() for i in range(len(rs))] == want


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------
def status(call):
    try:
        call()
    except PgqError as e:
        return int(re.search(r"error (-?\d+)", str(e)).group(1))
    return 0


def test_errors():
    V, off, adj, eid, w, rs, rd = P.diamond(False)
    dev = device(P.diamond(False))
    assert status(lambda: dev.cheapest_path_within(rs, rd, -1)) == -4
    assert bulk_raw(dev, rs, rd, -1, 64)[0] == -4
    with pytest.raises(PgqError):
        udf_state(P.diamond(False)).cheapest_path_within(0, V, rs, rd, -1)
    for bad_s, bad_d in (([V], [0]), ([0], [V])):
        bs, bd = np.array(bad_s, dtype=np.int64), np.array(bad_d, dtype=np.int64)
        assert status(lambda: dev.cheapest_path_within(bs, bd, 2)) == status(lambda: dev.cheapest_path_length(bs, bd)) == -4
    assert dev.cheapest_path_within(rs, rd, 2) == want_of(P.diamond(False), 2)  # the handle works on after the refused calls
    dev.close()
    plain = pgq.DeviceCSR(V, off, adj, eid, None)
    assert status(lambda: plain.cheapest_path_within(rs, rd, 2)) == status(lambda: plain.cheapest_path_length(rs, rd)) == -5
    plain.close()
    neg = pgq.DeviceCSR(V, off, adj, eid, -w)
    assert status(lambda: neg.cheapest_path_within(rs, rd, 2)) == status(lambda: neg.cheapest_path_length(rs, rd)) == -6
    neg.close()
