"""cheapest_path on the GPU: the cheapest path itself as a list, in every entry form (bulk, chunk, UDF), against the Python
model of its contract (cheapest_path_model.py — checked on the CPU against a brute-force enumeration, the oracle's
cheapest_path_length and, for unit weights, its shortestpath; the fixtures used here catch its mutants there).  Every
comparison is exact: whole lists, lengths, offsets and payload sizes."""
import re

import numpy as np
import pytest

import cheapest_path_model as M
import duckpgq_extension_amd as pgq
from cheapest_within_model import bits
from duckpgq_extension_amd.binding import PgqError

pytestmark = pytest.mark.gpu

# every option these calls depend on, at the value a test starts from (another file may have left its own); SHIPPED: the
# library's own value, read from it
SHIPPED = ("chain_cap", "relax_light", "relax_light_div", "relax_light_min_degree", "relax_labels32", "relax_split",
           "relax_small_limit", "chain", "wbibfs")
KEYS = {"streams": 1, "relax_streams": 0, "relax_delta_div": 0, "relax_bidir": 0}
BOTH = pytest.mark.parametrize("double", [False, True], ids=["int64", "double"])


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


def want_of(fx):
    V, off, adj, eid, w, rs, rd = fx
    return M.cheapest_paths(V, off, adj, eid, w, rs, rd)


def bulk_raw(dev, rs, rd, cap):
    """(rc, child_used, lengths, offsets, child) of the bulk form with a child buffer of `cap` elements."""
    import torch
    n = len(rs)
    t_s, t_d = torch.from_numpy(np.ascontiguousarray(rs)).cuda(), torch.from_numpy(np.ascontiguousarray(rd)).cuda()
    t_len = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    t_off = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    t_child = torch.full((max(cap, 1),), -7, dtype=torch.int64, device="cuda")
    rc, used = dev.cheapest_path_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), t_len.data_ptr(), t_off.data_ptr(), t_child.data_ptr(), cap)
    return rc, used, t_len.cpu().numpy(), t_off.cpu().numpy(), t_child.cpu().numpy()


def bulk(dev, rs, rd, want):
    """The bulk form's lists from a buffer of exactly the size the expected lists need; lengths, offsets and payload checked."""
    need = sum(len(p) for p in want if p is not None)
    rc, used, ln, off, child = bulk_raw(dev, rs, rd, need)
    assert rc == 0 and used == need, (rc, used, need)
    assert ln.tolist() == [-1 if p is None else len(p) // 2 for p in want]
    valid = ln >= 0
    assert (off[valid] == (np.cumsum(np.where(valid, 2 * ln + 1, 0)) - np.where(valid, 2 * ln + 1, 0))[valid]).all()  # packed in row order
    return [None if ln[i] < 0 else child[off[i]:off[i] + 2 * ln[i] + 1].tolist() for i in range(len(rs))]


def udf_state(fx):
    V, off, adj, eid, w = fx[:5]
    st = pgq.PgqState()
    st.build_csr(0, V, M.slot_sources(V, off), adj, eid, w)
    return st


def check_all_forms(fx, what):
    """Bulk, chunk and UDF form of one fixture against the model; returns the expected lists."""
    V, off, adj, eid, w, rs, rd = fx
    want = want_of(fx)
    dev = device(fx)
    try:
        for form, got in (("bulk", bulk(dev, rs, rd, want)), ("chunk", dev.cheapest_path(rs, rd)),
                          ("udf", udf_state(fx).cheapest_path(0, V, rs, rd))):
            bad = [i for i in range(len(rs)) if got[i] != want[i]]
            assert not bad, "%s, %s form: %d of %d rows differ, first: %d -> %d got %r, expected %r" % (
                what, form, len(bad), len(rs), rs[bad[0]], rd[bad[0]], got[bad[0]], want[bad[0]])
    finally:
        dev.close()
    return want


# ---- 1. the small fixtures: one property of the contract each --------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("name", ["diamond", "tied_parents", "parallel_edges", "zero_ring"])
def test_small_fixtures(name, double):
    want = check_all_forms(getattr(M, name)(double), name)
    assert want[0] is not None and len(want[0]) >= 3


def test_absorbed_cycle():
    want = check_all_forms(M.absorption(), "absorption")
    assert want[0] == [3, 1000, 0, 1001, 2, 1002, 1]


@BOTH
@pytest.mark.parametrize("n", [64, 65, 128, 129])
def test_long_in_list(n, double):
    want = check_all_forms(M.long_in_list(n, double), "in-list of %d" % n)
    assert want[0][-3:] == [n, 1000 + 2 * n, n + 2]  # the parent in the last slot of the in-list, past the smaller decoys


@BOTH
def test_long_chain(double):
    fx = M.long_chain(300, double)
    want = check_all_forms(fx, "chain of 300")
    assert want[0] == [x for v in range(299) for x in (v, 1000 + v)] + [299] and want[2] is None and want[3] == [17]


# ---- 2. lanes and batches ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lanes_graph():
    fx = M.random_weighted(500, 3000, False, seed=3, rows=1)
    return fx, device(fx)


@pytest.mark.parametrize("U", [63, 64, 65, 129])
def test_source_counts(lanes_graph, U):
    (V, off, adj, eid, w, _, _), dev = lanes_graph
    rng = np.random.default_rng(U)
    rs = np.repeat(rng.choice(V, U, replace=False), 3).astype(np.int64)
    rd = (rs + 1 + rng.integers(0, V - 1, len(rs))) % V  # never the source itself: every source needs a lane
    perm = rng.permutation(len(rs))
    rs, rd = rs[perm], rd[perm]
    want = M.cheapest_paths(V, off, adj, eid, w, rs, rd)
    assert sum(p is not None for p in want) > U
    pgq.reset_stats()
    got = bulk(dev, rs, rd, want)
    assert pgq.get_stats()["batches"] == (U + 63) // 64
    assert got == want
    assert dev.cheapest_path(rs, rd) == want


# ---- 3. random graphs: ties everywhere -------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["int64", "double"])
def random_case(request):
    fx = M.random_weighted(200, 1200, request.param)
    return fx, want_of(fx)


def test_random_weighted(random_case):
    fx, want = random_case
    assert check_all_forms(fx, "random, weights 0..3") == want
    assert sum(p is not None and len(p) > 5 for p in want) > 100


def test_rounds_through_k_relax(random_case):
    """With few changed vertices the labels settle inside k_relax_small (every graph of this file is that small); with its
    limit at 0 every round is a k_relax launch under the lifted lane bounds, and the out-list of 129 goes to the heavy pass."""
    fx, want = random_case
    pgq.set_option("relax_small_limit", 0)
    double = fx[4].dtype.kind == "f"
    assert check_all_forms(fx, "random, weights 0..3, k_relax rounds") == want
    for name, other in (("zero ring", M.zero_ring(double)), ("in-list of 129", M.long_in_list(129, double)), ("chain of 300", M.long_chain(300, double))):
        check_all_forms(other, name + ", k_relax rounds")
    pgq.reset_stats()
    dev = device(fx)
    assert dev.cheapest_path(fx[5], fx[6]) == want
    dev.close()
    assert pgq.get_stats()["launches"]["relax"] > 0 and pgq.get_stats()["launches"]["push"] > 0 and pgq.get_stats()["launches"]["recon"] > 0


def test_fold_of_returned_edges_is_the_length(random_case):
    fx, _ = random_case
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)
    out, ok = dev.cheapest_path_length(rs, rd)
    got = dev.cheapest_path(rs, rd)
    dev.close()
    assert [p is not None for p in got] == ok.tolist()
    folds = np.array([M.fold(w, eid, p) if p is not None else 0 for p in got], dtype=w.dtype)
    assert (bits(folds)[ok] == bits(out)[ok]).all()


def test_unit_weights_give_shortestpath():
    fx = M.random_weighted(200, 1200, False, unit=True)
    V, off, adj, eid, w, rs, rd = fx
    want = check_all_forms(fx, "random, unit weights")
    dev = device(fx)
    assert dev.shortestpath(rs, rd) == want
    dev.close()


# ---- 4. special rows, in the forms that have them ---------------------------------------------------------------------------
@BOTH
def test_special_rows(double):
    fx = M.random_weighted(200, 1200, double, rows=40)
    V, off, adj, eid, w, rs, rd = fx
    want = want_of(fx)
    dev = device(fx)
    # NULL src and NULL dst through validity masks; the row stays NULL whatever its ids say
    sv, dv = np.ones(len(rs), dtype=bool), np.ones(len(rs), dtype=bool)
    sv[3::7] = False
    dv[5::7] = False
    masked = [p if sv[i] and dv[i] else None for i, p in enumerate(want)]
    assert dev.cheapest_path(rs, rd, src_valid=sv, dst_valid=dv) == masked
    assert udf_state(fx).cheapest_path(0, V, rs, rd, src_valid=sv, dst_valid=dv) == masked
    # selection vectors: rows picked, repeated and reordered
    sel = np.array([7, 7, 0, 39, 12, 3, 12], dtype=np.uint32)
    assert dev.cheapest_path(rs, rd, src_sel=sel, dst_sel=sel) == [want[i] for i in sel]
    # the raw LIST vector: NULL rows keep entry {0, 0} and take no payload
    o, ln, ov, child = dev.cheapest_path(rs, rd, src_valid=sv, dst_valid=dv, raw=True)
    for i, p in enumerate(masked):
        if p is None:
            assert o[i] == 0 and ln[i] == 0 and not (int(ov[i >> 6]) >> (i & 63)) & 1
        else:
            assert child[int(o[i]):int(o[i]) + int(ln[i])].tolist() == p
    assert len(child) == sum(len(p) for p in masked if p is not None)
    # bulk form: a negative src is a NULL row; src == dst is [src]; an unreachable dst is NULL
    brs, brd = rs.copy(), rd.copy()
    brs[4::9] = -1
    brd[6::9] = brs[6::9]
    bwant = M.cheapest_paths(V, off, adj, eid, w, brs, brd)
    assert bulk(dev, brs, brd, bwant) == bwant
    assert any(p is None and s >= 0 for p, s in zip(bwant, brs)) and any(p is not None and len(p) == 1 for p in bwant)
    assert dev.cheapest_path([], []) == []
    dev.close()


# ---- 5. the child-capacity protocol -------------------------------------------------------------------------------------------
def test_child_capacity(random_case):
    fx, want = random_case
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)
    need = sum(len(p) for p in want if p is not None)
    lens = [-1 if p is None else len(p) // 2 for p in want]
    for cap in (0, need // 2, need - 1):
        rc, used, ln, _, _ = bulk_raw(dev, rs, rd, cap)
        assert rc == -4 and used == need, (cap, rc, used, need)  # PGQ_ERR_INVALID_ARG, and what to provide
        assert ln.tolist() == lens
    rc, used, ln, o, child = bulk_raw(dev, rs, rd, need + 5)
    assert rc == 0 and used == need and (child[need:] == -7).all()  # nothing written past the lists
    dev.close()


# ---- 6. errors: the length call's ---------------------------------------------------------------------------------------------
def status(call):
    try:
        call()
    except PgqError as e:
        return int(re.search(r"error (-?\d+)", str(e)).group(1))
    return 0


def test_errors_are_the_length_calls():
    V, off, adj, eid, w, rs, rd = M.diamond(False)
    plain = pgq.DeviceCSR(V, off, adj, eid, None)
    assert status(lambda: plain.cheapest_path(rs, rd)) == status(lambda: plain.cheapest_path_length(rs, rd)) == -5
    plain.close()
    neg = pgq.DeviceCSR(V, off, adj, eid, -w)
    assert status(lambda: neg.cheapest_path(rs, rd)) == status(lambda: neg.cheapest_path_length(rs, rd)) == -6
    neg.close()
    dev = device(M.diamond(False))
    for bad_s, bad_d in (([V], [0]), ([0], [V]), ([0], [-1])):
        bs, bd = np.array(bad_s, dtype=np.int64), np.array(bad_d, dtype=np.int64)
        assert status(lambda: dev.cheapest_path(bs, bd)) == status(lambda: dev.cheapest_path_length(bs, bd)) == -4
        import torch
        t_ok = torch.zeros(1, dtype=torch.uint8, device="cuda")
        t_out = torch.zeros(1, dtype=torch.int64, device="cuda")
        t_s, t_d = torch.from_numpy(bs).cuda(), torch.from_numpy(bd).cuda()
        assert bulk_raw(dev, bs, bd, 16)[0] == -4
        assert status(lambda: dev.cheapest_bulk_ptr(1, t_s.data_ptr(), t_d.data_ptr(), t_out.data_ptr(), t_ok.data_ptr())) == -4
    assert dev.cheapest_path(rs, rd) == want_of(M.diamond(False))  # the handle works on after the refused calls
    dev.close()


# ---- 7. the shared relaxation state is left clean -------------------------------------------------------------------------------
@BOTH
def test_no_side_effect_on_the_length_call(double):
    fx = M.random_weighted(200, 1200, double)
    V, off, adj, eid, w, rs, rd = fx
    dev = device(fx)
    for chain, light in ((1, 1), (0, 0), (0, 2)):  # the shipped route; plain rounds on the same label arrays; light edges first
        pgq.set_option("chain", chain)
        pgq.set_option("relax_light", light)
        before = dev.cheapest_path_length(rs, rd)
        first = dev.cheapest_path(rs, rd)
        after = dev.cheapest_path_length(rs, rd)
        assert (before[1] == after[1]).all() and (bits(before[0]) == bits(after[0])).all(), (chain, light)
        assert dev.cheapest_path(rs, rd) == first  # ... and its own second call finds its state as the first did
    dev.close()
