"""cheapest_walk_length / cheapest_walk without a GPU: the Python model (cheapest_walk_model.py) against a brute-force enumeration of
walks, against the _within models at lo = 0, against the identities of the contract, and the proof that the fixtures of
test_cheapest_walk_gpu.py tell every mutant from the model.  Then the layers: headers, glue, binding, documents, exported symbols."""
import os
import subprocess

import numpy as np
import pytest

import all_shortest_model as A
import cheapest_path_within_model as CPW
import cheapest_walk_model as M
import cheapest_within_model as CW
import k_walks_model as KW
import walk_length_model as WL
from cheapest_path_model import _fixture, fold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF_K = M.INT64_MAX


def tiny_graphs():
    """Graphs of at most 6 vertices with ties, zero weights, parallel edges and self-loops; int64 and double, one with absorption."""
    rng = np.random.default_rng(3)
    out = []
    for k in range(22):
        V = int(rng.integers(2, 7))
        E = int(rng.integers(2, 11))
        es, ed = rng.integers(0, V, E), rng.integers(0, V, E)
        ew = rng.integers(0, 4, E)
        rows = [(s, d) for s in range(V) for d in range(V)]
        out.append(_fixture(V, es, ed, ew * 0.25 if k % 2 else ew, rows, bool(k % 2)))
    out.append(_fixture(4, [0, 0, 1, 2, 3], [2, 1, 2, 3, 0], [1.0, 0.25, 0.25, 2.0 ** 53, 1.0], [(s, d) for s in range(4) for d in range(4)], True))
    return out


def test_the_model_is_the_brute_force_over_every_walk():
    checked = nulls = 0
    for V, off, adj, eid, w, rs, rd in tiny_graphs():
        for K in range(0, 6):
            for lo in range(0, K + 1):
                out, ok, hops, lists, _ = M.solve(V, off, adj, eid, w, rs, rd, lo, K)
                for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
                    want = M.brute_force(V, off, adj, eid, w, s, d, lo, K)
                    if want is None:
                        assert not ok[i] and lists[i] is None and hops[i] == -1, (s, d, lo, K)
                        nulls += 1
                        continue
                    assert ok[i] and CW.bits(out[i:i + 1])[0] == CW.bits(np.array([want[0]], dtype=w.dtype))[0], (s, d, lo, K)
                    assert hops[i] == want[1] and lists[i] == want[2], (s, d, lo, K, lists[i], want)
                    assert lo <= hops[i] <= K
                    assert CW.bits(np.array([fold(w, eid, lists[i])]))[0] == CW.bits(out[i:i + 1])[0]  # identity 2
                    checked += 1
    assert checked > 3000 and nulls > 1000


@pytest.mark.parametrize("kind", ["int_small", "double_special"])
def test_lo_zero_is_the_within_models(kind):
    V, off, adj, w = CW.random_graph(120, 700, kind)
    eid = 5000 + np.arange(len(adj), dtype=np.int64)[::-1].copy()
    rs, rd = CW.random_rows(V, scattered=80, group=6)
    for K in (0, 1, 3, INF_K):
        out, ok, hops, lists, _ = M.solve(V, off, adj, eid, w, rs, rd, 0, K)
        want_out, want_ok = CW.bounded_cheapest(V, off, adj, w, rs, rd, [min(K, V)])[min(K, V)]
        assert len(CW.differing(out, ok, want_out, want_ok)) == 0
        assert lists == CPW.bounded_paths(V, off, adj, eid, w, rs, rd, min(K, V))


@pytest.mark.parametrize("kind", ["int_small", "int_wide", "double_special"])
def test_identity_3_rows_the_lower_bound_does_not_bind(kind):
    V, off, adj, w = CW.random_graph(120, 500, kind)
    eid = np.arange(len(adj), dtype=np.int64)
    rs, rd = CW.random_rows(V, scattered=80, group=6)
    free = bound = 0
    for lo, K in ((1, 3), (2, 4), (3, 3), (2, INF_K)):
        out, ok, hops, lists, _ = M.solve(V, off, adj, eid, w, rs, rd, lo, K)
        w_out, w_ok, w_hops, w_lists, _ = M.solve(V, off, adj, eid, w, rs, rd, 0, K)
        for i in range(len(rs)):
            if w_ok[i] and w_hops[i] >= lo:
                assert ok[i] and CW.bits(out[i:i + 1])[0] == CW.bits(w_out[i:i + 1])[0]
                if w.dtype.kind == "i":
                    assert lists[i] == w_lists[i]
                free += 1
            elif ok[i]:
                assert hops[i] >= lo and (not w_ok[i] or out[i] >= w_out[i])
                bound += 1
    assert free > 50 and bound > 5  # (both kinds of row occur)


def test_identity_3_lists_can_differ_for_doubles():
    """0 -> 2 (1.0), 0 -> 1 (0.25), 1 -> 2 (0.25), 2 -> 3 (2^53), and 3 -> 3 (0.0) to let lo = 1 pass: the _within list of (0, 3) at
    K = 3 is [0, ., 2, ., 3] (h = 2, the bound 2 does not bind) and so is cheapest_walk's at {2,3}; at {3,3} the value is the same
    2^53 over ANOTHER list."""
    V, off, adj, eid, w, rs, rd = CPW.absorbed_shortcut()
    _, ok, hops, lists, _ = M.solve(V, off, adj, eid, w, rs, rd, 2, 3)
    out3, ok3, hops3, lists3, _ = M.solve(V, off, adj, eid, w, rs, rd, 3, 3)
    assert ok[0] and hops[0] == 2 and lists[0][::2] == [0, 2, 3]
    assert ok3[0] and hops3[0] == 3 and lists3[0][::2] == [0, 1, 2, 3] and out3[0] == 2.0 ** 53


@pytest.mark.parametrize("c", [1, 7])
def test_identity_4_unit_weights_are_walk_length_and_the_first_shortest_walk(c):
    V, off, adj, eid, rs, rd = WL.random_rows(V=60, E=200, rows=300)
    w = np.full(len(adj), c, dtype=np.int64)
    for lo, K in ((0, 3), (1, 3), (2, 4), (3, 3), (5, 64)):
        out, ok, hops, lists, _ = M.solve(V, off, adj, eid, w, rs, rd, lo, K)
        want = np.array(WL.reference(V, off, adj, rs, rd, lo, K))
        assert (ok == (want >= 0)).all() and (out[ok] == c * want[ok]).all() and (np.array(hops) == want).all()
        _, _, walks, _ = KW.solve(V, off, adj, eid, rs, rd, lo, K, 1)
        assert lists == [None if x is None else x[0] for x in walks]


def test_fixtures_say_what_they_claim():
    for double in (False, True):
        V, off, adj, eid, w, rs, rd = M.bound_binds(double)
        for (lo, K), (value, h) in M.BOUND_BINDS_EXPECTED.items():
            out, ok, hops, lists, _ = M.solve(V, off, adj, eid, w, rs, rd, lo, K)
            assert ok[0] and out[0] == value and hops[0] == h and len(lists[0]) == 2 * h + 1
        V, off, adj, eid, w, rs, rd = M.path4(double)
        out, ok, *_ = M.solve(V, off, adj, eid, w, rs, rd, 2, 3)
        assert ok.tolist() == [False, True, True, True, False, False]
        V, off, adj, eid, w, rs, rd = M.odd_walks(double)
        assert not M.solve(V, off, adj, eid, w, rs, rd, 2, 2)[1][0]
        out, ok, hops, lists, _ = M.solve(V, off, adj, eid, w, rs, rd, 2, 3)
        assert ok[0] and hops[0] == 3 and out[0] == 7 and lists[0][::2] == [0, 1, 2, 1]
        V, off, adj, eid, w, rs, rd = M.dead_ends(double)
        for lo in (1, 2):
            assert M.solve(V, off, adj, eid, w, rs, rd, lo, 4)[1].tolist() == [False, False, False, True, True, True]
        assert M.solve(V, off, adj, eid, w, rs, rd, 0, 4)[1].tolist() == [True, True, True, True, True, True]
    # the rounds a batch runs: the chain's queue empties behind round 21 (vertex 20 has no out-edge), the ring's never
    V, off, adj, eid, w, rs, rd = M.chain(20, False)
    assert [M.solve(V, off, adj, eid, w, rs[:1], rd[:1], lo, K)[4][0] for lo, K in M.CHAIN_BOUNDS] == [21, 21, 8, 9, 20]
    V, off, adj, eid, w, rs, rd = M.ring(5, False)
    assert [M.solve(V, off, adj, eid, w, rs[:1], rd[:1], lo, K)[4][0] for lo, K in M.RING_BOUNDS] == [4, 3, 4, 10]
    V, off, adj, eid, w, rs, rd = M.near_inf()
    out, ok, *_ = M.solve(V, off, adj, eid, w, rs, rd, 2, 2)
    assert ok[0] and out[0] == M.inf_of(w) - 1 and not ok[1]


@pytest.fixture(scope="module")
def cases():
    """(name, fixture, lo, K, the model's answer) of every GPU fixture with int64 weights, and the doubles' absorption example."""
    fx = dict(M.gpu_fixtures(False))
    fx["absorbed_shortcut"] = M.gpu_fixtures(True)["absorbed_shortcut"]
    out = []
    for name, (f, bounds) in fx.items():
        for lo, K in bounds:
            out.append((name, f, lo, K, M.solve(*f, lo, K)))
    return out


def _same(w, a, b, lists_only):
    if a[3] != b[3] or a[2] != b[2]:
        return False
    return lists_only or len(CW.differing(a[0], a[1], b[0], b[1])) == 0


# the fixture that MUST catch a mutant, under a bound with lo >= 1: at lo == 0 the calls are the _within pair, whose own tests hold them
CAUGHT_BY = {"no_reset": "path4", "filter": "bound_binds", "exact_to_K": "bound_binds", "seed_D": "path4", "lo_minus_1": "bound_binds",
             "lo_plus_1": "bound_binds", "src_eq_dst_zero": "loops_alone", "trivial_zero": "dead_ends", "stale_lookup": "stale_gadget",
             "h_unchecked": "path4", "max_parent": "tied_parents", "last_slot": "parallel_edges"}


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_gpu_fixtures_catch_the_mutants(mutant, cases):
    caught = set()
    for name, f, lo, K, want in cases:
        if lo < 1:
            continue
        got = M.solve(*f, lo, K, mutant=mutant)
        if not _same(f[4], want, got, False):
            caught.add(name)
        if mutant in M.LIST_ONLY and mutant != "h_unchecked":  # the value is right: only the list call can tell
            assert len(CW.differing(got[0], got[1], want[0], want[1])) == 0, name
            assert got[2] == want[2] or mutant == "stale_lookup", name  # (a walk-back that loses its way keeps h)
        if mutant == "h_unchecked":  # rows the model has NULL come back with a list of fewer than lo edges; every other row is the model's
            for i in range(len(f[5])):
                if got[3][i] != want[3][i]:
                    assert want[3][i] is None and not want[1][i] and 0 <= got[2][i] < lo, (name, lo, K, i)
                else:
                    assert got[2][i] == want[2][i] and got[1][i] == want[1][i]
    assert CAUGHT_BY[mutant] in caught, (mutant, sorted(caught))


def test_every_layer_names_the_functions():
    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()

    hip = text("include", "pgq_hip.h")
    for name in ("pgq_cheapest_walk_length", "pgq_cheapest_walk_length_bulk_device", "pgq_cheapest_walk", "pgq_cheapest_walk_bulk_device"):
        assert "int %s(" % name in hip, name
    udf = text("include", "pgq_udf.h")
    assert "int pgq_udf_cheapest_walk_length(" in udf and "int pgq_udf_cheapest_walk(" in udf
    glue = text("glue", "pgq_glue.cpp")
    assert "pgq_cheapest_walk_length(" in glue and "pgq_cheapest_walk(" in glue
    assert "void CheapestWalkLengthFunction(" in glue and "void CheapestWalkFunction(" in glue
    binding = text("duckpgq-extension_amd", "binding.py")
    for name in ("cheapest_walk_length", "cheapest_walk_length_bulk_ptr", "cheapest_walk", "cheapest_walk_bulk_ptr"):
        assert "def %s(" % name in binding, name
    assert "pgq_udf_cheapest_walk_length" in binding and "pgq_udf_cheapest_walk(" in binding
    rounds = text("duckpgq-extension_amd", "csrc", "pgq_cheapest.hip")
    assert "int take" in rounds and "closed walk" in rounds
    lists = text("duckpgq-extension_amd", "csrc", "pgq_cheapest_path_within.hip")
    assert "Λ" in lists and "int take" in lists
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        assert "cheapest_walk_length" in text(doc), doc
    assert "3.9j" in text("DESIGN.md") and "CheapestWalkLengthFunction" in text("INTEGRATION.md")
    for doc in ("README.md", "DESIGN.md"):  # the "not built" list stands beside the contract
        assert "`upper - lower >= V - 1`" in text(doc) and "a destination bound" in text(doc), doc
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "duckpgq-extension_amd", "csrc"), "glue-check"])


def test_both_libraries_export_the_symbols():
    import duckpgq_extension_amd as pgq

    L, U = pgq.load_hip(), pgq.load_udf()
    for name in ("pgq_cheapest_walk_length", "pgq_cheapest_walk_length_bulk_device", "pgq_cheapest_walk", "pgq_cheapest_walk_bulk_device"):
        assert getattr(L, name) is not None
    for name in ("pgq_udf_cheapest_walk_length", "pgq_udf_cheapest_walk"):
        assert getattr(U, name) is not None


def test_a_null_handle_is_answered_before_any_device_is_asked_for():
    import ctypes as C

    import duckpgq_extension_amd as pgq

    L = pgq.load_hip()
    vec = pgq.binding.Vec()
    used = C.c_int64(7)
    assert L.pgq_cheapest_walk_length_bulk_device(None, 1, None, None, 1, 3, None, None) == -4  # PGQ_ERR_INVALID_ARG
    assert L.pgq_last_error().decode() == "NULL csr"
    assert L.pgq_cheapest_walk_length(None, 1, 0, vec, vec, 1, 3, None, None) == -4
    assert L.pgq_last_error().decode() == "NULL csr"
    assert L.pgq_cheapest_walk_bulk_device(None, 1, None, None, 1, 3, None, None, None, 0, C.byref(used)) == -4
    assert L.pgq_last_error().decode() == "NULL csr" and used.value == 0
    assert L.pgq_cheapest_walk(None, 1, 0, vec, vec, 1, 3, None, None, None, None, None) == -4
    assert L.pgq_last_error().decode() == "NULL csr"
    # bad bounds behind it would be another error: the handle comes first
    assert L.pgq_cheapest_walk_length_bulk_device(None, 1, None, None, 5, 3, None, None) == -4
    assert L.pgq_last_error().decode() == "NULL csr"
