"""cheapest_path_within without a GPU: the Python model of its contract (cheapest_path_within_model.py) against a brute-force
enumeration of every walk of at most K edges, against the model of cheapest_path_length_within (the fold of the list's edges is
that number, bit for bit), the CPU oracle's shortestpath (unit weights: the same list, clamped at K) and the model of
cheapest_path (K = V - 1, int64 weights: the same list), and the mutants the GPU fixtures must tell from the model."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cheapest_path_model as P
import cheapest_path_within_model as M
from cheapest_within_model import bits, bounded_cheapest
from oracle.pgq_oracle import OracleCSR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = pytest.mark.parametrize("double", [False, True], ids=["int64", "double"])
KS = (0, 1, 2, 3, 5)


def model(fx, K, mutant=None):
    V, off, adj, eid, w, rs, rd = fx
    return M.bounded_paths(V, off, adj, eid, w, rs, rd, K, mutant)


def tiny_graphs():
    """Graphs of six vertices, every (src, dst): weights from {0, 1, 2} (ties, zero cycles), parallel edges and self-loops as
    they fall."""
    for seed in range(12):
        rng = np.random.default_rng(seed)
        V = 6
        E = int(rng.integers(V, 3 * V))
        es, ed = rng.integers(0, V, E), rng.integers(0, V, E)
        ew = rng.integers(0, 3, E)
        rows = [(s, d) for s in range(V) for d in range(V)]
        for double in (False, True):
            yield seed, double, P._fixture(V, es, ed, ew * 0.5 if double else ew, rows, double)


def test_model_against_brute_force():
    longer = 0
    for seed, double, fx in tiny_graphs():
        V, off, adj, eid, w, rs, rd = fx
        for K in KS:
            got = model(fx, K)
            for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
                want = M.brute_force(V, off, adj, eid, w, s, d, K)
                assert got[i] == want, (seed, double, K, s, d, got[i], want)
                longer += want is not None and len(want) > 3
    assert longer > 200  # walks of two edges and more


def cases(double):
    fx = dict(P.small_fixtures(double), shortcut=M.shortcut_path(double), long_out_list=M.long_out_list(65, double),
              many_sources=M.many_sources(65, double), path=M.directed_path(20, double), random=P.random_weighted(200, 1200, double))
    if double:
        fx["absorbed_shortcut"] = M.absorbed_shortcut()
    return fx


@BOTH
def test_fold_is_the_bounded_length(double):
    for name, fx in cases(double).items():
        V, off, adj, eid, w, rs, rd = fx
        Ks = [0, 1, 2, 3, 5, V - 1]
        lengths = bounded_cheapest(V, off, adj, w, rs, rd, Ks)
        for K in Ks:
            out, ok = lengths[K]
            got = model(fx, K)
            trivial = rs == rd
            assert [p is not None for p in got] == (ok | trivial).tolist(), (name, K)
            assert all(len(p) // 2 <= K for p in got if p is not None), (name, K)
            folds = np.array([M.fold(w, eid, p) if p is not None else 0 for p in got], dtype=w.dtype)
            assert (bits(folds)[ok] == bits(out)[ok]).all(), (name, K)


def test_unit_weights_give_the_oracles_shortestpath_clamped():
    for w_all in (1, 7):
        V, off, adj, eid, w, rs, rd = P.random_weighted(200, 1200, False, unit=True)
        fx = (V, off, adj, eid, w * w_all, rs, rd)
        plain = OracleCSR.adopt(V, off, adj, eid, w * w_all).shortestpath(V, rs, rd)
        seen = 0
        for K in (1, 2, 3, 4):
            want = [p if p is None or len(p) // 2 <= K else None for p in plain]
            assert model(fx, K) == want, (w_all, K)
            seen += sum(p is not None and len(p) // 2 == K for p in want)
        assert seen > 100


def test_a_large_bound_is_cheapest_path_for_int64_weights():
    for name, fx in dict(P.small_fixtures(False), chain=P.long_chain(300, False), random=P.random_weighted(200, 1200, False)).items():
        V, off, adj, eid, w, rs, rd = fx
        want = P.cheapest_paths(V, off, adj, eid, w, rs, rd)
        assert model(fx, V - 1) == want, name
        assert model(fx, np.iinfo(np.int64).max) == want, name


def test_a_large_bound_differs_where_a_double_label_absorbs():
    fx = M.absorbed_shortcut()
    V, off, adj, eid, w, rs, rd = fx
    assert P.cheapest_paths(V, off, adj, eid, w, rs, rd) == [[0, 1001, 1, 1002, 2, 1003, 3], [0, 1001, 1, 1002, 2]]
    assert model(fx, 1) == [None, [0, 1000, 2]]
    for K in (2, 3, V - 1, np.iinfo(np.int64).max):
        assert model(fx, K)[0] == [0, 1000, 2, 1003, 3], K  # two hops: 1.0 + 2^53 == 0.5 + 2^53, round 3 improves nothing
    assert model(fx, 2)[1] == [0, 1001, 1, 1002, 2] and model(fx, 3)[1] == [0, 1001, 1, 1002, 2]
    for p in (model(fx, 3)[0], P.cheapest_paths(V, off, adj, eid, w, rs, rd)[0]):
        assert M.fold(w, eid, p) == 2.0 ** 53
    # the other doubles of cheapest_path_model agree with cheapest_path at K = V - 1, absorption() included
    for name, other in P.small_fixtures(True).items():
        V, off, adj, eid, w, rs, rd = other
        assert model(other, V - 1) == P.cheapest_paths(V, off, adj, eid, w, rs, rd), name


def test_fixtures_say_what_they_claim():
    for double in (False, True):
        fx = M.shortcut_path(double)
        want6 = {0: None, 1: [0, 1010, 6], 2: [0, 1009, 5, 1005, 6], 3: [0, 1008, 4, 1004, 5, 1005, 6], 6: [0, 1000, 1, 1001, 2, 1002, 3, 1003, 4, 1004, 5, 1005, 6]}
        for K, want in want6.items():
            assert model(fx, K)[0] == want, (double, K)
        assert len({tuple(model(fx, K)[0] or ()) for K in range(7)}) == 7  # another list for every K
        n = 65
        assert model(M.long_out_list(n, double), 3)[0] == [0, 1000, 1, 1001, 2, 1001 + n, 3]
        got = model(M.many_sources(n, double), 3)
        assert got[0] == [0, 1000, n, 1000 + n, n + 1, 1001 + n, n + 2] and all(p is not None and p[0] == i for i, p in enumerate(got[:n]))
        assert all(p is None for p in model(M.many_sources(n, double), 2)[:n])
        path = M.directed_path(20, double)
        for K in (7, 8, 9, 19):
            got = model(path, K)
            assert [p is not None for p in got[:20]] == [j <= K for j in range(20)] and got[K] == [x for v in range(K) for x in (v, 1000 + v)] + [K]


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_fixtures_catch_the_mutants(mutant):
    def caught(fx, K):
        return model(fx, K, mutant) != model(fx, K)

    for double in (False, True):
        if mutant in ("final", "filter"):
            assert all(caught(M.shortcut_path(double), K) for K in (2, 3, 4, 5)), double
        elif mutant == "max_parent":
            assert caught(P.tied_parents(double), 2), double
        elif mutant == "first_slot":
            assert caught(P.parallel_edges(double), 2) and caught(M.long_out_list(65, double), 3), double
        elif mutant == "late":
            assert caught(P.diamond(double), 3), double
    fx = P.random_weighted(200, 1200, False)
    good, bad = model(fx, 3), model(fx, 3, mutant)
    assert sum(a != b for a, b in zip(good, bad)) > 0


@pytest.mark.parametrize("K", [2, 3])
def test_the_random_fixture_is_not_answered_by_nulls_alone(K):
    fx = P.random_weighted(200, 1200, False)
    V, off, adj, eid, w, rs, rd = fx
    got = model(fx, K)
    plain = P.cheapest_paths(V, off, adj, eid, w, rs, rd)
    assert sum(p is not None and len(p) > 1 for p in got) >= 40
    assert sum(p is None and q is not None for p, q in zip(got, plain)) >= 40


def test_every_layer_names_the_function():
    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()

    hip = text("include", "pgq_hip.h")
    assert "int pgq_cheapest_path_within(" in hip and "int pgq_cheapest_path_within_bulk_device(" in hip
    assert "int pgq_udf_cheapest_path_within(" in text("include", "pgq_udf.h")
    glue = text("glue", "pgq_glue.cpp")
    assert "pgq_cheapest_path_within(" in glue and "void CheapestPathWithinFunction(" in glue
    binding = text("duckpgq-extension_amd", "binding.py")
    assert "def cheapest_path_within(" in binding and "def cheapest_path_within_bulk_ptr(" in binding
    assert "pgq_udf_cheapest_path_within" in binding
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "duckpgq-extension_amd", "csrc"), "glue-check"])


def test_a_null_handle_is_answered_before_any_device_is_asked_for():
    import duckpgq_extension_amd as pgq

    L = pgq.load_hip()
    used = ctypes.c_int64(-7)
    assert L.pgq_cheapest_path_within_bulk_device(None, 1, None, None, 3, None, None, None, 0, ctypes.byref(used)) == -4  # PGQ_ERR_INVALID_ARG
    assert used.value == 0
    vec = pgq.binding.Vec()
    child, clen = ctypes.c_void_p(), ctypes.c_uint64()
    assert L.pgq_cheapest_path_within(None, 1, 0, vec, vec, 3, None, None, None, ctypes.byref(child), ctypes.byref(clen)) == -4
    assert L.pgq_last_error().decode() == "NULL csr"
