"""cheapest_path without a GPU: the Python model of its contract (cheapest_path_model.py) against a brute-force enumeration
of simple paths, against the CPU oracle's cheapest_path_length (the fold of the list's edges is that number, bit for bit) and
shortestpath (unit weights: the same list), and the mutants the GPU fixtures must tell from the model."""
import os

import numpy as np
import pytest

import cheapest_path_model as M
from cheapest_within_model import bits, inf_of
from oracle.pgq_oracle import OracleCSR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle(fx):
    V, off, adj, eid, w = fx[:5]
    return OracleCSR.adopt(V, off, adj, eid, w)


def model(fx, mutant=None):
    V, off, adj, eid, w, rs, rd = fx
    return M.cheapest_paths(V, off, adj, eid, w, rs, rd, mutant)


def tiny_graphs():
    """Graphs of at most 8 vertices: weights from {0, 1, 2} (ties, zero cycles), parallel edges and self-loops as they fall."""
    for seed in range(24):
        rng = np.random.default_rng(seed)
        V = int(rng.integers(3, 9))
        E = int(rng.integers(V, 3 * V))
        es, ed = rng.integers(0, V, E), rng.integers(0, V, E)
        ew = rng.integers(0, 3, E)
        rows = [(s, d) for s in range(V) for d in range(V)]
        for double in (False, True):
            yield seed, double, M._fixture(V, es, ed, ew * 0.5 if double else ew, rows, double)


def test_model_against_brute_force():
    checked = 0
    for seed, double, fx in tiny_graphs():
        V, off, adj, eid, w, rs, rd = fx
        got = model(fx)
        for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
            want = M.brute_force(V, off, adj, eid, w, s, d)
            assert got[i] == want, (seed, double, s, d, got[i], want)
            checked += want is not None and len(want) > 3
    assert checked > 200  # paths of two edges and more


@pytest.mark.parametrize("double", [False, True], ids=["int64", "double"])
def test_fixtures_against_brute_force(double):
    for name, fx in M.small_fixtures(double).items():
        if name.startswith("long_in_list"):
            continue  # 68 vertices; its expectation is spelled out below
        V, off, adj, eid, w, rs, rd = fx
        got = model(fx)
        if name == "absorption":  # a fold that rounds: checked against the paths written out, not the enumeration's ties
            assert got == [[3, 1000, 0, 1001, 2, 1002, 1], [3, 1000, 0, 1001, 2], [3, 1000, 0], [0, 1001, 2, 1002, 1]], got
            continue
        for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
            assert got[i] == M.brute_force(V, off, adj, eid, w, s, d), (name, s, d, got[i])


@pytest.mark.parametrize("double", [False, True], ids=["int64", "double"])
def test_fixtures_say_what_they_claim(double):
    fx = M.small_fixtures(double)
    assert model(fx["diamond"])[0] == [0, 1003, 4, 1004, 3]  # two hops beat three at equal cost
    assert model(fx["tied_parents"])[0] == [0, 1001, 2, 1003, 6]  # the smaller parent, listed second
    assert model(fx["parallel_edges"])[:2] == [[0, 1001, 1], [0, 1001, 1, 1003, 2]]  # first TIGHT slot; first of two equal ones
    assert model(fx["zero_ring"])[:3] == [[5, 1000, 1, 1001, 2, 1002, 3], [5, 1000, 1, 1001, 2, 1002, 3, 1003, 4, 1004, 0], [5, 1000, 1]]
    n = 65
    V, off, adj, eid, w, rs, rd = fx["long_in_list_65"]
    got = model(fx["long_in_list_65"])
    assert got[0][:3] == [0, 1000, n + 1] and got[0][-3:] == [n, 1000 + 2 * n, n + 2] and len(got[0]) == 7
    assert got[2] == [1, 1000 + n + 1, n + 2]


@pytest.mark.parametrize("double", [False, True], ids=["int64", "double"])
def test_fold_is_the_oracles_cheapest_path_length(double):
    cases = dict(M.small_fixtures(double), chain=M.long_chain(300, double), random=M.random_weighted(200, 1200, double))
    for name, fx in cases.items():
        V, off, adj, eid, w, rs, rd = fx
        out, ok = oracle(fx).cheapest_path_length(V, rs, rd)
        got = model(fx)
        assert [p is not None for p in got] == ok.tolist(), name
        folds = np.array([M.fold(w, eid, p) if p is not None else 0 for p in got], dtype=w.dtype)
        assert (bits(folds)[ok] == bits(out)[ok]).all(), name


def test_unit_weights_give_the_oracles_shortestpath():
    for seed in (5, 6):
        fx = M.random_weighted(200, 1200, False, seed=seed, unit=True)
        V, off, adj, eid, w, rs, rd = fx
        want = oracle(fx).shortestpath(V, rs, rd)
        assert model(fx) == want
        assert sum(p is not None and len(p) > 3 for p in want) > 100
    for w_all in (3, 7):  # any one positive weight
        V, off, adj, eid, w, rs, rd = M.random_weighted(60, 240, False, seed=9, unit=True)
        fx = (V, off, adj, eid, w * w_all, rs, rd)
        assert model(fx) == oracle(fx).shortestpath(V, rs, rd)


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_fixtures_catch_the_mutants(mutant):
    caught = {}
    for double in (False, True):
        for name, fx in M.small_fixtures(double).items():
            if model(fx, mutant) != model(fx):
                caught.setdefault(name, []).append(double)
    # every mutant on the fixture written for it, in both element types where the fixture has both
    written_for = {"greedy": "zero_ring", "first_slot": "parallel_edges", "max_parent": "tied_parents", "le": "long_in_list_65"}
    assert caught.get(written_for[mutant]) == [False, True], (mutant, caught)
    if mutant == "greedy":
        assert caught.get("absorption") == [True], caught
    fx = M.random_weighted(200, 1200, False)
    assert model(fx, mutant) != model(fx)


def test_hop_count_is_finite_wherever_the_label_is():
    cases = [M.zero_ring(False), M.zero_ring(True), M.absorption(), M.random_weighted(200, 1200, False), M.random_weighted(200, 1200, True)]
    for V, off, adj, eid, w, rs, rd in cases:
        for s in np.unique(rs).tolist():
            D = M.settle(V, off, adj, w, s)
            H = M.levels(V, off, adj, M.tight_slots(V, off, adj, w, D), s)
            assert ((H >= 0) == (D < inf_of(w))).all(), (V, s)


def test_every_layer_names_the_function():
    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()

    assert "int pgq_cheapest_path(" in text("include", "pgq_hip.h") and "int pgq_cheapest_path_bulk_device(" in text("include", "pgq_hip.h")
    assert "int pgq_udf_cheapest_path(" in text("include", "pgq_udf.h")
    glue = text("glue", "pgq_glue.cpp")
    assert "pgq_cheapest_path(" in glue and "CheapestPathFunction" in glue
    binding = text("duckpgq-extension_amd", "binding.py")
    assert "def cheapest_path(" in binding and "def cheapest_path_bulk_ptr(" in binding
