"""shortestpath_count / all_shortestpaths without a GPU: the Python model of their contract (all_shortest_model.py) against a
brute-force enumeration of every walk of d edges, against the CPU oracle's shortestpath and iterativelength (path 0 and the
hop counts), at the saturation of the count, and the mutants the GPU fixtures must tell from the model."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import all_shortest_model as M
from oracle.pgq_oracle import OracleCSR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64_MAX = M.INT64_MAX


def test_model_against_brute_force():
    graphs, rows, multi, deep = 0, 0, 0, 0
    for seed in range(300):
        V, off, adj, eid, rs, rd = M.tiny_multigraph(seed)
        counts, hops, lists = M.solve(V, off, adj, eid, rs, rd, INT64_MAX, M.MAX_PATHS_ALL)
        for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
            want = M.brute_force(V, off, adj, eid, s, d)
            assert counts[i] == (0 if want is None else len(want)), (seed, s, d)
            assert lists[i] == want, (seed, s, d, lists[i], want)  # the same lists, already in the contract's order
            if want is not None:
                assert len(set(map(tuple, want))) == len(want) and all(len(p) == 2 * hops[i] + 1 for p in want)
                multi += len(want) >= 2
                deep += hops[i] >= 3
        graphs += 1
        rows += len(rs)
    assert graphs == 300 and multi > 1000 and deep > 1000, (graphs, rows, multi, deep)


def test_model_against_brute_force_on_a_run_of_parallel_slots():
    """parallel_run(65): the m-th of 65 parallel slots, m up to 64, at in-position 1 + m and out-position 2 m + 1."""
    V, off, adj, eid, rs, rd = M.parallel_run(65)
    counts, hops, lists = M.solve(V, off, adj, eid, rs, rd, INT64_MAX, M.MAX_PATHS_ALL)
    assert counts == [66, 65] and hops == [2, 1]
    for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
        assert lists[i] == M.brute_force(V, off, adj, eid, s, d), (s, d)
    rin = M.in_lists(V, off, adj)
    assert [u for u, _ in rin[3]] == [1] + [2] * 65 and [slot - off[2] for _, slot in rin[3][1:]] == [2 * k + 1 for k in range(65)]
    assert len({p[-2] for p in lists[0]}) == 66  # distinct edge ids: every slot is told from the others


@pytest.fixture(scope="module")
def random_rows():
    V, off, adj, eid, rs, rd = fx = M.random_fixture()
    ora = OracleCSR.adopt(V, off, adj, eid)
    return fx, ora.shortestpath(V, rs, rd), ora.iterativelength(V, rs, rd)


@pytest.mark.parametrize("max_hops", [INT64_MAX, 2, 3])
def test_path_zero_and_lengths_are_the_oracles(random_rows, max_hops):
    (V, off, adj, eid, rs, rd), plain, (oln, ook) = random_rows
    counts, hops, lists = M.solve(V, off, adj, eid, rs, rd, max_hops, 1)
    within = ook & (oln <= max_hops)
    assert [c > 0 for c in counts] == within.tolist()
    assert [h for h, ok in zip(hops, within) if ok] == oln[within].tolist()
    assert [None if p is None else p[0] for p in lists] == [p if ok else None for p, ok in zip(plain, within)]
    assert within.sum() >= 40


def test_the_count_saturates_and_never_wraps():
    want = {62: 4611686018427387904, 63: INT64_MAX, 64: INT64_MAX}
    for k, count in want.items():
        V, off, adj, eid, rs, rd = M.diamond_chain(k)
        counts, hops, lists = M.solve(V, off, adj, eid, rs, rd, INT64_MAX, 3)
        assert counts[0] == count and hops[0] == 2 * k, k
        assert counts[1] == 2 ** (k // 2) and counts[2] == min(2 ** (k - 1), INT64_MAX)
        # the first three paths of the (saturated) row still unrank: all b's; then c in the FIRST diamond — the comparison runs
        # from the destination end, so the earliest vertex is the least significant; then b, c in the first two diamonds
        assert len(lists[0]) == 3 and all(len(p) == 4 * k + 1 and p[0] == 0 and p[-1] == 3 * k for p in lists[0])
        mids = [[p[2 + 4 * i] - 3 * i for i in range(k)] for p in lists[0]]
        assert mids[0] == [1] * k and mids[1] == [2] + [1] * (k - 1) and mids[2] == [1, 2] + [1] * (k - 2)
    V, off, adj, eid, rs, rd = M.diamond_chain(63)
    assert M.solve(V, off, adj, eid, rs, rd, INT64_MAX, 3, "wrap")[0][0] < 0  # where a signed sum goes negative
    V, off, adj, eid, rs, rd = M.diamond_chain(64)
    assert M.solve(V, off, adj, eid, rs, rd, INT64_MAX, 3, "wrap")[0][0] == 0  # where an unsigned sum wraps to 0


def test_fixtures_say_what_they_claim():
    fx, rows = M.random_fixture(), None
    V, off, adj, eid, rs, rd = fx
    counts, hops, _ = M.solve(V, off, adj, eid, rs, rd, INT64_MAX, 1)
    bounded = M.solve(V, off, adj, eid, rs, rd, 2, 1)[0]
    assert sum(c >= 2 for c in counts) >= 40 and sum(h >= 3 for h in hops) >= 40
    assert sum(c > 0 and b == 0 for c, b in zip(counts, bounded)) >= 40  # rows a bound of 2 turns to 0 / NULL
    V, off, adj, eid, rs, rd = M.parallel_edges()
    counts, hops, lists = M.solve(V, off, adj, eid, rs, rd, INT64_MAX, 11)
    assert counts == [10, 3, 1, 0] and hops == [2, 1, 1, -1]
    assert lists[0][0] == [0, 1001, 1, 1007, 3]  # the single-edge route through the smaller parent first
    assert lists[0][1:] == [[0, a, 2, b, 3] for b in (1003, 1004, 1006) for a in (1000, 1002, 1005)]
    assert len({e for p in lists[0][1:] for e in (p[1], p[3])}) == 6
    for deg in (63, 64, 65, 127, 128, 129):
        V, off, adj, eid, rs, rd = M.in_list_gadget(deg)
        counts, hops, lists = M.solve(V, off, adj, eid, rs, rd, INT64_MAX, M.MAX_PATHS_ALL)
        assert hops == [3, 2, 3] and counts[1] == 2 and counts[2] == 1
        rin = M.in_lists(V, off, adj)
        x = int(rd[0])
        assert len(rin[x]) == deg == off[int(rs[1]) + 1] - off[int(rs[1])]
        parents = [p[-3] for p in lists[0]]
        on_level = sorted(set(parents))
        assert parents == sorted(parents) and on_level[0] == rin[x][0][0] and on_level[-1] == rin[x][-1][0]  # first and LAST position
        assert 4 < len(on_level) < deg - 4 and len({parents.count(p) for p in on_level}) == 4  # some entries only, sigma 1 .. 4
        assert counts[0] == len(lists[0]) == len(set(map(tuple, lists[0])))
        assert [p[2] for p in lists[1]] == [int(rs[1]) + 1, int(rs[1]) + deg]  # through the out-list's first and last entry


@pytest.fixture(scope="module")
def expected():
    """(name, max_hops, max_paths) -> the model's answer, for the fixtures the GPU file runs (those of a kind once)."""
    out = {}
    for name, (fx, hops, paths) in M.gpu_fixtures().items():
        if name.startswith("sources") or (name.startswith("tiny") and name != "tiny0"):
            continue  # (the same kind of graph as `random` / `tiny0`)
        state = {}
        for h in hops:
            for p in paths:
                out[name, h, p] = (fx, M.solve(*fx, h, p, state=state))
    return out


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_gpu_fixtures_catch_the_mutants(mutant, expected):
    states = {}
    caught = [key for key, (fx, good) in expected.items()
              if M.solve(*fx, key[1], key[2], mutant, state=states.setdefault(key[0], {})) != good]
    assert caught, mutant
    names = {c[0] for c in caught}
    if mutant == "wrap":
        assert {"diamonds_63", "diamonds_64"} <= names
    if mutant in ("collapse", "first_slot"):
        assert "parallel" in names
    if mutant == "slot_order":  # needs a smaller parent with parallel slots beside a larger one: the random multigraph has them
        assert "random" in names
    if mutant == "paths_plus_1":
        assert ("parallel", INT64_MAX, 9) in caught and ("parallel", INT64_MAX, 10) not in caught
    if mutant in ("m_mod_64", "slot_first_64"):  # three parallel slots do not show them, a run of 65 does
        assert "parallel" not in names and "parallel_run_65" in names
    if mutant == "m_mod_64":
        assert all(name.startswith("parallel_run") for name in names)


def test_every_layer_names_the_functions():
    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()

    hip = text("include", "pgq_hip.h")
    for name in ("pgq_shortestpath_count", "pgq_shortestpath_count_bulk_device", "pgq_all_shortestpaths", "pgq_all_shortestpaths_bulk_device"):
        assert "int %s(" % name in hip, name
    udf = text("include", "pgq_udf.h")
    assert "int pgq_udf_shortestpath_count(" in udf and "int pgq_udf_all_shortestpaths(" in udf
    glue = text("glue", "pgq_glue.cpp")
    assert "pgq_shortestpath_count(" in glue and "void ShortestPathCountFunction(" in glue
    assert "pgq_all_shortestpaths(" in glue and "void AllShortestPathsFunction(" in glue
    binding = text("duckpgq-extension_amd", "binding.py")
    for name in ("shortestpath_count", "shortestpath_count_bulk_ptr", "all_shortestpaths", "all_shortestpaths_bulk_ptr"):
        assert "def %s(" % name in binding, name
    assert "pgq_udf_shortestpath_count" in binding and "pgq_udf_all_shortestpaths" in binding
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "all_shortestpaths" in text(doc) and "shortestpath_count" in text(doc), doc
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "duckpgq-extension_amd", "csrc"), "glue-check"])


def test_a_null_handle_is_answered_before_any_device_is_asked_for():
    import duckpgq_extension_amd as pgq

    L = pgq.load_hip()
    paths, used = ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert L.pgq_all_shortestpaths_bulk_device(None, 1, None, None, 3, 2, None, None, None, None, None, 0, None, 0, ctypes.byref(paths),
                                               ctypes.byref(used)) == -4  # PGQ_ERR_INVALID_ARG
    assert paths.value == 0 and used.value == 0
    assert L.pgq_last_error().decode() == "NULL csr"
    assert L.pgq_shortestpath_count_bulk_device(None, 1, None, None, 3, None) == -4
    vec = pgq.binding.Vec()
    po, pl, child = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    pt, clen = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.pgq_all_shortestpaths(None, 1, 0, vec, vec, 3, 2, None, None, None, ctypes.byref(po), ctypes.byref(pl), ctypes.byref(pt),
                                   ctypes.byref(child), ctypes.byref(clen)) == -4
    assert L.pgq_shortestpath_count(None, 1, 0, vec, vec, 3, None, None) == -4
    assert L.pgq_last_error().decode() == "NULL csr"
