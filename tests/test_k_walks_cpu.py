"""walk_count / k_shortest_walks without a GPU: the Python model of their contract (k_walks_model.py) against a brute-force
enumeration of every walk of at most K edges, against all_shortestpaths' model and the CPU oracle's shortestpath (the leading
walks of length d), at the saturation of the count, and the mutants the GPU fixtures must tell from the model."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import all_shortest_model as A
import k_walks_model as M
from oracle.pgq_oracle import OracleCSR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64_MAX = M.INT64_MAX


def test_model_against_brute_force():
    """Every (src, dst) of 300 tiny multigraphs, src == dst included, every lo in 0..K; K is the largest bound up to 5 that keeps
    the enumeration of one source's walks in the hundreds."""
    graphs, multi, mixed, closed = 0, 0, 0, 0
    for seed in range(300):
        V, off, adj, eid, rs, rd = A.tiny_multigraph(seed)
        deg = max(len(adj) / V, 1.0)
        K = max(k for k in range(2, 6) if k == 2 or deg ** k <= 250)
        brute = {s: M.brute_force(V, off, adj, eid, s, K) for s in range(V)}
        state = {}
        for lo in range(K + 1):
            counts, hops, lists, counts_k = M.solve(V, off, adj, eid, rs, rd, lo, K, M.K_ALL, state=state)
            for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
                want = [p for p in brute[s][d] if len(p) // 2 >= lo]
                assert counts[i] == counts_k[i] == len(want), (seed, lo, s, d)
                assert lists[i] == (want or None), (seed, lo, s, d)
                assert hops[i] == (len(want[0]) // 2 if want else -1)
                if lo == 1:
                    multi += len(want) >= 2
                    mixed += len({len(p) for p in want}) >= 2
                    closed += s == d and len(want) > 0
        graphs += 1
    assert graphs == 300 and multi > 1000 and mixed > 1000 and closed > 300, (graphs, multi, mixed, closed)


def test_model_against_brute_force_on_a_run_of_parallel_slots():
    """parallel_run(65): the m-th of 65 parallel slots, m up to 64, at in-position 1 + m and out-position 2 m + 1."""
    V, off, adj, eid, rs, rd = A.parallel_run(65)
    brute = {s: M.brute_force(V, off, adj, eid, s, 2) for s in set(rs.tolist())}
    for lo, K in ((2, 2), (1, 2)):
        counts, hops, lists, counts_k = M.solve(V, off, adj, eid, rs, rd, lo, K, M.K_ALL)
        for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
            want = [p for p in brute[s][d] if len(p) // 2 >= lo]
            assert counts[i] == counts_k[i] == len(want) and lists[i] == (want or None), (lo, K, s, d)
    assert counts == [66, 65] and hops == [2, 1]


def test_k_cuts_the_list_and_the_list_forms_count():
    V, off, adj, eid, rs, rd = A.tiny_multigraph(3)
    full = M.solve(V, off, adj, eid, rs, rd, 1, 4, M.K_ALL)
    cut_rows = 0
    for k in (1, 2, 5):
        counts, hops, lists, counts_k = M.solve(V, off, adj, eid, rs, rd, 1, 4, k)
        assert counts == full[0] and hops == full[1]
        assert lists == [None if ps is None else ps[:k] for ps in full[2]]
        for c, ck, ps in zip(counts, counts_k, full[2]):
            if c <= k:
                assert ck == c
            else:  # the walks no longer than the k-th
                T = len(ps[k - 1])
                assert k <= ck <= c and ck == sum(len(p) <= T for p in ps)
                cut_rows += ck < c
    assert cut_rows >= 10


@pytest.fixture(scope="module")
def random_rows():
    V, off, adj, eid, rs, rd = fx = A.random_fixture()
    return fx, OracleCSR.adopt(V, off, adj, eid).shortestpath(V, rs, rd)


@pytest.mark.parametrize("lo,K", [(0, 3), (1, 3), (2, 4), (3, 3)])
def test_leading_walks_are_all_shortestpaths_and_walk_zero_the_oracles(random_rows, lo, K):
    (V, off, adj, eid, rs, rd), plain = random_rows
    counts, hops, lists, _ = M.solve(V, off, adj, eid, rs, rd, lo, K, M.K_ALL)
    a_counts, a_hops, a_lists = A.solve(V, off, adj, eid, rs, rd, K, A.MAX_PATHS_ALL)
    checked, multi, mixed = 0, 0, 0
    for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
        if lists[i] is not None:
            multi += counts[i] >= 2
            mixed += len({len(p) for p in lists[i]}) >= 2
        if s == d or a_hops[i] < lo:  # (a_hops = -1: farther apart than K, or unreachable)
            continue
        dd = a_hops[i]
        assert hops[i] == dd and lists[i][:a_counts[i]] == a_lists[i] and lists[i][0] == plain[i], (s, d)
        assert all(len(p) // 2 > dd for p in lists[i][a_counts[i]:])
        checked += 1
    assert checked >= 40 and multi >= 40 and mixed >= (20 if K > lo else 0), (checked, multi, mixed)


def test_the_count_saturates_and_never_wraps():
    V, off, adj, eid, rs, rd = M.chain8()
    counts, hops, lists, counts_k = M.solve(V, off, adj, eid, rs, rd, 0, M.MAX_HOPS, 3)
    assert counts == [2 ** 60, INT64_MAX, INT64_MAX, 8 ** 5, 2 ** 60] and hops == [20, 21, 22, 5, 20] and counts_k == counts
    for ps, h in zip(lists, hops):  # the first three walks still unrank: the FIRST hop's slot is the least significant
        assert len(ps) == 3 and all(len(p) == 2 * h + 1 for p in ps)
        assert [p[1] for p in ps] == [ps[0][1], ps[0][1] + 1, ps[0][1] + 2] and all(p[3:] == ps[0][3:] for p in ps)
    assert M.solve(V, off, adj, eid, rs, rd, 0, M.MAX_HOPS, 3, "wrap")[0][1] == -2 ** 63  # where a signed sum goes negative
    V, off, adj, eid, rs, rd = M.two_loops()
    for K, want in ((62, INT64_MAX), (61, 2 ** 62 - 1), (63, INT64_MAX)):
        counts, hops, lists, _ = M.solve(V, off, adj, eid, rs, rd, 0, K, 3)
        assert counts == [want] and hops == [0] and lists[0] == [[0], [0, 1000, 0], [0, 1001, 0]]
    assert sum(2 ** t for t in range(63)) == INT64_MAX and sum(2 ** t for t in range(64)) > INT64_MAX  # K = 62 exact, K = 63 saturated
    assert M.solve(V, off, adj, eid, rs, rd, 0, 63, 3, "wrap")[0] != [INT64_MAX]
    V, off, adj, eid, rs, rd = M.loops_and_fan()
    counts, hops, lists, _ = M.solve(V, off, adj, eid, rs, rd, 1, 62, 3)
    assert 3 * 2 ** 61 < INT64_MAX < 3 * (2 ** 62 - 1)  # no single W_t[b] saturates, the sum does
    assert counts == [INT64_MAX, 2 ** 63 - 2, 0, 0] and hops[0] == 1 and lists[0] == [[0, 1002, 1], [0, 1003, 1], [0, 1004, 1]]
    assert M.solve(V, off, adj, eid, rs, rd, 1, 61, 3)[0][0] == 3 * (2 ** 61 - 1)
    assert M.solve(V, off, adj, eid, rs, rd, 1, 62, 3, "wrap")[0][0] < 0


def test_fixtures_say_what_they_claim():
    V, off, adj, eid, rs, rd = M.ring(5)
    counts, hops, lists, _ = M.solve(V, off, adj, eid, rs, rd, 1, 10, 3)
    assert counts == [2, 2, 2, 2, 2] and hops == [5, 2, 3, 5, 1]  # (a, a) with lo = 1: the closed walks of 5 and 10 edges
    assert [len(p) // 2 for p in lists[0]] == [5, 10] and [len(p) // 2 for p in lists[1]] == [2, 7]
    assert M.solve(V, off, adj, eid, rs, rd, 0, 10, 3)[0][0] == 3 and M.solve(V, off, adj, eid, rs, rd, 1, 4, 3)[2][0] is None
    V, off, adj, eid, rs, rd = A.dead_ends()  # (3, 3): no out-edge; (4, 4): isolated; (0, 0): no in-edge
    assert M.solve(V, off, adj, eid, rs, rd, 0, 2, 3)[2][3] == [[4]] and M.solve(V, off, adj, eid, rs, rd, 0, 2, 3)[0] == [0, 0, 2, 1, 0, 0, 1, 1]
    assert M.solve(V, off, adj, eid, rs, rd, 1, 2, 3)[0] == [0, 0, 2, 0, 0, 0, 0, 0]
    V, off, adj, eid, rs, rd = A.parallel_edges()
    counts, hops, lists, _ = M.solve(V, off, adj, eid, rs, rd, 0, 3, 11)
    assert counts == [10, 3, 1, 0] and lists[0] == A.solve(V, off, adj, eid, rs, rd, 3, 11)[2][0]
    for deg in (63, 64, 65, 127, 128, 129):
        V, off, adj, eid, rs, rd = M.in_list_gadget(deg)
        rin = A.in_lists(V, off, adj)
        s, x = int(rs[0]), int(rd[0])
        assert len(rin[x]) == deg == off[int(rs[1]) + 1] - off[int(rs[1])]
        counts, hops, lists, _ = M.solve(V, off, adj, eid, rs, rd, 0, 7, M.K_ALL)
        lens = [len(p) // 2 for p in lists[0]]
        n3, n4 = lens.count(3), lens.count(4)  # (4: through the level-3 parents)
        assert sorted(set(lens)) == [3, 4, 7] and counts[0] == len(lens) == n3 + n4 + n3 * n3 and n3 < 200  # d and d + c: k = 200 goes past d
        parents = [p[-3] for p in lists[0][:n3]]
        assert parents == sorted(parents) and parents[0] == rin[x][0][0] and parents[-1] == rin[x][-1][0]  # first .. LAST position
        assert counts[3] == counts[4] == 1 + n3 + n4 and hops[3:] == [0, 0, 1]  # the empty walk and the closed walks of 4 and 5 edges
        assert [p[2] for p in lists[1]] == [int(rs[1]) + 1, int(rs[1]) + deg]  # through the out-list's first and last entry


@pytest.fixture(scope="module")
def expected():
    """(name, lo, K, k) -> the model's answer, for the fixtures the GPU file runs (those of a kind once)."""
    out = {}
    for name, (fx, runs) in M.gpu_fixtures().items():
        if name.startswith("sources") or (name.startswith("in_list") and name != "in_list_65"):
            continue
        state = {}
        for lo, K, ks in runs:
            for k in ks:
                out[name, lo, K, k] = (fx, M.solve(*fx, lo, K, k, state=state))
    return out


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_gpu_fixtures_catch_the_mutants(mutant, expected):
    states = {}
    caught = [key for key, (fx, good) in expected.items()
              if M.solve(*fx, key[1], key[2], key[3], mutant, state=states.setdefault(key[0], {})) != good]
    assert caught, mutant
    names = {c[0] for c in caught}
    if mutant == "wrap":
        assert {"chain8", "two_loops", "loops_and_fan"} <= names
    if mutant in ("bfs_only", "trivial_src_eq_dst", "empty_walk_always"):
        assert "ring5" in names and "self_loop" in names
    if mutant == "lower_ignored":
        assert {"random", "ring5", "dead_ends"} <= names
    if mutant == "length_order":
        assert {"ring5", "random"} <= names
    if mutant == "collapse":
        assert "parallel" in names and "chain8" in names
    if mutant == "slot_order":  # needs a smaller parent with parallel slots beside a larger one: the random multigraph has them
        assert "random" in names
    if mutant == "k_plus_1":
        assert ("parallel", 0, 3, 9) in caught and ("parallel", 0, 3, 10) not in caught
    if mutant in ("m_mod_64", "slot_first_64"):  # three parallel slots do not show them, a run of 65 does
        assert "parallel" not in names and "parallel_run_65" in names
    if mutant == "m_mod_64":
        assert all(name.startswith("parallel_run") for name in names)


def test_every_layer_names_the_functions():
    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()

    hip = text("include", "pgq_hip.h")
    for name in ("pgq_walk_count", "pgq_walk_count_bulk_device", "pgq_k_shortest_walks", "pgq_k_shortest_walks_bulk_device"):
        assert "int %s(" % name in hip, name
    assert "#define PGQ_WALK_MAX_HOPS 64" in hip
    udf = text("include", "pgq_udf.h")
    assert "int pgq_udf_walk_count(" in udf and "int pgq_udf_k_shortest_walks(" in udf
    glue = text("glue", "pgq_glue.cpp")
    assert "pgq_walk_count(" in glue and "void WalkCountFunction(" in glue
    assert "pgq_k_shortest_walks(" in glue and "void KShortestWalksFunction(" in glue
    binding = text("duckpgq-extension_amd", "binding.py")
    for name in ("walk_count", "walk_count_bulk_ptr", "k_shortest_walks", "k_shortest_walks_bulk_ptr"):
        assert "def %s(" % name in binding, name
    assert "pgq_udf_walk_count" in binding and "pgq_udf_k_shortest_walks" in binding
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "k_shortest_walks" in text(doc) and "walk_count" in text(doc), doc
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "duckpgq-extension_amd", "csrc"), "glue-check"])


def test_both_libraries_export_the_symbols():
    import duckpgq_extension_amd as pgq

    L, U = pgq.load_hip(), pgq.load_udf()
    for name in ("pgq_walk_count", "pgq_walk_count_bulk_device", "pgq_k_shortest_walks", "pgq_k_shortest_walks_bulk_device"):
        assert getattr(L, name) is not None
    for name in ("pgq_udf_walk_count", "pgq_udf_k_shortest_walks"):
        assert getattr(U, name) is not None


def test_a_null_handle_is_answered_before_any_device_is_asked_for():
    import duckpgq_extension_amd as pgq

    L = pgq.load_hip()
    paths, used = ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert L.pgq_k_shortest_walks_bulk_device(None, 1, None, None, 1, 3, 2, None, None, None, None, None, None, 0, None, 0, ctypes.byref(paths),
                                              ctypes.byref(used)) == -4  # PGQ_ERR_INVALID_ARG
    assert paths.value == 0 and used.value == 0
    assert L.pgq_last_error().decode() == "NULL csr"
    assert L.pgq_walk_count_bulk_device(None, 1, None, None, 1, 3, None) == -4
    vec = pgq.binding.Vec()
    po, pl, child = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    pt, clen = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.pgq_k_shortest_walks(None, 1, 0, vec, vec, 1, 3, 2, None, None, None, ctypes.byref(po), ctypes.byref(pl), ctypes.byref(pt),
                                  ctypes.byref(child), ctypes.byref(clen)) == -4
    assert L.pgq_walk_count(None, 1, 0, vec, vec, 1, 3, None, None) == -4
    assert L.pgq_last_error().decode() == "NULL csr"
