"""k_shortest_walks_mode / walk_count_mode without a GPU: the two Python restatements of the contract (path_modes_model.py) against
each other — the depth-first search as the kernel does it against a brute-force enumeration of walks filtered by the mode — against
k_shortest_walks' and all_shortestpaths' models, and the mutants the GPU fixtures must tell from the model.  Also: every layer names
the new calls, both libraries export them, and a NULL handle is answered before any device is asked for."""
import ctypes
import os
import subprocess

import pytest

import all_shortest_model as A
import k_walks_model as W
import path_modes_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_model_against_the_filtered_enumeration():
    """200 random multigraphs of at most 7 vertices and 12 slots (every second one with the ids of its antiparallel slot pairs
    shared), every (src, dst), the three modes, every lo <= K <= 5, k in {1, 2, 5, all}.  A source has at most 12^5 walks of 5 edges
    and in these graphs a few thousand at the very most: the enumeration stays small."""
    rows, cut, rejected, shared = 0, 0, 0, 0
    for seed in range(200):
        fx = M.random_shared(seed)
        V, off, adj, eid, rs, rd = fx
        shared += len(set(eid.tolist())) < len(eid)
        state, brute = {}, {}
        for K in range(6):
            for lo in range(K + 1):
                for mode in M.MODES:
                    every = M.filter_model(*fx, lo, K, M.K_ALL, mode, brute=brute.setdefault(K, {}))
                    walks = M.filter_model(*fx, lo, K, M.K_ALL, M.WALK, brute=brute[K])
                    for k in (1, 2, 5, M.K_ALL):
                        counts, hops, lists, steps1, steps2, _ = M.search_model(*fx, lo, K, k, mode, state=state)
                        assert lists == [None if ps is None else ps[:k] for ps in every[2]], (seed, lo, K, k, mode)
                        assert counts == [min(c, k) for c in every[0]] and hops == every[1], (seed, lo, K, k, mode)
                        assert all(a >= b for a, b in zip(steps1, steps2))
                    rows += len(rs)
                    cut += sum(1 for c in every[0] if c > 2)
                    rejected += sum(1 for a, b in zip(every[0], walks[0]) if a < b)
    assert rows > 100000 and cut > 10000 and rejected > 10000 and shared > 20, (rows, cut, rejected, shared)


def test_none_and_walk_are_k_shortest_walks():
    for seed in range(40):
        fx = A.tiny_multigraph(seed)
        for lo, K, k in ((0, 3, 4), (1, 4, 2), (2, 3, M.K_ALL)):
            want = W.solve(*fx, lo, K, k)
            for mode in (M.NONE, M.WALK):
                counts, hops, lists, _, _, _ = M.search_model(*fx, lo, K, k, mode)
                assert lists == want[2] and hops == want[1], (seed, lo, K, k)
                assert counts == [min(c, k) for c in want[0]]  # min(walk_count, limit)


def test_leading_admitted_walks_are_all_shortestpaths_lists():
    """src != dst, lo <= d <= K: whatever the mode, the walks of d edges come first and are all_shortestpaths' lists."""
    checked = 0
    for seed in range(60):
        fx = M.random_shared(seed) if seed % 2 else A.tiny_multigraph(seed)
        V, off, adj, eid, rs, rd = fx
        shortest = A.solve(V, off, adj, eid, rs, rd, 4, A.MAX_PATHS_ALL)
        for mode in M.MODES:
            lists = M.search_model(*fx, 1, 4, M.K_ALL, mode)[2]
            for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
                if s != d and shortest[2][i] is not None:
                    assert lists[i][:len(shortest[2][i])] == shortest[2][i], (seed, mode, s, d)
                    checked += 1
    assert checked > 1000


def test_the_stop_rule_is_sound():
    """Searching over the tables of the rounds the rule asks for gives what searching over all K rounds gives (search_model does the
    former); k = 1 on a pair d >= lo apart asks for d rounds."""
    fx = W.chain8()
    counts, hops, lists, _, _, rounds = M.search_model(*fx, 0, M.MAX_HOPS, 1, M.TRAIL)
    assert rounds[3] == 5 and hops[3] == 5 and rounds[0] == 20
    V, off, adj, eid, rs, rd = M.detour()
    rounds = M.search_model(V, off, adj, eid, rs, rd, 2, 3, 1, M.ACYCLIC)[5]
    assert rounds[0] == 3  # (0, 1): distance 1 is below lo = 2, the row stays open


@pytest.fixture(scope="module")
def expected():
    """(name, lo, K, k, mode) -> (fixture, the model's answer), for the fixtures the GPU file runs (those of a kind once)."""
    out = {}
    for name, (fx, runs) in M.gpu_fixtures().items():
        if (name.startswith("sources") and name != "sources_65") or (name.startswith("in_list") and name != "in_list_129") or name == "parallel_run_63":
            continue
        state = {}
        for lo, K, ks, modes in runs:
            for k in ks:
                for mode in modes:
                    out[name, lo, K, k, mode] = (fx, M.search_model(*fx, lo, K, k, mode, state=state)[:5])
    return out


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_gpu_fixtures_catch_the_mutants(mutant, expected):
    states = {}
    caught = [key for key, (fx, good) in expected.items()
              if M.search_model(*fx, *key[1:], mutant=mutant, state=states.setdefault(key[0], {}))[:5] != good]
    assert caught, mutant
    names = {c[0] for c in caught}
    if mutant == "source_midwalk":  # the lists are the model's, the steps are not
        assert all(M.search_model(*expected[key][0], *key[1:], mutant=mutant)[:3] == expected[key][1][:3] for key in caught)
    if mutant == "trail_by_slot":
        assert names == {"pair_and_triangle"}
    if mutant == "stack_63":
        assert names == {"ring64"}
    if mutant == "m_mod_64":
        assert names <= {"parallel_run_65", "parallel_run_129"} and "parallel_run_65" in names
    if mutant == "stop_below_lo":
        assert "detour" in names
    if mutant in ("simple_as_acyclic", "acyclic_as_simple"):
        assert {"ring5", "self_loop", "two_loops"} <= names
    if mutant == "filter_first_k":
        assert "detour" in names and "pair_and_triangle" in names


def test_the_fixtures_are_what_their_names_say():
    fxs = M.gpu_fixtures()
    for deg in (63, 64, 65, 128, 129):
        V, off, adj, eid, rs, rd = fxs["in_list_%d" % deg][0]
        rin = A.in_lists(V, off, adj)
        assert [len(rin[d]) for d in rd[:4].tolist()] == [deg] * 4
        counts, hops, lists, steps1, _, _ = M.search_model(V, off, adj, eid, rs, rd, 0, 2, M.K_ALL, M.ACYCLIC)
        assert counts == [1, 1, 2, 2, 0] and lists[0][0][2] == rin[int(rd[0])][-1][0]  # the last slot
        assert steps1[0] == (deg + 63) // 64 + 2 + 1  # the trips over the list, two descents, the trip at the source's parent
    V, off, adj, eid, rs, rd = fxs["chain64"][0]
    assert [len(p) // 2 for p in M.search_model(V, off, adj, eid, rs, rd, 0, 64, 3, M.ACYCLIC)[2][0]] == [63, 64]
    for P in (63, 64, 65, 129):
        fx = fxs["parallel_run_%d" % P][0]
        counts = M.search_model(*fx, 3, 3, M.K_ALL, M.TRAIL)[0]
        assert counts[1] == P * (P - 1) and W.solve(*fx, 3, 3, 1)[0][1] == P * P
    fx = fxs["pair_and_triangle"][0]
    assert len(set(fx[3].tolist())) * 2 == len(fx[3])
    assert M.search_model(*fx, 2, 4, M.K_ALL, M.TRAIL)[2][0] is None and M.search_model(*fx, 2, 4, M.K_ALL, M.SIMPLE)[0][0] == 1
    counts, hops, lists, _, _, _ = M.search_model(*fxs["detour"][0], 2, 3, 1, M.ACYCLIC)
    assert hops[0] == 3 and W.solve(*fxs["detour"][0], 2, 3, 1)[1][0] == 2  # the shortest admitted walk is longer than the shortest walk


def test_every_layer_names_the_functions():
    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()

    hip = text("include", "pgq_hip.h")
    for name in ("pgq_walk_count_mode", "pgq_walk_count_mode_bulk_device", "pgq_k_shortest_walks_mode", "pgq_k_shortest_walks_mode_bulk_device",
                 "pgq_debug_mode_steps"):
        assert "int %s(" % name in hip, name
    for number, name in enumerate(("NONE", "WALK", "SIMPLE", "TRAIL", "ACYCLIC")):
        assert "#define PGQ_MODE_%s %d" % (name, number) in hip
    assert "#P-hard" in hip and "mode_step_cap" in hip
    udf = text("include", "pgq_udf.h")
    assert "int pgq_udf_walk_count_mode(" in udf and "int pgq_udf_k_shortest_walks_mode(" in udf
    glue = text("glue", "pgq_glue.cpp")
    assert "pgq_walk_count_mode(" in glue and "void WalkCountModeFunction(" in glue
    assert "pgq_k_shortest_walks_mode(" in glue and "void KShortestWalksModeFunction(" in glue
    binding = text("duckpgq-extension_amd", "binding.py")
    for name in ("walk_count_mode_bulk_ptr", "k_shortest_walks_mode_bulk_ptr", "mode_steps"):
        assert "def %s(" % name in binding, name
    assert "pgq_udf_walk_count_mode" in binding and "pgq_udf_k_shortest_walks_mode" in binding
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "k_shortest_walks_mode" in text(doc) and "mode_step_cap" in text(doc), doc
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "duckpgq-extension_amd", "csrc"), "glue-check"])


def test_both_libraries_export_the_symbols_and_the_option():
    import duckpgq_extension_amd as pgq

    L, U = pgq.load_hip(), pgq.load_udf()
    for name in ("pgq_walk_count_mode", "pgq_walk_count_mode_bulk_device", "pgq_k_shortest_walks_mode", "pgq_k_shortest_walks_mode_bulk_device",
                 "pgq_debug_mode_steps"):
        assert getattr(L, name) is not None
    for name in ("pgq_udf_walk_count_mode", "pgq_udf_k_shortest_walks_mode"):
        assert getattr(U, name) is not None
    assert pgq.get_default_option("mode_step_cap") == 1 << 24
    before = pgq.get_option("mode_step_cap")
    pgq.set_option("mode_step_cap", 1000)
    assert pgq.get_option("mode_step_cap") == 1000
    pgq.set_option("mode_step_cap", int(before))
    assert pgq.mode_steps() == (0, 0) or all(v >= 0 for v in pgq.mode_steps())
    assert (pgq.MODE_NONE, pgq.MODE_WALK, pgq.MODE_SIMPLE, pgq.MODE_TRAIL, pgq.MODE_ACYCLIC) == (M.NONE, M.WALK, M.SIMPLE, M.TRAIL, M.ACYCLIC)


def test_a_null_handle_is_answered_before_any_device_is_asked_for():
    import duckpgq_extension_amd as pgq

    L = pgq.load_hip()
    paths, used = ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert L.pgq_k_shortest_walks_mode_bulk_device(None, 1, None, None, 1, 3, 2, M.TRAIL, None, None, None, None, None, None, 0, None, 0,
                                                   ctypes.byref(paths), ctypes.byref(used)) == -4  # PGQ_ERR_INVALID_ARG
    assert paths.value == 0 and used.value == 0
    assert L.pgq_last_error().decode() == "NULL csr"
    assert L.pgq_walk_count_mode_bulk_device(None, 1, None, None, 1, 3, 5, M.SIMPLE, None) == -4
    vec = pgq.binding.Vec()
    po, pl, child = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    pt, clen = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.pgq_k_shortest_walks_mode(None, 1, 0, vec, vec, 1, 3, 2, M.ACYCLIC, None, None, None, ctypes.byref(po), ctypes.byref(pl), ctypes.byref(pt),
                                       ctypes.byref(child), ctypes.byref(clen)) == -4
    assert L.pgq_walk_count_mode(None, 1, 0, vec, vec, 1, 3, 5, M.TRAIL, None, None) == -4
    assert L.pgq_last_error().decode() == "NULL csr"
