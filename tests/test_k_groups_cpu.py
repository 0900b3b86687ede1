"""k_shortest_groups (SHORTEST k GROUP) without a GPU: the Python model (k_groups_model.py) against a brute-force enumeration of every
walk of at most 5 edges filtered by the mode and grouped by length; the three identities against all_shortestpaths', k_shortest_walks'
and the path modes' models; the mutants the GPU fixtures must tell from the model.  Also: every layer names the new calls, both
libraries export them, and a NULL handle is answered before any device is asked for."""
import ctypes
import os
import subprocess

import pytest

import all_shortest_model as A
import k_groups_model as G
import k_walks_model as W
import path_modes_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("lists", "npaths", "ngroups", "count", "len")


def test_model_against_the_grouped_enumeration():
    """25 random multigraphs of at most 7 vertices and 12 slots (every second one with shared ids), every (src, dst), the five modes,
    K = 5 and K = 3 with every lo, g in {1, 2, 3, all}, P in {1, 2, 4, all}."""
    rows = cut = cut_inside = gaps = 0
    for seed in range(25):
        fx = M.random_shared(seed)
        state, brute = {}, {}
        for K in (5, 3):
            for lo in range(K + 1):
                for mode in G.ALL_MODES:
                    for g in (1, 2, 3, G.G_ALL):
                        for P in (1, 2, 4, G.P_ALL):
                            got = G.groups_model(*fx, lo, K, g, P, mode, state=state)
                            want = G.brute_groups(*fx, lo, K, g, P, mode, brute=brute.setdefault(K, {}))
                            for key in KEYS:
                                assert got[key] == want[key], (seed, lo, K, g, P, mode, key)
                            assert all(a >= b for a, b in zip(got["steps1"], got["steps2"]))
                            rows += len(fx[4])
                            cut += sum(1 for c, n in zip(got["count"], got["npaths"]) if c > n)
                            cut_inside += sum(1 for ps, c, n in zip(got["lists"], got["count"], got["npaths"])
                                              if c > n and len(ps[-1]) > len(ps[0]) and P > 1)
                            gaps += sum(1 for ps in got["lists"] if ps and len({len(p) for p in ps}) > 1 and len(ps[-1]) - len(ps[0]) > 2 * (len({len(p) for p in ps}) - 1))
    # rows answered; rows the cap cut; ... inside a later group; rows whose groups have an empty or refused length between them
    assert rows > 500000 and cut > 30000 and cut_inside > 5000 and gaps > 2000, (rows, cut, cut_inside, gaps)


def test_identity_1_one_group_is_all_shortestpaths():
    for seed in range(40):
        fx = M.random_shared(seed)
        V, off, adj, eid, rs, rd = fx
        for lo, K, P in ((0, 4, 3), (1, 5, G.P_ALL), (2, 3, 1)):
            counts, hops, lists = A.solve(*fx, K, P)
            for mode in (G.NONE, G.WALK):
                got = G.groups_model(*fx, lo, K, 1, P, mode)
                for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
                    if s != d and hops[i] >= lo:  # (hops -1: farther than K or unreachable)
                        assert got["lists"][i] == lists[i] and got["len"][i] == hops[i], (seed, lo, K, P, s, d)


def test_identity_2_every_group_is_k_shortest_walks_mode():
    for seed in range(40):
        fx = M.random_shared(seed)
        state, mstate = {}, {}
        for lo, K, P in ((0, 4, 3), (1, 5, G.P_ALL), (2, 3, 1), (3, 5, 7)):
            walks = W.solve(*fx, lo, K, P)[2]
            for g in (K - lo + 1, K - lo + 2, G.G_ALL):
                for mode in (G.NONE, G.WALK):
                    assert G.groups_model(*fx, lo, K, g, P, mode, state=state)["lists"] == walks
                for mode in G.MODES:
                    want = M.search_model(*fx, lo, K, P, mode, state=mstate)
                    got = G.groups_model(*fx, lo, K, g, P, mode, state=state)
                    assert got["lists"] == want[2] and got["npaths"] == want[0] and got["len"] == want[1], (seed, lo, K, P, g, mode)
                    assert got["steps2"] == want[4]  # the emitting pass is the same search


def test_identity_3_one_path_is_shortestpath():
    for seed in range(40):
        fx = M.random_shared(seed)
        V, off, adj, eid, rs, rd = fx
        counts, hops, lists = A.solve(*fx, 5, 1)
        for lo in (0, 1, 2):
            for g in (1, 3):
                for mode in G.ALL_MODES:
                    got = G.groups_model(*fx, lo, 5, g, 1, mode)
                    for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
                        if s != d and hops[i] >= lo:
                            assert got["lists"][i] == [lists[i][0]] and got["ngroups"][i] == 1, (seed, lo, g, mode, s, d)


def test_what_the_contract_says_on_the_gadgets():
    fxs = G.gpu_fixtures()
    b = fxs["boundary"][0]
    r = G.groups_model(*b, 0, 5, 2, 3, G.WALK)  # P on the boundary, a later non-empty length inside K: count P + 1, one group emitted
    assert (r["npaths"][0], r["ngroups"][0], r["count"][0], r["len"][0]) == (3, 1, 4, 2)
    r = G.groups_model(*b, 2, 2, 2, 3, G.WALK)  # ... and none: the cap did not cut
    assert (r["npaths"][0], r["ngroups"][0], r["count"][0]) == (3, 1, 3)
    r = G.groups_model(*b, 0, 5, 2, 4, G.WALK)  # a cut inside group 2: it counts
    assert (r["npaths"][0], r["ngroups"][0], r["count"][0]) == (4, 2, 5) and [len(p) // 2 for p in r["lists"][0]] == [2, 2, 2, 3]
    r = G.groups_model(*b, 0, 5, 3, G.P_ALL, G.TRAIL)  # the loop twice is no trail: two groups, however many are asked for
    assert (r["npaths"][0], r["ngroups"][0], r["count"][0]) == (6, 2, 6)
    assert G.groups_model(*b, 0, 5, 3, G.P_ALL, G.ACYCLIC)["ngroups"][0] == 1
    gap = fxs["gap"][0]
    assert [[len(p) // 2 for p in G.groups_model(*gap, 0, 5, 3, G.P_ALL, m)["lists"][0]] for m in (G.WALK, G.TRAIL, G.SIMPLE)] == \
        [[1, 2, 3], [1, 2, 4], [1, 4]]
    bip = fxs["bipartite"][0]
    assert [len(p) // 2 for p in G.groups_model(*bip, 0, 6, 3, G.P_ALL, G.WALK)["lists"][0]] == [2, 2, 4, 4, 6, 6]  # d, d + 2, d + 4
    assert [len(p) // 2 for p in G.groups_model(*bip, 3, 7, 2, G.P_ALL, G.NONE)["lists"][0]] == [4, 4, 6, 6]  # lo above the distance
    ring = fxs["ring5"][0]
    assert [len(p) // 2 for p in G.groups_model(*ring, 0, 12, 3, G.P_ALL, G.WALK)["lists"][1]] == [2, 7, 12]  # d, d + n, d + 2 n
    r = G.groups_model(*ring, 0, 12, 2, G.P_ALL, G.ACYCLIC)  # src == dst, lo = 0: [src] is group 1, under ACYCLIC the only one
    assert r["lists"][0] == [[0]] and r["ngroups"][0] == 1
    assert [len(p) // 2 for p in G.groups_model(*ring, 0, 12, 2, G.P_ALL, G.SIMPLE)["lists"][0]] == [0, 5]
    assert [len(p) // 2 for p in G.groups_model(*ring, 1, 12, 2, G.P_ALL, G.WALK)["lists"][0]] == [5, 10]  # lo = 1: no empty walk
    loop = fxs["self_loop"][0]
    assert G.groups_model(*loop, 0, 4, G.G_ALL, G.P_ALL, G.WALK)["ngroups"][0] == 5  # a self-loop: every length is a group
    r = G.groups_model(*loop, 0, 4, 1, 1, G.WALK)
    assert r["lists"][5] == [[2]] and r["count"][5] == 1 and r["ngroups"][5] == 1  # (2, 2): no lane
    r = G.groups_model(*loop, 1, 3, 1, 1, G.WALK)
    assert r["lists"][5] is None and r["count"][5] == 0 and r["ngroups"][5] == 0 and r["len"][5] == -1
    chain = fxs["chain64"][0]
    assert [len(p) // 2 for p in G.groups_model(*chain, 0, 64, 2, G.P_ALL, G.ACYCLIC)["lists"][0]] == [63, 64]
    for deg in (63, 64, 65, 128, 129):
        r = G.groups_model(*fxs["in_list_%d" % deg][0], 0, 3, 2, G.P_ALL, G.ACYCLIC)
        assert r["npaths"] == [2, 2, 0] and r["ngroups"] == [2, 2, 0] and r["steps1"][0] >= 2 + (deg + 63) // 64


def _runs(name, fxs):
    fx, runs = fxs[name]
    for lo, K, gs, Ps, modes in runs:
        for mode in modes:
            for g in gs:
                for P in Ps:
                    yield fx, lo, K, g, P, mode


# the fixtures on which a mutant is looked for (it must differ on at least one of their runs)
WHERE = {"mode_group_by_w": ("gap",), "empty_length_group": ("bipartite",), "below_lo_group": ("gap", "bipartite"), "groups_as_k": ("boundary",),
         "cut_group_dropped": ("boundary",), "ngroups_planned": ("boundary",), "close_at_ge": ("boundary",), "mode_close_at_distance": ("gap",),
         "count_uncapped": ("boundary",)}


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_the_gpu_fixtures_catch_every_mutant(mutant):
    fxs = G.gpu_fixtures()
    caught = []
    for name in WHERE[mutant]:
        for fx, lo, K, g, P, mode in _runs(name, fxs):
            good, bad = G.groups_model(*fx, lo, K, g, P, mode), G.groups_model(*fx, lo, K, g, P, mode, mutant=mutant)
            if any(good[key] != bad[key] for key in KEYS + ("rounds", "steps1", "steps2")):
                caught.append((name, lo, K, g, P, mode, [key for key in KEYS + ("rounds", "steps1", "steps2") if good[key] != bad[key]]))
    assert caught, mutant
    if mutant in ("mode_group_by_w", "mode_close_at_distance"):
        assert all(c[5] in G.MODES for c in caught)
    if mutant == "close_at_ge":  # the count on the boundary, and the rounds
        assert any("count" in c[6] for c in caught) and any("rounds" in c[6] for c in caught)


def test_every_layer_names_the_functions():
    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()

    hip = text("include", "pgq_hip.h")
    for name in ("pgq_k_shortest_groups", "pgq_k_shortest_groups_bulk_device"):
        assert "int %s(" % name in hip, name
    assert "SHORTEST k GROUP" in hip and "_multi forms; a count-only form; an unbounded upper; several wavefronts per row; a split of long in-lists" in hip
    assert "int pgq_udf_k_shortest_groups(" in text("include", "pgq_udf.h")
    assert "int pgq_udf_k_shortest_groups(" in text("duckpgq-extension_amd", "csrc", "pgq_udf.cpp")
    glue = text("glue", "pgq_glue.cpp")
    assert "pgq_k_shortest_groups(" in glue and "void KShortestGroupsFunction(" in glue
    binding = text("duckpgq-extension_amd", "binding.py")
    for name in ("k_shortest_groups", "k_shortest_groups_bulk_ptr"):
        assert "def %s(" % name in binding, name
    assert binding.count("def k_shortest_groups(") == 2 and "pgq_udf_k_shortest_groups" in binding  # DeviceCSR and PgqState
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "k_shortest_groups" in text(doc), doc
    assert "3.9h" in text("DESIGN.md")
    for path in (("README.md",), ("DESIGN.md",), ("include", "pgq_hip.h"), ("duckpgq-extension_amd", "csrc", "pgq_k_walks.hip")):
        for line in text(*path).splitlines():  # no longer among what is not built
            assert not ("SHORTEST k GROUP" in line and ("Not built" in line or "NOT BUILT" in line or "not built" in line)), (path, line)
    for src in (("duckpgq-extension_amd", "csrc", "pgq_k_walks.hip"), ("duckpgq-extension_amd", "csrc", "pgq_path_modes.h")):
        assert "pgq_k_shortest_groups" in text(*src), src
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "duckpgq-extension_amd", "csrc"), "glue-check"])


def test_both_libraries_export_the_symbols():
    import duckpgq_extension_amd as pgq

    L, U = pgq.load_hip(), pgq.load_udf()
    for name in ("pgq_k_shortest_groups", "pgq_k_shortest_groups_bulk_device"):
        assert getattr(L, name).argtypes is not None, name
    assert U.pgq_udf_k_shortest_groups.argtypes is not None
    assert callable(pgq.DeviceCSR.k_shortest_groups) and callable(pgq.DeviceCSR.k_shortest_groups_bulk_ptr) and callable(pgq.PgqState.k_shortest_groups)


def test_a_null_handle_is_answered_before_any_device_is_asked_for():
    import duckpgq_extension_amd as pgq

    L = pgq.load_hip()
    paths, used = ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert L.pgq_k_shortest_groups_bulk_device(None, 1, None, None, 1, 3, 2, 5, G.TRAIL, None, None, None, None, None, None, None, 0, None, 0,
                                               ctypes.byref(paths), ctypes.byref(used)) == -4  # PGQ_ERR_INVALID_ARG
    assert paths.value == 0 and used.value == 0
    assert L.pgq_last_error().decode() == "NULL csr"
    vec = pgq.binding.Vec()
    po, pl, child = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    pt, clen = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.pgq_k_shortest_groups(None, 1, 0, vec, vec, 1, 3, 2, 5, G.ACYCLIC, None, None, None, None, ctypes.byref(po), ctypes.byref(pl), ctypes.byref(pt),
                                   ctypes.byref(child), ctypes.byref(clen)) == -4
    assert L.pgq_last_error().decode() == "NULL csr" and (pt.value, clen.value) == (7, 7)  # a failed call has written nothing
