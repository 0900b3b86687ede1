"""walk_length without a GPU: the Python model of its contract and of its two stages (walk_length_model.py) against a brute-force
enumeration of walks and walk_count's tables, the three identities that tie the call to k_shortest_walks(k = 1), walk_count and
iterativelength_within, the work partition against the upload's, the mutants the GPU fixtures must tell from the model, and the
layers that name the function."""
import os
import subprocess

import numpy as np
import pytest

import all_shortest_model as A
import k_walks_model as KW
import walk_length_model as W
from helpers import PULL_LIMITS, hub_slices_model, pull_parts_model
from oracle.pgq_oracle import OracleCSR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = ("push", "pull", "auto")


def test_model_against_brute_force_and_tables():
    """Every (src, dst) of 120 tiny multigraphs, src == dst included, every lower <= upper <= 5: the model in each direction and
    under both layouts against walk_count's tables, and against the enumeration of all walks where that stays in the hundreds."""
    closed, longer, none, brute_rows = 0, 0, 0, 0
    for seed in range(120):
        V, off, adj, eid, rs, rd = A.tiny_multigraph(seed)
        g = W.Graph(V, off, adj)
        deg = max(len(adj) / V, 1.0)
        Kb = max(k for k in range(2, 6) if k == 2 or deg ** k <= 250)
        brute = {s: KW.brute_force(V, off, adj, eid, s, Kb) for s in range(V)}
        tabs = {}
        for hi in range(6):
            for lo in range(hi + 1):
                want = W.reference(V, off, adj, rs, rd, lo, hi, tabs)
                for direction in DIRECTIONS:
                    for layout in (W.DEFAULT_LAYOUT, W.SMALL_LAYOUT):
                        got, stats = W.solve(V, off, adj, rs, rd, lo, hi, direction, layout, graph=g)
                        assert got == want, (seed, lo, hi, direction, layout)
                        assert stats["levels"] == stats["push_levels"] + stats["pull_levels"] and (lo > 0 or stats["batches"] == 0)
                if hi <= Kb:
                    for i, (s, d) in enumerate(zip(rs.tolist(), rd.tolist())):
                        lens = [len(p) // 2 for p in brute[s][d] if lo <= len(p) // 2 <= hi]
                        assert want[i] == (min(lens) if lens else -1), (seed, lo, hi, s, d)
                        brute_rows += 1
                dist = [g.dist(s).get(d, -1) for s, d in zip(rs.tolist(), rd.tolist())]
                closed += sum(1 for w, s, d in zip(want, rs.tolist(), rd.tolist()) if s == d and w > 0)
                longer += sum(1 for w, dd in zip(want, dist) if 0 <= dd < lo and w > 0)
                none += sum(1 for w, dd in zip(want, dist) if 0 <= dd < lo and w < 0)
    assert closed > 1000 and longer > 1000 and none > 300 and brute_rows > 10000, (closed, longer, none, brute_rows)


@pytest.fixture(scope="module")
def medium():
    fx = A.random_fixture()
    V, off, adj, eid, rs, rd = fx
    rs, rd = rs.copy(), rd.copy()
    rd[::9] = rs[::9]  # closed rows among the others
    ln, ok = OracleCSR.adopt(V, off, adj, eid).iterativelength(V, rs, rd)
    return (V, off, adj, eid, rs, rd), np.where(ok, ln, -1).tolist()


@pytest.mark.parametrize("lo,hi", [(0, 3), (1, 3), (2, 4), (3, 3), (0, 0), (4, 5)])
def test_the_three_identities(medium, lo, hi):
    (V, off, adj, eid, rs, rd), dist = medium
    got = W.solve(V, off, adj, rs, rd, lo, hi, "pull")[0]
    assert got == W.solve(V, off, adj, rs, rd, lo, hi, "push")[0]
    counts, hops, _, _ = KW.solve(V, off, adj, eid, rs, rd, lo, hi, 1)
    assert got == hops  # 1. k_shortest_walks(k = 1)'s hops
    assert [x >= 0 for x in got] == [c > 0 for c in counts]  # 2. non-NULL exactly where walk_count > 0
    within = [d if 0 <= d <= hi else -1 for d in dist]  # iterativelength_within(hi) from the oracle's iterativelength
    inside = [i for i, d in enumerate(dist) if lo <= d <= hi]
    assert len(inside) >= 30 or hi == 0
    assert all(got[i] == within[i] for i in inside)  # 3. for lower <= dist <= upper
    if lo == 0:
        assert got == within
    else:
        assert sum(1 for g, w in zip(got, within) if g != w) >= 10  # where the reference's filter is wrong


def test_the_partition_is_the_uploads():
    """walk_length_model.partition restates pgq_csr_pull_layout's description; helpers.pull_parts_model / hub_slices_model are
    checked against the device's partition by the expansion tests."""
    assert W.DEFAULT_LAYOUT == (PULL_LIMITS["part_weight"], PULL_LIMITS["hub_chunk"]) and W.SMALL_LAYOUT == (PULL_LIMITS["min_option"],) * 2
    rng = np.random.default_rng(4)
    for trial in range(20):
        V = int(rng.integers(1, 700))
        deg = rng.integers(0, 12, V)
        deg[rng.integers(0, V, 6)] = rng.integers(60, 300, 6)
        roff = np.concatenate([[0], np.cumsum(deg)])
        for layout in (W.SMALL_LAYOUT, W.DEFAULT_LAYOUT, (100, 130)):
            parts, hubs, slices = W.partition(roff, *layout)
            want_parts, want_hubs = pull_parts_model(roff, *layout)
            assert parts == [tuple(p) for p in want_parts.tolist()] and hubs == want_hubs.tolist()
            assert slices == [tuple(s) for s in hub_slices_model(roff, want_hubs, layout[1]).tolist()]
            covered = sorted([v for b, e in parts for v in range(b, e)] + hubs)
            assert covered == list(range(V))  # every vertex's word is written by a pull


def test_fixtures_say_what_they_claim():
    ring = lambda lo, hi: W.solve(*KW.ring(5)[:3], [0], [0], lo, hi)  # noqa: E731
    assert [ring(*b)[0] for b in ((1, 4), (1, 5), (6, 10), (0, 3))] == [[-1], [5], [10], [0]]
    assert W.solve(*KW.self_loop()[:3], [0], [0], 1, 1)[0] == [1]
    V, off, adj, eid, rs, rd = W.pair()
    assert W.solve(V, off, adj, rs, rd, 2, 2)[0][0] == -1 and W.solve(V, off, adj, rs, rd, 2, 3)[0][0] == 3
    V, off, adj, eid, rs, rd = W.chain3()
    for direction in DIRECTIONS:
        got, stats = W.solve(V, off, adj, rs, rd, 3, 5, direction)
        assert got == [-1] and stats["levels"] == 3 and stats["rest"] == 1  # round 3 activates nothing: the rounds end there, not at 5
    for deg in W.LIST_DEGREES:
        V, off, adj, eid, rs, rd = W.last_slot_gadget(deg)
        g = W.Graph(V, off, adj)
        x = int(rd[0])
        assert g.roff[x + 1] - g.roff[x] == deg and g.dist(0)[x] == 1
        live = [k for k in range(g.roff[x], g.roff[x + 1]) if g.dist(0).get(g.radj[k]) == 2]
        assert live == [g.roff[x + 1] - 1]  # the one parent with a walk of 2 edges sits in the last slot
        parts, hubs, slices = g.parts(W.SMALL_LAYOUT)
        assert (x in hubs) == (deg > 64) and g.parts(W.DEFAULT_LAYOUT)[1] == []
        if deg > 64:
            mine = [s for s in slices if s[0] == x]
            assert len(mine) == -(-deg // 64) and mine[-1][2] - mine[-1][1] == (deg - 1) % 64 + 1
            assert live[0] >= mine[-1][1] and all(live[0] >= s[2] for s in mine[:-1])  # only the last slice holds the witness
    for n in W.SOURCE_COUNTS:
        V, off, adj, eid, rs, rd = W.many_sources(n)
        got, stats = W.solve(V, off, adj, rs, rd, 1, 3)
        assert stats["rest"] == n and stats["batches"] == -(-n // 64), (n, stats)
    V, off, adj, eid, rs, rd = W.wide_exit()
    good, bad = (W.solve(V, off, adj, rs, rd, 3, 5, "pull", mutant=m)[1]["edges"] for m in (None, "exit_all_ones"))
    assert bad - good == 2 * (300 - 128)  # y's list is walked in rounds 2 and 5 while a row is open: 128 of 300 entries each


@pytest.fixture(scope="module")
def expected():
    """(name, lo, hi, layout, direction) -> (fixture, graph, the model's answers and statistics), for the fixtures the GPU file runs
    (those of a kind once, the largest bounds of the random graph left to the GPU file)."""
    out = {}
    for name, (fx, bounds, layouts) in W.gpu_fixtures().items():
        if (name.startswith("sources") and name != "sources_129") or (name.startswith("last_slot") and name not in ("last_slot_64", "last_slot_65")):
            continue
        g = W.Graph(*fx[:3])
        for lo, hi in bounds:
            if hi - lo > 40 and name == "random":
                continue
            for layout in layouts:
                for direction in DIRECTIONS:
                    out[name, lo, hi, layout, direction] = (fx, g, W.solve(*fx[:3], fx[4], fx[5], lo, hi, direction, layout, graph=g))
    return out


@pytest.mark.parametrize("mutant", W.MUTANTS)
def test_the_gpu_fixtures_catch_the_mutants(mutant, expected):
    """In the answers, or — where a mutant only wastes or saves work — in the statistics the GPU file compares."""
    by_answer, by_stats = set(), set()
    for key, (fx, g, (good, good_stats)) in expected.items():
        name, lo, hi, layout, direction = key
        got, stats = W.solve(*fx[:3], fx[4], fx[5], lo, hi, direction, layout, mutant=mutant, graph=g)
        if got != good:
            by_answer.add((name, direction, layout))
        elif stats != good_stats:
            by_stats.add((name, direction, layout))
    names = {c[0] for c in by_answer}
    if mutant in ("visited", "src_eq_dst_zero"):
        assert {"ring5", "self_loop", "pair", "random"} <= names
    if mutant in ("lower_ignored", "t_gt_lower", "far_rows_answered"):
        assert "random" in names and ("pair" in names or mutant == "far_rows_answered")
    if mutant == "trip_last_slot":
        assert ("last_slot_64", "pull", W.DEFAULT_LAYOUT) in by_answer and not any(c[1] == "push" for c in by_answer)
    if mutant == "hub_last_slice":
        assert ("last_slot_65", "pull", W.SMALL_LAYOUT) in by_answer and not any(c[2] == W.DEFAULT_LAYOUT for c in by_answer)
    if mutant == "exit_all_ones":
        assert not by_answer and ("wide_exit", "pull", W.DEFAULT_LAYOUT) in by_stats
    if mutant == "stop_early":
        assert not by_answer and {c[0] for c in by_stats} >= {"chain3"}
    if mutant == "masks_not_zeroed":
        assert ("sources_129", "pull", W.DEFAULT_LAYOUT) in by_answer and not any(c[1] == "push" for c in by_answer)
    assert by_answer or by_stats, mutant


def test_every_layer_names_the_function():
    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()

    hip = text("include", "pgq_hip.h")
    for name in ("pgq_walk_length", "pgq_walk_length_bulk_device"):
        assert "int %s(" % name in hip, name
    assert "int pgq_udf_walk_length(" in text("include", "pgq_udf.h")
    glue = text("glue", "pgq_glue.cpp")
    assert "pgq_walk_length(" in glue and "void WalkLengthFunction(" in glue
    binding = text("duckpgq-extension_amd", "binding.py")
    for name in ("walk_length", "walk_length_bulk_ptr"):
        assert "def %s(" % name in binding, name
    assert "pgq_udf_walk_length" in binding
    kernels = text("duckpgq-extension_amd", "csrc", "pgq_walk_length.hip")
    assert "void k_wl_pull(" in kernels and "void k_wl_after(" in kernels and "k_walk_activate" in kernels
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        assert "walk_length" in text(doc), doc
    assert "IS NOT NULL" in text("INTEGRATION.md") and "3.9i" in text("DESIGN.md")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "duckpgq-extension_amd", "csrc"), "glue-check"])


def test_both_libraries_export_the_symbols_and_the_options_exist():
    import duckpgq_extension_amd as pgq

    L, U = pgq.load_hip(), pgq.load_udf()
    for name in ("pgq_walk_length", "pgq_walk_length_bulk_device"):
        assert getattr(L, name) is not None
    assert getattr(U, "pgq_udf_walk_length") is not None
    assert pgq.get_default_option("walk_length_pull") == 2
    assert pgq.get_default_option("walk_length_pull_div") == W.PULL_DIV


def test_a_null_handle_is_answered_before_any_device_is_asked_for():
    import duckpgq_extension_amd as pgq

    L = pgq.load_hip()
    assert L.pgq_walk_length_bulk_device(None, 1, None, None, 1, 3, None) == -4  # PGQ_ERR_INVALID_ARG
    assert L.pgq_last_error().decode() == "NULL csr"
    vec = pgq.binding.Vec()
    assert L.pgq_walk_length(None, 1, 0, vec, vec, 1, 3, None, None) == -4
    assert L.pgq_last_error().decode() == "NULL csr"
