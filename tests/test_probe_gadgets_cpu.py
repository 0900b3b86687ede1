"""helpers.probe_gadgets is what test_probe_limits_gpu.py assumes: checked here with numpy and the CPU oracle alone.

Every row's distance is the oracle's; every gadget's witness sits at the stated position of the in-list as the upload orders
it (source id, then slot), the in-degree sums are the stated walk sizes, and without the edge into the destination (or out of
the source) the row is unreachable, so the path through that position is the only one.  The constants the gadgets stand on
are read back from pgq_msbfs.hip and pgq_internal.h.  A plain model of the three scans — one wavefront, 64 entries per trip
(k_probe); 1024 threads x 4 entries per step (k_probe's hub queue); 16 wavefronts striding N_in(dst), each 64 entries per
trip (k_probe2) — answers every row like the oracle, and each of its mutants, one per way such a scan loses an entry,
answers at least one row differently: the fixtures can see the faults they are built for."""
import os
import re

import numpy as np
import pytest

from helpers import (PROBE2_CAP, PROBE2_FAN_POSITIONS, PROBE2_FANS, PROBE2_LIST_POSITIONS, PROBE2_LISTS, PROBE_DEGREES,
                     PROBE_LIMITS, PROBE_POSITIONS, csr_arrays_from_rows, probe_gadgets)
from oracle.pgq_oracle import OracleCSR

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "duckpgq-extension_amd", "csrc")


class Built:
    def __init__(self, g):
        self.g = g
        self.off, self.adj, _ = csr_arrays_from_rows(g.V, g.src, g.dst)
        # in-lists as the upload builds them: the transpose's rows sorted by source id (stable), then by destination (stable)
        by_src = np.argsort(g.src, kind="stable")
        self.roff, self.radj, _ = csr_arrays_from_rows(g.V, g.dst[by_src], g.src[by_src])
        self.indeg = np.diff(self.roff)

    def out_list(self, v):
        return self.adj[self.off[v]:self.off[v + 1]]

    def in_list(self, v):
        return self.radj[self.roff[v]:self.roff[v + 1]]


@pytest.fixture(scope="module")
def built():
    return Built(probe_gadgets())


def oracle_dist(g, src=None, dst=None):
    ora = OracleCSR.from_edges(g.V, g.src if src is None else src, g.dst if dst is None else dst)
    ln, ok = ora.lean_iterativelength(g.V, g.rs, g.rd, nthreads=8)
    return np.where(ok, ln, -1)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def test_oracle_distances(built):
    g = built.g
    got = oracle_dist(g)
    bad = np.flatnonzero(got != g.dist)
    assert len(bad) == 0, (g.tag[bad[0]], int(got[bad[0]]), int(g.dist[bad[0]]))
    assert set(g.dist.tolist()) == {-1, 0, 1, 2, 3}
    assert len(set(g.tag.tolist())) == len(g.tag), "tags name one row each"
    assert g.src.min() >= 0 and g.src.max() < g.V and g.dst.min() >= 0 and g.dst.max() < g.V


@pytest.mark.parametrize("which", ["last_edge", "first_edge"])
def test_the_path_through_the_position_is_the_only_one(built, which):
    # every gadget's last (first) path edge removed at once: the gadgets' paths are disjoint, and each row is unreachable
    g = built.g
    cut = {(x["path"][-2], x["path"][-1]) if which == "last_edge" else (x["path"][0], x["path"][1]) for x in g.gadgets}
    keep = ~np.isin(g.src * g.V + g.dst, [s * g.V + d for s, d in cut])
    assert (~keep).sum() == len(g.gadgets), "one table row per path edge"
    got = oracle_dist(g, g.src[keep], g.dst[keep])
    rows = g.rows_where(lambda x: True)
    assert (got[rows] == -1).all(), g.tag[rows[got[rows] != -1]][:5]


# ---- positions and walk sizes -------------------------------------------------------------------------------------------
def test_positions_and_walks(built):
    g = built.g
    assert (built.indeg[:8192] == 0).all() and (built.indeg[-8192:] == 0).all(), "a decoy is in no frontier"
    for x in g.gadgets:
        inn = built.in_list(x["dst"])
        assert len(inn) == x["b"] and inn[x["p"]] == x["path"][-2] and (inn == x["path"][-2]).sum() == 1, x["tag"]
        assert (built.indeg[np.delete(inn, x["p"])] == 0).all() or x["kind"] == "two", x["tag"]
        assert len(x["path"]) == x["k"] + 1
        for u, v in zip(x["path"][:-1], x["path"][1:]):
            assert v in built.out_list(u), x["tag"]
        if x["kind"] == "two":
            mid = built.in_list(x["path"][-2])
            assert len(mid) == x["n"] and mid[x["pv"]] == x["path"][-3] and (mid == x["path"][-3]).sum() == 1, x["tag"]
            assert (built.indeg[np.delete(mid, x["pv"])] == 0).all(), x["tag"]
            assert int(built.indeg[inn].sum()) == x["walk"] == g.walk[x["row"]], x["tag"]
            for u in np.delete(inn, x["p"]):  # the other in-neighbours' lists are decoys
                assert (built.indeg[built.in_list(u)] == 0).all(), x["tag"]
        assert g.b[x["row"]] == x["b"] and g.p[x["row"]] == x["p"]
    for r in np.flatnonzero(g.kind == "indeg0"):
        assert built.indeg[g.rd[r]] == 0
    for r in np.flatnonzero(g.kind == "decoys"):
        inn = built.in_list(g.rd[r])
        assert len(inn) == g.b[r] and (built.indeg[inn] == 0).all()
    assert (g.rs[g.kind == "self"] == g.rd[g.kind == "self"]).all()


def test_every_cell_of_the_lists_exists(built):
    g = built.g
    idx = lambda pos, n: n - 1 if pos == "last" else pos
    for k in (1, 2, 3):
        have = {(x["b"], x["p"]) for x in g.gadgets if x["kind"] == "one" and x["k"] == k}
        want = {(b, idx(pos, b)) for b in PROBE_DEGREES for pos in PROBE_POSITIONS if idx(pos, b) < b}
        assert have == want, (k, want - have)
    two = [x for x in g.gadgets if x["kind"] == "two"]
    fans = {(b1, idx(pos, b1)) for b1 in PROBE2_FANS for pos in PROBE2_FAN_POSITIONS if idx(pos, b1) < b1}
    lists = {(n, idx(pos, n)) for n in PROBE2_LISTS for pos in PROBE2_LIST_POSITIONS}
    assert {(x["b"], x["p"]) for x in two} == fans
    for f in fans:
        at = {(x["n"], x["pv"]) for x in two if (x["b"], x["p"]) == f and x["k"] == 2 and (x["walk"] == PROBE2_CAP or f[0] == 1)}
        assert at == lists, f
        if f[0] > 1:
            for k in (2, 3):
                assert {x["walk"] - PROBE2_CAP for x in two if (x["b"], x["p"]) == f and x["k"] == k} == {-1, 0, 1}, (f, k)
    assert {g.b[r] for r in np.flatnonzero(g.kind == "decoys")} >= {64, 65, 4096, 4097}
    assert (g.kind == "indeg0").sum() >= 8 and (g.kind == "self").sum() >= 8
    # enough distance-2 rows within the cap, each with a source of its own, for test_probe_limits_gpu.py's calls of 64 rows
    near = g.rows_where(lambda x: x["kind"] == "two" and x["k"] == 2 and x["walk"] <= PROBE2_CAP)
    assert len(near) >= 128 and len(set(g.rs[near].tolist())) == len(near)


# ---- the constants ---------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    with open(os.path.join(CSRC, "pgq_msbfs.hip")) as f:
        msbfs = f.read()
    with open(os.path.join(CSRC, "pgq_internal.h")) as f:
        internal = f.read()
    num = lambda text, pattern: eval(re.search(pattern, text).group(1), {})  # "1 << 16", "4 * 1024": plain integer arithmetic
    probe = msbfs[msbfs.index("void k_probe("):msbfs.index("void k_probe2(")]
    got = {
        "kQueue": num(probe, r"constexpr int kQueue = ([0-9 <*]+);"),
        "kHubQueue": num(probe, r"constexpr int kHubQueue = ([0-9 <*]+);"),
        "kOpenGrid": num(msbfs, r"constexpr int kOpenGrid = ([0-9 <*]+);"),
        "hub_step": num(probe, r"for \(int64_t base = b; base < e; base \+= ([0-9 <*]+)\)"),
        "probe_max_in": num(internal, r"int probe_max_in = ([0-9 <*]+);"),
        "probe2_cap": num(internal, r"int probe2_cap = ([0-9 <*]+);"),
    }
    assert got == PROBE_LIMITS
    # the hub step is 4 entries per thread of a 1024-thread workgroup, and the row-count edges follow from the grid
    assert "j = base + u * 1024 + threadIdx.x" in probe and "__launch_bounds__(1024) void k_probe(" in msbfs
    assert PROBE_LIMITS["kOpenGrid"] * 16 == 8192 and PROBE_LIMITS["kOpenGrid"] * 16 * 64 // 2 == 262_144
    # the gadgets straddle every one of them
    for lim in (64, PROBE_LIMITS["kQueue"], PROBE_LIMITS["hub_step"], PROBE_LIMITS["probe_max_in"], 2 * PROBE_LIMITS["hub_step"]):
        assert {lim - 1, lim, lim + 1} <= set(PROBE_DEGREES), lim
    assert PROBE2_CAP < PROBE_LIMITS["probe2_cap"]


# ---- a model of the scans, and its mutants ---------------------------------------------------------------------------------
def wave_scan(hits, mut):
    """One wavefront, 64 entries per trip, until a trip has a hit (probe_row; k_probe2's inner loop)."""
    for trip, base in enumerate(range(0, len(hits), 64)):
        lanes = hits[base:base + 64].copy()
        if "lane63" in mut and len(lanes) == 64:
            lanes[63] = False
        if "trip2_first" in mut and trip == 1:
            lanes[0] = False
        if lanes.any():
            return True
    return False


def hub_scan(hits, mut):
    """1024 threads, 4 entries each per step, until a step has a hit (k_probe's hub queue)."""
    if "hub_blind" in mut:
        return False
    step = PROBE_LIMITS["hub_step"]
    for base in range(0, len(hits), step):
        if "last_partial" in mut and len(hits) - base < step:
            break
        part = hits[base:base + step].copy()
        for name, at in (("entry1023", 1023), ("entry1024", 1024)):
            if name in mut and len(part) > at:
                part[at] = False
        if part.any():
            return True
    return False


def member(ids, front):
    return (ids[:, None] == front[None, :]).any(axis=1)


class Model:
    """The lane batches' way to a row's answer with a probe pair before every level: k_probe(t) looks for an in-neighbour of dst
    in frontier t - 1, k_probe2(t) for one two hops back, the expansion of level t follows while the row is open.  Returns
    (hop count or -1, expansions that ran before the answer).  probe2 = False: option probe2 0, k_probe alone (the one-hop
    gadgets' setting: k_probe2 would answer a chain's end a level before k_probe scans the list the gadget is about)."""

    def __init__(self, built, max_in, cap, mut=(), probe2=True):
        self.b, self.max_in, self.cap, self.mut, self.with_probe2 = built, max_in, cap, set(mut), probe2

    def fronts(self, s):
        seen, front, out = {s}, [s], []
        while front:
            out.append(np.array(front, dtype=np.int64))
            nxt = []
            for u in front:
                for v in self.b.out_list(u).tolist():
                    if v not in seen:
                        seen.add(v)
                        nxt.append(v)
            front = nxt
        return out

    def probe(self, d, front):
        inn = self.b.in_list(d)
        hub = len(inn) >= self.max_in if "ge_max_in" in self.mut else len(inn) > self.max_in
        return (hub_scan if hub else wave_scan)(member(inn, front), self.mut)

    def probe2(self, d, front):
        inn = self.b.in_list(d)
        walk = int(self.b.indeg[inn].sum())
        if walk >= self.cap if "ge_cap" in self.mut else walk > self.cap:
            return False
        for wave in range(16):
            for k in range(wave, len(inn), 16):
                if "drop17" in self.mut and k == 16:
                    continue
                if wave_scan(member(self.b.in_list(inn[k]), front), self.mut):
                    return True
        return False

    def row(self, s, d):
        if s == d:
            return 0, 0
        if self.b.indeg[d] == 0:
            return -1, 0
        fronts = self.fronts(s)
        for t in range(1, len(fronts) + 1):
            if self.probe(d, fronts[t - 1]):
                return t, t - 1
            if self.with_probe2 and self.probe2(d, fronts[t - 1]):
                return t + 1, t - 1
        return -1, len(fronts)

    def rows(self, g):
        return [self.row(int(s), int(d)) for s, d in zip(g.rs, g.rd)]


@pytest.fixture(scope="module")
def plain(built):
    return {(m, p2): Model(built, m, PROBE2_CAP, probe2=p2).rows(built.g) for m, p2 in ((4096, False), (64, False), (4096, True))}


def test_the_model_is_the_oracle(built, plain):
    g = built.g
    for key, got in plain.items():
        bad = [i for i, (v, _) in enumerate(got) if v != g.dist[i]]
        assert not bad, (key, g.tag[bad[0]], got[bad[0]], int(g.dist[bad[0]]))
    # the expansions before the answer: k_probe2 answers a row within the cap one level early, one over it is k_probe's
    for x in g.gadgets:
        assert plain[4096, False][x["row"]][1] == plain[64, False][x["row"]][1] == x["k"] - 1, x["tag"]
        early = x["k"] >= 2 and (x["kind"] == "one" or x["walk"] <= PROBE2_CAP)
        assert plain[4096, True][x["row"]][1] == x["k"] - 1 - early, x["tag"]


MUTANTS = [
    # (name, probe_max_in, what the rows it must change look like)
    ("lane63", 4096, lambda x: x["kind"] == "one" and x["p"] % 64 == 63 and x["b"] <= 4096),
    ("trip2_first", 4096, lambda x: x["kind"] == "one" and x["p"] == 64 and x["b"] <= 4096),
    ("entry1023", 64, lambda x: x["kind"] == "one" and x["p"] == 1023),
    ("entry1024", 64, lambda x: x["kind"] == "one" and x["p"] == 1024),
    ("last_partial", 64, lambda x: x["kind"] == "one" and x["b"] > 64 and x["p"] >= x["b"] // 4096 * 4096),
    ("drop17", 4096, lambda x: x["kind"] == "two" and x["p"] == 16 and x["walk"] <= PROBE2_CAP),
    ("ge_cap", 4096, lambda x: x["kind"] == "two" and x["walk"] == PROBE2_CAP),
]


@pytest.mark.parametrize("name,max_in,expected", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_mutant_is_caught(built, plain, name, max_in, expected):
    g = built.g
    key = (max_in, name in ("drop17", "ge_cap"))
    got = Model(built, max_in, PROBE2_CAP, [name], probe2=key[1]).rows(g)
    changed = {i for i in range(len(got)) if got[i] != plain[key][i]}
    assert changed, "no gadget row sees mutant " + name
    want = set(g.rows_where(expected).tolist())
    assert changed == want, (sorted(g.tag[list(changed ^ want)])[:5])
    if key[1]:  # the hop count survives (the next level's k_probe finds the row): the levels run tell
        assert all(got[i][0] == plain[key][i][0] and got[i][1] == plain[key][i][1] + 1 for i in changed)
    else:
        assert all(got[i][0] != g.dist[i] for i in changed)
    print("%s: %d rows change, e.g. %s" % (name, len(changed), g.tag[min(changed)]))


@pytest.mark.parametrize("max_in", [4096, 64])
def test_the_hub_test_is_greater_than(built, max_in):
    # `>=` alone moves a row between two scans that agree; with a hub scan that finds nothing, the rows it moved show
    g = built.g
    gt = Model(built, max_in, PROBE2_CAP, ["hub_blind"], probe2=False).rows(g)
    ge = Model(built, max_in, PROBE2_CAP, ["hub_blind", "ge_max_in"], probe2=False).rows(g)
    changed = {i for i in range(len(gt)) if gt[i] != ge[i]}
    assert changed and changed == set(g.rows_where(lambda x: x["kind"] == "one" and x["b"] == max_in).tolist())
    assert all(gt[i][0] == g.dist[i] and ge[i][0] != g.dist[i] for i in changed)
