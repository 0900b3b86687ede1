"""tests/analytics_model.py is what test_analytics_gpu.py holds csrc/pgq_analytics.hip against; here the model itself is held
against the oracle, the reference's goldens, a run in extended precision and scipy, and its fixtures are shown to be sharp:
every way of getting PageRank subtly wrong that the model can switch on changes a bit on one of them.  CPU only."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import analytics_model as am
from helpers import directed_rows, load_golden
from oracle.pgq_oracle import OracleCSR

PR_NAMES = [f[0] for f in am.pagerank_fixtures()]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def oracle_csr(V, off, adj):
    return OracleCSR.adopt(V, off, adj if len(adj) else np.zeros(1, dtype=np.int64))


def fixture(name):
    return next(f for f in am.pagerank_fixtures() if f[0] == name)[1:]


def test_fixtures_are_what_the_gpu_test_needs():
    sizes = {V for _, V, _, _ in am.pagerank_fixtures()}
    assert sizes == set(am.PR_SIZES) and {V + 2 for V in sizes} >= {3, 64, 65, 1024, 1025, 2048, 2049}
    for name, V, off, adj in am.pagerank_fixtures():
        deg, vs = np.diff(off), V + 2
        per = (vs + 1023) // 1024
        if name.startswith("empty"):
            assert off[V] == 0
        else:  # multigraphs: parallel edges and self loops
            src = np.repeat(np.arange(V), deg)
            assert (src == adj).any(), name
            assert len(np.unique(src * V + adj)) < len(adj), name
        if name.startswith("cycle"):
            assert (deg > 0).all(), name  # only the two trailing entries dangle
        if name.startswith("edges"):
            n = (vs + per - 1) // per
            want = {i for k in (0, n // 2, n - 1) for i in (k * per - 1, k * per) if 0 <= i < V} | {V - 1}
            assert want <= set(np.flatnonzero(deg == 0).tolist()), name
            assert len(want) >= 4 and (deg > 0).sum() > V - 12, name
        if name.startswith("skew"):
            indeg = np.bincount(adj, minlength=V)
            hub = int(indeg.argmax())
            feeders = np.unique(src[adj == hub])
            assert indeg[hub] >= 1000 and deg[feeders].min() == 1 and deg[feeders].max() == 500, name


@pytest.mark.parametrize("name", PR_NAMES)
def test_pagerank_model_is_the_oracle_bit_for_bit(name):
    V, off, adj = fixture(name)
    rank, it, deltas = am.pagerank_of(name, "reference")
    want, wit = oracle_csr(V, off, adj).pagerank()
    assert it == wit and (bits(rank) == bits(want)).all()
    if name.startswith("empty"):
        assert it == 1
        if (V + 2) & (V + 1) == 0:  # vs a power of two: the chain of equal addends is exact
            assert deltas == [0.0]


def test_pagerank_model_reproduces_the_goldens_exactly():
    pr = load_golden("pagerank.json")
    rows = 0
    for key in ("g1", "g2"):
        g = pr[key]
        s, d, _ = directed_rows(g["edges"])
        off, adj = am.csr(g["V"], s, d)
        for mode in ("reference", "device"):
            rank, _ = am.pagerank(g["V"], off, adj, mode)
            for vid, txt in g["rows"]:
                assert float(txt) == rank[vid], (key, mode, vid, rank[vid], txt)
                rows += mode == "reference"
        unfused, _ = am.pagerank(g["V"], off, adj, mutant="unfused")
        assert any(float(txt) != unfused[vid] for vid, txt in g["rows"]), "the goldens pin the fused update"
    assert rows == 10


@pytest.mark.parametrize("mutant", am.PR_MUTANTS)
def test_every_mutant_changes_a_bit_on_a_gpu_fixture(mutant):
    """Killed by (first fixture in the list is the smallest): unfused, reverse_in_list: cycle_V62 and every larger graph with
    slots; no_trailing, drop_last_slice: every fixture, empty_V0 first; per_floor: every fixture but those with vs = 1024 and
    vs = 2048, where floor and ceiling agree."""
    killed = []
    for name, V, off, adj in am.pagerank_fixtures():
        want, wit, _ = am.pagerank_of(name, "device")
        got, it = am.pagerank(V, off, adj, "device", mutant=mutant)
        if it != wit or (bits(got) != bits(want)).any():
            killed.append(name)
            if len(killed) == 3:
                break
    print(mutant, "killed by", killed)
    assert killed, mutant


def test_the_two_switches_that_cannot_show():
    """dangling_contrib and stop_le change nothing at the sizes of these fixtures, for reasons checked here on every one of
    them: no in-list names a vertex without slots; every iteration's max delta is a multiple of 2^-66 (no rank is below
    2^-14), and the double 1e-6 is not."""
    assert am.EPS * 2.0 ** 66 != int(am.EPS * 2.0 ** 66) and am.EPS * 2.0 ** 72 == int(am.EPS * 2.0 ** 72)
    for name, V, off, adj in am.pagerank_fixtures():
        rank, it, deltas = am.pagerank_of(name, "device")
        deg = np.diff(off)
        _, psrc = am.in_lists(V, off, adj)
        assert (deg[psrc] > 0).all(), name
        assert V + 2 <= 2049 and rank.min() > 2.0 ** -14, name
        assert all(d * 2.0 ** 66 == int(d * 2.0 ** 66) for d in deltas), name
        if off[V] < 10000:
            for mutant in am.PR_EQUIVALENT:
                got, git = am.pagerank(V, off, adj, "device", mutant=mutant)
                assert git == it and (bits(got) == bits(rank)).all(), (name, mutant)


def test_device_mode_is_reference_mode_up_to_1024_entries():
    """One entry per slice: the slices' ordered sum is the reference's chain with +0.0 between its terms.  Above: largest
    difference 435 ulp = 4.83e-14 relative on empty_V2047 (2049 equal addends: the chain rounds, three per slice do not);
    8 ulp on skew_V2047, 1 ulp on edges_V1023."""
    differ = []
    for name, V, off, adj in am.pagerank_fixtures():
        ref, rit, _ = am.pagerank_of(name, "reference")
        dev, dit, _ = am.pagerank_of(name, "device")
        assert rit == dit, name
        if V + 2 <= 1024:
            assert (bits(ref) == bits(dev)).all(), name
        elif (bits(ref) != bits(dev)).any():
            differ.append(name)
            assert np.max(np.abs(ref - dev) / ref) <= 1e-12, name  # the bound the 20,000-vertex random check keeps
    assert differ, "no fixture above 1024 entries tells the two modes apart"


def test_pagerank_model_against_extended_precision():
    """The same recurrence, same order, same iteration count, in numpy.longdouble (64-bit significand).  The largest relative
    deviation over the fixtures was measured at 3.6201e-14 (empty_V2047: the ordered chain of 2049 equal addends; the largest
    on a graph with slots is 8.7e-15, skew_V1022).  The bound is 4 x the measured value: it depends on the graphs and the
    iteration counts, not on a format alone."""
    assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is no wider than double here"
    measured = 3.6201e-14
    worst = 0.0
    for name, V, off, adj in am.pagerank_fixtures():
        rank, it, _ = am.pagerank_of(name, "reference")
        wide = am.pagerank_extended(V, off, adj, it)
        worst = max(worst, float(np.max(np.abs(rank.astype(np.longdouble) - wide) / wide)))
    print("largest relative deviation from the extended-precision run: %.4e" % worst)
    assert worst <= 4 * measured


# ---- weakly connected components -------------------------------------------------------------------------------------------
def test_boruvka_model_certifies_the_wcc_fixtures():
    seen = {}
    for name, V, s, d in am.wcc_fixtures():
        off, adj = am.csr(V, s, d)
        rounds, chain, chosen = am.boruvka(V, off, adj)
        ncomp = connected_components(coo_matrix((np.ones(len(s)), (s, d)), shape=(V, V)), directed=False)[0]
        assert chosen == V - ncomp, name
        seen[name] = (rounds, chain)
        if name.startswith("loops_"):  # the leaving slot is the last of a list of 63, 64, 65, 129
            n = int(name.split("_")[1])
            assert off[2] - off[1] == n + 1 and adj[off[2] - 1] == 3 and (adj[off[1]:off[2] - 1] == 1).all()
    assert seen["shuffled_path"][0] >= 6 and seen["shuffled_path"][1] >= 4
    assert seen["chain"] == (1, am.WCC_CHAIN_V - 1)
    assert seen["self_loops_only"] == (0, 0) and seen["empty_V256"] == (0, 0)  # the first round hooks nothing
    assert seen["star_centre_lowest"][0] == 1 and seen["star_centre_highest"][0] == 1


# ---- local clustering coefficient ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(am.LCC_GADGETS))
def test_lcc_gadget_rounds_its_count(kernel):
    p, q = am.LCC_GADGETS[kernel]
    V, off, adj = am.lcc_gadget(p, q)
    deg = int(off[1] - off[0])
    assert deg == p + 1 and (deg == 512 if kernel == "k_lcc" else deg >= 513)
    count = am.lcc_count(V, off, adj, 0)
    assert count == 1 + p + p * q and count > 1 << 24 and count % 2 == 1  # no float32 holds it
    rounded, chopped = am.lcc_value(count, deg), am.lcc_value(count, deg, truncate=True)
    assert rounded.dtype == np.float32 and rounded.view(np.uint32) != chopped.view(np.uint32)
    assert am.lcc_value(1 + 4096 + 4096 * 4096, 4097).view(np.uint32) == am.lcc_value(1 + 4096 + 4096 * 4096, 4097, True).view(np.uint32), \
        "p = q = 4096 would not tell: the parameters need this check"
    got = am.lcc(V, off, adj, am.LCC_ROWS)
    want = OracleCSR.adopt(V, off, adj).local_clustering_coefficient(am.LCC_ROWS[:-1])
    assert (got[:-1].view(np.uint32) == want.view(np.uint32)).all() and got[-1] == 0
    assert off[3] - off[2] == 2 and got[0] > 1 and got[2] > 1 and got[3] == 0 and got[4] == 0
