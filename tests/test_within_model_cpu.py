"""Host models of the hop-bounded search (iterativelength_within), checked against the CPU oracle.

within(src, dst, U) is iterativelength(src, dst) where that is at most U, else NULL.  Two rules carry it on the device:

  - k_bibfs<*, true>: one bidirectional search per row, the cheaper side expanded level by level; BEFORE a side is chosen,
    a + b >= U ends the row with NULL (a, b: levels expanded from src and from dst).  Before an expansion the two visited sets
    are disjoint, so the distance exceeds a + b; a meeting reports a + b + 1.
  - the pre-pass stages: a test that ran to its END excludes its distance (k_meet3's two-hop walk: "Known4", distance >= 4, NULL
    under U = 3); a walk CUT at the stage's cap excludes nothing beyond what the tests before it did, so the row stays open for
    the next stage whatever the bound.

Each model is restated here in plain Python and run for U = 0 .. 6; a deliberately wrong variant of each (stopping one level
early; closing cut rows) must disagree with the oracle on the same rows, which shows the rows can tell the difference."""
import numpy as np
import pytest

from helpers import sparse_ids_graph
from oracle.pgq_oracle import OracleCSR

BOUNDS = range(0, 7)


class Graph:
    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.V = V = 3000
        act, s, d, hubs, chains = sparse_ids_graph(rng, V, 400, 900, hubs=1, chains=4, chain_len=8)
        self.out = [[] for _ in range(V)]
        self.inn = [[] for _ in range(V)]
        for a, b in zip(s.tolist(), d.tolist()):
            self.out[a].append(b)
            self.inn[b].append(a)
        ps = [act[rng.integers(0, len(act), 250)], np.repeat(hubs, 20), act[rng.integers(0, len(act), 20)]]
        pd = [act[rng.integers(0, len(act), 250)], act[rng.integers(0, len(act), 20)], np.repeat(hubs, 20)]
        for c in chains:
            i, j = np.triu_indices(len(c), 1)
            ps += [c[i], c[j]]
            pd += [c[j], c[i]]
        self.ps, self.pd = np.concatenate(ps).astype(np.int64), np.concatenate(pd).astype(np.int64)
        self.pd[::53] = self.ps[::53]  # src == dst rows
        oln, ook = OracleCSR.from_edges(V, s, d).lean_iterativelength(V, self.ps, self.pd, nthreads=4)
        self.dist = np.where(ook, oln, -1)
        for U in BOUNDS:  # the rows can tell every bound from its neighbours
            assert (self.dist == U).any() and (self.dist == U + 1).any(), U
        assert (self.dist < 0).any()

    def want(self, U):
        return [int(x) if 0 <= x <= U else None for x in self.dist]


@pytest.fixture(scope="module", params=[11, 12])
def graph(request):
    return Graph(request.param)


def bounded_bibfs(g, s, d, U, slack=0):
    """k_bibfs's loop with the bound in front of the side choice.  slack = 1 is the wrong rule (a + b + 1 >= U)."""
    if s == d:
        return 0
    seen = [{s}, {d}]
    front = [[s], [d]]
    lvl = [0, 0]
    adj = [g.out, g.inn]
    while True:
        if lvl[0] + lvl[1] + slack >= U:
            return None
        work = [sum(len(adj[k][v]) for v in front[k]) for k in (0, 1)]
        side = 0 if work[0] <= work[1] else 1
        nxt = []
        for v in front[side]:
            for x in adj[side][v]:
                if x in seen[side ^ 1]:
                    return lvl[0] + lvl[1] + 1
                if x not in seen[side]:
                    seen[side].add(x)
                    nxt.append(x)
        if not nxt:
            return None  # this side's closure is complete
        front[side] = nxt
        lvl[side] += 1


def test_bounded_bidirectional_rule(graph):
    g = graph
    for U in BOUNDS:
        got = [bounded_bibfs(g, int(s), int(d), U) for s, d in zip(g.ps, g.pd)]
        assert got == g.want(U), U


def test_stopping_one_level_early_is_caught(graph):
    g = graph
    for U in range(1, 7):
        got = [bounded_bibfs(g, int(s), int(d), U, slack=1) for s, d in zip(g.ps, g.pd)]
        want = g.want(U)
        assert got != want, U
        # it only ever loses rows at exactly U hops
        assert all(a == b or (a is None and b == U) for a, b in zip(got, want)), U


OPEN = "open"


def meet3_stage(g, s, d, U, cap, close_cut=False):
    """What k_meet3<..., BND> concludes for one row: a hop count, None (NULL) or OPEN.  `cap` bounds the entries of the two-hop
    walk; close_cut = True is the wrong rule that treats a cut walk like one that ran to its end."""
    if s == d:
        return 0
    if not g.out[s] or not g.inn[d]:
        return None
    target = set(g.inn[d])
    if s in target:
        return 1 if U >= 1 else None
    if U < 2:
        return None
    if any(v in target for v in g.out[s]):
        return 2
    if U < 3:
        return None  # the two-hop walk is not started
    walked = 0
    for v in g.out[s]:
        for x in g.out[v]:
            if walked >= cap:  # cut: distances 1 and 2 are excluded, nothing else
                return None if (close_cut and U == 3) else OPEN
            walked += 1
            if x in target:
                return 3
    return None if U == 3 else OPEN  # ran to its end: distance >= 4 ("Known4")


@pytest.mark.parametrize("cap", [1 << 30, 8])
def test_stage_conclusions_under_a_bound(graph, cap):
    g = graph
    n_open = n_cut_close = 0
    for U in BOUNDS:
        got = []
        for s, d in zip(g.ps.tolist(), g.pd.tolist()):
            r = meet3_stage(g, s, d, U, cap)
            if r is OPEN:
                n_open += 1
                r = bounded_bibfs(g, s, d, U)  # the next stage
            got.append(r)
        assert got == g.want(U), (U, cap)
        if U == 3 and cap == 1 << 30:  # without a cap nothing is open under a bound of 3: Known4 rows are NULL there
            assert all(meet3_stage(g, s, d, 3, cap) is not OPEN for s, d in zip(g.ps.tolist(), g.pd.tolist()))
        if U == 3 and cap == 8:
            n_cut_close = sum(meet3_stage(g, s, d, 3, cap) is OPEN and x == 3
                              for s, d, x in zip(g.ps.tolist(), g.pd.tolist(), g.dist.tolist()))
    assert n_open > 0
    if cap == 8:
        assert n_cut_close > 0, "no cut row at exactly 3 hops: the cap does not bite on this graph"


def test_closing_cut_rows_is_caught(graph):
    g = graph
    got = [meet3_stage(g, s, d, 3, 8, close_cut=True) for s, d in zip(g.ps.tolist(), g.pd.tolist())]
    assert OPEN not in got
    assert got != g.want(3)
