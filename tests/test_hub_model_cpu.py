"""The numpy model of the hub tables (tests/hub_model.py) against brute force on random directed graphs: a proof read from
the tables is never wrong (P3: a 3-edge walk exists, so the distance is at most 3; P4: a 4-edge walk, at most 4), the proofs
follow the edges' direction, and the hub selection does what the upload documents at its edges (ties at rank H, fewer hubs
than H, one hub, none)."""
import numpy as np
import pytest

import hub_model

V = 300


def random_graph(seed):
    """About 300 vertices, asymmetric edges, a few heavy vertices in each direction, the last 20 ids isolated."""
    rng = np.random.default_rng(seed)
    live = V - 20
    s, d = rng.integers(0, live, 500), rng.integers(0, live, 500)
    heavy = rng.choice(live, 6, replace=False)
    for k, h in enumerate(heavy):  # half of them collect in-edges, half send out-edges
        other = rng.integers(0, live, 25)
        s = np.concatenate([s, other if k % 2 else np.full(25, h)])
        d = np.concatenate([d, np.full(25, h) if k % 2 else other])
    return s.astype(np.int64), d.astype(np.int64)


def walks(s, d):
    """A[k][u, v]: a walk of exactly k edges u -> v exists (k = 1 .. 4), and the BFS distance matrix (-1: unreachable)."""
    A1 = np.zeros((V, V), dtype=bool)
    A1[s, d] = True
    A = {1: A1}
    for k in (2, 3, 4):
        A[k] = (A[k - 1].astype(np.int32) @ A1.astype(np.int32)) > 0
    dist = np.full((V, V), -1, dtype=np.int64)
    reach = np.eye(V, dtype=bool)
    dist[reach] = 0
    frontier = reach
    for k in range(1, V):
        nxt = ((frontier.astype(np.int32) @ A1.astype(np.int32)) > 0) & ~reach
        if not nxt.any():
            break
        dist[nxt] = k
        reach |= nxt
        frontier = nxt
    return A, dist


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("hubs", [4, 64, 256])
def test_a_proof_is_never_wrong(seed, hubs):
    s, d = random_graph(seed)
    ids = hub_model.select_hubs(V, s, d, 256, min_degree=1, min_count=1)
    ids[hubs:] = -1  # the first `hubs` of the ranking
    t = hub_model.build_tables(V, s, d, ids)
    A, dist = walks(s, d)
    a, b = (x.ravel() for x in np.meshgrid(np.arange(V), np.arange(V), indexing="ij"))
    p3, p4 = hub_model.proofs(t, a, b)
    p3, p4 = p3.reshape(V, V), p4.reshape(V, V)
    assert p3.any() and p4.any() and not p3.all()
    assert (A[3] | ~p3).all(), "P3 without a 3-edge walk"
    assert (A[4] | ~p4).all(), "P4 without a 4-edge walk"
    assert ((dist[p3] >= 0) & (dist[p3] <= 3)).all()
    assert ((dist[p4] >= 0) & (dist[p4] <= 4)).all()
    # and the tables say what they are documented to say, bit by bit
    used = np.flatnonzero(ids >= 0)
    bit = lambda tab, h: (tab[:, h >> 6] >> np.uint64(h & 63)) & np.uint64(1)
    for h in used[:: max(1, len(used) // 8)]:
        assert (bit(t["hub1_out"], h) == A[1][:, ids[h]]).all()
        assert (bit(t["hub1_in"], h) == A[1][ids[h], :]).all()
        assert (bit(t["hub2_out"], h) == A[2][:, ids[h]]).all()
        assert (bit(t["hub2_in"], h) == A[2][ids[h], :]).all()
    for tab in t.values():  # bits of unused slots are zero
        for h in range(hubs, 256):
            assert not bit(tab, h).any()


def test_proofs_follow_the_direction():
    """s -> a -> h -> d and s2 -> a2 -> h -> c -> d2 are the only edges: the rows have their proofs, the reversed rows none."""
    s, a, h, d, s2, a2, c, d2 = range(8)
    src = np.array([s, a, h, s2, a2, h, c])
    dst = np.array([a, h, d, a2, h, c, d2])
    ids = hub_model.select_hubs(V, src, dst, 256, min_degree=4, min_count=1)  # h alone has four edges
    assert ids[0] == h and (ids[1:] == -1).all()
    t = hub_model.build_tables(V, src, dst, ids)
    p3, p4 = hub_model.proofs(t, [s, d, s2, d2, s, s2], [d, s, d2, s2, d2, d])
    assert list(p3) == [True, False, False, False, False, True]
    assert list(p4) == [False, False, True, False, True, False]


def star(center, leaves):
    return np.full(len(leaves), center), np.asarray(leaves)


def test_selection():
    # degrees: vertex 10 has 12 edges, 20 and 5 have 9 each (a tie), 7 has 9 too, the leaves 1 or 2
    parts = [star(10, range(100, 112)), star(20, range(120, 129)), star(5, range(130, 139)), star(7, range(140, 149))]
    src = np.concatenate([p[0] for p in parts])
    dst = np.concatenate([p[1] for p in parts])
    ids = hub_model.select_hubs(V, src, dst, 256, min_degree=9, min_count=1)
    assert list(ids[:5]) == [10, 5, 7, 20, -1] and (ids[4:] == -1).all()  # fewer hubs than H; a tie goes to the smaller id
    # ties at rank H: H slots, more vertices with the deciding degree than are left
    ids = hub_model.select_hubs(V, src, dst, 2, min_degree=1, min_count=1)
    assert list(ids) == [10, 5]
    ids = hub_model.select_hubs(V, src, dst, 3, min_degree=1, min_count=1)
    assert list(ids) == [10, 5, 7]
    # exactly one hub
    ids = hub_model.select_hubs(V, src, dst, 256, min_degree=10, min_count=1)
    assert ids[0] == 10 and (ids[1:] == -1).all()
    # in-degree counts like out-degree: the edges turned round select the same hubs
    assert (hub_model.select_hubs(V, dst, src, 256, min_degree=9, min_count=1) ==
            hub_model.select_hubs(V, src, dst, 256, min_degree=9, min_count=1)).all()
    # no qualifying vertex, or fewer than min_count: no tables
    assert hub_model.select_hubs(V, src, dst, 256, min_degree=13, min_count=1) is None
    assert hub_model.select_hubs(V, src, dst, 256, min_degree=9, min_count=5) is None
    assert hub_model.select_hubs(V, src, dst, 256, min_degree=9, min_count=4) is not None


def test_table_budget():
    assert hub_model.fit_hubs(448_626, 1024, 512) == 1024  # 219 MB
    assert hub_model.fit_hubs(1 << 22, 1024, 512) == 0  # R-MAT-22: 2 GB, 1 GB, then 512 MB of tables and 1 KB of ids
    assert hub_model.fit_hubs((1 << 22) - 8, 1024, 512) == 256
    assert hub_model.fit_hubs(5000, 1024, 2) == 512 and hub_model.fit_hubs(5000, 1024, 0) == 0
    assert hub_model.fit_hubs(5000, 0, 512) == 0 and hub_model.fit_hubs(5000, 300, 512) == 256
