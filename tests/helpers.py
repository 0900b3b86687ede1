"""Shared helpers for the parity tests (graph feeds shaped like the reference's SQL)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def directed_rows(edges):
    """Row feed of CreateDirectedCSRCTE (compressed_sparse_row.cpp:234-251): one row per edge-table row, in table
    order, edge id = edge rowid."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return e[:, 0].copy(), e[:, 1].copy(), np.arange(len(e), dtype=np.int64)


def undirected_rows(edges):
    """Row feed of CreateUndirectedCSRCTE (compressed_sparse_row.cpp:208-223): one row per distinct ordered pair in
    forward U reverse (GROUP BY src,dst), edge id = any_value -> we take the smallest contributing edge rowid, and
    emit rows sorted by (src,dst) (the reference's order is hash-aggregate order, i.e. unspecified)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    best = {}
    for rid, (s, d) in enumerate(e.tolist()):
        for a, b in ((s, d), (d, s)):
            if (a, b) not in best:
                best[(a, b)] = rid
    keys = sorted(best)
    src = np.array([k[0] for k in keys], dtype=np.int64)
    dst = np.array([k[1] for k in keys], dtype=np.int64)
    eid = np.array([best[k] for k in keys], dtype=np.int64)
    return src, dst, eid


def all_pairs(V):
    s, d = np.meshgrid(np.arange(V, dtype=np.int64), np.arange(V, dtype=np.int64), indexing="ij")
    return s.ravel().copy(), d.ravel().copy()


def csr_arrays_from_rows(V, src, dst):
    """offsets[V+1], adj[E], slot permutation (stable counting sort on src == reference single-thread slot order)."""
    order = np.argsort(src, kind="stable")
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=V), out=off[1:])
    return off, dst[order].astype(np.int64), order


def sparse_ids_graph(rng, V, n_active, E, hubs=4, chains=0, chain_len=10):
    """A graph on about n_active vertices spread over [0, V), for kernels whose per-vertex bit maps are sized by V.  Among
    the active ids: 0, V // 2, V - 2, V - 1, and ids of the last 32-vertex word and of the last 128-vertex block of such a
    map.  Random edges between them, a few hubs whose out- and in-lists span a good part of the active set, and 50
    duplicated edges.  `chains` directed paths of `chain_len` edges over ids of their own, which no other edge touches:
    pairs along a chain are at distances 1 .. chain_len, pairs against its direction are unreachable.
    Returns (active ids, src, dst, hub ids, chains as a list of id arrays)."""
    top = V - 1
    tail = [0, V - 1, V - 2, V // 2, top // 32 * 32, top // 128 * 128]
    tail += list(rng.integers(top // 32 * 32, V, 3)) + list(rng.integers(top // 128 * 128, V, 3))
    act = np.unique(np.concatenate([rng.integers(0, V, n_active), tail]))
    act = act[(act >= 0) & (act < V)]
    n = len(act)
    s = rng.integers(0, n, E)
    d = rng.integers(0, n, E)
    hub = rng.choice(n, hubs, replace=False)
    hs = np.repeat(hub, n // 3)
    hd = rng.integers(0, n, len(hs))
    s = np.concatenate([s, hs, hd, s[:50]])  # hub out- and in-lists, 50 duplicated edges
    d = np.concatenate([d, hd, hs, d[:50]])
    s, d = act[s].astype(np.int64), act[d].astype(np.int64)
    paths = []
    if chains:
        free = np.setdiff1d(np.unique(rng.integers(0, V, 4 * chains * (chain_len + 1))), act)
        rng.shuffle(free)
        assert len(free) >= chains * (chain_len + 1), "V too small for the chains"
        for k in range(chains):
            c = free[k * (chain_len + 1):(k + 1) * (chain_len + 1)].astype(np.int64)
            paths.append(c)
            s, d = np.concatenate([s, c[:-1]]), np.concatenate([d, c[1:]])
    return act, s, d, act[hub], paths


# The largest V at which each bit-map kernel keeps its map in LDS (or, for k_src_ball, runs two workgroups per CU).  One vertex
# more and the host picks the global-memory variant (or one workgroup per CU).  test_lds_limits_gpu.py runs both sides of
# every entry; test_lds_budget_cpu.py recomputes every entry from the host rules and the static LDS of the built kernels.
LDS_LIMITS = {
    "ball_2_per_cu": 466_944,    # k_src_ball, two workgroups per CU (above: one, its map still in LDS)
    "ball_1_per_cu": 1_122_304,  # k_src_ball, one workgroup per CU with 137 KB of dynamic LDS (above: global maps)
    "meet4": 1_212_416,          # k_meet4d, k_meet4<paths>
    "bibfs": 606_080,            # k_bibfs, both visited maps
    # k_pull_lanes<WD, *, true> (lanes = 1) and k_pull_sparse<WD, *, 16, *> (lanes = 0), by lane words WD
    "pull_lanes": {1: 974_272, 2: 961_792, 4: 836_992, 8: 787_008, 16: 687_168, 32: 487_424},
    "pull_sparse": {1: 803_392, 2: 792_448, 4: 770_624, 8: 726_912, 16: 639_552, 32: 464_768},
}
