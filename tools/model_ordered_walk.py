#!/usr/bin/env python3
"""CPU model of the entries k_meet3's two-hop walk scans per row, for several orders of the packed lists and several ways of
walking them in parts (needs numpy only, no GPU).

    python tools/model_ordered_walk.py [--rows 2000] [--vertices V --friendships F]

The graph is bench.py's default (graphgen.snb_knows_like, seed 100), the rows are the first --rows of its pairs
(default_rng(4)).  A row is modelled as k_meet3 treats it: rows answered before the walk (src = dst, an empty list, distance 1
or 2) and rows it hands on unwalked (set list over 512 ids, expanded list over 4096) are left out; the walk runs from the
endpoint with the smaller sum of neighbour list lengths (the other one if that endpoint's own list is the only one that fits
the register set), over lists of K = 6 ids per group, 64 groups per request, the stop looked at every two requests, at most
--cap entries.  A part split walks part 0 of ALL the row's lists, then part 1, ...

Left out (the model reads ~10 % under the device's count): the rounds of 64 descriptors (a round's last request is partly
empty), the two requests already in flight when the walk stops, and the padding of a list's last group.

Printed per variant: entries scanned per walking row, its ratio to the id order, and the mean position of the first witness."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from duckpgq_extension_amd import graphgen  # noqa: E402

K = 6
PASS = 2 * 64  # groups between two looks at the stop
SET_MAX, EXP_MAX = 512, 4096


def bucket(x):
    return np.floor(np.log2(np.maximum(x, 1))).astype(np.int64)


# name -> (sort key of an entry from its degree (None: id order), cumulative part boundaries as functions of a list's groups)
def variants(median):
    quarter, half, eighth = (lambda g: (g + 3) >> 2), (lambda g: (g + 1) >> 1), (lambda g: (g + 7) >> 3)
    return [
        ("id order, one part", None, []),
        ("exact degree order, heads 1/4", lambda d: d, [quarter]),
        ("log2 buckets, heads 1/4", bucket, [quarter]),
        ("log2 buckets, one part", bucket, []),
        ("two classes at the median, heads 1/4", lambda d: (d > median).astype(np.int64), [quarter]),
        ("two classes at the median, heads 1/2", lambda d: (d > median).astype(np.int64), [half]),
        ("exact, three parts 1/8, 1/2, rest", lambda d: d, [eighth, half]),
    ]


def walk(off, adj, deg, exp, mark, key, bounds, cap):
    """Entries scanned and the first witness's position for one row; `mark`: membership in the set side."""
    lens = deg[exp]
    starts = np.concatenate([[0], np.cumsum(lens)])
    n = int(starts[-1])
    if n == 0:
        return 0, -1
    lid = np.repeat(np.arange(len(exp)), lens)
    pos = np.arange(n) - starts[lid]
    ent = adj[np.repeat(off[exp], lens) + pos]
    if key is not None:  # stable: equal keys keep the id order
        order = np.lexsort((pos, -key(deg[ent]), lid))
        ent = ent[order]
    g = pos // K  # (pos is the rank inside the list either way: lexsort keeps the lists together)
    ng = (lens + K - 1) // K
    b = [np.zeros(len(exp), dtype=np.int64)] + [f(ng) for f in bounds] + [ng]
    rank = np.zeros(n, dtype=np.int64)
    base = 0
    for i in range(len(b) - 1):
        cnt = b[i + 1] - b[i]
        before = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        here = (g >= b[i][lid]) & (g < b[i + 1][lid])
        rank[here] = base + before[lid[here]] + g[here] - b[i][lid[here]]
        base += int(cnt.sum())
    total = base
    hits = np.flatnonzero(mark[ent])
    cut = (cap // (PASS * K) + 1) * PASS  # groups requested when the cap ends the walk
    if len(hits):
        first = int(rank[hits].min())
        groups = min(total, (first // PASS + 1) * PASS)
        if groups <= cut:
            return groups * K, first * K
    return min(total, cut) * K, -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--vertices", type=int, default=448626)
    ap.add_argument("--friendships", type=int, default=19_940_000)
    ap.add_argument("--cap", type=int, default=16384)
    a = ap.parse_args()
    V, s, d = graphgen.snb_knows_like(a.vertices, a.friendships, seed=100)
    off, adj, _ = graphgen.csr_from_rows(V, s, d)  # symmetric: in-lists = out-lists
    deg = np.diff(off)
    work = np.add.reduceat(deg[adj], off[:-1]) * (deg > 0)  # entries of a vertex's two-hop walk
    pairs = np.random.default_rng(4).integers(0, V, size=(65536, 2))[:a.rows]
    vs = variants(float(np.median(deg[adj])))
    scanned = np.zeros(len(vs))
    first = [[] for _ in vs]
    mark = np.zeros(V, dtype=bool)
    walking = no_witness = early = handed_on = 0
    for src, dst in pairs.tolist():
        ns, nd = adj[off[src]:off[src + 1]], adj[off[dst]:off[dst + 1]]
        if src == dst or len(ns) == 0 or len(nd) == 0 or dst in ns or len(np.intersect1d(ns, nd)):
            early += 1
            continue
        fwd = work[src] <= work[dst]
        if len(nd if fwd else ns) > SET_MAX:
            fwd = not fwd
        exp, members = (ns, nd) if fwd else (nd, ns)
        if len(members) > SET_MAX or len(exp) > EXP_MAX:
            handed_on += 1
            continue
        walking += 1
        mark[members] = True
        for i, (_, key, bounds) in enumerate(vs):
            e, f = walk(off, adj, deg, exp, mark, key, bounds, a.cap)
            scanned[i] += e
            if f >= 0:
                first[i].append(f)
            elif i == 0:
                no_witness += 1
        mark[members] = False
    print("graph V=%d E=%d; %d rows: %d answered before the walk, %d handed on unwalked, %d walking (%.1f %% of them without a witness "
          "under the cap)" % (V, len(adj), len(pairs), early, handed_on, walking, 100.0 * no_witness / max(walking, 1)))
    print("%-42s %18s %8s %22s" % ("order of the lists, parts walked", "entries / row", "ratio", "first witness at entry"))
    for i, (name, _, _) in enumerate(vs):
        print("%-42s %18.0f %8.2f %22.0f" % (name, scanned[i] / max(walking, 1), scanned[i] / max(scanned[0], 1),
                                           np.mean(first[i]) if first[i] else -1))


if __name__ == "__main__":
    main()
