#!/usr/bin/env python3
"""tools/bench_within_paths.py — what the upper bound saves shortestpath: pgq_shortestpath_bulk_device (unchanged code: what a
caller had before the bounded call existed) against pgq_shortestpath_within_bulk_device at max_hops = 3, same process, same
handle, same rows, on the SF100-shaped knows graph of bench.py.

    python tools/bench_within_paths.py --out profiles/r10/within_paths.json

The generated knows graph is one component, so 16 more vertices in a ring of their own (friendships both ways, like every
other edge) are appended to it.  Two row sets: `cross`, a 2048 x 128 cross product (rows grouped by source) whose destination
pool holds 112 random vertices and those 16, so that unreachable rows exist; `random`, 4096 random pairs, where little is
expected.  Per row
set: --rounds rounds, each --warmup + --steps unbounded calls and then as many bounded ones (the two alternate, so that a drift of
the machine shows in both), every call bracketed by a device synchronisation; the medians over all timed calls and per round;
one more call of each with the statistics reset in front (levels, batches, launches per kernel class); how many rows lie beyond
the bound; and a check that the bounded call's lengths are the unbounded ones clamped at the bound and that its child_used is
the sum of 2 h + 1 over the rows within it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUND = 3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="JSON file for the results (default: stdout alone)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import duckpgq_extension_amd as pgq

    assert torch.cuda.is_available(), "needs the GPU: a time taken elsewhere says nothing"
    argv, sys.argv = sys.argv, ["bench.py", "--workload", "snb_sf100"]
    try:
        ba = bench.parse()
    finally:
        sys.argv = argv
    name, V0, off, adj, eid, _, _ = bench.build_graph(ba)
    ring = 16  # a second component: vertex V0 + i knows V0 + (i - 1) % ring and V0 + (i + 1) % ring
    V, E0 = V0 + ring, len(adj)
    nb = np.sort(np.stack([(np.arange(ring) - 1) % ring, (np.arange(ring) + 1) % ring], axis=1), axis=1) + V0
    off = np.concatenate([off, E0 + 2 * np.arange(1, ring + 1)]).astype(np.int64)
    adj = np.concatenate([adj, nb.ravel()]).astype(adj.dtype)
    eid = np.concatenate([eid, E0 + np.arange(2 * ring)]).astype(eid.dtype)
    name += " + a ring of %d" % ring
    dev = pgq.DeviceCSR(V, off, adj, eid)
    rng = np.random.default_rng(41)

    def dists(ps, pd):
        t_s, t_d = torch.from_numpy(ps).cuda(), torch.from_numpy(pd).cuda()
        t_o = torch.empty(len(ps), dtype=torch.int64, device="cuda")
        dev.iterativelength_bulk_ptr(len(ps), t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr())
        return t_o.cpu().numpy()

    sources = np.sort(rng.choice(V0, 2048, replace=False)).astype(np.int64)
    pool = np.concatenate([rng.choice(V0, 112, replace=False), V0 + np.arange(ring)]).astype(np.int64)
    row_sets = {
        "cross": (np.repeat(sources, len(pool)), np.tile(pool, len(sources))),
        "random": (rng.integers(0, V, 4096).astype(np.int64), rng.integers(0, V, 4096).astype(np.int64)),
    }
    out = {"graph": name, "V": int(V), "E": int(len(adj)), "max_hops": BOUND, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "version": pgq.load_hip().pgq_version().decode()}
    for label, (ps, pd) in row_sets.items():
        n = len(ps)
        dist = dists(ps, pd)
        within = (dist >= 0) & (dist <= BOUND)
        cap = int((2 * dist[dist >= 0] + 1).sum()) + 64
        t_s, t_d = torch.from_numpy(np.ascontiguousarray(ps)).cuda(), torch.from_numpy(np.ascontiguousarray(pd)).cuda()
        t_len = torch.empty(n, dtype=torch.int64, device="cuda")
        t_off = torch.zeros(n, dtype=torch.int64, device="cuda")
        t_child = torch.empty(cap, dtype=torch.int64, device="cuda")
        ptrs = (t_len.data_ptr(), t_off.data_ptr(), t_child.data_ptr(), cap)

        def unbounded():
            return dev.shortestpath_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), *ptrs)

        def bounded():
            return dev.shortestpath_within_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), BOUND, *ptrs)

        def timed(call):
            ms = []
            for k in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc, _ = call()
                torch.cuda.synchronize()
                assert rc == 0, rc
                if k >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            return ms

        def observed(call):
            pgq.reset_stats()
            rc, used = call()
            torch.cuda.synchronize()
            st = pgq.get_stats()
            assert rc == 0, rc
            return used, {"levels": st["levels"], "batches": st["batches"], "meet_pairs": st["meet_pairs"],
                          "launches": {k: v for k, v in st["launches"].items() if v}}

        ms = {"unbounded": [], "within": []}
        rounds = []
        for _ in range(a.rounds):
            u, w = timed(unbounded), timed(bounded)
            ms["unbounded"] += u
            ms["within"] += w
            rounds.append({"unbounded_median_ms": statistics.median(u), "within_median_ms": statistics.median(w)})
        used_u, stats_u = observed(unbounded)
        assert (t_len.cpu().numpy() == dist).all() and used_u == cap - 64
        used_w, stats_w = observed(bounded)
        assert (t_len.cpu().numpy() == np.where(within, dist, -1)).all(), "bounded lengths != the unbounded ones clamped"
        assert used_w == int((2 * dist[within] + 1).sum()), (used_w, int((2 * dist[within] + 1).sum()))
        out[label] = {
            "rows": n, "rows_within": int(within.sum()), "rows_beyond": int((~within).sum()), "rows_unreachable": int((dist < 0).sum()),
            "rows_by_distance": {str(int(k)): int(v) for k, v in zip(*np.unique(dist, return_counts=True))},
            "unbounded": {"median_ms": statistics.median(ms["unbounded"]), "min_ms": min(ms["unbounded"]), "max_ms": max(ms["unbounded"]),
                          "child_used": int(used_u), "stats": stats_u},
            "within": {"median_ms": statistics.median(ms["within"]), "min_ms": min(ms["within"]), "max_ms": max(ms["within"]),
                       "child_used": int(used_w), "stats": stats_w},
            "rounds": rounds,
        }
        print(json.dumps({label: out[label]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
