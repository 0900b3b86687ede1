#!/usr/bin/env python3
"""tools/bench_k_walks.py — what the walks of a bounded quantifier cost next to the shortest paths: pgq_walk_count_bulk_device and
pgq_k_shortest_walks_bulk_device (k = 1 and 16) for {lower,upper} = {1,3} and {1,4}, beside pgq_shortestpath_count_bulk_device and
pgq_all_shortestpaths_bulk_device (16) at the same max_hops, same process, same handle, same rows, on the SF100-shaped knows graph
of bench.py's snb_sf100 workload.  The two existing calls are the yardstick: the new ones do more work from round 3 on, because a
walk may revisit — the whole reachable graph is active in every round, no vertex ever leaves the queue — and are expected to cost more.

    timeout -k 10 900 python tools/bench_k_walks.py --sets grouped --out profiles/r18/k_walks_grouped.json && \\
    timeout -k 10 1100 python tools/bench_k_walks.py --sets random --out profiles/r18/k_walks_random.json

(each GPU step under a time limit of its own, chained with &&).

Two row sets: `random`, 4096 random pairs; `grouped`, a 64 x 64 product grouped by source (one lane batch).  Per row set, bounds
and call: --warmup + --steps calls, every call bracketed by a device synchronisation, the median, the minimum and the maximum over
the timed ones.  Then one more call of each with the statistics reset and per-kernel-class event timing on (option `profile`; the
timed calls run without it): the walk calls book their rounds (activation + pull + the rows' counts) as `push`, plan, unranking and
gather as `recon`, the lane assignment as `prep`.  Also reported: rounds, walked edges (out-list entries of the activation plus
in-list entries of the pull), the largest count, the rows with walks of two or more lengths, emitted walks and elements, and the
peak table bytes of a batch (walk_count: two rounds of 520 B per vertex; k_shortest_walks: one per round run, round 0 included).
NOT separated: the host round trip behind every round (one wait per round and batch), the growth of the staging buffer and the
mask resets, which no class books; activation from pull inside `push`; and the share of the long in-lists, which one wavefront
walks alone in the pull and in the unranking."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="JSON file for the results (default: stdout alone)")
    ap.add_argument("--bounds", default="1:3,1:4", help="the {lower,upper} pairs to measure, lower:upper, comma-separated")
    ap.add_argument("--ks", default="1,16", help="the k values of k_shortest_walks, comma-separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="grouped,random", help="row sets to measure, comma-separated")
    a = ap.parse_args()
    bounds = [tuple(int(x) for x in b.split(":")) for b in a.bounds.split(",") if b]
    ks = [int(k) for k in a.ks.split(",") if k]

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
    name, V, off, adj, eid, _, _ = bench.build_graph(ba)
    dev = pgq.DeviceCSR(V, off, adj, eid)
    rng = np.random.default_rng(43)
    row_sets = {
        "random": (rng.integers(0, V, 4096).astype(np.int64), rng.integers(0, V, 4096).astype(np.int64)),
        "grouped": (np.repeat(rng.choice(V, 64, replace=False), 64).astype(np.int64), np.tile(rng.choice(V, 64, replace=False), 64).astype(np.int64)),
    }
    out = {"graph": name, "V": int(V), "E": int(len(adj)), "steps": a.steps, "warmup": a.warmup, "table_bytes_per_round_and_batch": int(V) * 520,
           "device": torch.cuda.get_device_name(0), "version": pgq.load_hip().pgq_version().decode()}
    for label in [s for s in a.sets.split(",") if s]:
        ps, pd = row_sets[label]
        n = len(ps)
        t_s, t_d = torch.from_numpy(np.ascontiguousarray(ps)).cuda(), torch.from_numpy(np.ascontiguousarray(pd)).cuda()
        t_len, t_cnt, t_first, t_np, t_wc, t_sc = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(6))
        kmax = max(ks + [16])
        path_cap, child_cap = kmax * n, 16 * kmax * n + 1024
        t_po = torch.zeros(path_cap, dtype=torch.int64, device="cuda")
        t_ph = torch.zeros(path_cap, dtype=torch.int64, device="cuda")
        t_child = torch.zeros(child_cap, dtype=torch.int64, device="cuda")

        def measure(call):
            ms = []
            for j in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if j >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            pgq.set_option("profile", 1)
            pgq.reset_stats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            profiled_ms = (time.perf_counter() - t0) * 1e3
            st = pgq.get_stats()
            pgq.set_option("profile", 0)
            return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "profiled_call_ms": profiled_ms,
                    "rounds": st["levels"], "batches": st["batches"], "walked_edges": st["edges_scanned"],
                    "push_ms": st["kernel_ms"].get("push", 0.0), "recon_ms": st["kernel_ms"].get("recon", 0.0), "prep_ms": st["kernel_ms"].get("prep", 0.0),
                    "launches": {k: v for k, v in st["launches"].items() if v}}

        res = {"rows": n, "distinct_sources": int(len(np.unique(ps)))}
        for lo, hi in bounds:
            def walk_count_call():
                dev.walk_count_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, t_wc.data_ptr())

            def sp_count_call():
                dev.shortestpath_count_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), hi, t_sc.data_ptr())

            def asp_call():
                rc, pu, cu = dev.all_shortestpaths_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), hi, 16, t_len.data_ptr(), t_cnt.data_ptr(), t_first.data_ptr(),
                                                            t_np.data_ptr(), t_po.data_ptr(), path_cap, t_child.data_ptr(), child_cap)
                assert rc == 0, (rc, pu, cu, path_cap, child_cap)

            r = {"walk_count": measure(walk_count_call), "shortestpath_count": measure(sp_count_call), "all_shortestpaths_16": measure(asp_call)}
            wc, sc = t_wc.cpu().numpy(), t_sc.cpu().numpy()
            closed = ps == pd
            assert ((wc > 0) >= ((sc > 0) & ~closed)).all()  # a row with a shortest path of lo..hi edges has a walk (lo = 1: src == dst has none of 0 edges)
            r["rows_with_a_walk"] = int((wc > 0).sum())
            r["rows_with_a_shortest_path"] = int((sc > 0).sum())
            r["largest_count"] = int(wc.max())
            r["walk_count"]["peak_table_bytes"] = 2 * 520 * int(V)
            for k in ks:
                used = {}

                def walks_call():
                    rc, pu, cu = dev.k_shortest_walks_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, k, t_len.data_ptr(), t_cnt.data_ptr(), t_first.data_ptr(),
                                                               t_np.data_ptr(), t_po.data_ptr(), t_ph.data_ptr(), path_cap, t_child.data_ptr(), child_cap)
                    assert rc == 0, (rc, pu, cu, path_cap, child_cap)
                    used["walks"], used["elements"] = pu, cu

                m = measure(walks_call)
                npaths, first, ph = t_np.cpu().numpy(), t_first.cpu().numpy(), t_ph.cpu().numpy()
                assert (npaths == np.minimum(wc, k)).all()
                m["emitted_walks"], m["emitted_elements"] = int(used["walks"]), int(used["elements"])
                m["rows_with_two_or_more_lengths"] = int(sum(len(set(ph[f:f + c].tolist())) >= 2 for f, c in zip(first, npaths) if c >= 2))
                m["peak_table_bytes"] = 520 * int(V) * (-(-m["rounds"] // max(m["batches"], 1)) + 1)  # (the longest batch runs at least the mean, rounded up)
                r["k_shortest_walks_%d" % k] = m
            res["walks_%d_%d" % (lo, hi)] = r
            print("%s: {%d,%d}: walk_count %.3f ms, k_shortest_walks(%s) %s ms; shortestpath_count %.3f ms, all_shortestpaths(16) %.3f ms" % (
                label, lo, hi, r["walk_count"]["median_ms"], ",".join(map(str, ks)),
                " / ".join("%.3f" % r["k_shortest_walks_%d" % k]["median_ms"] for k in ks), r["shortestpath_count"]["median_ms"],
                r["all_shortestpaths_16"]["median_ms"]), file=sys.stderr, flush=True)
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
