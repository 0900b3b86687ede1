#!/usr/bin/env python3
"""tools/bench_walk_length.py — what the filter of a quantified pattern in WALK mode costs: pgq_walk_length_bulk_device under the
automatic direction and under forced push and forced pull (option walk_length_pull, per handle), beside the two calls that answer the
same question with strictly more work — pgq_walk_count_bulk_device and pgq_k_shortest_walks_bulk_device(k = 1) — and beside the
floor whose answers are wrong for walks, pgq_iterativelength_within_bulk_device(upper).  Same process, same handle, same rows, on
the SF100-shaped knows graph of bench.py's snb_sf100 workload, with the two row sets of tools/bench_k_walks.py.

    timeout -k 10 600 python tools/bench_walk_length.py --sets grouped --out profiles/r21/walk_length_grouped.json && \\
    timeout -k 10 1100 python tools/bench_walk_length.py --sets random --out profiles/r21/walk_length_random.json

(each GPU step under a time limit of its own, chained with &&).

Per row set, bounds and call: --warmup + --steps calls, every call bracketed by a device synchronisation; the median, the minimum
and the maximum over the timed ones.  Then one more call of each with the statistics reset and per-kernel-class event timing on.
Also reported per bounds: the rows stage 1 left (0 <= dist < lower, from the floor's answers), and per walk_length line its
batches, its rounds by direction, the adjacency entries its rounds walked and the peak bytes of a batch (two mask arrays and two
queues: 24 B per vertex).  Every walk_length answer is compared with k_shortest_walks(k = 1)'s hops and with walk_count > 0.
`condition_1`: on every line walk_length's median is at most k_shortest_walks(k = 1)'s on the same rows; a line above it is named.
NOT separated: the host wait behind every round (one per round and batch), stage 1's share (its kernels book under their own
classes: meet, ball, the lane batches' push / pull) and the classifying kernel, which no class books."""
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
    ap.add_argument("--bounds", default="1:3,2:3,2:4,3:4", help="the {lower,upper} pairs to measure, lower:upper, comma-separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="grouped,random", help="row sets to measure, comma-separated")
    a = ap.parse_args()
    bounds = [tuple(int(x) for x in b.split(":")) for b in a.bounds.split(",") if b]

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
    out = {"graph": name, "V": int(V), "E": int(len(adj)), "steps": a.steps, "warmup": a.warmup, "peak_bytes_per_batch": 24 * int(V),
           "walk_length_pull_div": pgq.get_default_option("walk_length_pull_div"), "device": torch.cuda.get_device_name(0),
           "version": pgq.load_hip().pgq_version().decode(), "condition_1_broken": []}
    for label in [s for s in a.sets.split(",") if s]:
        ps, pd = row_sets[label]
        n = len(ps)
        t_s, t_d = torch.from_numpy(np.ascontiguousarray(ps)).cuda(), torch.from_numpy(np.ascontiguousarray(pd)).cuda()
        t_wl, t_len, t_cnt, t_first, t_np, t_wc, t_il, t_po, t_ph = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(9))

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
            dev.set_option("profile", 1)
            pgq.reset_stats()
            call()
            torch.cuda.synchronize()
            st = pgq.get_stats()
            pgq.set_option("profile", 0)
            dev.set_option("profile", 0)
            return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "batches": st["batches"], "rounds": st["levels"],
                    "push_rounds": st["push_levels"], "pull_rounds": st["pull_levels"], "walked_edges": st["edges_scanned"],
                    "kernel_ms": {k: round(v, 4) for k, v in st["kernel_ms"].items() if v}, "launches": {k: v for k, v in st["launches"].items() if v}}

        res = {"rows": n, "distinct_sources": int(len(np.unique(ps)))}
        for lo, hi in bounds:
            child = torch.zeros(n * (2 * hi + 1), dtype=torch.int64, device="cuda")

            def walk_length_call():
                dev.walk_length_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, t_wl.data_ptr())

            def walk_count_call():
                dev.walk_count_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, t_wc.data_ptr())

            def k1_call():
                rc, pu, cu = dev.k_shortest_walks_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, 1, t_len.data_ptr(), t_cnt.data_ptr(), t_first.data_ptr(),
                                                           t_np.data_ptr(), t_po.data_ptr(), t_ph.data_ptr(), n, child.data_ptr(), child.numel())
                assert rc == 0, (rc, pu, cu)

            def within_call():
                dev.iterativelength_within_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), hi, t_il.data_ptr())

            r = {"walk_count": measure(walk_count_call), "k_shortest_walks_1": measure(k1_call), "iterativelength_within": measure(within_call)}
            hops, wc, dist = t_len.cpu().numpy(), t_wc.cpu().numpy(), t_il.cpu().numpy()
            r["rows_stage_1_left"] = int(((dist >= 0) & (dist < lo)).sum())
            r["rows_with_a_walk"] = int((wc > 0).sum())
            r["rows_the_floor_answers_differently"] = int((np.where((dist >= lo), dist, -1) != hops).sum())
            for direction, mode in (("auto", 2), ("push", 0), ("pull", 1)):
                dev.set_option("walk_length_pull", mode)
                m = measure(walk_length_call)
                got = t_wl.cpu().numpy()
                assert (got == hops).all() and ((got >= 0) == (wc > 0)).all(), (label, lo, hi, direction)
                m["peak_bytes_of_a_batch"] = 24 * int(V) if m["batches"] else 0
                r["walk_length_" + direction] = m
                if m["median_ms"] > r["k_shortest_walks_1"]["median_ms"]:
                    out["condition_1_broken"].append([label, lo, hi, direction, m["median_ms"], r["k_shortest_walks_1"]["median_ms"]])
            dev.set_option("walk_length_pull", 2)
            res["walks_%d_%d" % (lo, hi)] = r
            print("%s: {%d,%d}: walk_length auto %.3f / push %.3f / pull %.3f ms (%d rows left, %d batches); walk_count %.3f, k_shortest_walks(1) %.3f, "
                  "iterativelength_within %.3f ms" % (label, lo, hi, r["walk_length_auto"]["median_ms"], r["walk_length_push"]["median_ms"],
                                                      r["walk_length_pull"]["median_ms"], r["rows_stage_1_left"], r["walk_length_auto"]["batches"],
                                                      r["walk_count"]["median_ms"], r["k_shortest_walks_1"]["median_ms"],
                                                      r["iterativelength_within"]["median_ms"]), file=sys.stderr, flush=True)
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
