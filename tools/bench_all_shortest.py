#!/usr/bin/env python3
"""tools/bench_all_shortest.py — what ALL SHORTEST costs next to ANY SHORTEST: pgq_shortestpath_count_bulk_device and
pgq_all_shortestpaths_bulk_device (max_paths 1 and 16) beside pgq_shortestpath_within_bulk_device and
pgq_iterativelength_within_bulk_device at the same max_hops, same process, same handle, same rows, on the SF100-shaped knows
graph of bench.py's snb_sf100 workload.  The two existing calls are the yardstick: the new ones do strictly more work (every
level of every source's search, a 512-byte sigma row per counted in-slot, one wavefront per emitted path) and are expected to
cost more.

    timeout -k 10 900 python tools/bench_all_shortest.py --sets grouped --out profiles/r17/all_shortest_grouped.json && \\
    timeout -k 10 1100 python tools/bench_all_shortest.py --sets random --out profiles/r17/all_shortest_random.json

(each GPU step under a time limit of its own, chained with &&).

Two row sets: `random`, 4096 random pairs; `grouped`, a 64 x 64 product grouped by source (one lane batch).  Per row set,
max_hops and call: --warmup + --steps calls, every call bracketed by a device synchronisation, the median, the minimum and the
maximum over the timed ones.  Then one more call of each with the statistics reset and per-kernel-class event timing on (option
`profile`; the timed calls run without it): the new calls book their rounds (levels + sigma pull + frontier upkeep) as `push`,
plan, unranking and gather as `recon`, the lane assignment as `prep`.  Also reported: rounds, walked edges (out-list entries of
the level kernel plus in-list entries of the sigma pull), rows with sigma >= 2, the largest sigma, emitted paths and elements,
and the workspace of a batch (768 B per vertex: hop counts and sigma).  NOT separated: the host round trip behind every round,
the growth of the staging buffer, the resets, which no class books; levels from the sigma pull inside `push`; and the share of
the long in-lists, which one wavefront walks alone in the pull and in the unranking."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INT64_MAX = (1 << 63) - 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="JSON file for the results (default: stdout alone)")
    ap.add_argument("--hops", default="3,4,max", help="the bounds to measure, comma-separated; max = INT64_MAX")
    ap.add_argument("--paths", default="1,16", help="the max_paths values of all_shortestpaths, comma-separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="grouped,random", help="row sets to measure, comma-separated")
    a = ap.parse_args()
    hops = [INT64_MAX if h == "max" else int(h) for h in a.hops.split(",") if h]
    paths = [int(p) for p in a.paths.split(",") if p]

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
    out = {"graph": name, "V": int(V), "E": int(len(adj)), "steps": a.steps, "warmup": a.warmup, "workspace_bytes_per_batch": int(V) * 768,
           "device": torch.cuda.get_device_name(0), "version": pgq.load_hip().pgq_version().decode()}
    for label in [s for s in a.sets.split(",") if s]:
        ps, pd = row_sets[label]
        n = len(ps)
        t_s, t_d = torch.from_numpy(np.ascontiguousarray(ps)).cuda(), torch.from_numpy(np.ascontiguousarray(pd)).cuda()
        t_len, t_cnt, t_first, t_np, t_off, t_il = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(6))
        path_cap, child_cap = max(paths) * n, 64 * max(paths) * n + 1024
        t_po = torch.zeros(path_cap, dtype=torch.int64, device="cuda")
        t_child = torch.zeros(child_cap, dtype=torch.int64, device="cuda")

        def measure(call):
            ms = []
            for k in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if k >= a.warmup:
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
                    "rounds": st["levels"], "batches": st["batches"], "walked_edges": st["edges_scanned"], "host_waits": st["host_waits"],
                    "kernel_ms": {k: v for k, v in st["kernel_ms"].items() if v}, "launches": {k: v for k, v in st["launches"].items() if v}}

        res = {"rows": n, "distinct_sources": int(len(np.unique(ps)))}
        for h in hops:
            def length_call():
                dev.iterativelength_within_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), h, t_il.data_ptr())

            def path_call():
                rc, used = dev.shortestpath_within_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), h, t_len.data_ptr(), t_off.data_ptr(), t_child.data_ptr(), child_cap)
                assert rc == 0, (rc, used, child_cap)

            def count_call():
                dev.shortestpath_count_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), h, t_cnt.data_ptr())

            r = {"iterativelength_within": measure(length_call), "shortestpath_within": measure(path_call), "shortestpath_count": measure(count_call)}
            cnt = t_cnt.cpu().numpy()
            il = t_il.cpu().numpy()
            assert ((cnt > 0) == (il >= 0)).all()  # the same rows are within the bound
            r["rows_within_bound"] = int((cnt > 0).sum())
            r["rows_sigma_ge_2"] = int((cnt >= 2).sum())
            r["largest_sigma"] = int(cnt.max())
            for p in paths:
                used = {}

                def all_call():
                    rc, pu, cu = dev.all_shortestpaths_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), h, p, t_len.data_ptr(), t_cnt.data_ptr(), t_first.data_ptr(),
                                                                t_np.data_ptr(), t_po.data_ptr(), path_cap, t_child.data_ptr(), child_cap)
                    assert rc == 0, (rc, pu, cu, path_cap, child_cap)
                    used["paths"], used["elements"] = pu, cu

                m = measure(all_call)
                assert (t_len.cpu().numpy() == il).all() and (t_np.cpu().numpy() == np.minimum(cnt, p)).all()
                m["emitted_paths"], m["emitted_elements"] = int(used["paths"]), int(used["elements"])
                m["split_ms"] = {"rounds (push)": m["kernel_ms"].get("push", 0.0), "plan, unranking, gather (recon)": m["kernel_ms"].get("recon", 0.0),
                                 "lane assignment (prep)": m["kernel_ms"].get("prep", 0.0)}
                r["all_shortestpaths_%d" % p] = m
            res["within_%s" % ("max" if h == INT64_MAX else h)] = r
            print("%s: max_hops %s: count %.3f ms, all(%s) %s ms, shortestpath %.3f ms, iterativelength %.3f ms" % (
                label, "max" if h == INT64_MAX else h, r["shortestpath_count"]["median_ms"], ",".join(map(str, paths)),
                " / ".join("%.3f" % r["all_shortestpaths_%d" % p]["median_ms"] for p in paths), r["shortestpath_within"]["median_ms"],
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
