#!/usr/bin/env python3
"""tools/bench_cheapest_within.py — what a hop bound costs or saves cheapest_path_length: pgq_cheapest_path_length_within_bulk_device
at max_hops = 2, 3, 4 beside pgq_cheapest_path_length_bulk_device (unchanged code: the only number a caller could get before,
though a DIFFERENT one — the two compute different things, so the comparison says what the bound costs or saves, not which is
faster), same process, same handle, same rows, on the weighted SF100-shaped knows graph of bench.py's snb_cheapest workload.

    timeout -k 10 900 python tools/bench_cheapest_within.py --ks 2 --out profiles/r11/cheapest_within_k2.json && \\
    timeout -k 10 900 python tools/bench_cheapest_within.py --ks 3 --out profiles/r11/cheapest_within_k3.json && ...

(each GPU step under a time limit of its own, chained with &&; one call with --ks 2,3,4 where a single limit is enough).

Two row sets: `random`, 4096 random pairs; `grouped`, a 64 x 64 product grouped by source (one lane batch).  Per row set and K:
--warmup + --steps calls, every call bracketed by a device synchronisation, the median over the timed ones; one more call with
the statistics reset in front: rounds (`levels`), walked edges (`edges_scanned`), lane batches, launches, and the relax class's
algo_bytes over the median time against the 8 TB/s HBM peak (a whole-call rate, not a kernel's share of peak); the share of
NULL rows.  The same for the unbounded call."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="JSON file for the results (default: stdout alone)")
    ap.add_argument("--ks", default="2,3,4", help="the bounds to measure, comma-separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",") if k]

    import numpy as np
    import torch

    import bench
    import duckpgq_extension_amd as pgq

    assert torch.cuda.is_available(), "needs the GPU: a time taken elsewhere says nothing"
    argv, sys.argv = sys.argv, ["bench.py", "--workload", "snb_cheapest"]
    try:
        ba = bench.parse()
    finally:
        sys.argv = argv
    name, V, off, adj, eid, w, _ = bench.build_graph(ba)
    dev = pgq.DeviceCSR(V, off, adj, eid, w)
    deg = np.diff(off)
    rng = np.random.default_rng(43)
    row_sets = {
        "random": (rng.integers(0, V, 4096).astype(np.int64), rng.integers(0, V, 4096).astype(np.int64)),
        "grouped": (np.repeat(rng.choice(V, 64, replace=False), 64).astype(np.int64), np.tile(rng.choice(V, 64, replace=False), 64).astype(np.int64)),
    }
    out = {"graph": name, "V": int(V), "E": int(len(adj)), "max_out_degree": int(deg.max()), "lists_over_128_edges": int((deg > 128).sum()),
           "edges_in_lists_over_128": int(deg[deg > 128].sum()), "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "version": pgq.load_hip().pgq_version().decode()}
    for label, (ps, pd) in row_sets.items():
        n = len(ps)
        t_s, t_d = torch.from_numpy(np.ascontiguousarray(ps)).cuda(), torch.from_numpy(np.ascontiguousarray(pd)).cuda()
        t_val = torch.zeros(n, dtype=torch.int64, device="cuda")
        t_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        ptrs = (t_val.data_ptr(), t_ok.data_ptr())

        def measure(call):
            ms = []
            for k in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if k >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            pgq.reset_stats()
            call()
            torch.cuda.synchronize()
            st = pgq.get_stats()
            med = statistics.median(ms)
            ok = t_ok.cpu().numpy().astype(bool)
            return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "rounds": st["levels"], "batches": st["batches"],
                    "walked_edges": st["edges_scanned"], "relax_algo_bytes": st["algo_bytes"]["relax"],
                    "relax_bytes_per_s_over_hbm_peak": st["algo_bytes"]["relax"] / (med * 1e-3) / HBM_PEAK,
                    "null_rows": int((~ok).sum()), "null_share": float((~ok).mean()),
                    "launches": {k: v for k, v in st["launches"].items() if v}}, t_val.cpu().numpy().copy(), ok

        res = {"rows": n, "distinct_sources": int(len(np.unique(ps)))}
        res["unbounded"], u_val, u_ok = measure(lambda: dev.cheapest_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), *ptrs))
        for K in ks:
            r, b_val, b_ok = measure(lambda: dev.cheapest_within_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), K, *ptrs))
            # what must hold between the two: a row within the bound is reachable, and costs at least the unbounded cost
            assert not (b_ok & ~u_ok).any() and (b_val[b_ok] >= u_val[b_ok]).all()
            r["rows_costlier_than_unbounded"] = int((b_val[b_ok] > u_val[b_ok]).sum())
            res["within_%d" % K] = r
            print("%s: max_hops %d: %.3f ms, %d rounds" % (label, K, r["median_ms"], r["rounds"]), file=sys.stderr, flush=True)
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
