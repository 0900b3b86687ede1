#!/usr/bin/env python3
"""tools/bench_cheapest_path.py — what the list costs next to the number: pgq_cheapest_path_bulk_device beside
pgq_cheapest_path_length_bulk_device, same process, same handle, same rows, on the weighted SF100-shaped knows graph of
bench.py's snb_cheapest workload (the graph and the rows of tools/bench_cheapest_within.py).

    timeout -k 10 1100 python tools/bench_cheapest_path.py --out profiles/r12/cheapest_path.json

Two row sets: `random`, 4096 random pairs; `grouped`, a 64 x 64 product grouped by source (one lane batch).  Per row set and
call: --warmup + --steps calls, every call bracketed by a device synchronisation, the median, the minimum and the maximum over
the timed ones.  Then one more call of each with the statistics reset and per-kernel-class event timing on (option `profile`;
the timed calls run without it): cheapest_path's settling is the `relax` class, its tight-level rounds the `push` class, its
lengths, walk-back and gather the `recon` class, the lane assignment `prep`.  NOT separated: the host round trip behind every
round (the gap between the sum of the classes and the call's wall time is mostly that), the staging buffer's growth and the
resets of the labels and hop counts, which no class books.  The two calls do different work on purpose: the length call
prunes every lane at its destinations' bound and takes the chain pre-pass and the weight-sorted lists where they pay,
cheapest_path settles every label a source reaches over the plain lists."""
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="grouped,random", help="row sets to measure, comma-separated")
    ap.add_argument("--random-rows", type=int, default=4096, help="rows of the `random` set")
    a = ap.parse_args()

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
    rng = np.random.default_rng(43)
    row_sets = {
        "random": (rng.integers(0, V, 4096).astype(np.int64)[:a.random_rows], rng.integers(0, V, 4096).astype(np.int64)[:a.random_rows]),
        "grouped": (np.repeat(rng.choice(V, 64, replace=False), 64).astype(np.int64), np.tile(rng.choice(V, 64, replace=False), 64).astype(np.int64)),
    }
    out = {"graph": name, "V": int(V), "E": int(len(adj)), "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "version": pgq.load_hip().pgq_version().decode()}
    for label in [s for s in a.sets.split(",") if s]:
        ps, pd = row_sets[label]
        n = len(ps)
        t_s, t_d = torch.from_numpy(np.ascontiguousarray(ps)).cuda(), torch.from_numpy(np.ascontiguousarray(pd)).cuda()
        t_val = torch.zeros(n, dtype=torch.int64, device="cuda")
        t_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        t_len = torch.zeros(n, dtype=torch.int64, device="cuda")
        t_off = torch.zeros(n, dtype=torch.int64, device="cuda")
        cap = 64 * n + 1024
        t_child = torch.zeros(cap, dtype=torch.int64, device="cuda")

        def length_call():
            dev.cheapest_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), t_val.data_ptr(), t_ok.data_ptr())

        def path_call():
            rc, used = dev.cheapest_path_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), t_len.data_ptr(), t_off.data_ptr(), t_child.data_ptr(), cap)
            assert rc == 0, (rc, used, cap)
            return used

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
        res["cheapest_path_length"] = measure(length_call)
        res["cheapest_path"] = measure(path_call)
        km = res["cheapest_path"]["kernel_ms"]
        res["cheapest_path"]["split_ms"] = {"settle (relax)": km.get("relax", 0.0), "levels (push)": km.get("push", 0.0),
                                            "walk-back, lengths, gather (recon)": km.get("recon", 0.0), "lane assignment (prep)": km.get("prep", 0.0)}
        # what must hold between the two: the same rows have a path, and the list's hop count fits its length
        ok, ln = t_ok.cpu().numpy().astype(bool), t_len.cpu().numpy()
        assert ((ln >= 0) == ok).all()
        res["null_rows"] = int((~ok).sum())
        res["list_elements"] = int(path_call())
        res["max_hops"] = int(ln.max())
        out[label] = res
        print("%s: cheapest_path %.3f ms, cheapest_path_length %.3f ms" % (label, res["cheapest_path"]["median_ms"],
                                                                           res["cheapest_path_length"]["median_ms"]), file=sys.stderr, flush=True)
        print(json.dumps({label: res}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
