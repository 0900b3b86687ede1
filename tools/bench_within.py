#!/usr/bin/env python3
"""tools/bench_within.py — what a hop bound saves: the bounded bulk call against the unbounded one on bench.py's graphs.

    python tools/bench_within.py --out profiles/r08/within.json            # this build
    PGQ_HIP_LIB=/path/to/parent/libpgq_hip.so python tools/bench_within.py --baseline --out profiles/r08/within_parent.json

One child process per workload (snb_sf100: 65,536 random pairs; snb_cross and rmat22_cross: 2048 x 1024 cross products), each
under its own `timeout`; the script stops at the first child that fails.  A child builds the workload's graph and rows with
bench.py's generators, times pgq_iterativelength_bulk_device and, for max_hops in (2, 3, 4, 6), the bounded bulk call (median
and min of --steps calls after --warmup, each call bracketed by a device synchronisation) and checks every bounded result equal
to the unbounded one clamped at the bound.  --baseline times the unbounded call alone: that is what a parent build, which has
no bounded call, can run (PGQ_HIP_LIB selects its library)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("snb_sf100", "snb_cross", "rmat22_cross")
BOUNDS = (2, 3, 4, 6)


def child(a):
    import numpy as np
    import torch

    import bench
    import duckpgq_extension_amd as pgq

    argv, sys.argv = sys.argv, ["bench.py", "--workload", a.child]
    try:
        ba = bench.parse()
    finally:
        sys.argv = argv
    name, V, off, adj, eid, _, _ = bench.build_graph(ba)
    pairs = bench.make_pairs(ba, V, bench.DEFAULT_PAIRS[a.child], off, adj)
    dev = pgq.DeviceCSR(V, off, adj, eid)
    n = len(pairs)
    t_s = torch.from_numpy(np.ascontiguousarray(pairs[:, 0])).cuda()
    t_d = torch.from_numpy(np.ascontiguousarray(pairs[:, 1])).cuda()
    t_o = torch.empty(n, dtype=torch.int64, device="cuda")

    def timed(call):
        ms = []
        for k in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    out = {"workload": a.child, "graph": name, "rows": n, "steps": a.steps, "warmup": a.warmup,
           "library": os.environ.get("PGQ_HIP_LIB", "this build")}
    out["unbounded"] = timed(lambda: dev.iterativelength_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr()))
    full = t_o.clone()
    for U in () if a.baseline else BOUNDS:
        r = timed(lambda: dev.iterativelength_within_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), U, t_o.data_ptr()))
        want = torch.where(full > U, torch.full_like(full, -1), full)
        if not bool((t_o == want).all()):
            raise SystemExit("max_hops %d: %d rows differ from the clamped unbounded result" % (U, int((t_o != want).sum())))
        r["rows_within"] = int((want >= 0).sum())
        out["within_%d" % U] = r
    # the unbounded call again: whether the bounded calls in between moved its route
    out["unbounded_after"] = timed(lambda: dev.iterativelength_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), t_o.data_ptr()))
    if not bool((t_o == full).all()):
        raise SystemExit("the unbounded result changed between calls")
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="JSON file for the collected results (default: stdout alone)")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per workload (its own `timeout`)")
    ap.add_argument("--baseline", action="store_true", help="time the unbounded call alone (a build without the bounded call)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    results = []
    for wl in a.workloads.split(","):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", wl,
               "--steps", str(a.steps), "--warmup", str(a.warmup)] + (["--baseline"] if a.baseline else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:  # nothing more is started on the device after a failure
            sys.stderr.write("%s failed with status %d: stopping\n" % (wl, p.returncode))
            return p.returncode
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(p.stdout.strip().splitlines()[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
