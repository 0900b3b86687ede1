#!/usr/bin/env python3
"""tools/bench_cheapest_path_within.py — what the list costs next to the number under a hop bound:
pgq_cheapest_path_within_bulk_device beside pgq_cheapest_path_length_within_bulk_device at the same max_hops, same process,
same handle, same rows, on the weighted SF100-shaped knows graph of bench.py's snb_cheapest workload (the graph and the rows
of tools/bench_cheapest_within.py and tools/bench_cheapest_path.py), and pgq_cheapest_path_bulk_device (unbounded) beside them.

    timeout -k 10 900 python tools/bench_cheapest_path_within.py --sets grouped --out profiles/r16/cheapest_path_within_grouped.json && \\
    timeout -k 10 1100 python tools/bench_cheapest_path_within.py --sets random --out profiles/r16/cheapest_path_within_random.json

(each GPU step under a time limit of its own, chained with &&).

Two row sets: `random`, 4096 random pairs; `grouped`, a 64 x 64 product grouped by source (one lane batch).  Per row set, K
and call: --warmup + --steps calls, every call bracketed by a device synchronisation, the median, the minimum and the maximum
over the timed ones.  Then one more call of each with the statistics reset and per-kernel-class event timing on (option
`profile`; the timed calls run without it).  The bounded list call books its rounds AND its log passes as the `relax` class —
the log pass stands where the length call's snapshot launch stands, which that call books as `relax` too, so the class compares
like with like; the two are not separated — and lengths, walk-back and gather as `recon`, the lane assignment as `prep`.  NOT
separated: the host round trip behind every round (the list call waits after every round, the length call once per eight),
the growth of the log and of the staging buffer, the resets, which no class books.  One more call of the list form runs with
PGQ_RELAX_TRACE set and the library's stderr read back: its last line says the peak bytes of a batch's round log.
cheapest_path (unbounded) is timed with --path-steps calls: on the random set a call takes about ten seconds."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def traced(call):
    """What the library writes to stderr during one call with PGQ_RELAX_TRACE set."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["PGQ_RELAX_TRACE"] = "1"
        try:
            call()
        finally:
            del os.environ["PGQ_RELAX_TRACE"]
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="JSON file for the results (default: stdout alone)")
    ap.add_argument("--ks", default="2,3,4", help="the bounds to measure, comma-separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--path-steps", type=int, default=3, help="timed calls of the unbounded cheapest_path (one warm-up); 0: skip it")
    ap.add_argument("--sets", default="grouped,random", help="row sets to measure, comma-separated")
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
    rng = np.random.default_rng(43)
    row_sets = {
        "random": (rng.integers(0, V, 4096).astype(np.int64), rng.integers(0, V, 4096).astype(np.int64)),
        "grouped": (np.repeat(rng.choice(V, 64, replace=False), 64).astype(np.int64), np.tile(rng.choice(V, 64, replace=False), 64).astype(np.int64)),
    }
    out = {"graph": name, "V": int(V), "E": int(len(adj)), "steps": a.steps, "warmup": a.warmup, "path_steps": a.path_steps,
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

        def measure(call, steps, warmup):
            ms = []
            for k in range(warmup + steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if k >= warmup:
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
        for K in ks:
            def length_call():
                dev.cheapest_within_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), K, t_val.data_ptr(), t_ok.data_ptr())

            def path_call():
                rc, used = dev.cheapest_path_within_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), K, t_len.data_ptr(), t_off.data_ptr(), t_child.data_ptr(), cap)
                assert rc == 0, (rc, used, cap)
                return used

            r = {"cheapest_path_length_within": measure(length_call, a.steps, a.warmup), "cheapest_path_within": measure(path_call, a.steps, a.warmup)}
            lk, pk = r["cheapest_path_length_within"]["kernel_ms"], r["cheapest_path_within"]["kernel_ms"]
            r["split_ms"] = {"rounds + log passes (relax)": pk.get("relax", 0.0), "lengths, walk-back, gather (recon)": pk.get("recon", 0.0),
                             "lane assignment (prep)": pk.get("prep", 0.0)}
            r["list_minus_length_by_class_ms"] = {k: pk.get(k, 0.0) - lk.get(k, 0.0) for k in sorted(set(pk) | set(lk))}
            # what must hold between the two: the same rows have a walk, and the list's hop count is within the bound
            ok, ln = t_ok.cpu().numpy().astype(bool), t_len.cpu().numpy()
            trivial = ps == pd
            assert ((ln >= 0) == (ok | trivial)).all() and ln.max() <= K
            r["null_rows"] = int((ln < 0).sum())
            r["list_elements"] = int(path_call())
            m = re.findall(r"hop log: peak (\d+) bytes", traced(path_call))
            r["peak_log_bytes_per_batch"] = int(m[-1]) if m else None
            res["within_%d" % K] = r
            print("%s: max_hops %d: list %.3f ms, length %.3f ms" % (label, K, r["cheapest_path_within"]["median_ms"],
                                                                     r["cheapest_path_length_within"]["median_ms"]), file=sys.stderr, flush=True)
        if a.path_steps > 0:
            def unbounded_call():
                rc, used = dev.cheapest_path_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), t_len.data_ptr(), t_off.data_ptr(), t_child.data_ptr(), cap)
                assert rc == 0, (rc, used, cap)

            res["cheapest_path"] = measure(unbounded_call, a.path_steps, 1)
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
