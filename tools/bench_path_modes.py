#!/usr/bin/env python3
"""tools/bench_path_modes.py — what SHORTEST k costs under the path modes next to the walks themselves:
pgq_k_shortest_walks_mode_bulk_device under TRAIL, ACYCLIC and SIMPLE (k = 1 and 16) for {lower,upper} = {1,3} and {1,4}, beside
pgq_k_shortest_walks_bulk_device at the same arguments, same process, same handle, same rows, on the SF100-shaped knows graph of
bench.py's snb_sf100 workload with the two row sets of tools/bench_k_walks.py.  k_shortest_walks is the yardstick: the mode calls
run its rounds — more of them, a row closes by its distance alone — keep every round's table and then search each row twice, so
they do strictly more work.  No number is a target.

    timeout -k 10 900 python tools/bench_path_modes.py --sets grouped --out profiles/r19/path_modes_grouped.json && \\
    timeout -k 10 1100 python tools/bench_path_modes.py --sets random --out profiles/r19/path_modes_random.json

(each GPU step under a time limit of its own, chained with &&).

Per row set, bounds, k and call: --warmup + --steps calls, every call bracketed by a device synchronisation, the median, the
minimum and the maximum over the timed ones.  Then one more call with the statistics reset and per-kernel-class event timing on
(option `profile`; the timed calls run without it): rounds as `push`; the two search passes, the scans and the gather as `recon`.
Also reported: rounds, admitted walks and elements emitted, the `recon` share of the classes' time, and the steps of the search
(pgq_debug_mode_steps): their total over rows and both passes and the most one row took in one pass — the figure the shipped
mode_step_cap (2^24, a safety limit) is to be judged by.  A call that ends over the cap is recorded as such, not timed.
NOT separated: the host wait behind every round (one per round and batch) and behind the counting pass; the counting pass from
the emitting pass (both are `recon`, one launch each per batch: `recon` launches say how many); the long in-lists, which one
wavefront walks alone."""
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
    ap.add_argument("--ks", default="1,16", help="the k values, comma-separated")
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
    rng = np.random.default_rng(43)  # (bench_k_walks.py's rows)
    row_sets = {
        "random": (rng.integers(0, V, 4096).astype(np.int64), rng.integers(0, V, 4096).astype(np.int64)),
        "grouped": (np.repeat(rng.choice(V, 64, replace=False), 64).astype(np.int64), np.tile(rng.choice(V, 64, replace=False), 64).astype(np.int64)),
    }
    modes = (("trail", pgq.MODE_TRAIL), ("acyclic", pgq.MODE_ACYCLIC), ("simple", pgq.MODE_SIMPLE))
    out = {"graph": name, "V": int(V), "E": int(len(adj)), "steps": a.steps, "warmup": a.warmup, "mode_step_cap": pgq.get_option("mode_step_cap"),
           "device": torch.cuda.get_device_name(0), "version": pgq.load_hip().pgq_version().decode()}
    for label in [s for s in a.sets.split(",") if s]:
        ps, pd = row_sets[label]
        n = len(ps)
        t_s, t_d = torch.from_numpy(np.ascontiguousarray(ps)).cuda(), torch.from_numpy(np.ascontiguousarray(pd)).cuda()
        t_len, t_cnt, t_first, t_np = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(4))
        kmax = max(ks)
        path_cap, child_cap = kmax * n, (2 * max(hi for _, hi in bounds) + 1) * kmax * n
        t_po = torch.zeros(path_cap, dtype=torch.int64, device="cuda")
        t_ph = torch.zeros(path_cap, dtype=torch.int64, device="cuda")
        t_child = torch.zeros(child_cap, dtype=torch.int64, device="cuda")

        def measure(call, searched):
            used = {}
            rc = call(used)
            if rc != 0:  # over the step cap (or another refusal): recorded, not timed
                return {"failed": rc, "error": pgq.load_hip().pgq_last_error().decode()}
            ms = []
            for j in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(used)
                torch.cuda.synchronize()
                if j >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            pgq.set_option("profile", 1)
            pgq.reset_stats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(used)
            torch.cuda.synchronize()
            profiled_ms = (time.perf_counter() - t0) * 1e3
            st = pgq.get_stats()
            pgq.set_option("profile", 0)
            total, row_max = pgq.mode_steps() if searched else (0, 0)  # (the steps of the thread's last MODE call)
            class_ms = sum(st["kernel_ms"].values())
            recon = st["kernel_ms"].get("recon", 0.0)
            npaths = t_np.cpu().numpy()
            return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "profiled_call_ms": profiled_ms,
                    "rounds": st["levels"], "batches": st["batches"], "walked_edges": st["edges_scanned"],
                    "push_ms": st["kernel_ms"].get("push", 0.0), "recon_ms": recon, "prep_ms": st["kernel_ms"].get("prep", 0.0),
                    "recon_share_of_class_time": recon / class_ms if class_ms > 0 else 0.0,
                    "launches": {k: v for k, v in st["launches"].items() if v},
                    "emitted_walks": int(used["walks"]), "emitted_elements": int(used["elements"]), "rows_with_a_walk": int((npaths > 0).sum()),
                    "rows_with_k_walks": int((npaths >= used["k"]).sum()), "steps_total": int(total), "steps_row_max": int(row_max),
                    "peak_table_bytes": 520 * int(V) * (-(-st["levels"] // max(st["batches"], 1)) + 1)}

        res = {"rows": n, "distinct_sources": int(len(np.unique(ps)))}
        for lo, hi in bounds:
            r = {}
            for k in ks:
                def walks_call(used):
                    rc, pu, cu = dev.k_shortest_walks_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, k, t_len.data_ptr(), t_cnt.data_ptr(), t_first.data_ptr(),
                                                               t_np.data_ptr(), t_po.data_ptr(), t_ph.data_ptr(), path_cap, t_child.data_ptr(), child_cap)
                    used["walks"], used["elements"], used["k"] = pu, cu, k
                    return rc

                r["k_shortest_walks_%d" % k] = measure(walks_call, False)
                walk_np = t_np.cpu().numpy().copy()
                for mname, mode in modes:
                    def mode_call(used):
                        rc, pu, cu = dev.k_shortest_walks_mode_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, k, mode, t_len.data_ptr(), t_cnt.data_ptr(),
                                                                        t_first.data_ptr(), t_np.data_ptr(), t_po.data_ptr(), t_ph.data_ptr(), path_cap,
                                                                        t_child.data_ptr(), child_cap)
                        used["walks"], used["elements"], used["k"] = pu, cu, k
                        return rc

                    m = measure(mode_call, True)
                    if "failed" not in m:
                        assert (t_np.cpu().numpy() <= walk_np).all()  # a mode admits no more than there are walks
                    r["%s_%d" % (mname, k)] = m
                print("%s: {%d,%d}, k = %d: k_shortest_walks %s ms; %s" % (
                    label, lo, hi, k, "%.3f" % r["k_shortest_walks_%d" % k].get("median_ms", float("nan")),
                    ", ".join("%s %s ms (%s steps, row max %s)" % (mname, "%.3f" % r["%s_%d" % (mname, k)].get("median_ms", float("nan")),
                                                                   r["%s_%d" % (mname, k)].get("steps_total"), r["%s_%d" % (mname, k)].get("steps_row_max"))
                              for mname, _ in modes)), file=sys.stderr, flush=True)
            res["walks_%d_%d" % (lo, hi)] = r
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
