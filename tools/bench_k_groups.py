#!/usr/bin/env python3
"""tools/bench_k_groups.py — what SHORTEST k GROUP costs next to SHORTEST k: pgq_k_shortest_groups_bulk_device at groups = 1 and 2
and max_paths = 16 and 4096 under WALK, TRAIL, ACYCLIC and SIMPLE for {lower,upper} = {1,3} and {1,4}, beside
pgq_k_shortest_walks_mode_bulk_device with k = max_paths at the same bounds, same process, same handle, same rows, on the
SF100-shaped knows graph of bench.py's snb_sf100 workload with the two row sets of tools/bench_k_walks.py.  The yardstick lists the
first max_paths walks whatever their lengths; the group call stops at a group boundary, so it emits no more than the yardstick and
under WALK may stop its rounds sooner — under a mode with groups >= 2 it runs them to `upper`.  No number is a target.

    timeout -k 10 600 python tools/bench_k_groups.py --sets grouped --out profiles/r20/k_groups_grouped.json && \\
    timeout -k 10 900 python tools/bench_k_groups.py --sets random --max-paths 16 --out profiles/r20/k_groups_random.json

(each GPU step under a time limit of its own, chained with &&).

Per row set, bounds, max_paths, mode and call: --warmup + --steps calls, every call bracketed by a device synchronisation, the
median, the minimum and the maximum over the timed ones.  Then one more call with the statistics reset and per-kernel-class event
timing on (option `profile`; the timed calls run without it): rounds as `push`; plan / unranking or the two search passes, the scans
and the gather as `recon`.  Also reported: rounds, walks and elements emitted, the rows the cap cut (count > npaths), the groups per
row (their sum, and the rows with 0, 1 and 2 of them) and, under a mode, the steps of the search (pgq_debug_mode_steps).
NOT separated: the host wait behind every round (one per round and batch) and behind the plan / the counting pass; the counting
pass from the emitting pass (both `recon`); the row-closing step from the round it follows (`push`); the long in-lists, which one
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
    ap.add_argument("--groups", default="1,2", help="the groups values, comma-separated")
    ap.add_argument("--max-paths", default="16,4096", help="the max_paths values (the yardstick's k), comma-separated")
    ap.add_argument("--modes", default="walk,trail,acyclic,simple")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", default="grouped,random", help="row sets to measure, comma-separated")
    a = ap.parse_args()
    bounds = [tuple(int(x) for x in b.split(":")) for b in a.bounds.split(",") if b]
    gs = [int(g) for g in a.groups.split(",") if g]
    caps = [int(p) for p in a.max_paths.split(",") if p]

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
    all_modes = {"walk": pgq.MODE_WALK, "trail": pgq.MODE_TRAIL, "acyclic": pgq.MODE_ACYCLIC, "simple": pgq.MODE_SIMPLE}
    modes = [(m, all_modes[m]) for m in a.modes.split(",") if m]
    out = {"graph": name, "V": int(V), "E": int(len(adj)), "steps": a.steps, "warmup": a.warmup, "mode_step_cap": pgq.get_option("mode_step_cap"),
           "device": torch.cuda.get_device_name(0), "version": pgq.load_hip().pgq_version().decode()}
    for label in [s for s in a.sets.split(",") if s]:
        ps, pd = row_sets[label]
        n = len(ps)
        t_s, t_d = torch.from_numpy(np.ascontiguousarray(ps)).cuda(), torch.from_numpy(np.ascontiguousarray(pd)).cuda()
        t_len, t_cnt, t_first, t_np, t_ng = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(5))
        pmax = max(caps)
        path_cap, child_cap = pmax * n, (2 * max(hi for _, hi in bounds) + 1) * pmax * n
        t_po = torch.zeros(path_cap, dtype=torch.int64, device="cuda")
        t_ph = torch.zeros(path_cap, dtype=torch.int64, device="cuda")
        t_child = torch.zeros(child_cap, dtype=torch.int64, device="cuda")

        def measure(call, searched, grouped):
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
            total, row_max = pgq.mode_steps() if searched else (0, 0)
            class_ms = sum(st["kernel_ms"].values())
            recon = st["kernel_ms"].get("recon", 0.0)
            npaths, cnt = t_np.cpu().numpy(), t_cnt.cpu().numpy()
            r = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "profiled_call_ms": profiled_ms,
                 "rounds": st["levels"], "batches": st["batches"], "walked_edges": st["edges_scanned"],
                 "push_ms": st["kernel_ms"].get("push", 0.0), "recon_ms": recon, "prep_ms": st["kernel_ms"].get("prep", 0.0),
                 "recon_share_of_class_time": recon / class_ms if class_ms > 0 else 0.0,
                 "launches": {k: v for k, v in st["launches"].items() if v},
                 "emitted_walks": int(used["walks"]), "emitted_elements": int(used["elements"]), "rows_with_a_walk": int((npaths > 0).sum()),
                 "steps_total": int(total), "steps_row_max": int(row_max)}
            if grouped:
                ng = t_ng.cpu().numpy()
                r.update({"rows_cut_by_max_paths": int((cnt > npaths).sum()), "groups_total": int(ng.sum()),
                          "rows_by_groups": {str(g): int((ng == g).sum()) for g in range(0, int(ng.max()) + 1)}})
            return r

        res = {"rows": n, "distinct_sources": int(len(np.unique(ps)))}
        for lo, hi in bounds:
            r = {}
            for P in caps:
                for mname, mode in modes:
                    def yard_call(used):
                        rc, pu, cu = dev.k_shortest_walks_mode_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, P, mode, t_len.data_ptr(), t_cnt.data_ptr(),
                                                                        t_first.data_ptr(), t_np.data_ptr(), t_po.data_ptr(), t_ph.data_ptr(), path_cap,
                                                                        t_child.data_ptr(), child_cap)
                        used["walks"], used["elements"] = pu, cu
                        return rc

                    y = r["k_shortest_walks_mode_%s_k%d" % (mname, P)] = measure(yard_call, mode != pgq.MODE_WALK, False)
                    yard_np = t_np.cpu().numpy().copy()
                    line = ["%s: {%d,%d}, max_paths = %d, %s: k_shortest_walks_mode %s ms" % (label, lo, hi, P, mname, "%.3f" % y.get("median_ms", float("nan")))]
                    for g in gs:
                        def group_call(used):
                            rc, pu, cu = dev.k_shortest_groups_bulk_ptr(n, t_s.data_ptr(), t_d.data_ptr(), lo, hi, g, P, mode, t_len.data_ptr(), t_cnt.data_ptr(),
                                                                        t_first.data_ptr(), t_np.data_ptr(), t_ng.data_ptr(), t_po.data_ptr(), t_ph.data_ptr(),
                                                                        path_cap, t_child.data_ptr(), child_cap)
                            used["walks"], used["elements"] = pu, cu
                            return rc

                        m = r["k_shortest_groups_%s_g%d_p%d" % (mname, g, P)] = measure(group_call, mode != pgq.MODE_WALK, True)
                        if "failed" not in m and "failed" not in y:
                            assert (t_np.cpu().numpy() <= yard_np).all()  # a prefix of the yardstick's list
                        line.append("groups = %d %s ms (%s rounds, %s walks, %s groups, %s steps)" % (
                            g, "%.3f" % m.get("median_ms", float("nan")), m.get("rounds"), m.get("emitted_walks"), m.get("groups_total"), m.get("steps_total")))
                    print("; ".join(line), file=sys.stderr, flush=True)
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
