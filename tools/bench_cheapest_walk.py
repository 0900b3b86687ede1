#!/usr/bin/env python3
"""tools/bench_cheapest_walk.py — what the lower bound of a weighted {lower,upper} costs: pgq_cheapest_walk_length_bulk_device and
pgq_cheapest_walk_bulk_device beside pgq_cheapest_path_length_within_bulk_device and pgq_cheapest_path_within_bulk_device at the
same upper bound, same process, same handle, same rows, on the weighted SF100-shaped knows graph of bench.py's snb_cheapest
workload (the graph and the rows of tools/bench_cheapest_within.py and tools/bench_cheapest_path_within.py).

    timeout -k 10 600 python tools/bench_cheapest_walk.py --sets grouped --out profiles/r23/cheapest_walk_grouped.json && \\
    timeout -k 10 1100 python tools/bench_cheapest_walk.py --sets random --out profiles/r23/cheapest_walk_random.json

(each GPU step under a time limit of its own, chained with &&).

The two yardsticks run as many rounds and answer ANOTHER question (lower = 0), so the difference is what the lower bound costs; it
is not a race.  Two row sets: `random`, 4096 random pairs; `grouped`, a 64 x 64 product grouped by source (one lane batch).  Per
row set, bounds and call: --warmup + --steps calls, every call bracketed by a device synchronisation, the median, the minimum and
the maximum over the timed ones.  Then one more call of each with the statistics reset and per-kernel-class event timing on
(option `profile`; the timed calls run without it): rounds, walked edges, the `relax` class (rounds, snapshot or log passes, takes)
and the `recon` class (lengths, walk-back, gather).  Recorded besides: the rows whose value or validity differs from the
yardstick's — the rows a filter around the _within call gets wrong —, NULL rows, list elements, and the peak bytes of a batch's round
log (PGQ_RELAX_TRACE, the library's stderr read back).  NOT separated: the host round trip behind every round of the list calls
and behind every eight of the length calls, the growth of the log and of the staging buffer, the resets, the lane assignment's
share (`prep`, reported as it is)."""
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
    ap.add_argument("--bounds", default="1:3,2:3,2:4,3:4", help="lower:upper pairs, comma-separated")
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
        rows = (n, t_s.data_ptr(), t_d.data_ptr())
        lists = (t_len.data_ptr(), t_off.data_ptr(), t_child.data_ptr(), cap)

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
            call()
            torch.cuda.synchronize()
            st = pgq.get_stats()
            pgq.set_option("profile", 0)
            return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": st["levels"], "batches": st["batches"],
                    "walked_edges": st["edges_scanned"], "relax_algo_bytes": st["algo_bytes"]["relax"],
                    "kernel_ms": {k: v for k, v in st["kernel_ms"].items() if v}, "launches": {k: v for k, v in st["launches"].items() if v}}

        def checked(fn, *args):
            rc, used = fn(*args)
            assert rc == 0, (rc, used, cap)
            return used

        res = {"rows": n, "distinct_sources": int(len(np.unique(ps))), "src_eq_dst_rows": int((ps == pd).sum())}
        for lo, K in bounds:
            r = {}
            r["cheapest_path_length_within"] = measure(lambda: dev.cheapest_within_bulk_ptr(*rows, K, t_val.data_ptr(), t_ok.data_ptr()))
            y_val, y_ok = t_val.cpu().numpy().copy(), t_ok.cpu().numpy().astype(bool)
            r["cheapest_walk_length"] = measure(lambda: dev.cheapest_walk_length_bulk_ptr(*rows, lo, K, t_val.data_ptr(), t_ok.data_ptr()))
            val, ok = t_val.cpu().numpy().copy(), t_ok.cpu().numpy().astype(bool)
            r["cheapest_path_within"] = measure(lambda: checked(dev.cheapest_path_within_bulk_ptr, *rows, K, *lists))
            r["cheapest_path_within"]["list_elements"] = int(checked(dev.cheapest_path_within_bulk_ptr, *rows, K, *lists))
            y_len = t_len.cpu().numpy().copy()
            r["cheapest_walk"] = measure(lambda: checked(dev.cheapest_walk_bulk_ptr, *rows, lo, K, *lists))
            r["cheapest_walk"]["list_elements"] = int(checked(dev.cheapest_walk_bulk_ptr, *rows, lo, K, *lists))
            ln = t_len.cpu().numpy().copy()
            # what must hold: the list call and the length call agree on the rows, h lies within the bounds, a walk of lo..K edges costs
            # at least the cheapest of at most K, and a row the bound does not bind keeps the yardstick's value
            assert ((ln >= 0) == ok).all() and (ln[ok] >= lo).all() and (ln[ok] <= K).all()
            assert not (ok & ~y_ok).any() and (val[ok] >= y_val[ok]).all()
            free = y_ok & (y_len >= lo)
            assert (ok[free]).all() and (val[free] == y_val[free]).all()
            r["rows_differing_from_the_yardstick"] = int(((ok != y_ok) | (ok & y_ok & (val != y_val))).sum())
            r["rows_costlier_than_the_yardstick"] = int((ok & y_ok & (val > y_val)).sum())
            r["rows_null_where_the_yardstick_is_not"] = int((~ok & y_ok).sum())
            r["null_rows"] = int((~ok).sum())
            r["yardstick_null_rows"] = int((~y_ok).sum())
            for call, key in ((lambda: checked(dev.cheapest_walk_bulk_ptr, *rows, lo, K, *lists), "cheapest_walk"),
                              (lambda: checked(dev.cheapest_path_within_bulk_ptr, *rows, K, *lists), "cheapest_path_within")):
                m = re.findall(r"hop log: peak (\d+) bytes", traced(call))
                r[key]["peak_log_bytes_per_batch"] = int(m[-1]) if m else None
            res["walk_%d_%d" % (lo, K)] = r
            print("%s: {%d,%d}: length %.3f ms (yardstick %.3f), list %.3f ms (yardstick %.3f), %d rows differ" % (
                label, lo, K, r["cheapest_walk_length"]["median_ms"], r["cheapest_path_length_within"]["median_ms"], r["cheapest_walk"]["median_ms"],
                r["cheapest_path_within"]["median_ms"], r["rows_differing_from_the_yardstick"]), file=sys.stderr, flush=True)
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
