#!/usr/bin/env python3
"""tools/collect_runs.py DIR > profiles/rNN/runs.json: the figures of a round's raw outputs in one small file, one run per line.

DIR holds what the round's runs wrote: NAME.json = the one JSON line of `bench.py` or of `tools/bench_within.py` (a name with
`within` in it) or the --out file of `tools/bench_k_walks.py`, `bench_path_modes.py` or `bench_k_groups.py`, and
stats_NAME/s_kernel_stats.csv = `rocprofv3 --kernel-trace --stats` tables.  Kept per bench run: ms per
step and the three per-step statistics that must not move; per bounded-call run: the medians; per table: the k_meet3 / k_meet4d
rows; per column of a walk benchmark: [median, min, max] ms of the timed calls, the event-timed call's `recon` ms and the
counters WALK_COUNTS (null where a column has none).  The raw files (a few KB each, some fifty per round) stay out of the
repository."""
import csv
import glob
import json
import os
import re
import sys

KEEP = ("ms_per_step", "rows_answered_by_prepass_per_step", "levels_per_step", "physical_edges_scanned_per_step")
WALK_COUNTS = ("rounds", "walked_edges", "emitted_walks", "emitted_elements", "steps_total")


def walk_columns(x, path=()):
    if not isinstance(x, dict):
        return {}
    if "median_ms" in x:
        recon = x.get("recon_ms", x.get("kernel_ms", {}).get("recon"))  # (the cheapest-path tools keep their classes in kernel_ms)
        return {" ".join(path): {"ms": [round(x[k], 3) for k in ("median_ms", "min_ms", "max_ms")], "recon_ms": None if recon is None else round(recon, 3),
                                 "counts": [x.get(k, x.get("emitted_paths") if k == "emitted_walks" else None) for k in WALK_COUNTS]}}
    out = {}
    for k, v in x.items():
        out.update(walk_columns(v, path + (k,)))
    return out


def collect(d):
    out = {"bench": {}, "within_median_ms": {}, "walk_calls": {}, "kernel_stats_us": {}}
    for f in sorted(glob.glob(os.path.join(d, "*.json"))):
        name = os.path.basename(f)[:-5]
        text = open(f).read().strip()
        r = json.loads(text if text.startswith("{\n") else text.splitlines()[-1])  # (an --out file is indented: the whole of it)
        if walk_columns(r):
            out["walk_calls"][name] = walk_columns(r)
        elif "within" in name:
            out["within_median_ms"][name] = {k: round(v["median_ms"], 4) for k, v in r.items() if isinstance(v, dict)}
        else:
            out["bench"][name] = {k: (round(r[k], 5) if k == "ms_per_step" else r[k]) for k in KEEP}
    for f in sorted(glob.glob(os.path.join(d, "stats_*", "s_kernel_stats.csv"))):
        name = os.path.basename(os.path.dirname(f))[6:]
        for r in csv.DictReader(open(f)):
            if "k_meet3<" in r["Name"] or "k_meet4d<" in r["Name"]:
                k = re.sub(r"\(.*", "", r["Name"]).replace("void pgq::", "")
                out["kernel_stats_us"].setdefault(name, {})[k] = {
                    "calls": int(r["Calls"]), "avg": round(float(r["AverageNs"]) / 1000, 2),
                    "min": round(int(r["MinNs"]) / 1000, 2), "max": round(int(r["MaxNs"]) / 1000, 2)}
    return out


def main():
    out = collect(sys.argv[1])
    lines = ["{"]
    for si, (sec, runs) in enumerate(out.items()):
        lines.append(" %s: {" % json.dumps(sec))
        lines += ["  %s: %s%s" % (json.dumps(k), json.dumps(v), "," if i < len(runs) - 1 else "") for i, (k, v) in enumerate(runs.items())]
        lines.append(" }" + ("," if si < len(out) - 1 else ""))
    print("\n".join(lines + ["}"]))


if __name__ == "__main__":
    main()
