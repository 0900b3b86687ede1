#!/usr/bin/env python3
"""tools/collect_runs.py DIR > profiles/rNN/runs.json: the figures of a round's raw outputs in one small file, one run per line.

DIR holds what the round's runs wrote: NAME.json = the one JSON line of `bench.py` or of `tools/bench_within.py` (a name with
`within` in it), and stats_NAME/s_kernel_stats.csv = `rocprofv3 --kernel-trace --stats` tables.  Kept per bench run: ms per
step and the three per-step statistics that must not move; per bounded-call run: the medians; per table: the k_meet3 / k_meet4d
rows.  The raw files (a few KB each, some fifty per round) stay out of the repository."""
import csv
import glob
import json
import os
import re
import sys

KEEP = ("ms_per_step", "rows_answered_by_prepass_per_step", "levels_per_step", "physical_edges_scanned_per_step")


def collect(d):
    out = {"bench": {}, "within_median_ms": {}, "kernel_stats_us": {}}
    for f in sorted(glob.glob(os.path.join(d, "*.json"))):
        name = os.path.basename(f)[:-5]
        r = json.loads(open(f).read().strip().splitlines()[-1])
        if "within" in name:
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
