#!/usr/bin/env python3
"""What a step costs in a rim-strip workgroup of the workgroup-row 2D kernel beside a step in any other workgroup, from one
launch's timeline (tools/probes/wg_stamps.hip > stamps.csv):

    wg_rim_ratio.py stamps.csv [rows_i rows_e [strips]]

A workgroup of a chunk of `rows` rows runs rows + 41 steps (six applications; its last chunk may be shorter: those workgroups
are left out).  The chunk rows are read from the probe's "# layout" line, or given (a build whose probe prints none).  Prints
one JSON line: median microseconds per step of both classes and their ratio, and the same ratio between the slowest workgroups
of both classes (finish_ratio) -- the figures behind the wg_edge_pct default.
"""
import json
import statistics
import sys


def main(argv):
    rows_i = rows_e = strips = None
    launch_us = None
    wgs = []
    for line in open(argv[1]):
        if line.startswith("# launch"):
            launch_us = float(line.split()[2])
        elif line.startswith("# layout"):
            f = line.split()
            lay = {f[i]: int(f[i + 1]) for i in range(2, len(f) - 1, 2)}
            rows_i, rows_e, strips = lay["rows_i"], lay["rows_e"], lay["strips"]
        elif line[0].isdigit():
            f = line.split(",")
            wgs.append((float(f[2]) - float(f[1]), int(f[6]), int(f[7])))
    if len(argv) > 3:
        rows_i, rows_e = int(argv[2]), int(argv[3])
    if len(argv) > 4:
        strips = int(argv[4])
    if strips is None:
        strips = max(s for _, s, _ in wgs) + 1
    per_step = {"rim": [], "other": []}
    last = {}
    for _, s, c in wgs:
        last[s] = max(last.get(s, 0), c)
    for us, s, c in wgs:
        rim = s == 0 or s == strips - 1
        if c == last[s] and c > 0:
            continue  # (the strip's last chunk: shorter)
        per_step["rim" if rim else "other"].append(us / ((rows_e if rim else rows_i) + 41))
    out = {"launch_us": launch_us, "strips": strips, "rows_i": rows_i, "rows_e": rows_e, "workgroups": len(wgs)}
    for k, v in per_step.items():
        out[k + "_us_per_step"] = round(statistics.median(v), 4) if v else None
        out[k + "_us_max_workgroup"] = round(max(us for us, s, c in wgs if (s == 0 or s == strips - 1) == (k == "rim")), 1) if v else None
    if per_step["rim"] and per_step["other"]:
        out["rim_ratio"] = round(out["rim_us_per_step"] / out["other_us_per_step"], 4)
        # the same between the slowest workgroups of both classes: what the launch's finish sees
        out["finish_ratio"] = round((out["rim_us_max_workgroup"] / (rows_e + 41)) / (out["other_us_max_workgroup"] / (rows_i + 41)), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv)
