#!/usr/bin/env python3
"""Summary of interleaved bench.py runs: for each label, the files holding its runs' result lines (one JSON
line per run) -> medians and ranges of MB/s, and the stream counts and ATZ bytes of the last run.
usage: python tools/bench_runs.py label=file[,file...] [label=...]   -> one JSON object"""
import json
import statistics
import sys

out = {}
for arg in sys.argv[1:]:
    label, files = arg.split("=", 1)
    runs = []
    for f in files.split(","):
        for line in open(f):
            line = line.strip()
            if line.startswith("{"):
                runs.append(json.loads(line))
    v = [r["value"] for r in runs]
    d = runs[-1]["detail"]
    out[label] = {"runs_MB_per_s": v, "median_MB_per_s": round(statistics.median(v), 1), "min": min(v), "max": max(v),
                  "n_streams": d["n_streams"], "n_recomp": d["n_recomp"], "atz_bytes": d["atz_bytes"],
                  "file_bytes": d["file_bytes"], "n_trials": d["n_trials"], "scan_ms": d["scan_ms"],
                  "sweep_ms": d["sweep_ms"], "k_other_ms": d["k_other_ms"]}
print(json.dumps(out, indent=1))
