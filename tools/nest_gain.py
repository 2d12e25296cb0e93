#!/usr/bin/env python3
"""The nesting extension's gain on a file of containers of containers: gzip members and zlib streams
(zlib's deflater, levels 1-9, alternating), each holding a tar-like run of datagen's C3 pieces (PDF-like zlib streams,
PNG-like Z_FILTERED streams, JAR-like ZIP entries), under ATZ_CONTAINERS=zip,gzip ATZ_DEFLATERS=gnu
ATZ_STRATEGIES=filtered, three ways, 3 interleaved host-to-host runs each after a warm-up:
  flat    one call, depth 0
  twice   the flat call, then a second call over the first one's .atz file (what a user can do without the switch)
  nest    one call at depth 1
Per level: records, n_recomp, trials, scan_ms, sweep_ms, k_trial_ms; per way: ATZ bytes, call time, dev_bytes_peak.
usage: python tools/nest_gain.py [out.json] [containers] [bytes per container]   -> one JSON line"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import antiz_amd
from antiz_amd import datagen
import zraw

args = [a for a in sys.argv[1:] if not a.startswith("--")]
CONTAINERS = int(args[1]) if len(args) > 1 else 240
PER = int(args[2]) if len(args) > 2 else 60000
MASKS = dict(containers=("zip", "gzip"), deflaters=("gnu",), strategies=("filtered",))


def build_file(seed=81):
    rng = np.random.default_rng(seed)
    parts, inside = [], 0
    for i in range(CONTAINERS):
        run = datagen._c3_piece((seed * 1000003 + i, PER))
        level = int(rng.integers(1, 10))
        parts.append(bytes(rng.integers(1, 255, int(rng.integers(20, 200)), dtype=np.uint8)))
        if i % 2:
            parts.append(datagen.zstream(run, level))
        else:
            parts.append(zraw.gzip_member(zraw.raw_deflate(run, level, 8), run, name=b"run%d.tar" % i))
        inside += len(run)
    return b"".join(parts), inside


def level(st):
    return {"records": st["n_streams"], "n_recomp": st["n_recomp"], "n_trials": st["n_trials"],
            "file_bytes": st["file_bytes"], "scan_ms": round(st["scan_ms"], 1), "sweep_ms": round(st["sweep_ms"], 1),
            "k_trial_ms": round(st["k_trial_ms"], 2), "k_inflate_ms": round(st["k_inflate_ms"], 2),
            "write_ms": round(st["write_ms"], 2)}


data, inside = build_file()
out = {"file_bytes": len(data), "containers": CONTAINERS, "payload_bytes": inside, "masks": {k: list(v) for k, v in MASKS.items()}}
flat = antiz_amd.Context(device=0, **MASKS)
nest = antiz_amd.Context(device=0, nest=1, **MASKS)


def run_flat():
    t0 = time.perf_counter()
    atz, st = flat.precompress(data)
    return {"call_ms": round(1e3 * (time.perf_counter() - t0), 1), "atz_bytes": len(atz), "magic": atz[:4].hex(),
            "dev_bytes_peak": st["dev_bytes_peak"], "levels": [level(st)]}, atz


def run_twice():
    t0 = time.perf_counter()
    atz, st = flat.precompress(data)
    t1 = time.perf_counter()
    atz2, st2 = flat.precompress(atz)
    t2 = time.perf_counter()
    return {"call_ms": round(1e3 * (t2 - t0), 1), "first_ms": round(1e3 * (t1 - t0), 1), "second_ms": round(1e3 * (t2 - t1), 1),
            "atz_bytes": len(atz2), "magic": atz2[:4].hex(), "second_input_bytes": len(atz),
            "dev_bytes_peak": max(st["dev_bytes_peak"], st2["dev_bytes_peak"]), "levels": [level(st), level(st2)]}, atz2


def run_nest():
    t0 = time.perf_counter()
    atz, st = nest.precompress(data)
    dt = time.perf_counter() - t0
    lv = [level(st)]
    try:
        lv.append(level(nest.nest_stats(1)))
    except antiz_amd.AtzError:
        pass
    return {"call_ms": round(1e3 * dt, 1), "atz_bytes": len(atz), "magic": atz[:4].hex(),
            "dev_bytes_peak": st["dev_bytes_peak"], "levels": lv}, atz


ways = (("flat", run_flat), ("twice", run_twice), ("nest", run_nest))
for _, fn in ways:   # (buffers sized, kernels loaded; the first context of a process runs slower)
    fn()
    fn()
runs = {tag: [] for tag, _ in ways}
last = {}
for _ in range(3):
    for tag, fn in ways:
        res, atz = fn()
        runs[tag].append(res)
        last[tag] = atz
for tag, _ in ways:
    out[tag] = dict(runs[tag][-1], call_ms=[r["call_ms"] for r in runs[tag]],
                    levels_sweep_ms=[[lv["sweep_ms"] for lv in r["levels"]] for r in runs[tag]],
                    levels_scan_ms=[[lv["scan_ms"] for lv in r["levels"]] for r in runs[tag]],
                    levels_k_trial_ms=[[lv["k_trial_ms"] for lv in r["levels"]] for r in runs[tag]])
out["flat"]["roundtrip_ok"] = flat.reconstruct(last["flat"]) == data
out["twice"]["roundtrip_ok"] = flat.reconstruct(flat.reconstruct(last["twice"])) == data
out["nest"]["roundtrip_ok"] = flat.reconstruct(last["nest"]) == data
flat.close()
nest.close()
print(json.dumps(out))
if args:
    with open(args[0], "w") as f:
        f.write(json.dumps(out) + "\n")
