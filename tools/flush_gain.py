#!/usr/bin/env python3
"""The segment extension's gain on a file of gzip members and zlib streams (window 15), each made
of full-flush segments of datagen's text at mixed levels and memLevels, written by the reference's zlib 1.2.8
(tests/zflush.py), under ATZ_CONTAINERS=gzip without and with ATZ_SEGMENTS=flush: records, n_recomp, trials, ATZ
bytes and sweep_ms of 3 interleaved host-to-host calls each after a warm-up, the library's ATZ_TIMING line of one
child run, and k_marker_ordered's time per GB on a 1 GiB buffer.
usage: python tools/flush_gain.py [out.json]   -> one JSON line"""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import antiz_amd
from antiz_amd import datagen
import zflush
import zraw

STREAMS, GZIP = 240, ("gzip",)


def build_file(seed=61):
    rng = np.random.default_rng(seed)
    parts, nseg, payload = [], 0, 0
    for i in range(STREAMS):
        k = int(rng.integers(2, 9))
        segs = [datagen.text(rng, int(rng.integers(300, 60000))) for _ in range(k)]
        level, memlevel = int(rng.integers(1, 10)), int(rng.choice((8, 8, 8, 9, 7, 4)))
        parts.append(bytes(rng.integers(1, 255, int(rng.integers(20, 200)), dtype=np.uint8)))
        if i % 2:
            parts.append(zflush.flush_stream(segs, level, memlevel, 15)[0])
        else:
            parts.append(zraw.gzip_member(zflush.flush_stream(segs, level, memlevel, -15)[0], b"".join(segs)))
        nseg += k
        payload += sum(len(s) for s in segs)
    return b"".join(parts), nseg, payload


data, nseg, payload = build_file()

if "--timing-child" in sys.argv:   # (run with ATZ_TIMING=1: the library prints its phase times on stderr)
    with antiz_amd.Context(device=0, containers=GZIP, segments=("flush",)) as c:
        c.precompress(data)
        sys.stderr.write("atz: measured call\n")
        c.precompress(data)
    sys.exit(0)

if "--marker-child" in sys.argv:
    big = (data * ((1 << 30) // len(data) + 1))[:1 << 30]
    with antiz_amd.Context(device=0) as c:
        c.flush_markers(big)
        sys.stderr.write("atz: measured call\n")
        c.flush_markers(big)
    sys.exit(0)

out = {"file_bytes": len(data), "streams": STREAMS, "segments": nseg, "payload_bytes": payload}
ctxs = {tag: antiz_amd.Context(device=0, containers=GZIP, segments=names) for tag, names in (("off", ()), ("on", ("flush",)))}
runs = {tag: [] for tag in ctxs}
last = {}
for tag, c in ctxs.items():   # (buffers sized, kernels loaded; the first context of a process runs slower)
    c.precompress(data)
    c.precompress(data)
for _ in range(3):
    for tag, c in ctxs.items():
        t0 = time.perf_counter()
        atz, st = c.precompress(data)
        runs[tag].append((time.perf_counter() - t0, st))
        last[tag] = (atz, st)
for tag, c in ctxs.items():
    atz, st = last[tag]
    out[tag] = {"magic": atz[3], "records": st["n_streams"], "n_recomp": st["n_recomp"], "n_trials": st["n_trials"],
                "atz_bytes": len(atz), "call_ms": [round(1e3 * dt, 1) for dt, _ in runs[tag]],
                "scan_ms": [round(s["scan_ms"], 1) for _, s in runs[tag]],
                "sweep_ms": [round(s["sweep_ms"], 1) for _, s in runs[tag]],
                "k_inflate_ms": [round(s["k_inflate_ms"], 2) for _, s in runs[tag]],
                "k_trial_ms": [round(s["k_trial_ms"], 2) for _, s in runs[tag]],
                "roundtrip_ok": c.reconstruct(atz) == data}
    c.close()
r = subprocess.run([sys.executable, os.path.abspath(__file__), "--timing-child"], env=dict(os.environ, ATZ_TIMING="1"),
                   capture_output=True, text=True)
log = r.stderr.split("atz: measured call\n")[-1]
m = re.search(r"atz: k_marker_ordered: .*", log)
if r.returncode == 0 and m:
    out["timing_line"] = m.group(0)
# the marker kernel alone: 1 GiB of the file's bytes repeated, both passes' device time from the parity call's
# ATZ_TIMING line (the second call of a child process)
r = subprocess.run([sys.executable, os.path.abspath(__file__), "--marker-child"], env=dict(os.environ, ATZ_TIMING="1"),
                   capture_output=True, text=True)
log = r.stderr.split("atz: measured call\n")[-1]
m = re.search(r"atz: k_marker_ordered: (\d+) markers, kernels ([\d.]+) ms", log)
if r.returncode == 0 and m:
    out["marker_kernel"] = {"bytes": 1 << 30, "markers": int(m.group(1)), "kernels_ms_both_passes": float(m.group(2)),
                            "ms_per_GB": round(float(m.group(2)) / ((1 << 30) / 1e9), 3)}
print(json.dumps(out))
if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
    with open(sys.argv[1], "w") as f:
        f.write(json.dumps(out) + "\n")
