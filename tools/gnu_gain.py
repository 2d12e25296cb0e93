#!/usr/bin/env python3
"""The deflater extension's gain on the end-to-end file of tests/test_gpu_gnu.py (gzip members
around the bodies of tests/golden/gnu.json / gnu.bin, written by GNU gzip, plus the zip-made archive), under
ATZ_CONTAINERS=zip,gzip without and with ATZ_DEFLATERS=gnu: records, n_recomp, raw bodies recorded exactly, with
a diff list and as GNU's, trials, ATZ bytes, sweep_ms of 3 interleaved calls each after a warm-up, and from one
ATZ_TIMING=1 child run the summed time of k_trial_fast_gnu and k_trial_slow_gnu beside the raw pass's k_trial time.
usage: python tools/gnu_gain.py   -> one JSON line"""
import json
import os
import re
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import antiz_amd
import test_gpu_gnu as T

data, recs = T.build_file(T.ENTRIES)
BOTH = ("zip", "gzip")

if "--timing-child" in sys.argv:   # (run with ATZ_TIMING=1: the library prints its phase times on stderr)
    with antiz_amd.Context(device=0, containers=BOTH, deflaters=("gnu",)) as c:
        c.precompress(data)
        sys.stderr.write("atz: measured call\n")
        c.precompress(data)
    sys.exit(0)


def summary(atz):
    """-> (descriptors, raw ones, exact raw ones, raw ones with a diff list, GNU ones)"""
    n, pos = struct.unpack_from("<Q", atz, 20)[0], 28
    raw = exact = diff = gnu = 0
    for _ in range(n):
        _, _, il = struct.unpack_from("<QQQ", atz, pos)
        c, m = atz[pos + 24], atz[pos + 26]
        nd = struct.unpack_from("<Q", atz, pos + 27)[0]
        pos += 35 + (8 + 9 * nd if nd else 0) + il
        if c & 0x40:
            raw += 1
            exact += nd == 0
            diff += nd != 0
            gnu += m == 0
    return n, raw, exact, diff, gnu


out = {"file_bytes": len(data), "bodies": len(recs), "versions": T.G["versions"],
       "bodies_by_class": {k: sum(1 for r in recs if r[3] == k) for k in "abcdef"}}
ctxs = {tag: antiz_amd.Context(device=0, containers=BOTH, deflaters=names) for tag, names in (("off", ()), ("on", ("gnu",)))}
runs = {tag: [] for tag in ctxs}
last = {}
for tag, c in ctxs.items():   # (buffers sized, kernels loaded; the first context of a process runs slower)
    c.precompress(data)
    c.precompress(data)
for _ in range(3):
    for tag, c in ctxs.items():
        t0 = time.perf_counter()
        atz, st = c.precompress(data)
        runs[tag].append((time.perf_counter() - t0, st["sweep_ms"], st["k_trial_ms"]))
        last[tag] = (atz, st)
for tag, c in ctxs.items():
    atz, st = last[tag]
    n, raw, exact, diff, gnu = summary(atz)
    out[tag] = {"magic": atz[3], "n_streams": st["n_streams"], "n_recomp": st["n_recomp"], "raw_recorded": raw,
                "raw_exact": exact, "raw_with_diffs": diff, "gnu_recorded": gnu, "atz_bytes": len(atz),
                "n_trials": st["n_trials"], "call_ms": [round(1e3 * dt, 1) for dt, _, _ in runs[tag]],
                "sweep_ms": [round(x, 1) for _, x, _ in runs[tag]], "k_trial_ms": [round(x, 2) for _, _, x in runs[tag]],
                "roundtrip_ok": c.reconstruct(atz) == data}
    c.close()
r = subprocess.run([sys.executable, os.path.abspath(__file__), "--timing-child"], env=dict(os.environ, ATZ_TIMING="1"),
                   capture_output=True, text=True)
log = r.stderr.split("atz: measured call\n")[-1]
m = re.search(r"raw pass: k_trial_fast_gnu \+ k_trial_slow_gnu\s+([\d.]+) ms of k_trial\s+([\d.]+) ms", log)
p = re.search(r"raw pass: (\d+) streams, (\d+) trials\s+([\d.]+) ms", log)
if r.returncode == 0 and m and p:
    out["timing"] = {"gnu_kernels_ms": float(m.group(1)), "raw_pass_k_trial_ms": float(m.group(2)),
                     "raw_pass_streams": int(p.group(1)), "raw_pass_trials": int(p.group(2)), "raw_pass_ms": float(p.group(3))}
print(json.dumps(out))
