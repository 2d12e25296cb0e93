#!/usr/bin/env python3
"""A workload (default C3) precompressed without and with the probe extension alone (ATZ_PROBE=deflate, no
container mask): records, n_recomp, the raw records among them and how many of the file's
JAR-like ZIP bodies they are (the container extension finds every one through its anchor), ATZ bytes, MB/s, scan_ms
and sweep_ms of 3 interleaved host calls each after a warm-up (upload included), and from one ATZ_TIMING=1 child
run the probe's counts (survivors, decoded, accepted, kept), k_probe_ordered's time (both passes) and the probe
decode's k_inflate time.
usage: python tools/probe_gain.py [cache_dir] [--workload c3|c4]   -> one JSON line"""
import json
import os
import re
import struct
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import antiz_amd
from antiz_amd import datagen

cache = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "/tmp/atz_bench_cache"
workload = sys.argv[sys.argv.index("--workload") + 1] if "--workload" in sys.argv else "c3"
data = open(datagen.cached(workload, cache), "rb").read()

if "--timing-child" in sys.argv:   # (run with ATZ_TIMING=1: the library prints its phase times on stderr)
    with antiz_amd.Context(device=0, probe=("deflate",)) as c:
        c.precompress(data)
        sys.stderr.write("atz: measured call\n")
        c.precompress(data)
    sys.exit(0)


def zip_bodies():
    """{offset of the body: BTYPE of its first block} over the file's ZIP local headers with method 8."""
    out, at = {}, data.find(b"PK\3\4")
    while at >= 0:
        if at + 30 <= len(data) and data[at + 8:at + 10] == b"\x08\0":
            nlen, xlen = struct.unpack_from("<HH", data, at + 26)
            d = at + 30 + nlen + xlen
            if d < len(data):
                out[d] = (data[d] >> 1) & 3
        at = data.find(b"PK\3\4", at + 1)
    return out


def summary(atz, bodies):
    """-> (descriptors, raw ones, raw ones that are a ZIP body, and exact among those)"""
    n, pos = struct.unpack_from("<Q", atz, 20)[0], 28
    raw = hit = exact = 0
    for _ in range(n):
        off, _, il = struct.unpack_from("<QQQ", atz, pos)
        c = atz[pos + 24]
        nd = struct.unpack_from("<Q", atz, pos + 27)[0]
        pos += 35 + (8 + 9 * nd if nd else 0) + il
        if atz[3] == 3 and c & 0x40:
            raw += 1
            hit += off in bodies
            exact += off in bodies and nd == 0
    return n, raw, hit, exact


bodies = zip_bodies()
out = {"workload": workload, "file_bytes": len(data), "zip_bodies": len(bodies),
       "zip_bodies_by_first_btype": {str(t): sum(1 for v in bodies.values() if v == t) for t in (0, 1, 2)}}
ctxs = {tag: antiz_amd.Context(device=0, probe=names) for tag, names in (("off", ()), ("on", ("deflate",)))}
runs = {tag: [] for tag in ctxs}
last = {}
for tag, c in ctxs.items():   # (buffers sized, kernels loaded; the first context of a process runs slower)
    c.precompress(data)
    c.precompress(data)
for _ in range(3):
    for tag, c in ctxs.items():
        t0 = time.perf_counter()
        atz, st = c.precompress(data)
        runs[tag].append((time.perf_counter() - t0, st["sweep_ms"], st["scan_ms"]))
        last[tag] = (atz, st)
for tag, c in ctxs.items():
    atz, st = last[tag]
    n, raw, hit, exact = summary(atz, bodies)
    out[tag] = {"magic": atz[3], "n_streams": st["n_streams"], "n_recomp": st["n_recomp"], "raw_recorded": raw,
                "zip_bodies_recorded": hit, "zip_bodies_exact": exact, "atz_bytes": len(atz), "n_trials": st["n_trials"],
                "MB_per_s": [round(len(data) / 1e6 / dt, 1) for dt, _, _ in runs[tag]],
                "sweep_ms": [round(x, 1) for _, x, _ in runs[tag]], "scan_ms": [round(x, 1) for _, _, x in runs[tag]],
                "k_inflate_ms": round(st["k_inflate_ms"], 3), "dev_bytes_peak": st["dev_bytes_peak"],
                "roundtrip_ok": c.reconstruct(atz) == data}
    c.close()
r = subprocess.run([sys.executable, os.path.abspath(__file__), cache, "--workload", workload, "--timing-child"],
                   env=dict(os.environ, ATZ_TIMING="1"), capture_output=True, text=True)
log = r.stderr.split("atz: measured call\n")[-1]
m = re.search(r"k_probe_ordered: (\d+) survivors, kernels ([\d.]+) ms \(both passes\), (\d+) decoded, k_inflate ([\d.]+) ms, "
              r"(\d+) accepted, (\d+) kept", log)
if r.returncode == 0 and m:
    out["timing"] = {"survivors": int(m.group(1)), "probe_kernel_ms": float(m.group(2)),
                     "probe_kernel_ms_per_GB": round(float(m.group(2)) / (len(data) / 1e9), 3),
                     "decoded": int(m.group(3)), "probe_inflate_ms": float(m.group(4)), "accepted": int(m.group(5)),
                     "kept": int(m.group(6))}
print(json.dumps(out))
